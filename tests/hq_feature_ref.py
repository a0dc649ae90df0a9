"""Float64 reference, fp32 yardsticks and input builders for the SAM-HQ FEATURE branch as the product runs it
(csrc/sam_model.cpp: SamModel::hq_branch, twice per encoder pass, then k::hq_features_finish), shared by
tests/test_hq_feature_ref.py (CPU) and tests/test_gpu_hq_features.py (GPU).  No test functions here.

Written from the contracts (kernels.hpp: GemmArgs, k::layernorm, k::hq_features_finish; sam_weights.cpp: conv_transpose_h), not
from the kernels.  One branch, a [M][K] f16, M = 4096 tokens per image:

  * loader   a ConvTranspose2d(kernel 2, stride 2) weight [ci][co][2][2] becomes the GEMM weight [4 co][ci], row = s * co + channel
             with the sub-pixel s = ky * 2 + kx, rounded to f16; its bias [co] is repeated for the four sub-pixels; norms as they are
  * A        A[m, s1 * C + c] = sum_k a[m, k] W1[s1 * C + c, k] + b1[c]                      fp32 [M][4 C]     (gemm_ref.plain)
  * H        H[m * 4 + s1, c] = f16(GELU(LN_C(A[m, s1 * C : (s1 + 1) * C]) * ln_w + ln_b))   f16 [4 M][C]      A read as [4 M][C];
             biased variance, eps 1e-6, erf-form GELU                                                           (row_ref.layernorm64)
  * Y        Y[r, s2 * 32 + c] = sum_k H[r, k] W2[s2 * 32 + c, k]                            fp32 [4 M][128]   no bias here
  * features out[pixel, c] = Y_vit[...] + Y_emb[...] + b2_vit[c] + b2_emb[c], pixel (4 ty + 2 (s1 >> 1) + (s2 >> 1),
             4 tx + 2 (s1 & 1) + (s2 & 1)) of token (ty, tx)                                                    (hq_kernel_ref.finish)

C = 256 and K = embed_dim for the ViT branch (the 16-byte LayerNorm kernel, a second GEMM of four K steps), C = 64 and K = 256
for the embedding branch (the scalar LayerNorm kernel, one K step).

Measure and allowance are gemm_ref's: every stage is computed from the operands that stage was given ON THE DEVICE (teacher
forcing: A from a, H from the delivered A, Y from the delivered H), everything else in float64; a kernel may need ALLOW = 1.25
times what the larger numpy fp32 yardstick needs on the same inputs (GEMMs: chain / trunc16; LayerNorm: row_ref.yardsticks), f16
results half an f16 spacing on top.  Only the finished features are compared free-running (`emulate`), at 3 times the distance
between the emulation in float64 and in float32 (tests/test_gpu_encoder.py, test_free_running_distance).
"""
from typing import Dict, Optional

import numpy as np

import gemm_ref as G
import hq_kernel_ref as HK
import row_ref as RR
from gemm_ref import ACCUMULATIONS, ALLOW, check, check_f16, gelu64, plain, round_f16, ulp16  # noqa: F401
from hq_kernel_ref import finish  # noqa: F401

f16, f32, f64 = np.float16, np.float32, np.float64

EPS = 1e-6
TOKENS = 4096
BRANCHES = {"vit": ("dec.hq.vit", 256), "emb": ("dec.hq.emb", 64)}      # name -> (tensor prefix, C)
OPERANDS = ("w1", "b1", "ln_w", "ln_b", "w2", "b2")


# ------------------------------------------------------------------------------------------ loader

def permute_conv_t(w, order: str = "yx") -> np.ndarray:
    """[ci][co][2][2] -> [4 co][ci], row = s * co + channel, s = ky * 2 + kx ("yx", the contract) or kx * 2 + ky ("xy", a modified
    model).  Keeps the dtype: it only moves values."""
    w = np.asarray(w)
    ci, co = w.shape[:2]
    axes = (2, 3, 1, 0) if order == "yx" else (3, 2, 1, 0)
    return np.ascontiguousarray(w.transpose(axes)).reshape(4 * co, ci)


def loader_operands(params, branch: str, round_weights: bool = True, order: str = "yx", bias1: str = "all",
                    bias2_scale: float = 1.0) -> Dict[str, np.ndarray]:
    """The six operands of one branch from the raw tensors, as the loader leaves them: w1 [4 C][K] and w2 [128][C] permuted and
    rounded to f16 (float64 and unrounded with round_weights=False), b1 [4 C] and b2 [128] the biases four times over, the norms
    unchanged.  Modified models: order="xy"; bias1="first" (conv1's bias on sub-pixel 0 only); bias2_scale=2 (conv2's bias twice)."""
    pre, _ = BRANCHES[branch]
    cast = (lambda v: np.asarray(v, f32).astype(f16)) if round_weights else (lambda v: np.asarray(v, f64))
    b1 = np.tile(np.asarray(params[pre + ".conv1.b"], f32), 4)
    if bias1 == "first":
        b1[len(b1) // 4:] = 0
    return {"w1": cast(permute_conv_t(params[pre + ".conv1.w"], order)), "b1": b1,
            "ln_w": np.asarray(params[pre + ".ln.w"], f32), "ln_b": np.asarray(params[pre + ".ln.b"], f32),
            "w2": cast(permute_conv_t(params[pre + ".conv2.w"], order)),
            "b2": np.tile(np.asarray(params[pre + ".conv2.b"], f32), 4) * f32(bias2_scale)}


# ------------------------------------------------------------------------------------------ stages (float64)

def stage_a(a16, ops) -> np.ndarray:
    """[M][4 C] float64 from the f16 input and the branch's operands."""
    return plain(a16, ops["w1"], ops["b1"])


def stage_h(A32, ops, eps: float = EPS, gelu: str = "erf", unbiased: bool = False, over_4c: bool = False) -> np.ndarray:
    """[4 M][C] float64, not rounded, from the fp32 A as delivered.  Modified models: gelu="tanh", unbiased, another eps,
    over_4c (the LayerNorm taken over the 4 C columns of a token; scale and shift still per channel)."""
    A = np.asarray(A32, f32)
    C = len(ops["ln_w"])
    if over_4c:
        y = RR.layernorm64(A, np.tile(ops["ln_w"], 4), np.tile(ops["ln_b"], 4), eps, 1, unbiased, gelu)
        return y.reshape(-1, C)
    return RR.layernorm64(A.reshape(-1, C), ops["ln_w"], ops["ln_b"], eps, 1, unbiased, gelu)


def stage_h_yardsticks(A32, ops, eps: float = EPS) -> Dict[str, np.ndarray]:
    """fp32 [4 M][C] before the rounding to f16: row_ref's LayerNorm yardsticks with GELU on A read as [4 M][C]."""
    C = len(ops["ln_w"])
    return RR.yardsticks(np.asarray(A32, f32).reshape(-1, C), ops["ln_w"], ops["ln_b"], eps, 1)


def stage_y(H16, ops) -> np.ndarray:
    """[4 M][128] float64 from the f16 H as delivered; no bias."""
    return plain(H16, ops["w2"])


def gemm_yardsticks(A16, W16, bias=None, chunk: int = 256) -> Dict[str, np.ndarray]:
    """chain / trunc16 of gemm_ref on the WHOLE tensor, `chunk` rows at a time (rows are independent, and a block of 256 rows
    of the accumulator stays in cache over the K steps: seconds for 4096 x 1024 x 320 instead of tens of seconds).  A row subset
    would do for the rms, but the largest error of 4 million elements is not the largest of a tenth of them."""
    A16 = np.asarray(A16)
    parts = [G.plain_yardsticks(A16[r:r + chunk], W16, bias) for r in range(0, len(A16), chunk)]
    return {name: np.concatenate([p[name] for p in parts]) for name in parts[0]}


def check_gemm(name: str, got32, A16, W16, bias=None) -> None:
    """A GEMM result [M][N] against gemm_ref.plain through gemm_ref.check, in units of the fp32 rounding model."""
    ref = plain(A16, W16, bias)
    check(name, got32, ref, G.output_model(ref), gemm_yardsticks(A16, W16, bias))


def check_h(name: str, got16, A32, ops) -> float:
    """H as delivered against float64 GELU(LN(A delivered)) element by element (gemm_ref.check_f16 on the whole tensor)."""
    return check_f16(name, got16, stage_h(A32, ops), stage_h_yardsticks(A32, ops))


# ------------------------------------------------------------------------------------------ free-running emulation

def emulate_branch(a, ops, ft=f64, round_h: bool = True, **h_variant) -> np.ndarray:
    """Y [4 M][128] of one branch from its input, every stage feeding the next, arithmetic in `ft` (float64, or float32 for the
    distance the free-running comparison is allowed); H rounded to f16 as the contract says (round_h=False: a modified model)."""
    a, w1, w2 = np.asarray(a).astype(ft), np.asarray(ops["w1"]).astype(ft), np.asarray(ops["w2"]).astype(ft)
    A = a @ w1.T + np.asarray(ops["b1"]).astype(ft)
    C = len(ops["ln_w"])
    if ft is f64:
        over = h_variant.pop("over_4c", False)
        x = A if over else A.reshape(-1, C)
        lw, lb = (np.tile(ops["ln_w"], 4), np.tile(ops["ln_b"], 4)) if over else (ops["ln_w"], ops["ln_b"])
        d = x - x.mean(axis=1, keepdims=True)
        n = x.shape[1] - (1 if h_variant.get("unbiased") and x.shape[1] > 1 else 0)
        y = d / np.sqrt((d * d).sum(axis=1, keepdims=True) / n + h_variant.get("eps", EPS)) * np.asarray(lw, f64) + np.asarray(lb, f64)
        h = G.GELUS[h_variant.get("gelu", "erf")](y).reshape(-1, C)
    else:
        assert not h_variant
        x = A.reshape(-1, C)
        d = x - x.mean(axis=1, keepdims=True, dtype=ft)
        y = d / np.sqrt((d * d).mean(axis=1, keepdims=True, dtype=ft) + ft(EPS)) * np.asarray(ops["ln_w"], ft) + np.asarray(ops["ln_b"], ft)
        h = gelu64(y.astype(f64)).astype(ft)
    if round_h:
        h = h.astype(f16).astype(ft)
    return h @ w2.T


def emulate(a_vit, a_emb, ops_vit, ops_emb, ft=f64, round_h: bool = True, **h_variant) -> np.ndarray:
    """The finished features [256, 256, 32] of one image from the two branches' inputs."""
    yv = emulate_branch(a_vit, ops_vit, ft, round_h, **dict(h_variant))
    ye = emulate_branch(a_emb, ops_emb, ft, round_h, **dict(h_variant))
    return finish(yv, ye, ops_vit["b2"][:32], ops_emb["b2"][:32]).astype(f64)


# ------------------------------------------------------------------------------------------ inputs

KINDS = ("gaussian", "spike", "offset")
SPIKE_ROW = G.SPIKE_ROW
SPIKE_CHANNEL = 5            # a column of A: sub-pixel 0, channel 5 in both branches
OFFSET_BIAS = 40.0           # what offset_params adds to both conv1 biases
OFFSET_SCALE = 0.08          # ... and the scale of the input that goes with it


def offset_params(params) -> dict:
    """A copy of the raw tensors with 40 added to the conv1 bias of both branches.  The hook runs the model's own operands, and
    no input can move the 4 C columns of A together (K < 4 C): rows whose mean dwarfs their spread need the bias, as the offset
    rows of gemm_ref.stream_case need their residual.  With an input of scale 0.08, A's LayerNorm rows have a spread near 0.055
    (0.046 from the product, 0.029 from the bias's own U(-0.05, 0.05)) around 40: |mean| >= 300 spread."""
    out = dict(params)
    for pre, _ in BRANCHES.values():
        out[pre + ".conv1.b"] = (np.asarray(params[pre + ".conv1.b"], f32) + f32(OFFSET_BIAS)).astype(f32)
    return out


def branch_input(kind: str, seed: int, ops, images: int = 1) -> np.ndarray:
    """f16 [images * 4096][K] for a branch whose loaded operands are `ops`:
      gaussian  N(0, 1): a LayerNorm'ed embedding, a residual stream of unit scale
      spike     the same, and row SPIKE_ROW of every image aimed at column SPIKE_CHANNEL of A: gemm_ref.add_spike with the roles of
                the operands exchanged (the hook runs the model's own W1, so the spike is made on the input's side) -- the input
                row is the minimum-norm solution u of W1[0:C] u = t e_channel on top of its Gaussian, t = 300 times the rms of the
                row's other columns.  Exact when K >= C (both branches at D = 320, the embedding branch always); with K < C the
                other columns take what the least squares leaves them (spike_conditions says how much is asked for)
      offset    0.08 N(0, 1), for a model written from offset_params"""
    rng = np.random.default_rng(seed)
    K = np.asarray(ops["w1"]).shape[1]
    M = images * TOKENS
    if kind == "offset":
        return (OFFSET_SCALE * rng.standard_normal((M, K))).astype(f16)
    a = rng.standard_normal((M, K))
    if kind == "spike":
        C = len(ops["ln_w"])
        block = np.asarray(ops["w1"], f64)[:C]
        target = np.zeros(C)
        target[SPIKE_CHANNEL] = 1.0
        u = np.linalg.lstsq(block, target, rcond=None)[0]
        for b in range(images):
            row = b * TOKENS + SPIKE_ROW
            rest = G.rms(np.delete(block @ a[row] + np.asarray(ops["b1"], f64)[:C], SPIKE_CHANNEL))
            a[row] += 300.0 * rest * u / (block[SPIKE_CHANNEL] @ u)
    else:
        assert kind == "gaussian", kind
    assert np.abs(a).max() < G.F16_LIMIT
    return a.astype(f16)


def spike_floor(K: int, C: int) -> float:
    """What the spike row's column must reach, in rms of the row's other columns: 250 where the aim is exact (K >= C); with K < C
    a random W1 block lets the least squares put K / C of the target into the column and spreads the rest over the C - 1
    others, a ratio near sqrt(K C / (C - K)) (16 at K = 128, C = 256): 10 is asked for."""
    return 250.0 if K >= C else 10.0


def input_conditions(kind: str, A_ref, ops) -> None:
    """On the float64 A of the very input a kernel gets."""
    A = np.asarray(A_ref, f64)
    C = len(ops["ln_w"])
    K = np.asarray(ops["w1"]).shape[1]
    assert np.abs(A).max() < G.F16_LIMIT
    rows = A.reshape(-1, C)
    if kind == "gaussian":
        assert 0.2 <= G.rms(A) <= 5.0, G.rms(A)
    if kind == "spike":
        for r in range(SPIKE_ROW, len(A), TOKENS):
            rest = np.delete(A[r, :C], SPIKE_CHANNEL)
            assert abs(A[r, SPIKE_CHANNEL]) >= spike_floor(K, C) * G.rms(rest), (abs(A[r, SPIKE_CHANNEL]) / G.rms(rest))
    if kind == "offset":
        ratio = np.abs(rows.mean(axis=1)) / rows.std(axis=1)
        assert ratio.min() >= 300, float(ratio.min())
