"""Float64 references, fp32 yardsticks and input builders for the SAM-HQ kernels alone and the kernel that feeds them
(kernels.hpp: k::hq_mask_path, k::upscale_logits, k::hq_features_finish), shared by tests/test_hq_kernel_ref.py (CPU) and
tests/test_gpu_hq_kernels.py (GPU).  No test functions here.

Written from the launches' CONTRACTS (kernels.hpp), not from the kernels:

  * hq_mask_path   stage 1  H[Y, X, :] = f16(GELU(LN2d_64(sum_taps W1[tap] . U[Y + ky - 1, X + kx - 1, :] + b1)))   zero padding
                   stage 2  plane[Y, X] = hyper_hq . (sum_taps W2[tap] . H[Y + ky - 1, X + kx - 1, :] + b2 + features[Y, X, :])
                            logits[m] += plane for the four planes m
                   W1 [9][64][32], W2 [9][32][64]: tap = ky * 3 + kx, then output channel, then input channel; LN2d with the
                   biased variance and eps; GELU in the erf form
  * upscale_logits up1 = keys . W1^T + b1 (columns s1 * 64 + channel), LN2d_64 per sub-pixel s1, GELU, f16;
                   u = GELU(. W2^T + b2) (columns s2 * 32 + channel); pixel (4 ty + 2 (s1 >> 1) + (s2 >> 1),
                   4 tx + 2 (s1 & 1) + (s2 & 1)) of token (ty, tx): a transposed convolution of kernel 2 and stride 2 puts
                   sub-pixel s = dy * 2 + dx of position (y, x) at (2 y + dy, 2 x + dx), twice;
                   logits[m] = hyper[m] . u, u_out = f16(u)
  * hq_features_finish  out[pixel, c] = vit[token * 4 + s1, s2 * 32 + c] + emb[same] + b_vit[c] + b_emb[c], the same pixel mapping

Measure and allowance are gemm_ref's: the REFERENCE takes a launch's own operands (for stage 2 of the HQ path: the H the launch
delivered) and does everything else in float64; errors count in units of the reference rounded once to the output's format; a
kernel may need ALLOW = 1.25 times what the LARGER of two numpy fp32 yardsticks (`chain`, `trunc16`) needs on the same inputs.
A yardstick accumulates over an im2col of the operand in the contract's column order (tap, then input channel) and applies the
epilogue once per operation in fp32, in the order the contract writes it.  Which GELU: hq_mask_path evaluates the erf form, and
so do its yardsticks; upscale_logits evaluates the fitted form of the GEMM epilogues (gemm_ref, convention (2)), so its
yardsticks apply gelu_fitted while its reference keeps the erf form.  The yardsticks of upscale_logits round the intermediate
between the two transposed convolutions to f16, as the contract says; its reference does not.
"""
from typing import Dict, Tuple

import numpy as np

import gemm_ref as G
from gemm_ref import ALLOW, F16_LIMIT, check, check_f16, gelu64, gelu_fitted, output_model, ratios, round_f16  # noqa: F401

f16, f32, f64 = np.float16, np.float32, np.float64

RES = 256                   # the low-res grid
PIXELS = RES * RES
C_U, C_H, C_OUT = 32, 64, 32
EPS = 1e-6
TILE = 16                   # hq_mask_path's pixel tile
U1 = 2.0 ** -24             # fp32 unit round-off


# ------------------------------------------------------------------------------------------ shared pieces

def im2col(fmap, pad=None, tap_order: str = "yx") -> np.ndarray:
    """[256, 256, C] -> [65536, 9 C], column = tap * C + c with tap = ky * 3 + kx ("yx", the contract) or kx * 3 + ky ("xy", a
    modified model).  Outside the map: zeros (the contract), or the vector `pad` [C] (a modified model).  Keeps the dtype."""
    fmap = np.asarray(fmap)
    ch = fmap.shape[2]
    padded = np.zeros((RES + 2, RES + 2, ch), fmap.dtype)
    if pad is not None:
        padded[:] = np.asarray(pad).astype(fmap.dtype)
    padded[1:-1, 1:-1] = fmap
    cols = np.empty((RES, RES, 9, ch), fmap.dtype)
    for ky in range(3):
        for kx in range(3):
            cols[:, :, ky * 3 + kx if tap_order == "yx" else kx * 3 + ky] = padded[ky:ky + RES, kx:kx + RES]
    return cols.reshape(PIXELS, 9 * ch)


def conv_matrix(w, layout: str = "toi") -> np.ndarray:
    """[9][O][I] -> the GEMM's weight [O, 9 I], column = tap * I + i.  layout "tio": a modified model that reads the same buffer
    as [tap][in][out]."""
    w = np.asarray(w)
    _, o, i = w.shape
    if layout == "tio":
        w = w.reshape(9, i, o).transpose(0, 2, 1)
    else:
        assert layout == "toi", layout
    return np.ascontiguousarray(w.transpose(1, 0, 2).reshape(o, 9 * i))


def layernorm64(v, ln_w, ln_b, eps: float = EPS, unbiased: bool = False) -> np.ndarray:
    """float64 LayerNorm2d over the last axis: biased variance (the contract); unbiased: a modified model, / (n - 1)."""
    v = np.asarray(v, f64)
    d = v - v.mean(axis=-1, keepdims=True)
    var = (d * d).sum(axis=-1, keepdims=True) / (v.shape[-1] - (1 if unbiased else 0))
    return d / np.sqrt(var + eps) * np.asarray(ln_w, f64) + np.asarray(ln_b, f64)


def layernorm_f32(v32, ln_w, ln_b, eps: float = EPS) -> np.ndarray:
    """fp32 LayerNorm2d over the last axis, one fp32 operation each: sequential sum, mean, two-pass squares, rstd, scale, shift."""
    v = np.asarray(v32, f32)
    n = v.shape[-1]
    s = np.zeros(v.shape[:-1], f32)
    for c in range(n):
        s += v[..., c]
    d = v - (s / f32(n))[..., None]
    sq = np.zeros(v.shape[:-1], f32)
    for c in range(n):
        sq += d[..., c] * d[..., c]
    rstd = (f32(1) / np.sqrt(sq / f32(n) + f32(eps))).astype(f32)
    return d * rstd[..., None] * np.asarray(ln_w, f32) + np.asarray(ln_b, f32)


def dot_f32(v32, h32) -> np.ndarray:
    """fp32 sum_c v[..., c] * h[c], one product and one add at a time in channel order."""
    v, h = np.asarray(v32, f32), np.asarray(h32, f32)
    d = np.zeros(v.shape[:-1], f32)
    for c in range(v.shape[-1]):
        d += v[..., c] * h[c]
    return d


def _gelu_f32(v32, gelu: str) -> np.ndarray:
    return G.GELUS[gelu](np.asarray(v32, f32).astype(f64)).astype(f32)


# ------------------------------------------------------------------------------------------ hq_mask_path

def conv1(U16, p: dict, gelu: str = "erf", tap_order: str = "yx", unbiased: bool = False, rows=slice(None)) -> np.ndarray:
    """Stage 1 in float64 from the f16 U [256, 256, 32]: H [65536, 64] (or the pixels `rows` of it), not rounded."""
    v = G.product(im2col(np.asarray(U16, f16), tap_order=tap_order)[rows], conv_matrix(p["w1"])) + np.asarray(p["b1"], f64)
    return G.GELUS[gelu](layernorm64(v, p["ln_w"], p["ln_b"], p["eps"], unbiased))


def conv1_yardsticks(U16, p: dict, gelu: str = "erf", rows=slice(None)) -> Dict[str, np.ndarray]:
    """Stage 1 in fp32 [65536, 64] (or the pixels `rows` of it), before the rounding to f16."""
    cols, w = im2col(np.asarray(U16, f16))[rows], conv_matrix(p["w1"])
    return {name: _gelu_f32(layernorm_f32(acc(cols, w) + np.asarray(p["b1"], f32), p["ln_w"], p["ln_b"], p["eps"]), gelu)
            for name, acc in G.ACCUMULATIONS.items()}


def outside_value(p: dict) -> np.ndarray:
    """What the first convolution evaluates to where all of its taps read padding, f16 [64]: GELU(LN2d(b1)).  It is what a
    second convolution sees beyond the border when the padding of H is forgotten -- a modified model, the contract says zero."""
    return gelu64(layernorm64(np.asarray(p["b1"], f64)[None, :], p["ln_w"], p["ln_b"], p["eps"]))[0].astype(f16)


def conv2_plane(H16, p: dict, feat, hyper_hq, pad=None, tap_order: str = "yx", layout: str = "toi") -> np.ndarray:
    """Stage 2 in float64 from the f16 H [256, 256, 64] as delivered: the HQ plane [256, 256]."""
    v = G.product(im2col(np.asarray(H16, f16).reshape(RES, RES, C_H), pad, tap_order), conv_matrix(p["w2"], layout))
    v = v + np.asarray(p["b2"], f64) + np.asarray(feat, f64).reshape(PIXELS, C_OUT)
    return (v @ np.asarray(hyper_hq, f64)).reshape(RES, RES)


def conv2_yardsticks(H16, p: dict, feat, hyper_hq) -> Dict[str, np.ndarray]:
    """Stage 2 in fp32 [256, 256]: (acc + b2) + features per channel, then the product with hyper_hq in channel order."""
    cols, w = im2col(np.asarray(H16, f16).reshape(RES, RES, C_H)), conv_matrix(p["w2"])
    feat = np.asarray(feat, f32).reshape(PIXELS, C_OUT)
    return {name: dot_f32((acc(cols, w) + np.asarray(p["b2"], f32)) + feat, hyper_hq).reshape(RES, RES)
            for name, acc in G.ACCUMULATIONS.items()}


def add_plane(logits_in, plane, planes=(0, 1, 2, 3)) -> np.ndarray:
    """float64 [4, 256, 256]: logits_in with the HQ plane added to all four planes (the contract); `planes`: a modified model."""
    out = np.array(logits_in, f64)
    for m in planes:
        out[m] += np.asarray(plane, f64)
    return out


def seam_mask() -> np.ndarray:
    """The image border and both sides of every seam of the 16 x 16 tiles (tests/test_gpu_hq.py)."""
    edge = np.zeros((RES, RES), bool)
    edge[[0, RES - 1], :] = edge[:, [0, RES - 1]] = True
    edge[TILE - 1::TILE, :] = edge[TILE::TILE, :] = edge[:, TILE - 1::TILE] = edge[:, TILE::TILE] = True
    return edge


# ------------------------------------------------------------------------------------------ upscale_logits

def to_raster(u, exchanged: bool = False) -> np.ndarray:
    """[4096 tokens][4 s1][4 s2][C] -> [256, 256, C]: pixel (4 ty + 2 (s1 >> 1) + (s2 >> 1), 4 tx + 2 (s1 & 1) + (s2 & 1)).
    exchanged: a modified model with s1 and s2 in each other's place."""
    u = np.asarray(u)
    ch = u.shape[-1]
    u = u.reshape(64, 64, 2, 2, 2, 2, ch)                           # ty, tx, s1 >> 1, s1 & 1, s2 >> 1, s2 & 1, c
    order = (0, 4, 2, 1, 5, 3, 6) if exchanged else (0, 2, 4, 1, 3, 5, 6)
    return np.ascontiguousarray(u.transpose(order)).reshape(RES, RES, ch)


def upscale(keys16, q: dict, hyper, exchanged: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The whole chain in float64 for one prompt, keys [4096, 256] f16, hyper [4, 32]: (u [256, 256, 32], logits [4, 256, 256])."""
    up1 = (G.product(keys16, q["w1"]) + np.asarray(q["b1"], f64)).reshape(4096, 4, 64)
    a = gelu64(layernorm64(up1, q["ln_w"], q["ln_b"], q["eps"]))
    u = gelu64(a.reshape(4096 * 4, 64) @ np.asarray(q["w2"], f64).T + np.asarray(q["b2"], f64))
    u = to_raster(u.reshape(4096, 4, 4, 32), exchanged)
    return u, np.einsum("mc,yxc->myx", np.asarray(hyper, f64), u)


def upscale_yardsticks(keys16, q: dict, hyper, gelu: str = "fitted") -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
    """The chain in fp32, the intermediate rounded to f16: name -> (u fp32 [256, 256, 32] before its rounding, logits fp32)."""
    out = {}
    for name, acc in G.ACCUMULATIONS.items():
        up1 = (acc(keys16, q["w1"]) + np.asarray(q["b1"], f32)).reshape(4096, 4, 64)
        a = _gelu_f32(layernorm_f32(up1, q["ln_w"], q["ln_b"], q["eps"]), gelu).astype(f16)
        u = _gelu_f32(acc(a.reshape(4096 * 4, 64), q["w2"]) + np.asarray(q["b2"], f32), gelu)
        u = to_raster(u.reshape(4096, 4, 4, 32))
        out[name] = (u, np.stack([dot_f32(u, h) for h in np.asarray(hyper, f32)]))
    return out


def tie_bound(U16, hyper) -> np.ndarray:
    """[4, 256, 256]: how far logits[m] may be from sum_c hyper[m][c] * float(U[c]) when U is the f16 rounding of the values the
    product was taken with: sum_c |hyper[m][c]| times half an f16 spacing of U[c], plus ALLOW * 32 * 2^-24 * sum |hyper| |U| for
    the product's own fp32 roundings (32 products and adds)."""
    U, h = np.asarray(U16).astype(f64), np.abs(np.asarray(hyper, f64))
    return np.einsum("mc,yxc->myx", h, G.ulp16(U) / 2) + ALLOW * 32 * U1 * np.einsum("mc,yxc->myx", h, np.abs(U))


# ------------------------------------------------------------------------------------------ hq_features_finish

def finish(vit, emb, b_vit, b_emb, exchanged: bool = False) -> np.ndarray:
    """float64 [256, 256, 32]; exchanged: a modified model with the two sub-pixel levels in each other's place."""
    v = (np.asarray(vit, f64) + np.asarray(emb, f64)).reshape(4096, 4, 4, 32) + (np.asarray(b_vit, f64) + np.asarray(b_emb, f64))
    return to_raster(v, exchanged)


def finish_index_case():
    """Integers that encode their own place: vit[r, c] = 128 r + c, emb = twice that, b_vit[c] = c, b_emb[c] = 100 c.  Every sum
    of the four is an integer below 2^24, so every order of the three adds is exact in fp32."""
    idx = (np.arange(16384)[:, None] * 128 + np.arange(128)[None, :]).astype(f32)
    b_vit, b_emb = np.arange(32, dtype=f32), 100 * np.arange(32, dtype=f32)
    assert 3 * idx.max() + 101 * 31 < 2 ** 24
    return idx, 2 * idx, b_vit, b_emb


def finish_gaussian_case(seed: int):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((16384, 128)).astype(f32), rng.standard_normal((16384, 128)).astype(f32),
            rng.standard_normal(32).astype(f32), rng.standard_normal(32).astype(f32))


def finish_bound(vit, emb, b_vit, b_emb) -> np.ndarray:
    """[256, 256, 32]: three fp32 adds, each within 2^-24 of the magnitudes it sums: 3 * 2^-24 * (|vit| + |emb| + |b_vit| + |b_emb|)."""
    return 3 * U1 * finish(np.abs(vit), np.abs(emb), np.abs(b_vit), np.abs(b_emb))


# ------------------------------------------------------------------------------------------ inputs

SPIKE_PIXEL, SPIKE_CHANNEL = (137, 77), 5
FLAT_PIXEL = (88, 200)                  # centre of the 5 x 5 block of zeros of the flat case


def hq_params(seed: int, flat: bool = False) -> dict:
    """The six tensors of HqMaskWeights and eps.  The weights differ per tap: tap t carries its own scale 1 + t / 4 on top of the
    noise (neck_ref.conv3x3_weights).  flat: b1 is the constant 0.5, so that a pixel whose nine taps read zeros has 64 equal
    channels in front of the LayerNorm."""
    rng = np.random.default_rng(seed)
    scale = (1.0 + np.arange(9) / 4.0)[:, None, None]
    return {"w1": (rng.standard_normal((9, C_H, C_U)) / np.sqrt(9 * C_U) * scale).astype(f16),
            "b1": np.full(C_H, 0.5, f32) if flat else rng.normal(0, 0.3, C_H).astype(f32),
            "ln_w": rng.uniform(0.5, 1.5, C_H).astype(f32), "ln_b": rng.normal(0, 0.3, C_H).astype(f32),
            "w2": (rng.standard_normal((9, C_OUT, C_H)) / np.sqrt(9 * C_H) * scale).astype(f16),
            "b2": rng.normal(0, 0.3, C_OUT).astype(f32), "eps": EPS}


def weights_tuple(p: dict):
    return p["w1"], p["b1"], p["ln_w"], p["ln_b"], p["w2"], p["b2"]


def hq_inputs(seed: int, spike: bool = True, flat: bool = False):
    """U [256, 256, 32] f16, a GELU of Gaussians (non-negative on the whole, a non-zero mean per pixel); spike: channel
    SPIKE_CHANNEL of pixel SPIKE_PIXEL is 300 times the rms of the rest; flat: the 5 x 5 block around FLAT_PIXEL is zero.
    features [256, 256, 32] ~ N(0, 1) fp32, hyper_hq [32] ~ N(0, 1) fp32."""
    rng = np.random.default_rng(seed)
    U = gelu64(rng.standard_normal((RES, RES, C_U)))
    if spike:
        U[SPIKE_PIXEL][SPIKE_CHANNEL] = 300 * G.rms(np.delete(U[SPIKE_PIXEL], SPIKE_CHANNEL))
    if flat:
        y, x = FLAT_PIXEL
        U[y - 2:y + 3, x - 2:x + 3] = 0
    feat = rng.standard_normal((RES, RES, C_OUT)).astype(f32)
    return U.astype(f16), feat, rng.standard_normal(C_OUT).astype(f32)


def hq_input_conditions(U16, p: dict, flat: bool = False, spike: bool = True) -> None:
    """What hq_inputs promises, and that every pixel away from the flat block has a conv1 variance above 1e4 * eps."""
    U = np.asarray(U16, f64)
    assert (U >= -0.17).all() and (U.mean(axis=2) > 0).mean() > 0.999, "U is a GELU: bounded below, a positive mean per pixel"
    if spike:
        rest = np.delete(U[SPIKE_PIXEL], SPIKE_CHANNEL)
        assert U[SPIKE_PIXEL][SPIKE_CHANNEL] >= 250 * G.rms(rest)
    v = G.product(im2col(np.asarray(U16, f16)), conv_matrix(p["w1"])) + np.asarray(p["b1"], f64)
    var = v.var(axis=1).reshape(RES, RES)
    away = np.ones((RES, RES), bool)
    if flat:
        y, x = FLAT_PIXEL
        assert not U[y - 2:y + 3, x - 2:x + 3].any()
        away[y - 1:y + 2, x - 1:x + 2] = False
        assert (var[~away] == 0).all(), "the flat pixels' 64 channels are equal"
    assert var[away].min() > 1e4 * p["eps"], var[away].min()


PROBES = [(0, 0), (0, 255), (255, 0), (255, 255),         # corners
          (0, 100), (255, 101), (102, 0), (103, 255),     # edges
          (100, 180),                                     # interior
          (40, 15), (40, 16), (15, 200), (16, 200)]       # both sides of a tile seam, in x and in y
PROBE_HEIGHT, PROBE_NOISE = 8.0, 0.05


def probe_inputs(seed: int):
    """U [256, 256, 32] f16: noise of sigma 0.05 plus an impulse of height 8 at each PROBES pixel, in a channel of its own: every
    pixel within one step of a probe sees its impulse through exactly one tap of the first convolution."""
    rng = np.random.default_rng(seed)
    U = rng.normal(0, PROBE_NOISE, (RES, RES, C_U))
    assert len(PROBES) <= C_U
    for i, (y, x) in enumerate(PROBES):
        U[y, x, i] += PROBE_HEIGHT
    feat = rng.standard_normal((RES, RES, C_OUT)).astype(f32)
    return U.astype(f16), feat, rng.standard_normal(C_OUT).astype(f32)


def probe_neighbourhood() -> np.ndarray:
    """bool [256, 256]: every PROBES pixel and its up to 8 neighbours inside the image."""
    m = np.zeros((RES, RES), bool)
    for y, x in PROBES:
        m[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    return m


def probe_bounds(U16, H16, p: dict, feat, hyper_hq) -> Tuple[float, float]:
    """Absolute bounds for H and for the plane over the probe neighbourhoods, from the operands alone (not from any result but
    the delivered H that stage 2 reads):

      H      conv1's fp32 sum of K = 288 products is within K u S1 of the exact one, S1 = sum |U| |W1| of the pixel and
             channel (u = 2^-24); adding the bias and taking the statistics of 64 values adds at most (64 + 4) u of the
             largest |v|, which K u S1 covers twice over, hence the factor 3; the LayerNorm divides by the pixel's sigma and
             multiplies by ln_w, GELU's slope is at most 1.13; and the result is rounded to f16, half a spacing at the largest
             |H| a LayerNorm of 64 values can give, sqrt(63) max ln_w + max |ln_b|.
      plane  conv2's sum of K = 576 products is within K u S2 of the exact one, S2 = sum |H| |W2|; bias, features and the 32
             products with hyper_hq add (32 + 2) u sum_c |hyper_c| (S2_c + |b2_c| + |feat_c|).
    """
    nb = probe_neighbourhood().reshape(-1)
    cols = np.abs(im2col(np.asarray(U16, f16)).astype(f64))[nb]
    s1 = cols @ np.abs(conv_matrix(p["w1"]).astype(f64)).T
    v = G.product(im2col(np.asarray(U16, f16))[nb], conv_matrix(p["w1"])) + np.asarray(p["b1"], f64)
    sigma = v.std(axis=1)
    h_max = np.sqrt(63.0) * float(np.max(np.abs(p["ln_w"]))) + float(np.max(np.abs(p["ln_b"])))
    bound_h = 1.13 * float(np.max(np.abs(p["ln_w"]))) * 3 * 288 * U1 * float((s1.max(axis=1) / sigma).max()) + float(G.ulp16(h_max)) / 2
    cols2 = np.abs(im2col(np.asarray(H16, f16).reshape(RES, RES, C_H)).astype(f64))[nb]
    s2 = cols2 @ np.abs(conv_matrix(p["w2"]).astype(f64)).T + np.abs(np.asarray(p["b2"], f64)) + np.abs(np.asarray(feat, f64)).reshape(PIXELS, C_OUT)[nb]
    bound_plane = (576 + 34) * U1 * float((s2 @ np.abs(np.asarray(hyper_hq, f64))).max())
    return bound_h, bound_plane


def upscale_params(seed: int) -> dict:
    rng = np.random.default_rng(seed)
    return {"w1": (rng.standard_normal((256, 256)) / 16).astype(f16), "b1": rng.normal(0, 0.3, 256).astype(f32),
            "ln_w": rng.uniform(0.5, 1.5, 64).astype(f32), "ln_b": rng.normal(0, 0.3, 64).astype(f32),
            "w2": (rng.standard_normal((128, 64)) / 8).astype(f16), "b2": rng.normal(0, 0.3, 128).astype(f32), "eps": EPS}


def upscale_inputs(seed: int, P: int):
    """keys [P * 4096, 256] f16 ~ N(0, 1) (the decoder's keys are LayerNorm'ed), hyper [P, 4, 32] ~ N(0, 1), different per prompt."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((P * 4096, 256)).astype(f16), rng.standard_normal((P, 4, 32)).astype(f32)


def upscale_args(q: dict):
    return q["w1"], q["b1"], q["ln_w"], q["ln_b"], q["eps"], q["w2"], q["b2"]
