"""Float64 reference of the encoder CHAIN in the configuration the product runs: the f16-pair residual stream (xn_ + xlo_),
LayerNorms folded into the qkv and fc1 GEMMs, row statistics handed from each stream writer to the next consumer, and the
load-time fold of sam_weights.cpp.  Shared by tests/test_encoder_ref.py (CPU) and tests/test_gpu_encoder.py (GPU).  No test
functions here.

Written from the contracts in kernels.hpp; composes gemm_ref, attention_ref and neck_ref.  Every stage is computed from the
DEVICE'S OWN operands of that stage (teacher forcing), so a stage's tolerance stays in the rounding units of its own launch
instead of growing along the chain:

  S0  stream 0  = patches . Wp^T + bp + pos_embed                                        pair result
  S1  qkv_j     = consumer(stream hi, folded qkv operands; moments of hi + lo)           f16 result
  S2  x_mid_j   = stream + f16(attention(qkv_j)) . Wproj^T + bproj                       pair result
  S3  hidden_j  = gelu(consumer(x_mid hi, folded fc1 operands; moments of hi + lo))      f16 result
  S4  stream_j  = x_mid + hidden_j . Wfc2^T + bfc2, and its row statistics (bn = 256)    pair result
  S5  embedding = neck(final stream hi)                                                  fp32 result

A stage returns MEASURES (name, value, bound): value <= bound is what a correct kernel needs.  Every bound is measured on
reference-side yardsticks on the same inputs (gemm_ref's two accumulation models, attention_ref's rounding model, an fp32
LayerNorm), never on a device.  hold() asserts and logs them; worst() is what the CPU file's stand-ins are measured with.
The k-sequential yardsticks run on a subset of rows (yardstick_rows); the comparison itself always covers the whole tensor.

fold64 / loader_model restate the loader's arithmetic (the only place it is held to anything); emulate() runs the whole chain
from the patches, rounding where the product rounds, in float64 or float32.
"""
import math
from typing import Dict, List, Optional, Tuple

import numpy as np

import attention_ref as A
import gemm_ref as G
import neck_ref as N

f16, f32, f64 = np.float16, np.float32, np.float64

TOKENS = 4096
PATCH_K = 768
Measure = Tuple[str, float, float]


def q_scale(hd: int) -> float:
    """k::attention_global_q_scale: log2(e) / sqrt(hd), evaluated in fp32."""
    return float(f32(1.44269504088896341) / np.sqrt(f32(hd)))


def rel_scale(hd: int) -> float:
    return float(np.sqrt(f32(hd)))


def pair(v) -> Tuple[np.ndarray, np.ndarray]:
    """(hi, lo) of the f16-pair stream, float64 arrays holding f16 values."""
    v = np.asarray(v, f64)
    hi = G.round_f16(v)
    return hi, G.round_f16(v - hi)


def delivered(yardsticks: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """fp32 yardsticks of a stream writer as the stream delivers them: split into the pair, like the kernel's fp32 result (on
    the massive channels of trained-like weights that last rounding is the largest error of all)."""
    return {name: G.output_model(y, "pair") for name, y in yardsticks.items()}


# ------------------------------------------------------------------------------------------ measures

def hold(measures: List[Measure]) -> None:
    """Every measure logged through conftest.within (bounds are inclusive, hence the nextafter), then asserted together."""
    from conftest import within
    failed = []
    for name, value, bound in measures:
        try:
            within(name, value, np.nextafter(bound, np.inf))
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)


def worst(measures: List[Measure]) -> float:
    """The largest value / bound: what a stand-in must push to 3 or more."""
    return max((v / b if b > 0 else (np.inf if v > 0 else 0.0)) for _, v, b in measures)


def units(name: str, got, ref, model, yardsticks: Dict[str, np.ndarray], rows, margin_rms: float, margin_max: float) -> List[Measure]:
    """got (whole tensor) against ref in units of the rounding model's error, bounded by margin x the larger yardstick's units;
    the yardsticks cover `rows` only and are measured in the units of those rows.  Yardstick ratios are logged."""
    from conftest import within
    got = np.asarray(got, f64)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    g = G.ratios(got, ref, model)
    bound = {"rms": 0.0, "max": 0.0}
    for yname, y in yardsticks.items():
        r = G.ratios(y, ref[rows], model[rows])
        within(f"{name} {yname} rms/model", r["rms"], np.inf)
        within(f"{name} {yname} max/model", r["max"], np.inf)
        bound = {k: max(bound[k], r[k]) for k in bound}
    return [(name + " rms/model", g["rms"], margin_rms * bound["rms"]), (name + " max/model", g["max"], margin_max * bound["max"])]


def f16_units(name: str, got16, ref, yardsticks: Dict[str, np.ndarray], rows, extra=0.0) -> List[Measure]:
    """gemm_ref.check_f16's measure with yardsticks on `rows`: the largest |got - ref| / f16_bound over the whole tensor.
    extra: an element-wise allowance on top (consumer_stage: operands that are not observable)."""
    ref = np.asarray(ref, f64)
    assert np.abs(ref).max() < G.F16_LIMIT, f"{name}: the reference leaves the f16 range"
    got = np.asarray(got16, f64)
    assert got.shape == ref.shape and np.isfinite(got).all(), f"{name}: shape or non-finite output"
    slack = max(float(np.abs(np.asarray(y, f64) - ref[rows]).max()) for y in yardsticks.values())
    # (the spacing is taken at |ref| + extra: where the operand itself is uncertain by extra, so is the magnitude that is rounded)
    bound = G.ulp16(np.abs(ref) + extra) / 2 * (1 + 2.0 ** -10) + G.ALLOW * slack + extra
    return [(name + " f16 err/bound", float((np.abs(got - ref) / bound).max()), 1.0)]


def yardstick_rows(count: int, patches=None) -> np.ndarray:
    """The rows the k-sequential yardsticks run on: 0, 63, 64, 255, 256, 4095, one row of every window of index 4 on either
    axis (the padded ones), the zero-patch rows of grid rows that hold nothing else (first and last such grid row), and evenly
    spread rows up to `count` (>= 512)."""
    assert count >= 512
    rows = {0, 63, 64, 255, 256, 4095}
    for w in range(A.NW):
        rows.add((4 * A.WS + 3) * A.GRID + min(w * A.WS + 5, A.GRID - 1))
        rows.add(min(w * A.WS + 5, A.GRID - 1) * A.GRID + 4 * A.WS + 3)
    if patches is not None:
        zero = np.nonzero(~np.asarray(patches).reshape(TOKENS, -1).any(axis=1))[0]
        grid_rows = sorted({int(z) // A.GRID for z in zero if np.isin(np.arange(A.GRID) + (int(z) // A.GRID) * A.GRID, zero).all()})
        for gy in grid_rows[:1] + grid_rows[-1:]:
            rows.update(range(gy * A.GRID, (gy + 1) * A.GRID))
    i = 0
    while len(rows) < count:
        rows.add((i * 1237 + 11) % TOKENS)          # 1237 is prime: every residue modulo the tile heights
        i += 1
    return np.array(sorted(rows))


# ------------------------------------------------------------------------------------------ the loader's fold

FOLD_VARIANTS = ("no_beta", "tables_unscaled", "q_bias_unscaled", "k_scaled", "pad_zero")


def fold64(params, cfg, layer: int, variant: Optional[str] = None) -> Dict[str, np.ndarray]:
    """Block `layer`'s operands from the raw parameters in float64, before any rounding: w = W diag(gamma), b = b + W beta, the q
    rows (weight and bias) of a global block times log2(e) / sqrt(hd) and its tables times sqrt(hd); windowed blocks: the
    padding token's q|k|v = the plain qkv bias.  `variant` names a MODIFIED fold (tests/test_encoder_ref.py)."""
    assert variant is None or variant in FOLD_VARIANTS, variant
    p = lambda n: np.asarray(params[f"enc.L{layer}.{n}"], f64)
    D, hd = cfg.embed_dim, cfg.head_dim
    is_global = layer in cfg.global_attn_indexes
    rs = np.ones(3 * D)
    if is_global:
        rs[:D] = q_scale(hd)
        if variant == "k_scaled":
            rs[D:2 * D] = q_scale(hd)
    shift = 0.0 if variant == "no_beta" else p("qkv.w") @ p("ln1.b")
    rs_b = rs.copy()
    if variant == "q_bias_unscaled":
        rs_b[:D] = 1.0
    ts = rel_scale(hd) if is_global and variant != "tables_unscaled" else 1.0
    out = {"qkv.w": rs[:, None] * p("qkv.w") * p("ln1.w")[None, :], "qkv.b": rs_b * p("qkv.b") + rs * shift,
           "fc1.w": p("fc1.w") * p("ln2.w")[None, :], "fc1.b": p("fc1.b") + p("fc1.w") @ p("ln2.b"),
           "proj.w": p("proj.w"), "proj.b": p("proj.b"), "fc2.w": p("fc2.w"), "fc2.b": p("fc2.b"),
           "rel_h16": p("rel_h") * ts, "rel_w16": p("rel_w") * ts, "global": np.array([float(is_global)])}
    out["qkv_pad"] = np.zeros(0) if is_global else (np.zeros(3 * D) if variant == "pad_zero" else p("qkv.b"))
    return out


def loader_model(folded: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """fold64's values as the device holds them: weights, tables and the padding token f16, biases fp32, colsum the fp32 sum of
    the f16-ROUNDED scaled weight."""
    out = {}
    for name, v in folded.items():
        if name.endswith(".w") or name in ("rel_h16", "rel_w16", "qkv_pad"):
            out[name] = G.round_f16(v)
        elif name.endswith(".b"):
            out[name] = G.round_f32(v)
        else:
            out[name] = v
    for lin in ("qkv", "fc1"):
        out[lin + ".colsum"] = G.round_f32(out[lin + ".w"].sum(axis=1))
    return out


def outer_model(params) -> Dict[str, np.ndarray]:
    """Layer -1 as the device holds it: patch embed, pos_embed and the neck (3x3 weight tap-major: column = (ky 3 + kx) 256 + c)."""
    p = lambda n: np.asarray(params[n], f64)
    w2 = p("enc.neck.conv2.w")
    return {"patch.w": G.round_f16(p("enc.patch.w")), "patch.b": p("enc.patch.b"), "pos_embed": p("enc.pos"),
            "neck1.w": G.round_f16(p("enc.neck.conv1.w")), "neck_ln1.w": p("enc.neck.ln1.w"), "neck_ln1.b": p("enc.neck.ln1.b"),
            "neck2.w": G.round_f16(w2.transpose(0, 2, 3, 1).reshape(w2.shape[0], -1)),
            "neck_ln2.w": p("enc.neck.ln2.w"), "neck_ln2.b": p("enc.neck.ln2.b")}


def shape_operands(flat: Dict[str, np.ndarray], cfg, layer: int) -> Dict[str, np.ndarray]:
    """The hook's flat float32 arrays -> float64 arrays of the operands' shapes."""
    D, mlp, hd = cfg.embed_dim, cfg.mlp_dim, cfg.head_dim
    shapes = {"patch.w": (D, PATCH_K), "pos_embed": (TOKENS, D), "neck1.w": (256, D), "neck2.w": (256, 2304),
              "qkv.w": (3 * D, D), "fc1.w": (mlp, D), "proj.w": (D, D), "fc2.w": (D, mlp), "rel_h16": (-1, hd), "rel_w16": (-1, hd)}
    return {n: np.asarray(v, f64).reshape(shapes.get(n, (-1,))) for n, v in flat.items()}


def spacing32(x) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(x, f64)).astype(f32)).astype(f64)


def fold_measures(name: str, dev: Dict[str, np.ndarray], params, cfg, layer: int) -> List[Measure]:
    """The device's folded operands of block `layer` against the float64 fold of the raw parameters: f16 operands within half an
    f16 spacing at the float64 value times (1 + 2^-10), fp32 ones within one fp32 spacing, colsum against the float64 sum of
    the device's OWN f16 weight, what is only converted (proj, fc2, the padding token) exactly its rounded value."""
    want = fold64(params, cfg, layer)
    out: List[Measure] = []
    for n in ("qkv.w", "fc1.w", "rel_h16", "rel_w16"):
        out.append((f"{name} {n} / half f16 spacing", float((np.abs(dev[n] - want[n]) / (G.ulp16(want[n]) / 2 * (1 + 2.0 ** -10))).max()), 1.0))
    for n in ("qkv.b", "fc1.b"):
        out.append((f"{name} {n} / fp32 spacing", float((np.abs(dev[n] - want[n]) / spacing32(want[n])).max()), 1.0))
    for lin in ("qkv", "fc1"):
        s = dev[lin + ".w"].sum(axis=1)
        out.append((f"{name} {lin}.colsum / fp32 spacing", float((np.abs(dev[lin + ".colsum"] - s) / spacing32(s)).max()), 1.0))
    exact = loader_model(want)
    for n in ("proj.w", "proj.b", "fc2.w", "fc2.b", "qkv_pad", "global"):
        assert dev[n].shape == exact[n].shape, (n, dev[n].shape, exact[n].shape)
        out.append((f"{name} {n} differing elements", float((dev[n] != exact[n]).sum()), 0.0))
    return out


def outer_measures(name: str, dev: Dict[str, np.ndarray], params) -> List[Measure]:
    exact = outer_model(params)
    return [(f"{name} {n} differing elements", float((dev[n] != exact[n]).sum()), 0.0) for n in exact]


# ------------------------------------------------------------------------------------------ stages

def stage0(name: str, got_pair, patches16, outer, rows) -> List[Measure]:
    ref = G.plain(patches16, outer["patch.w"], outer["patch.b"], outer["pos_embed"])
    yard = delivered(G.plain_yardsticks(patches16[rows], outer["patch.w"], outer["patch.b"], outer["pos_embed"][rows]))
    return units(name, got_pair[0] + got_pair[1], ref, G.output_model(ref, "pair"), yard, rows, G.ALLOW, G.ALLOW)


def resplit_ties(stream_pair) -> np.ndarray:
    """Where a pair read from a TWIN may differ from the pair the untouched model's consumer read.  A writer splits its fp32
    result v into hi = f16(v), lo = f16(v - hi); when v lies within 2^-11 of half a spacing from a midpoint, lo rounds to exactly
    half the spacing and hi + lo IS the midpoint.  The twin's last writer adds nothing to that value and splits it again:
    hi' = f16(midpoint) is the EVEN neighbour, which is the other one in half of these cases (about one element in 5000).
    The value is the same; the A operand of the next consumer is not, and cannot be observed.  Returns |hi' - other candidate|
    (= 2 |lo|) at those elements, 0 elsewhere."""
    hi, lo = stream_pair
    other = hi + 2 * lo
    return np.where((lo != 0) & (G.round_f16(other) == other), np.abs(2 * lo), 0.0)


def consumer_stage(name: str, got16, stream_pair, ops, lin: str, act: int, rows, resplit: bool = False) -> List[Measure]:
    """S1 (lin "qkv", act 0) and S3 (lin "fc1", act 1): the folded consumer of the stream hi with the moments of hi + lo, the
    device's weight, bias and colsum as passed.  Yardsticks of a GELU launch evaluate the fitted form (gemm_ref, note 2).
    resplit: the pair comes from a twin (resplit_ties): an element's allowance grows by what the unobservable choice of hi can
    move it, rstd_m sum_k |dA[m, k]| |W[n, k]| (times 1.13, the largest slope of GELU); the moments are those of the value and
    do not depend on it."""
    hi, lo = stream_pair
    x = hi + lo
    # the fp32 error of a row grows with rstd_m sum_k |A[m, k]|: the yardsticks also cover the 32 rows where that is largest
    rows = np.union1d(rows, np.argsort(G.row_moments(x)[1] * np.abs(hi).sum(axis=1))[-32:])
    extra = 0.0
    if resplit:
        extra = G.row_moments(x)[1][:, None] * (resplit_ties(stream_pair) @ np.abs(ops[lin + ".w"]).T) * (1.13 if act else 1.0)
    ref = G.consumer(hi, ops[lin + ".w"], ops[lin + ".colsum"], ops[lin + ".b"], x, act=act)
    yard = G.consumer_yardsticks(hi[rows], ops[lin + ".w"], ops[lin + ".colsum"], ops[lin + ".b"], x[rows], act=act,
                                 gelu="fitted" if act else "erf")
    if resplit:
        # how much of the tensor is checked at the plain bound, and how large the allowance is where it applies
        from conftest import within
        base = G.ulp16(ref) / 2 * (1 + 2.0 ** -10)
        within(name + " rows with a re-split tie / rows", float((resplit_ties(stream_pair) > 0).any(axis=1).mean()), np.inf)
        within(name + " elements with a re-split allowance above a tenth of half an f16 spacing / elements",
               float((extra > 0.1 * base).mean()), np.inf)
        within(name + " largest re-split allowance / half an f16 spacing", float((extra / base).max()), np.inf)
    return f16_units(name, got16, ref, yard, rows, extra)


def attention64(qkv16, ops, cfg, rows=None, want_model: bool = False, ft=f64) -> np.ndarray:
    """[4096, D] float64 attention of one image from the device's qkv (f16) and tables, all heads; the global block's operands
    arrive pre-scaled (its scores are q'.k + q'.R'h + q'.R'w in units of log2), the windowed block's padding tokens carry
    qkv_pad.  want_model: attention_ref's rounding model instead (global blocks: on `rows` only; windowed: every row).
    ft float32: the scores rounded to fp32 (the float32 evaluation of emulate())."""
    scores = (lambda S: S) if ft is f64 else (lambda S: S.astype(f32).astype(f64))
    D, H, hd = cfg.embed_dim, cfg.num_heads, cfg.head_dim
    is_global = bool(ops["global"][0])
    out = np.empty((TOKENS if (rows is None or not is_global) else len(rows), D), f64)
    if is_global:
        q = np.asarray(qkv16, f64).reshape(TOKENS, 3, H, hd)
        for h in range(H):
            gops = {"q": q[None, None, :, 0, h], "k": q[None, None, :, 1, h], "v": q[None, None, :, 2, h],
                    "rh": ops["rel_h16"], "rw": ops["rel_w16"]}
            S = scores(A.global_scores(gops, 0, 0, rows))
            V = gops["v"][0, 0]
            out[:, h * hd:(h + 1) * hd] = A.rounding_model(S, V, A.GLOBAL_TILE) if want_model else A.softmax2(S, V)
        return out
    wops = A.window_operands(np.asarray(qkv16).astype(f16), np.asarray(ops["qkv_pad"], f32),
                             ops["rel_h16"], ops["rel_w16"], 1, H, hd)
    for h in range(H):
        S, V = scores(A.window_scores(wops, 0, h)), wops["v"][0, h]
        fn = (lambda s, v: A.rounding_model(s, v, A.WINDOW_TILE)) if want_model else A.softmax2
        out[:, h * hd:(h + 1) * hd] = A.window_apply(S, V, fn)
    return out if rows is None or not want_model else out[rows]


def stage2(name: str, got_pair, qkv16, stream_pair, ops, cfg, rows) -> List[Measure]:
    """x_mid: float64 attention over all heads and queries rounded once to f16, through proj in float64, plus the residual.
    Yardsticks: attention_ref's rounding model, then gemm_ref's two accumulations for proj; the margins are the attention
    kernels' own (attention_ref.RMS_MARGIN / MAX_MARGIN), since the stage contains them."""
    resid = stream_pair[0] + stream_pair[1]
    att = G.round_f16(attention64(qkv16, ops, cfg))
    ref = G.plain(att, ops["proj.w"], ops["proj.b"], resid)
    att_model = attention64(qkv16, ops, cfg, rows, want_model=True)
    yard = delivered(G.plain_yardsticks(att_model, ops["proj.w"], ops["proj.b"], resid[rows]))
    return units(name, got_pair[0] + got_pair[1], ref, G.output_model(ref, "pair"), yard, rows, A.RMS_MARGIN, A.MAX_MARGIN)


def stage4(name: str, got_pair, hidden16, mid_pair, ops, rows) -> List[Measure]:
    resid = mid_pair[0] + mid_pair[1]
    ref = G.plain(hidden16, ops["fc2.w"], ops["fc2.b"], resid)
    yard = delivered(G.plain_yardsticks(np.asarray(hidden16)[rows], ops["fc2.w"], ops["fc2.b"], resid[rows]))
    return units(name, got_pair[0] + got_pair[1], ref, G.output_model(ref, "pair"), yard, rows, G.ALLOW, G.ALLOW)


def layernorm_f32(v32, gamma, beta, eps: float = N.EPS) -> np.ndarray:
    """fp32 yardstick of LayerNorm2d: sequential sums, two-pass variance, one fp32 operation each."""
    v = np.asarray(v32, f32)
    n = v.shape[1]
    s = np.zeros(v.shape[0], f32)
    for c in range(n):
        s += v[:, c]
    d = v - (s / f32(n))[:, None]
    m2 = np.zeros(v.shape[0], f32)
    for c in range(n):
        m2 += d[:, c] * d[:, c]
    rstd = (f32(1) / np.sqrt(m2 / f32(n) + f32(eps))).astype(f32)
    return d * rstd[:, None] * np.asarray(gamma, f32) + np.asarray(beta, f32)


def neck64(hi16, outer, **variant) -> np.ndarray:
    return N.neck(hi16, outer["neck1.w"], outer["neck_ln1.w"], outer["neck_ln1.b"], outer["neck2.w"], outer["neck_ln2.w"],
                  outer["neck_ln2.b"], **variant)


def stage5(name: str, got32, hi16, outer, rows) -> List[Measure]:
    """The embedding from the final stream hi: neck_ref's chained reference (the map rounded to f16 between the launches)
    against fp32 yardsticks of both launches -- chain accumulation, fp32 LayerNorm; the 3x3 one on `rows`."""
    ref = neck64(hi16, outer)
    yard = {}
    for acc_name, acc in G.ACCUMULATIONS.items():
        fmap = layernorm_f32(acc(hi16, outer["neck1.w"]), outer["neck_ln1.w"], outer["neck_ln1.b"]).astype(f16)
        cols = N.im2col3x3(fmap.reshape(1, N.GRID, N.GRID, N.C))[rows]
        yard[acc_name] = layernorm_f32(acc(cols, outer["neck2.w"]), outer["neck_ln2.w"], outer["neck_ln2.b"])
    return units(name, got32, ref, N.output_model(ref, "f32"), yard, rows, N.ALLOW, N.ALLOW)


def structure_measures(name: str, taps, cfg) -> List[Measure]:
    """Exact: hi is a nearest f16 of hi + lo everywhere (== f16(hi + lo) but at exact midpoints, which a writer reaches when lo
    rounds to half a spacing: there hi is the neighbour its fp32 value was nearer to), the pair stream in use with D / 256
    statistics groups, no overflow report."""
    hi, lo = np.asarray(taps["stream_hi"], f64), np.asarray(taps["stream_lo"], f64)
    nearest = G.round_f16(hi + lo)
    return [(name + " hi not a nearest f16 of hi + lo", float((np.abs(lo) > np.abs(hi + lo - nearest)).sum()), 0.0),
            (name + " split stream missing", 1.0 - float(taps["split"][0]), 0.0),
            (name + " groups off D / 256", abs(float(taps["groups"][0]) - cfg.embed_dim // 256), 0.0),
            (name + " non-finite flag", float(taps["nonfinite"][0]), 0.0)]


# ------------------------------------------------------------------------------------------ free-running emulation

def patches_from_image(img: np.ndarray) -> np.ndarray:
    """k::preprocess: u8 [h][w][>= 3] -> f16 [4096][768], row = patch, column = c 256 + iy 16 + ix, (u8 - mean) / std in fp32,
    zero outside the image."""
    from dlimgedit_amd.sam_config import PIXEL_MEAN, PIXEL_STD
    h, w = img.shape[:2]
    full = np.zeros((1024, 1024, 3), f32)
    full[:h, :w] = (img[:, :, :3].astype(f32) - np.array(PIXEL_MEAN, f32)) / np.array(PIXEL_STD, f32)
    return full.reshape(64, 16, 64, 16, 3).transpose(0, 2, 4, 1, 3).reshape(TOKENS, PATCH_K).astype(f16)


EMULATION_VARIANTS = ("writer_hi_only", "proj_resid_hi_only", "stats_from_f16", "gelu_tanh", "neck_tap_order")


def emulate(patches16, outer, layers: List[Dict[str, np.ndarray]], cfg, ft=f64, variant: Optional[str] = None,
            at: Optional[int] = None, start=None) -> Dict[str, object]:
    """The whole chain from the patches, rounding where the product rounds (pair stream, f16 qkv / attention / hidden / map),
    every other operation in `ft` (float64, or float32 for the distance between the two).  Returns per block the taps the
    staged checks take ("stream_in", "qkv", "x_mid", "hidden", "stream_out", all pairs as (hi, lo)) and the embedding.
    variant: a MODIFIED chain (tests/test_encoder_ref.py) applied at block `at`.  start = (block, stream pair): resume there."""
    assert variant is None or variant in EMULATION_VARIANTS, variant
    c = lambda a: np.asarray(a, ft)
    split = lambda v: tuple(c(p) for p in pair(v))
    blocks = []
    if start is None:
        first, stream = 0, split(c(patches16) @ c(outer["patch.w"]).T + c(outer["patch.b"]) + c(outer["pos_embed"]))
    else:
        first, stream = start
    for j in range(first, len(layers)):
        L = layers[j]
        here = variant if at == j else None

        def consume(sp, lin, act):
            x = sp[0] if here == "stats_from_f16" else sp[0] + sp[1]
            mean = x.mean(axis=1, dtype=ft)
            rstd = 1 / np.sqrt(((x - mean[:, None]) ** 2).mean(axis=1, dtype=ft) + ft(G.EPS))
            v = rstd[:, None] * (sp[0] @ c(L[lin + ".w"]).T - mean[:, None] * c(L[lin + ".colsum"])[None, :]) + c(L[lin + ".b"])
            if act:
                v = c((G.gelu_tanh if here == "gelu_tanh" else G.gelu64)(v))
            return G.round_f16(v)

        taps = {"stream_in": stream, "qkv": consume(stream, "qkv", 0)}
        att = G.round_f16(attention64(taps["qkv"], L, cfg, ft=ft))
        resid = stream[0] if here == "proj_resid_hi_only" else stream[0] + stream[1]
        taps["x_mid"] = split(c(att) @ c(L["proj.w"]).T + c(L["proj.b"]) + resid)
        taps["hidden"] = consume(taps["x_mid"], "fc1", 1)
        v = c(taps["hidden"]) @ c(L["fc2.w"]).T + c(L["fc2.b"]) + taps["x_mid"][0] + taps["x_mid"][1]
        stream = split(v)
        if here == "writer_hi_only":
            stream = (stream[0], np.zeros_like(stream[1]))
        taps["stream_out"] = stream
        blocks.append(taps)
    if ft is f64:
        emb = neck64(stream[0], outer, **({"tap_order": "xy"} if variant == "neck_tap_order" else {}))
    else:
        fmap = layernorm_f32(c(stream[0]) @ c(outer["neck1.w"]).T, outer["neck_ln1.w"], outer["neck_ln1.b"]).astype(f16)
        cols = N.im2col3x3(fmap.reshape(1, N.GRID, N.GRID, N.C))
        emb = layernorm_f32(c(cols) @ c(outer["neck2.w"]).T, outer["neck_ln2.w"], outer["neck_ln2.b"])
    return {"blocks": blocks, "first": first, "embedding": np.asarray(emb, f64)}
