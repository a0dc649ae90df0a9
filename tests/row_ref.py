"""Float64 reference, fp32 yardsticks and input builders for the row kernels of kernels/elementwise.hip alone (kernels.hpp:
k::layernorm, k::add_cast, k::cast_f16, k::im2col3x3), shared by tests/test_row_ref.py (CPU) and tests/test_gpu_row_kernels.py
(GPU).  No test functions here.

Written from the launch's CONTRACT (kernels.hpp), not from the kernels:

  * layernorm   y[r, c] = act((x[r, c] - mean_r) / sqrt(var_r + eps) * w[c] + b[c]), mean and the BIASED variance over the D
                columns of row r of the fp32 input; act: none or the erf-form GELU; out_f32 and / or out_h = f16(y)

Measure and allowance are gemm_ref's.  The REFERENCE takes the fp32 input and does everything else in float64; errors count in
units of the reference rounded once to the output's format; a kernel may need ALLOW = 1.25 times what the LARGER of two numpy
fp32 yardsticks needs on the same inputs.  The contract does not say in which order a row is summed, so the two yardsticks differ
in exactly that, and do everything else once per operation in fp32, in the order the contract writes it:

  * sequential  both sums (of x, and of the squared deviations from the mean: two passes) one column at a time
                (encoder_ref.layernorm_f32)
  * tree        both sums as 64 partial sums of stride 64 (partial l takes the columns l, l + 64, ...; short rows pad with
                zeros), the 64 partials then added as a binary tree: the order of a reduction over the 64 lanes of a wave

The GELU of these two is the erf form evaluated once and rounded once to fp32 (gemm_ref._gelu_f32).  A launch with GELU gets a
third yardstick, written down before any kernel was measured against it:

  * steps       the sequential LayerNorm, then the GELU as its formula is written, 0.5 x (1 + erf(x / sqrt 2)), one fp32
                operation each with a correctly rounded erf.  For x < 0 the sum 1 + erf cancels, so ANY fp32 evaluation of the
                formula carries up to |x| 2^-25 of absolute error where the result itself is far smaller: the single rounding of
                the other two hides that, and where the LayerNorm has no error of its own (D = 1, constant rows: y = b exactly)
                nothing else would cover it
"""
from typing import Dict, Optional

import numpy as np

import gemm_ref as G
from encoder_ref import layernorm_f32 as layernorm_sequential_f32
from gemm_ref import ALLOW, check, check_f16, gelu64, gelu_tanh, round_f32  # noqa: F401

f16, f32, f64 = np.float16, np.float32, np.float64

EPS = 1e-6
LANES = 64
MAX_D = 1280                # the launcher's longest row


# ------------------------------------------------------------------------------------------ reference (float64)

def layernorm64(x32, w, b, eps: float = EPS, act: int = 0, unbiased: bool = False, gelu: str = "erf") -> np.ndarray:
    """The contract in float64 from the fp32 input.  Modified models: unbiased (/ (D - 1); D = 1 keeps / D), gelu="tanh"."""
    x = np.asarray(x32, f32).astype(f64)
    D = x.shape[1]
    d = x - x.mean(axis=1, keepdims=True)
    var = (d * d).sum(axis=1, keepdims=True) / (D - 1 if unbiased and D > 1 else D)
    y = d / np.sqrt(var + eps) * np.asarray(w, f64) + np.asarray(b, f64)
    return G.GELUS[gelu](y) if act else y


def row_variance(x32) -> np.ndarray:
    """Biased variance per row in float64."""
    return np.asarray(x32, f32).astype(f64).var(axis=1)


# ------------------------------------------------------------------------------------------ yardsticks (fp32, numpy)

def _tree_sum(v32) -> np.ndarray:
    """fp32 [rows]: 64 partial sums of stride 64, each sequential, then a binary tree over the 64 partials."""
    v = np.asarray(v32, f32)
    rows, D = v.shape
    steps = -(-D // LANES)
    padded = np.zeros((rows, steps * LANES), f32)
    padded[:, :D] = v
    part = np.zeros((rows, LANES), f32)
    for i in range(steps):
        part += padded[:, i * LANES:(i + 1) * LANES]
    n = LANES
    while n > 1:
        n //= 2
        part = part[:, :n] + part[:, n:2 * n]
    return part[:, 0]


def layernorm_tree_f32(x32, w, b, eps: float = EPS) -> np.ndarray:
    """fp32 LayerNorm, the two sums in the order of a wave reduction, one fp32 operation each otherwise."""
    v = np.asarray(x32, f32)
    D = v.shape[1]
    d = v - (_tree_sum(v) / f32(D))[:, None]
    rstd = (f32(1) / np.sqrt(_tree_sum(d * d) / f32(D) + f32(eps))).astype(f32)
    return d * rstd[:, None] * np.asarray(w, f32) + np.asarray(b, f32)


def layernorm_one_pass_f32(x32, w, b, eps: float = EPS) -> np.ndarray:
    """A modified model: the variance as E[x^2] - mean^2 in fp32 (sequential sums), clamped at zero."""
    v = np.asarray(x32, f32)
    D = v.shape[1]
    s, s2 = np.zeros(v.shape[0], f32), np.zeros(v.shape[0], f32)
    for c in range(D):
        s += v[:, c]
        s2 += v[:, c] * v[:, c]
    mean = s / f32(D)
    var = np.maximum(s2 / f32(D) - mean * mean, f32(0))
    rstd = (f32(1) / np.sqrt(var + f32(eps))).astype(f32)
    return (v - mean[:, None]) * rstd[:, None] * np.asarray(w, f32) + np.asarray(b, f32)


def _act_f32(y32, act: int) -> np.ndarray:
    return G._gelu_f32(np.asarray(y32, f32), "erf") if act else np.asarray(y32, f32)


def gelu_steps_f32(y32) -> np.ndarray:
    """fp32: t = y * (1 / sqrt 2), e = erf(t) rounded once, u = 1 + e, h = 0.5 * y, h * u."""
    y = np.asarray(y32, f32)
    t = y * f32(0.70710678118654752)
    e = (1.0 - G._erfc(t.astype(f64))).astype(f32)
    return (f32(0.5) * y) * (f32(1) + e)


def yardsticks(x32, w, b, eps: float = EPS, act: int = 0) -> Dict[str, np.ndarray]:
    """name -> fp32 [rows, D], before any rounding to f16."""
    seq = layernorm_sequential_f32(x32, w, b, eps)
    out = {"sequential": _act_f32(seq, act), "tree": _act_f32(layernorm_tree_f32(x32, w, b, eps), act)}
    if act:
        out["steps"] = gelu_steps_f32(seq)
    return out


def check_rows(name: str, got32, got16, x32, w, b, eps: float = EPS, act: int = 0, yard: Optional[Dict[str, np.ndarray]] = None,
               ref: Optional[np.ndarray] = None) -> None:
    """What a launch delivered against the float64 reference: the fp32 result through gemm_ref.check in units of the fp32 output
    model, the f16 result through check_f16; where both were asked for, out_h is f16(out_f32) bit for bit."""
    ref = layernorm64(x32, w, b, eps, act) if ref is None else ref
    yard = yardsticks(x32, w, b, eps, act) if yard is None else yard
    if got32 is not None:
        check(name + " f32", got32, ref, round_f32(ref), yard)
    if got16 is not None:
        check_f16(name + " f16", got16, ref, yard)
    if got32 is not None and got16 is not None:
        assert np.array_equal(np.asarray(got32, f32).astype(f16).view(np.uint16), np.asarray(got16, f16).view(np.uint16)), \
            f"{name}: out_h is not f16(out_f32)"


# ------------------------------------------------------------------------------------------ inputs

def affine(seed: int, D: int):
    """w ~ U(0.5, 1.5), b ~ N(0, 0.3), fp32 [D]."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, D).astype(f32), rng.normal(0, 0.3, D).astype(f32)


def rows_input(kind: str, seed: int, rows: int, D: int) -> np.ndarray:
    """fp32 [rows, D]:
      gaussian  N(1, 3), what test_layernorm_parity draws
      offset    mean 1000, spread 1: the mean dwarfs the spread (conditions: |mean| >= 300 sigma, asserted for D >= 63)
      near_eps  every row standardised exactly and scaled to a variance s * eps with s log-uniform in [0.3, 3.5], around a
                mean of 0.01 (conditions: variance within a factor 4 of eps; D = 1 has none)
      constant  every row one value of its own, a multiple of 1 / 8 between -8 and 8: 7 significant bits, so every partial sum
                of up to 1280 of them is exact in fp32 in any order, the mean is the value itself and every deviation is zero"""
    rng = np.random.default_rng(seed)
    if kind == "gaussian":
        return (rng.standard_normal((rows, D)) * 3 + 1).astype(f32)
    if kind == "offset":
        return (rng.standard_normal((rows, D)) + 1000.0).astype(f32)
    if kind == "near_eps":
        z = rng.standard_normal((rows, D))
        if D > 1:
            z = (z - z.mean(axis=1, keepdims=True)) / z.std(axis=1, keepdims=True)
        scale = np.sqrt(EPS * np.exp(rng.uniform(np.log(0.3), np.log(3.5), (rows, 1))))
        return (z * scale + 0.01).astype(f32)
    assert kind == "constant", kind
    return np.repeat(rng.integers(-64, 65, (rows, 1)) / 8.0, D, axis=1).astype(f32)


def input_conditions(kind: str, x32, eps: float = EPS) -> None:
    x = np.asarray(x32, f32).astype(f64)
    D = x.shape[1]
    if kind == "offset" and D >= 63:
        assert (np.abs(x.mean(axis=1)) >= 300 * x.std(axis=1)).all(), float((np.abs(x.mean(axis=1)) / x.std(axis=1)).min())
    if kind == "near_eps" and D > 1:
        var = row_variance(x32)
        assert (var > eps / 4).all() and (var < eps * 4).all(), (float(var.min()), float(var.max()))
    if kind == "constant":
        assert (x == x[:, :1]).all()


# ------------------------------------------------------------------------------------------ cast_f16, add_cast, im2col3x3

def cast_values(n: int, seed: int = 0) -> np.ndarray:
    """fp32 [n]: every rounding case of the conversion to f16 first (as many as fit), then Gaussians over six decades.
    Ties to even on both sides (1 + 2^-11 -> 1, 1 + 3 * 2^-11 -> 1 + 2^-9), just off those ties, the smallest subnormal 2^-24, the
    tie to zero 2^-25 and its neighbour above, a subnormal tie (3 * 2^-25 -> 2^-23), the largest normal 65504, the largest value
    that still rounds to it (65519.996), 65520 (a tie, to infinity), zeros of both signs, infinities and a NaN."""
    one = np.float64(1.0)
    special = [one + 2.0 ** -11, one + 3 * 2.0 ** -11, one + 2.0 ** -11 + 2.0 ** -23, one + 2.0 ** -11 - 2.0 ** -23,
               2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25,
               65504.0, 65519.996, 65520.0, 1e30, 0.0]
    special = np.array(special + [-v for v in special] + [np.inf, -np.inf, np.nan], f64).astype(f32)
    rng = np.random.default_rng(seed)
    out = (rng.standard_normal(n) * 10.0 ** rng.uniform(-7, 5, n)).astype(f32)
    k = min(n, len(special))
    out[:k] = special[:k]
    if n >= 2 * len(special):
        out[-len(special):] = special                       # and behind the last full sweep of the grid
    return out


def same_bits(a, b) -> bool:
    """Equal bit for bit, any NaN counting as any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a) & np.isnan(b)
    view = np.uint16 if a.dtype == f16 else np.uint32
    return bool(np.array_equal(a.view(view)[~nan], b.view(view)[~nan]) and np.array_equal(np.isnan(a), np.isnan(b)))


def add_cast_ref(a32, b32, b_mod: int) -> np.ndarray:
    """fp32 [n]: a[i] + b[i % b_mod], one fp32 add (b None: a itself)."""
    a = np.asarray(a32, f32)
    if b32 is None:
        return a.copy()
    return a + np.asarray(b32, f32)[np.arange(a.size) % b_mod]


def place_map(B: int, C: int) -> np.ndarray:
    """f16 [B, 64, 64, C] of integers below 2048 (exact in f16) that name their own place: image, position and channel all
    change the value, and no value is zero, so a zero in the result is a border."""
    b, y, x, c = np.meshgrid(np.arange(B), np.arange(64), np.arange(64), np.arange(C), indexing="ij")
    v = 1 + (b * 977 + y * 131 + x * 17 + c * 3) % 2039
    assert v.min() >= 1 and v.max() < 2048
    return v.astype(f16)
