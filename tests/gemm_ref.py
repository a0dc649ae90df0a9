"""Float64 references, rounding model, fp32 yardsticks and input builders for the GEMM family (kernels.hpp: GemmArgs, k::gemm),
shared by tests/test_gemm_ref.py (CPU) and tests/test_gpu_gemm.py (GPU).  No test functions here.

Written from the launch's CONTRACT (kernels.hpp, GemmArgs), not from the kernels:

  * plain       out[m, n] = act(sum_k A[m, k] W[n, k] + bias[n]) + resid[m % resid_mod, n]       A, W f16; act: erf-form GELU
  * statistics  stats[n / bn, m] = (sum, sum (x - block mean)^2) over each block of bn columns of the delivered fp32 result x
  * consumer    out[m, n] = act(rstd_m * (sum_k A[m, k] W[n, k] - mean_m * colsum[n]) + bias[n])   A the f16 stream, W the f16
                scaled weight, colsum the fp32 vector AS PASSED, mean_m / rstd_m of the fp32 stream x the producer delivered
                (not of its f16 copy), biased variance, eps

The REFERENCE takes the kernel's own operands and does everything else in float64.  The ROUNDING MODEL is the reference rounded
once to the output's format.  Errors are measured in units of the model's own error (rms and max).

How many units a correct kernel needs is not a guessed number.  It is measured on the same inputs on YARDSTICKS, plain numpy
fp32 computations that only differ in how the K products are accumulated -- neither guide of the hardware says how the
f16-input MFMA rounds inside an instruction, so two models bracket it:

  * chain    products exact (f16 x f16 is exact in fp32), added one at a time in k order, every sum rounded to nearest: the
             documented behaviour of the f32-input MFMA
  * trunc16  exact blocks of 16 products, each added to the fp32 accumulator with rounding TOWARD ZERO: pessimistic for both
             MFMA shapes in use (32x32x16, 16x16x32)

and then evaluate the epilogue once per operation in fp32, in the order the contract writes it.  A kernel may need ALLOW = 1.25
times the LARGER yardstick's units, the project's allowance for "another summation order and nothing else" (neck_ref.ALLOW).

What the yardsticks lacked when the kernels were first held to them, and the reference-only models that supply it.

(1) Row statistics of rows with |mean| >> sigma: statistics_merged_yardstick, written there.

(2) gelu="fitted".  The contract's activation is the erf-form GELU, but the GEMM epilogues evaluate a fitted sigmoid form,
x * sigmoid(x (a + b x^2 + c x^4)) (device_common.hpp, gelu_pair), whose documented distance from the erf form is 2.5e-5 -- about
400 fp32 units at |x| ~ 1, which no summation order explains.  It is not a rounding but an approximation, so it is not folded
into the reference: the REFERENCE keeps the erf form, and the yardsticks of a GELU launch apply `gelu_fitted` (float64
evaluation of the committed constants, rounded to fp32) in place of the erf form.  The allowance this buys is the function's own
2.519e-5 (test_gemm_ref.py pins that number) times 1.25; the tanh form (4.7e-4) and a GELU skipped for x < 0 stay far outside
it, which test_gemm_ref.py shows.  GELU as the GEMM applies it is also held to 2.6e-5 directly (test_gpu_gemm.py, A = I).
"""
import math
from typing import Dict, Optional

import numpy as np

try:
    from scipy.special import erfc as _erfc
except Exception:  # pragma: no cover
    _erfc = np.vectorize(math.erfc, otypes=[np.float64])

f16, f32, f64 = np.float16, np.float32, np.float64

ALLOW = 1.25                # units a kernel may need, relative to the larger yardstick (neck_ref.ALLOW: another summation order)
EPS = 1e-6
F16_LIMIT = 6e4             # |reference| of every f16 result stays below it (f16 max 65504)


def round_f16(x) -> np.ndarray:
    return np.asarray(x, f64).astype(f16).astype(f64)


def round_f32(x) -> np.ndarray:
    return np.asarray(x, f64).astype(f32).astype(f64)


def rms(x) -> float:
    x = np.asarray(x, f64)
    return float(np.sqrt(np.mean(x * x)))


def ulp16(x) -> np.ndarray:
    """Spacing of f16 at |x| (float64 in, float64 out), floored at 2^-24, the spacing of the subnormals."""
    x = np.abs(np.asarray(x, f64))
    _, e = np.frexp(x)                                   # |x| in [2^(e-1), 2^e); frexp(0) gives e = 0
    return np.ldexp(1.0, np.where(x == 0, -24, np.maximum(e - 11, -24)))


# ------------------------------------------------------------------------------------------ GELU

GELU_FIT = (1.5950157685363155, 0.07401129206536386, -0.0007030335806902641)    # a, b, c of device_common.hpp, gelu_pair


def gelu64(x) -> np.ndarray:
    """Erf form, 0.5 x (1 + erf(x / sqrt 2)) = 0.5 x erfc(-x / sqrt 2): the second spelling keeps the tail's relative accuracy."""
    x = np.asarray(x, f64)
    return 0.5 * x * _erfc(-x * math.sqrt(0.5))


def gelu_fitted(x) -> np.ndarray:
    """The fitted form the GEMM epilogues evaluate, in float64: x * sigmoid(t (a + b t^2 + c t^4)), t = x clamped to +-8."""
    x = np.asarray(x, f64)
    a, b, c = GELU_FIT
    t = np.clip(x, -8.0, 8.0)
    t2 = t * t
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-t * (a + t2 * (b + c * t2))))


def gelu_tanh(x) -> np.ndarray:
    """A modified model: the tanh form, up to 4.7e-4 from the erf form."""
    x = np.asarray(x, f64)
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_skip_negative(x) -> np.ndarray:
    """A modified model: the identity for x >= 0 is wrong too, so keep the erf form there and return 0 for x < 0."""
    x = np.asarray(x, f64)
    return np.where(x < 0, 0.0, gelu64(x))


GELUS = {"erf": gelu64, "fitted": gelu_fitted, "tanh": gelu_tanh, "skip_negative": gelu_skip_negative}


# ------------------------------------------------------------------------------------------ references (float64)

def product(A16, W16) -> np.ndarray:
    return np.asarray(A16, f64) @ np.asarray(W16, f64).T


def plain(A16, W16, bias=None, resid=None, act: int = 0) -> np.ndarray:
    """act(A W^T + bias) + resid[m % resid_mod], resid_mod = rows of resid."""
    v = product(A16, W16)
    if bias is not None:
        v = v + np.asarray(bias, f64)
    if act:
        v = gelu64(v)
    if resid is not None:
        resid = np.asarray(resid, f64)
        assert v.shape[0] % resid.shape[0] == 0
        v = v + np.tile(resid, (v.shape[0] // resid.shape[0], 1))
    return v


def statistics(x32, bn: int) -> np.ndarray:
    """[N / bn, M, 2] float64: per block of bn columns and per row (sum, sum of squared deviations from the block mean) of the
    delivered fp32 result x32 -- the layout of GemmArgs::stats_out."""
    x = np.asarray(x32, f64)
    M, N = x.shape
    assert N % bn == 0
    blocks = x.reshape(M, N // bn, bn)
    s = blocks.sum(axis=2)
    d = blocks - (s / bn)[:, :, None]
    return np.stack([s.T, (d * d).sum(axis=2).T], axis=2)


def row_moments(x32, eps: float = EPS):
    """(mean, rstd) per row in float64 from the fp32 stream: biased variance."""
    x = np.asarray(x32, f64)
    mean = x.mean(axis=1)
    var = ((x - mean[:, None]) ** 2).mean(axis=1)
    return mean, 1.0 / np.sqrt(var + eps)


def consumer(A16, Wg16, colsum32, bias32, x32, eps: float = EPS, act: int = 0) -> np.ndarray:
    """rstd_m * (A Wg^T - mean_m * colsum_n) + bias_n, then act; mean / rstd of x32."""
    m, rstd = row_moments(x32, eps)
    v = rstd[:, None] * (product(A16, Wg16) - m[:, None] * np.asarray(colsum32, f64)[None, :])
    if bias32 is not None:
        v = v + np.asarray(bias32, f64)
    return gelu64(v) if act else v


def output_model(ref, fmt: str = "f32") -> np.ndarray:
    """The rounding model: the reference rounded once to the output's format.  "pair": the residual stream as an f16 pair
    (kernels.hpp, GemmArgs::out_l), hi = f16(v), lo = f16(v - hi), value hi + lo."""
    if fmt == "pair":
        hi = round_f16(ref)
        return hi + round_f16(np.asarray(ref, f64) - hi)
    return round_f16(ref) if fmt == "f16" else round_f32(ref)


# ------------------------------------------------------------------------------------------ yardsticks (fp32, numpy)

def accumulate_chain(A16, W16, drop=None) -> np.ndarray:
    """fp32 [M, N]: exact products added one at a time in k order, round to nearest.  drop = (k0, k1, n0, n1): a modified model
    that leaves the products k0 <= k < k1 out of the columns n0 <= n < n1 (one k slice lost in one column tile)."""
    A = np.asarray(A16, f16).astype(f32)
    W = np.ascontiguousarray(np.asarray(W16, f16).astype(f32).T)          # [K, N]
    acc = np.zeros((A.shape[0], W.shape[1]), f32)
    for kk in range(A.shape[1]):
        p = A[:, kk:kk + 1] * W[kk:kk + 1, :]                              # exact: 11 x 11 significant bits
        if drop is not None and drop[0] <= kk < drop[1]:
            p[:, drop[2]:drop[3]] = 0
        acc += p
    return acc


def _toward_zero(s64: np.ndarray) -> np.ndarray:
    t = s64.astype(f32)
    over = np.abs(t.astype(f64)) > np.abs(s64)
    t[over] = np.nextafter(t[over], f32(0))
    return t


def accumulate_trunc16(A16, W16, block: int = 16) -> np.ndarray:
    """fp32 [M, N]: blocks of 16 products summed exactly (float64: 16 products of 22 bits), each block added to the fp32
    accumulator with rounding toward zero."""
    A, W = np.asarray(A16, f64), np.asarray(W16, f64)
    acc = np.zeros((A.shape[0], W.shape[0]), f32)
    for k0 in range(0, A.shape[1], block):
        acc = _toward_zero(acc.astype(f64) + A[:, k0:k0 + block] @ W[:, k0:k0 + block].T)
    return acc


ACCUMULATIONS = {"chain": accumulate_chain, "trunc16": accumulate_trunc16}


def _gelu_f32(v32: np.ndarray, gelu: str) -> np.ndarray:
    return GELUS[gelu](v32.astype(f64)).astype(f32)          # one evaluation, one rounding


def plain_epilogue(acc32, bias=None, resid=None, act: int = 0, gelu: str = "erf", bias_f16: bool = False,
                   resid_shift: int = 0) -> np.ndarray:
    """fp32: acc + bias, GELU, + resid[m % resid_mod], one fp32 operation each.  Modified models: bias_f16 (the bias rounded to
    f16), resid_shift (the residual row taken `resid_shift` rows late: a wrap one tile off)."""
    v = np.asarray(acc32, f32).copy()
    if bias is not None:
        b = np.asarray(bias, f32)
        v += b.astype(f16).astype(f32) if bias_f16 else b
    if act:
        v = _gelu_f32(v, gelu)
    if resid is not None:
        resid = np.asarray(resid, f32)
        rows = (np.arange(v.shape[0]) + resid_shift) % resid.shape[0]
        v += resid[rows]
    return v


def plain_yardsticks(A16, W16, bias=None, resid=None, act: int = 0, gelu: str = "erf") -> Dict[str, np.ndarray]:
    return {name: plain_epilogue(acc(A16, W16), bias, resid, act, gelu) for name, acc in ACCUMULATIONS.items()}


def statistics_yardstick(x32, bn: int, raw_moments: bool = False) -> np.ndarray:
    """[N / bn, M, 2] fp32: sequential fp32 column sums, then a two-pass fp32 sum of squared deviations.  raw_moments: a
    modified model, sum x^2 - (sum x)^2 / n in fp32."""
    x = np.asarray(x32, f32)
    M, N = x.shape
    out = np.empty((N // bn, M, 2), f32)
    for g in range(N // bn):
        cols = x[:, g * bn:(g + 1) * bn]
        s = np.zeros(M, f32)
        for c in range(bn):
            s += cols[:, c]
        m2 = np.zeros(M, f32)
        if raw_moments:
            for c in range(bn):
                m2 += cols[:, c] * cols[:, c]
            m2 = m2 - s * s / f32(bn)
        else:
            mean = s / f32(bn)
            for c in range(bn):
                d = cols[:, c] - mean
                m2 += d * d
        out[g, :, 0], out[g, :, 1] = s, m2
    return out


def statistics_merged_yardstick(x32, bn: int, group: int) -> np.ndarray:
    """[N / bn, M, 2] fp32, a reference-only model of what the sequential yardstick lacks: the block's columns in groups of
    `group`, per group the sequential sum and the two-pass squares about the GROUP mean, merged as parallel variance algorithms
    do it, m2 = sum_g (m2_g + group * (mean_g - mean)^2), every operation once in fp32.  The group means and the block mean are
    rounded at the magnitude of the MEAN, not of the deviations, so rows with |mean| >> sigma lose 2 * group * |mean_g - mean| *
    ulp(mean) per group: about 20 units at |mean| = 40 sigma where the two-pass sum over the whole block needs 5.  Any
    implementation that spreads a block over several lanes merges partial statistics this way; the contract (kernels.hpp)
    asks for the squares from a group mean because of the spike rows."""
    x = np.asarray(x32, f32)
    M, N = x.shape
    assert bn % group == 0
    out = np.empty((N // bn, M, 2), f32)
    for b in range(N // bn):
        parts = [statistics_yardstick(x[:, b * bn + g * group:b * bn + (g + 1) * group], group)[0] for g in range(bn // group)]
        s = np.zeros(M, f32)
        for part in parts:
            s += part[:, 0]
        mean = s * f32(1.0 / bn)
        m2 = np.zeros(M, f32)
        for part in parts:
            dm = part[:, 0] * f32(1.0 / group) - mean
            m2 += part[:, 1] + f32(group) * dm * dm
        out[b, :, 0], out[b, :, 1] = s, m2
    return out


STAT_GROUPS = (32, 64)      # columns a lane group of the epilogues holds (gemm_epilogue.inc: 32, gemm.hip's ping-pong epilogue: 64)


def statistics_yardsticks(x32, bn: int) -> Dict[str, np.ndarray]:
    """The sequential yardstick and the merged model for every group size that divides the block."""
    out = {"sequential": statistics_yardstick(x32, bn)}
    for group in STAT_GROUPS:
        if bn % group == 0 and group < bn:
            out[f"merged{group}"] = statistics_merged_yardstick(x32, bn, group)
    return out


def check_statistics(name: str, got, x32, bn: int, yardsticks: Optional[Dict[str, np.ndarray]] = None) -> None:
    """got [N / bn, M, 2] against the float64 statistics of the delivered x32, sums and squares through check().
    The squares are positive and span orders of magnitude between rows (a spike row's are up to 10^4 times the others'), so each
    entry -- of got, the reference, the model and the yardsticks alike -- is first divided by the power of two of its
    reference: exact, and every row then counts in its own fp32 spacing.  Unscaled, rms and max would be those of the two or
    three largest entries alone.  The sums are not scaled: a sum may cancel to nearly nothing, where the absolute error stays
    and the spacing shrinks (the reason f16 results are not measured in f16 units either)."""
    ref = statistics(x32, bn)
    yardsticks = statistics_yardsticks(x32, bn) if yardsticks is None else yardsticks
    got = np.asarray(got, f64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    check(name + " sum", got[..., 0], ref[..., 0], round_f32(ref[..., 0]), {k: y[..., 0] for k, y in yardsticks.items()})
    sq = ref[..., 1]
    assert (sq > 0).all()
    scale = np.ldexp(1.0, np.frexp(sq)[1] - 1)
    check(name + " squares", got[..., 1] / scale, sq / scale, round_f32(sq) / scale,
          {k: np.asarray(y[..., 1], f64) / scale for k, y in yardsticks.items()})


def consumer_epilogue(acc32, colsum32, bias32, mean32, rstd32, act: int = 0, gelu: str = "erf") -> np.ndarray:
    """fp32: rstd * (acc - mean * colsum) + bias, then GELU, one fp32 operation each."""
    v = np.asarray(acc32, f32) - np.asarray(mean32, f32)[:, None] * np.asarray(colsum32, f32)[None, :]
    v = v * np.asarray(rstd32, f32)[:, None]
    if bias32 is not None:
        v = v + np.asarray(bias32, f32)
    return _gelu_f32(v, gelu) if act else v


def moments_yardstick(x32, eps: float = EPS):
    """(mean, rstd) fp32 per row from the statistics yardstick over the whole row."""
    x32 = np.asarray(x32, f32)
    D = x32.shape[1]
    st = statistics_yardstick(x32, D)[0]
    mean = st[:, 0] / f32(D)
    rstd = (f32(1) / np.sqrt(st[:, 1] / f32(D) + f32(eps))).astype(f32)
    return mean, rstd


def consumer_yardsticks(A16, Wg16, colsum32, bias32, x32, eps: float = EPS, act: int = 0, gelu: str = "erf") -> Dict[str, np.ndarray]:
    mean, rstd = moments_yardstick(x32, eps)
    return {name: consumer_epilogue(acc(A16, Wg16), colsum32, bias32, mean, rstd, act, gelu) for name, acc in ACCUMULATIONS.items()}


# ------------------------------------------------------------------------------------------ comparison

def ratios(got, ref, model) -> Dict[str, float]:
    """rms and max error of `got` against `ref` in units of the rounding model's own rms / max error."""
    got, ref, model = np.asarray(got, f64), np.asarray(ref, f64), np.asarray(model, f64)
    assert got.shape == ref.shape == model.shape, (got.shape, ref.shape, model.shape)
    unit_rms, unit_max = rms(model - ref), float(np.abs(model - ref).max())
    assert unit_rms > 0 and unit_max > 0, "the rounding model has no error on this input, nothing to measure in"
    return {"rms": rms(got - ref) / unit_rms, "max": float(np.abs(got - ref).max()) / unit_max}


def check(name: str, got, ref, model, yardsticks: Dict[str, np.ndarray]) -> Dict[str, float]:
    """got (a kernel, or a modified model) against ref (float64) in units of the rounding model's error: finite, and at most
    ALLOW times the units the LARGER yardstick needs on the same inputs, rms and max.  Every ratio is logged through
    conftest.within."""
    from conftest import within
    assert yardsticks, "no yardstick"
    assert np.isfinite(np.asarray(got, f64)).all(), f"{name}: non-finite output"
    g = ratios(got, ref, model)
    bound = {"rms": 0.0, "max": 0.0}
    for yname, y in yardsticks.items():
        assert np.isfinite(np.asarray(y, f64)).all(), f"{name}: non-finite yardstick {yname}"
        r = ratios(y, ref, model)
        within(f"{name} {yname} rms/model", r["rms"], np.inf)
        within(f"{name} {yname} max/model", r["max"], np.inf)
        bound = {k: max(bound[k], r[k]) for k in bound}
    print(f"{name}: rms {g['rms']:.3f} units (larger yardstick {bound['rms']:.3f}), max {g['max']:.3f} units "
          f"(larger yardstick {bound['max']:.3f})")
    ok = g["rms"] <= ALLOW * bound["rms"] and g["max"] <= ALLOW * bound["max"]
    try:
        within(name + " rms/model", g["rms"], np.nextafter(ALLOW * bound["rms"], np.inf))
    finally:
        within(name + " max/model", g["max"], np.nextafter(ALLOW * bound["max"], np.inf))
    assert ok
    return g


def f16_bound(ref, yardsticks: Dict[str, np.ndarray]) -> np.ndarray:
    """Element-wise allowance of an f16 result: half an f16 spacing at the reference (floored at 2^-24; the 1 + 2^-10 covers a
    reference just below a power of two) plus ALLOW times the larger fp32 yardstick's largest error.  A ratio in f16 units
    would be meaningless near zero, where the absolute fp32 error stays and the f16 spacing shrinks."""
    ref = np.asarray(ref, f64)
    slack = max(float(np.abs(np.asarray(y, f64) - ref).max()) for y in yardsticks.values())
    return ulp16(ref) / 2 * (1 + 2.0 ** -10) + ALLOW * slack


def check_f16(name: str, got16, ref, yardsticks: Dict[str, np.ndarray]) -> float:
    """An f16 result element by element against f16_bound; logs the largest |got - ref| / bound through conftest.within."""
    from conftest import within
    ref = np.asarray(ref, f64)
    assert np.abs(ref).max() < F16_LIMIT, f"{name}: the reference leaves the f16 range"
    got = np.asarray(got16).astype(f64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    worst = float((np.abs(got - ref) / f16_bound(ref, yardsticks)).max())
    print(f"{name}: largest |got - ref| / bound {worst:.4f}")
    return within(name + " f16 err/bound", worst, np.nextafter(1.0, np.inf))


# ------------------------------------------------------------------------------------------ inputs

def gaussian_case(seed: int, M: int, N: int, K: int):
    """A [M, K] ~ N(0, 1), W [N, K] ~ N(0, 1 / K) as f16, bias [N] ~ N(0, 1) fp32.  Condition: the product's entries are of
    order 1 (rms within [0.5, 2])."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K)).astype(f16)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(f16)
    bias = rng.standard_normal(N).astype(f32)
    return A, W, bias


def gaussian_conditions(A, W) -> None:
    r = rms(product(A, W))
    assert 0.5 <= r <= 2.0, r


def residual_rows(seed: int, rows: int, N: int) -> np.ndarray:
    """fp32 [rows, N]: 3 N(0, 1) + 1 with every 35th entry times 40, the few large channels a SAM stream carries.  35 is coprime
    to every tile width, so the large entries fall on every column position."""
    rng = np.random.default_rng(seed)
    r = (rng.standard_normal((rows, N)) * 3 + 1).astype(f32)
    r.reshape(-1)[::35] *= 40
    return r


def residual_conditions(r) -> None:
    r = np.asarray(r, f64)
    big = np.abs(r) > 30
    assert 0.01 <= big.mean() <= 0.04 and big.any(axis=0).mean() > 0.5, (big.mean(), big.any(axis=0).mean())


SPIKE_ROW, SPIKE_CHANNEL = 37, 77


def add_spike(A, W, rest_rms: float, factor: float = 300.0, row: int = SPIKE_ROW, channel: int = SPIKE_CHANNEL):
    """Returns W with row `channel` aligned with A[row], so that out[row, channel] is about factor * rest_rms: one massive
    channel in one row, the reason the squared deviations are taken from a group mean."""
    direction = np.asarray(A[row], f64)
    W = np.array(W, f16)
    W[channel] = (factor * rest_rms * direction / (direction @ direction)).astype(f16)
    return W


def spike_conditions(ref, row: int = SPIKE_ROW, channel: int = SPIKE_CHANNEL) -> None:
    """The spike row's result has a channel at least 250 times the rms of the row's other channels."""
    ref = np.asarray(ref, f64)
    rest = np.delete(ref[row], channel)
    assert abs(ref[row, channel]) >= 250 * rms(rest), (ref[row, channel], rms(rest))


def stream_case(seed: int, M: int, D: int, K1: int, kind: str):
    """A stream writer's operands: A1 [M, K1], W1 [D, K1] f16, bias [D], resid [M, D] fp32; x = A1 W1^T + bias + resid.
      gaussian  residual_rows (3 N + 1, every 35th entry times 40)
      spike     the same with add_spike on row SPIKE_ROW
      offset    resid = N(0, 1) + 40, product scaled to sigma 0.25: every row has |mean| >= 25 sigma (38 on average; the
                sample sigma of a 128-column row strays by up to a fifth)"""
    A1, W1, b1 = gaussian_case(seed, M, D, K1)
    if kind == "offset":
        rng = np.random.default_rng(seed + 1)
        W1 = (W1.astype(f32) * f32(0.25)).astype(f16)
        b1 = (b1 * f32(0.1)).astype(f32)
        resid = (rng.standard_normal((M, D)) + 40.0).astype(f32)
    else:
        resid = residual_rows(seed + 1, M, D)
        if kind == "spike":
            W1 = add_spike(A1, W1, rms(plain(A1[SPIKE_ROW:SPIKE_ROW + 1], W1, b1, resid[SPIKE_ROW:SPIKE_ROW + 1])))
        else:
            assert kind == "gaussian", kind
    return A1, W1, b1, resid


def stream_conditions(x_ref, kind: str) -> None:
    x = np.asarray(x_ref, f64)
    assert np.abs(x).max() < F16_LIMIT
    if kind == "spike":
        spike_conditions(x)
    if kind == "offset":
        mean, sigma = x.mean(axis=1), x.std(axis=1)
        assert (np.abs(mean) >= 25 * sigma).all(), float((np.abs(mean) / sigma).min())


def consumer_weights(seed: int, N: int, D: int):
    """W2 [N, D] ~ N(0, 1 / D), gamma = 1 + 0.2 N, beta = 0.2 N, bias2 ~ N(0, 1), all fp32: what ext.test_gemm_ln folds."""
    rng = np.random.default_rng(seed)
    W2 = (rng.standard_normal((N, D)) / np.sqrt(D)).astype(f32)
    gamma = (1 + 0.2 * rng.standard_normal(D)).astype(f32)
    beta = (0.2 * rng.standard_normal(D)).astype(f32)
    b2 = rng.standard_normal(N).astype(f32)
    return W2, gamma, beta, b2


def fold_layernorm(W2, gamma, beta, bias2, round_weight: bool = True):
    """The consumer's operands as the loader prepares them: wg = f16(W2 * gamma), colsum = fp32 row sums of wg (of the
    UN-ROUNDED scaled weight with round_weight=False: a modified model), bias = b + W2 . beta."""
    scaled = np.asarray(W2, f32) * np.asarray(gamma, f32)[None, :]
    wg = scaled.astype(f16)
    colsum = (wg if round_weight else scaled).astype(f64).sum(axis=1).astype(f32)
    bias = (np.asarray(bias2, f64) + np.asarray(W2, f64) @ np.asarray(beta, f64)).astype(f32)
    return wg, colsum, bias


def identity_case(M: int, N: int):
    """A = I [M, M], W [N, M] small asymmetric integers: the result is W^T exactly, in fp32 and in f16."""
    A = np.eye(M, dtype=f16)
    W = ((np.arange(N * M).reshape(N, M) * 7 + np.arange(N)[:, None]) % 251).astype(f16)
    return A, W


GELU_SPECIAL = (-0.5645, 8.0, -8.0, 0.0, -0.0, 100.0, -100.0, 1000.0, -1000.0, 6e4, -6e4)
GELU_GRID_COLUMNS = 250


def gelu_grid(M: int = 256, N: int = 256):
    """For GELU as the GEMM applies it: A = I [M, M], W [N, M] f16 and bias [N] fp32 with x[m, n] = W[n, m] + bias[n] EXACT in
    fp32 (asserted).  Columns n < 250: W[n, m] = (m - M / 2) * 3 / 32 (exact f16 within +-12) and bias[n] = n * (3 / 32) / 250
    rounded to a multiple of 2^-16, so these x cover [-12, 12) at a spacing of 3.75e-4 + 1.5e-5.  Columns n >= 250: bias 0 and
    W[n, m] = GELU_SPECIAL[m % 11] rounded to f16 (-0.5645 moves by less than 2.5e-4; the others are exact).  The operand
    -0.0 reaches the epilogue as +0.0: the accumulator's sum of zeros is +0.  Returns (A, W, bias, x float64)."""
    assert M % 2 == 0 and N > GELU_GRID_COLUMNS
    step = 3.0 / 32.0
    A = np.eye(M, dtype=f16)
    W = np.empty((N, M), f16)
    W[:GELU_GRID_COLUMNS] = ((np.arange(M) - M // 2) * step).astype(f16)[None, :]
    W[GELU_GRID_COLUMNS:] = np.array(GELU_SPECIAL, f16)[np.arange(M) % len(GELU_SPECIAL)][None, :]
    bias = np.zeros(N, f32)
    bias[:GELU_GRID_COLUMNS] = (np.round(np.arange(GELU_GRID_COLUMNS) * step / GELU_GRID_COLUMNS * 65536) / 65536).astype(f32)
    x = W.astype(f64).T + bias.astype(f64)[None, :]
    assert np.array_equal(x, (W.astype(f32).T + bias[None, :]).astype(f64)), "x is not exact in fp32"
    return A, W, bias, x


def gelu_grid_conditions(x) -> None:
    """The x values cover [-12, 12] at a spacing of 4e-4 or finer and come within 1e-3 of every special point."""
    v = np.unique(np.asarray(x, f64))
    inside = v[(v >= -12) & (v <= 12)]
    assert inside.min() == -12 and inside.max() >= 12 - 4e-4 and np.diff(inside).max() <= 4e-4, np.diff(inside).max()
    for s in GELU_SPECIAL:
        assert np.abs(v - s).min() <= 1e-3, s
