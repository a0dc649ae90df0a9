"""Float64 reference, rounding model and input builders for the two launches of the encoder neck
(kernels.hpp: neck_conv1x1_ln, neck_conv3x3_ln), shared by tests/test_neck_ref.py (CPU) and tests/test_gpu_neck.py (GPU).
No test functions here.

Written from the launches' CONTRACT (kernels.hpp), not from their code:

  * 1x1:  v[m, n] = sum_k x[m, k] w[n, k]                                  x, w f16; no bias
  * 3x3:  v[b, y, x, n] = sum_{ky, kx, c} map[b, y + ky - 1, x + kx - 1, c] w[n, (ky * 3 + kx) * 256 + c],
          taps outside the 64 x 64 grid OF THE SAME IMAGE contribute zero
  * both: out[m, :] = gamma * (v[m, :] - mean_m) / sqrt(var_m + eps) + beta over the 256 channels (biased variance),
          written as fp32 and / or f16

The reference takes the kernel's own f16 operands and does everything else in float64.  The rounding model is that same
computation with the roundings the contract states and no others: exact products and sums, the result rounded to the
output's format (and, for the chained neck, the f16 rounding of the map between the two launches).  Errors are measured in
units of the model's own error.  How many units a correct kernel needs is NOT fixed here: fp32 accumulation over K = 768 or
2304 terms costs tens of fp32 units.  It is measured, on the same inputs, on the five launches the two replace (GEMM,
LayerNorm, im2col, GEMM, LayerNorm through their own hooks), and the fused launches may need 1.25 times that -- their
accumulation order differs (K order, MFMA shape), nothing else may.
"""
from typing import Dict, Optional

import numpy as np

f16, f32, f64 = np.float16, np.float32, np.float64

GRID = 64
TOKENS = GRID * GRID
C = 256                     # channels of the neck
EPS = 1e-6
ALLOW = 1.25                # units the fused launches may need, relative to the launches they replace


def round_f16(x: np.ndarray) -> np.ndarray:
    return np.asarray(x, f64).astype(f16).astype(f64)


def round_f32(x: np.ndarray) -> np.ndarray:
    return np.asarray(x, f64).astype(f32).astype(f64)


def rms(x: np.ndarray) -> float:
    x = np.asarray(x, f64)
    return float(np.sqrt(np.mean(x * x)))


# ------------------------------------------------------------------------------------------ reference

def layernorm2d(v: np.ndarray, gamma, beta, eps: float = EPS) -> np.ndarray:
    v = np.asarray(v, f64)
    mean = v.mean(axis=-1, keepdims=True)
    d = v - mean
    var = (d * d).mean(axis=-1, keepdims=True)
    return d / np.sqrt(var + eps) * np.asarray(gamma, f64) + np.asarray(beta, f64)


def im2col3x3(fmap: np.ndarray, pad: str = "zero", tap_order: str = "yx") -> np.ndarray:
    """[B, 64, 64, C] -> [B * 4096, 9 * C], column = tap * C + c with tap = ky * 3 + kx ("yx", the contract) or kx * 3 + ky
    ("xy", a modified model); pad "zero" (the contract) or "clamp" (a modified model: the border repeated).  Keeps the dtype:
    it only copies."""
    fmap = np.asarray(fmap)
    B, g, _, ch = fmap.shape
    padded = np.pad(fmap, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="constant" if pad == "zero" else "edge")
    cols = np.empty((B, g, g, 9, ch), fmap.dtype)
    for ky in range(3):
        for kx in range(3):
            tap = ky * 3 + kx if tap_order == "yx" else kx * 3 + ky
            cols[:, :, :, tap] = padded[:, ky:ky + g, kx:kx + g]
    return cols.reshape(B * g * g, 9 * ch)


def conv1x1_ln(x16, w16, gamma, beta, eps: float = EPS) -> np.ndarray:
    """float64 [M, 256] from f16 x [M, K] and w [256, K]."""
    return layernorm2d(np.asarray(x16, f64) @ np.asarray(w16, f64).T, gamma, beta, eps)


def conv3x3_ln(map16, w16, gamma, beta, eps: float = EPS, pad: str = "zero", tap_order: str = "yx") -> np.ndarray:
    """float64 [B * 4096, 256] from the f16 map [B, 64, 64, 256] and w [256, 2304]."""
    cols = im2col3x3(np.asarray(map16, f64), pad, tap_order)
    return layernorm2d(cols @ np.asarray(w16, f64).T, gamma, beta, eps)


def neck(x16, w1_16, g1, b1, w2_16, g2, b2, round_map: bool = True, **variant) -> np.ndarray:
    """Both launches chained, [B * 4096, K] -> [B * 4096, 256] float64; round_map: the map between them rounded to f16, as the
    real path stores it (False: the un-rounded chain, what an fp32 implementation approximates)."""
    y = conv1x1_ln(x16, w1_16, g1, b1, variant.get("eps", EPS))
    if round_map:
        y = round_f16(y)
    return conv3x3_ln(y.reshape(-1, GRID, GRID, C), w2_16, g2, b2, **variant)


def output_model(ref: np.ndarray, fmt: str) -> np.ndarray:
    """The rounding model of ONE launch: its operands are f16 already, products and sums exact, the result rounded to fmt."""
    return round_f16(ref) if fmt == "f16" else round_f32(ref)


# ------------------------------------------------------------------------------------------ comparison

def ratios(got: np.ndarray, ref: np.ndarray, model: np.ndarray) -> Dict[str, float]:
    """rms and max error of `got` against `ref` in units of the rounding model's own rms / max error."""
    got, ref, model = np.asarray(got, f64), np.asarray(ref, f64), np.asarray(model, f64)
    assert got.shape == ref.shape == model.shape, (got.shape, ref.shape, model.shape)
    unit_rms, unit_max = rms(model - ref), float(np.abs(model - ref).max())
    assert unit_rms > 0 and unit_max > 0, "the rounding model has no error on this input, nothing to measure in"
    return {"rms": rms(got - ref) / unit_rms, "max": float(np.abs(got - ref).max()) / unit_max}


def check(name: str, got: np.ndarray, parent: np.ndarray, ref: np.ndarray, model: np.ndarray) -> Dict[str, float]:
    """got (a fused launch, or a modified model) against ref (float64) in units of the rounding model's error: finite, and
    at most ALLOW times the units `parent` (the launches it replaces, same inputs) needs, rms and max.  The parent's and
    got's ratios are logged through conftest.within."""
    from conftest import within
    assert np.isfinite(np.asarray(got, f64)).all(), f"{name}: non-finite output"
    assert np.isfinite(np.asarray(parent, f64)).all(), f"{name}: non-finite output of the launches it replaces"
    p, g = ratios(parent, ref, model), ratios(got, ref, model)
    print(f"{name}: rms {g['rms']:.3f} units (parent {p['rms']:.3f}), max {g['max']:.3f} units (parent {p['max']:.3f})")
    within(name + " parent rms/model", p["rms"], np.inf)
    within(name + " parent max/model", p["max"], np.inf)
    ok = g["rms"] <= ALLOW * p["rms"] and g["max"] <= ALLOW * p["max"]
    try:
        within(name + " rms/model", g["rms"], np.nextafter(ALLOW * p["rms"], np.inf))
    finally:
        within(name + " max/model", g["max"], np.nextafter(ALLOW * p["max"], np.inf))
    assert ok
    return g


# ------------------------------------------------------------------------------------------ inputs

def affine(seed: int):
    """Non-trivial LayerNorm2d scale and shift."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, C).astype(f32), rng.normal(0, 0.3, C).astype(f32)


def conv1x1_case(seed: int, B: int, K: int, spike_row: Optional[int] = None):
    """x [B * 4096, K], w [256, K] f16.  spike_row: that row's result has one channel about 300 times the rest (a trained
    model's statistic: the reason the squared deviations are taken from the 64-column group mean) -- w's row `spike channel`
    is aligned with the row's input."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (B * TOKENS, K)).astype(f16)
    w = (rng.normal(0, 1, (C, K)) / np.sqrt(K)).astype(f16)
    if spike_row is not None:
        ch = 77
        direction = x[spike_row].astype(f64)
        w[ch] = (300.0 * direction / (direction @ direction)).astype(f16)        # the others are ~N(0, 1)
    return x, w


def conv3x3_weights(seed: int) -> np.ndarray:
    """[256, 2304] f16, distinct per tap: tap t carries its own scale 1 + t / 4 on top of the noise."""
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 1, (C, 9, C)) / np.sqrt(9 * C)
    w *= (1.0 + np.arange(9) / 4.0)[None, :, None]
    return w.reshape(C, 9 * C).astype(f16)


PROBES = [(0, 0), (0, 63), (63, 0), (63, 63),          # corners
          (0, 31), (63, 32), (30, 0), (33, 63),        # edges
          (20, 41)]                                    # interior


def impulse_map(seed: int, B: int, noise: float = 0.05, height: float = 8.0) -> np.ndarray:
    """[B, 64, 64, 256] f16: noise plus, in every image, an impulse (one channel per probe) at each PROBES token.  Every
    output token within one step of a probe sees the impulse through exactly one tap, the others through none."""
    rng = np.random.default_rng(seed)
    m = rng.normal(0, noise, (B, GRID, GRID, C))
    for b in range(B):
        for i, (y, x) in enumerate(PROBES):
            m[b, y, x, (17 * i + 5 * b) % C] += height
    return m.astype(f16)


def probe_neighbourhood() -> np.ndarray:
    """Token indices (within an image) of every PROBES token and its up to 8 neighbours inside the grid: the outputs that
    each of the 9 taps must route correctly."""
    out = set()
    for y, x in PROBES:
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if 0 <= y + dy < GRID and 0 <= x + dx < GRID:
                    out.add((y + dy) * GRID + x + dx)
    return np.array(sorted(out))
