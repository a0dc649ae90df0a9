"""The matte of a mask guided by a grey image, restated in numpy int64: the definition k::mask_matte (kernels.hpp, K21)
implements, formula for formula, by summed-area tables.  No GPU, no library.

    grey(guide)                      (h, w) or (h, w, c) uint8, c = 1, 3, 4 -> (h, w) int64
    matte(mask, grey, radius, eps)   -> (out uint8 (h, w), A int64, B int64)
    guided_filter_f64(...)           He et al.'s guided filter in float64 on the same window (what the integers approximate)
"""
from __future__ import annotations

import numpy as np

F = 16
DEFAULT_EPS = 650


def grey(guide: np.ndarray) -> np.ndarray:
    g = np.asarray(guide)
    assert g.dtype == np.uint8
    if g.ndim == 2:
        return g.astype(np.int64)
    assert g.ndim == 3 and g.shape[2] in (1, 3, 4)
    if g.shape[2] == 1:
        return g[:, :, 0].astype(np.int64)
    c = g.astype(np.int64)
    return (c[:, :, 0] + 2 * c[:, :, 1] + c[:, :, 2] + 2) >> 2


def box_sum(v: np.ndarray, r: int) -> np.ndarray:
    """Sum of v over the (2 r + 1)^2 square around every pixel, clipped to the image; exact (int64, or float64 as given)."""
    h, w = v.shape
    sat = np.zeros((h + 1, w + 1), v.dtype)
    sat[1:, 1:] = v.cumsum(0).cumsum(1)
    y0 = np.clip(np.arange(h) - r, 0, h)[:, None]
    y1 = np.clip(np.arange(h) + r + 1, 0, h)[:, None]
    x0 = np.clip(np.arange(w) - r, 0, w)[None, :]
    x1 = np.clip(np.arange(w) + r + 1, 0, w)[None, :]
    return sat[y1, x1] - sat[y0, x1] - sat[y1, x0] + sat[y0, x0]


def window_count(h: int, w: int, r: int) -> np.ndarray:
    ny = np.minimum(np.arange(h) + r, h - 1) - np.maximum(np.arange(h) - r, 0) + 1
    nx = np.minimum(np.arange(w) + r, w - 1) - np.maximum(np.arange(w) - r, 0) + 1
    return ny[:, None].astype(np.int64) * nx[None, :].astype(np.int64)


def matte(mask: np.ndarray, G: np.ndarray, radius: int, eps: int):
    p = np.asarray(mask).astype(np.int64)
    G = np.asarray(G).astype(np.int64)
    assert p.shape == G.shape and p.ndim == 2 and 1 <= radius <= 32 and 1 <= eps <= 65025
    h, w = p.shape
    N = window_count(h, w, radius)
    S_G, S_p, S_GG, S_Gp = box_sum(G, radius), box_sum(p, radius), box_sum(G * G, radius), box_sum(G * p, radius)
    assert max(S_G.max(), S_p.max(), S_GG.max(), S_Gp.max()) < 2 ** 31
    cov = N * S_Gp - S_G * S_p
    den = N * S_GG - S_G * S_G + eps * N * N
    assert den.min() > 0
    A = (2 * cov * 2 ** F + den) // (2 * den)
    B = (2 * (S_p * 2 ** F - A * S_G) + N) // (2 * N)
    S_A, S_B = box_sum(A, radius), box_sum(B, radius)
    q = S_A * G + S_B
    out = np.clip((2 * q + N * 2 ** F) // (2 * N * 2 ** F), 0, 255)
    return out.astype(np.uint8), A, B


def guided_filter_f64(mask: np.ndarray, G: np.ndarray, radius: int, eps: float) -> np.ndarray:
    """round(q) clamped to 0 .. 255, q the guided filter of the mask by G (both on the 0 .. 255 scale, eps in squared grey
    levels) with box means over the clipped window, in float64."""
    p = np.asarray(mask).astype(np.float64)
    I = np.asarray(G).astype(np.float64)
    h, w = p.shape
    N = window_count(h, w, radius).astype(np.float64)
    mean = lambda v: box_sum(v, radius) / N
    mI, mp = mean(I), mean(p)
    a = (mean(I * p) - mI * mp) / (mean(I * I) - mI * mI + eps)
    b = mp - a * mI
    q = mean(a) * I + mean(b)
    return np.clip(np.floor(q + 0.5), 0, 255).astype(np.uint8)
