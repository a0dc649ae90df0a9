"""The cut-out of an image by a coverage, restated in numpy int64: the definition k::mask_cutout (kernels.hpp, K22) implements,
formula for formula, by summed-area tables.  No GPU, no library.

    cutout(image, coverage, radius)             (h, w, 3 | 4) uint8, (h, w) uint8 -> (h, w, 4) uint8: foreground colour, coverage
    cutout_parts(image, coverage, radius)       the intermediates as a dict of int64 arrays (widths, tests)
    blur_fusion_f64(image, coverage, radius)    Forte's Blur-Fusion, one pass, in float64 on the same window -> (h, w, 3) float64
"""
from __future__ import annotations

import numpy as np

from matte_ref import box_sum, window_count

DEFAULT_RADIUS = 16
MAX_RADIUS = 32
D = 65025 * 256


def cutout_parts(image: np.ndarray, coverage: np.ndarray, radius: int) -> dict:
    img = np.asarray(image)
    a = np.asarray(coverage)
    assert img.dtype == np.uint8 and a.dtype == np.uint8
    assert img.ndim == 3 and img.shape[2] in (3, 4) and a.shape == img.shape[:2] and 1 <= radius <= MAX_RADIUS
    h, w = a.shape
    a = a.astype(np.int64)
    I = img[:, :, :3].astype(np.int64)
    N = window_count(h, w, radius)
    S_a = box_sum(a, radius)
    S_b = 255 * N - S_a
    out = np.empty((h, w, 4), np.uint8)
    parts = {"N": N, "S_a": S_a, "S_b": S_b, "S_I": [], "S_Ia": [], "S_Ib": [], "Fh": [], "Bh": [], "num": []}
    for c in range(3):
        Ic = I[:, :, c]
        S_I, S_Ia = box_sum(Ic, radius), box_sum(Ic * a, radius)
        S_Ib = 255 * S_I - S_Ia
        Fh = np.where(S_a > 0, (512 * S_Ia + S_a) // np.maximum(2 * S_a, 1), 256 * Ic)
        Bh = np.where(S_b > 0, (512 * S_Ib + S_b) // np.maximum(2 * S_b, 1), 256 * Ic)
        num = 65025 * Fh + a * (65280 * Ic - a * Fh - (255 - a) * Bh)
        out[:, :, c] = np.clip((2 * num + D) // (2 * D), 0, 255)
        for name, v in (("S_I", S_I), ("S_Ia", S_Ia), ("S_Ib", S_Ib), ("Fh", Fh), ("Bh", Bh), ("num", num)):
            parts[name].append(v)
    out[:, :, 3] = a
    parts["out"] = out
    return parts


def cutout(image: np.ndarray, coverage: np.ndarray, radius: int) -> np.ndarray:
    return cutout_parts(image, coverage, radius)["out"]


def blur_fusion_f64(image: np.ndarray, coverage: np.ndarray, radius: int) -> np.ndarray:
    """F = Fh + alpha (I - alpha Fh - (1 - alpha) Bh), Fh and Bh the alpha- and (1 - alpha)-weighted box means of the image (the
    image's own colour where the weights of a window sum to nothing), on the 0 .. 255 scale, unrounded and unclamped."""
    I = np.asarray(image)[:, :, :3].astype(np.float64)
    al = np.asarray(coverage).astype(np.float64) / 255.0
    S_a, S_b = box_sum(al, radius), box_sum(1.0 - al, radius)
    # (weights that sum to nothing exactly: coverage all 0 or all 255 over the window, which float64 sums represent exactly too)
    S_a_int = box_sum(np.asarray(coverage).astype(np.int64), radius)
    N = window_count(*al.shape, radius)
    out = np.empty_like(I)
    for c in range(3):
        Ic = I[:, :, c]
        Fh = np.where(S_a_int > 0, box_sum(Ic * al, radius) / np.where(S_a_int > 0, S_a, 1.0), Ic)
        Bh = np.where(S_a_int < 255 * N, box_sum(Ic * (1.0 - al), radius) / np.where(S_a_int < 255 * N, S_b, 1.0), Ic)
        out[:, :, c] = Fh + al * (Ic - al * Fh - (1.0 - al) * Bh)
    return out
