"""The edge mark of a mask, restated in numpy and math.isqrt: the definition k::mask_edge (kernels.hpp, K24) implements.  Integer
arithmetic throughout; no GPU, no library.

    edge(mask, offset, feather, border)         (h, w) uint8 -> (h, w) uint8: grown, shrunk, feathered, bordered
    squared_distance(mask, R)                   (h, w) int64: min(d2, R^2), by a brute-force minimum over the clipped (2R+1)^2 window
    squared_distance_separable(mask, R)         the same numbers by a column pass and a row pass of 2R-1 shifts (the shape of the
                                                kernels; tests/test_edge_ref.py holds the two equal), for the larger cases: edge()
                                                takes it where the brute force would cost more than 10^8 pixel visits
    level(d2, foreground, offset, feather, border)   the byte of a pixel from its d2 and polarity (arrays or scalars)
    q(d2)                                       isqrt(65536 d2), the distance in 1/256 pixel

A pixel is foreground when its byte is >= 128.  Pixels outside the image do not exist: they are neither foreground nor background.
d2 is the exact squared Euclidean distance to the nearest pixel of the other kind, infinite where there is none; every
d2 >= R^2, R = |offset| + feather + border + 1, gives the byte of d2 == R^2, so min(d2, R^2) is all that is computed.
"""
from __future__ import annotations

import math

import numpy as np

MAX_OFFSET = 64
MAX_FEATHER = 32
MAX_BORDER = 32


def reach(offset: int, feather: int, border: int) -> int:
    return abs(offset) + feather + border + 1


def check(offset: int, feather: int, border: int) -> None:
    assert -MAX_OFFSET <= offset <= MAX_OFFSET and 0 <= feather <= MAX_FEATHER and 0 <= border <= MAX_BORDER
    assert (offset, feather, border) != (0, 0, 0)


def q(d2: int) -> int:
    return math.isqrt(65536 * int(d2))


def _shifted(a: np.ndarray, dy: int, dx: int, fill) -> np.ndarray:
    """out[y, x] = a[y + dy, x + dx] where that pixel exists, else fill"""
    h, w = a.shape
    out = np.full_like(a, fill)
    ys, yd = (dy, 0) if dy >= 0 else (0, -dy)
    xs, xd = (dx, 0) if dx >= 0 else (0, -dx)
    nh, nw = h - abs(dy), w - abs(dx)
    if nh > 0 and nw > 0:
        out[yd:yd + nh, xd:xd + nw] = a[ys:ys + nh, xs:xs + nw]
    return out


def squared_distance(mask: np.ndarray, R: int) -> np.ndarray:
    fg = np.asarray(mask) >= 128
    d2 = np.full(fg.shape, R * R, np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            dd = dx * dx + dy * dy
            if dd >= R * R or dd == 0:
                continue
            other = _shifted(fg, dy, dx, False) != fg           # a pixel of the other kind ...
            exists = _shifted(np.ones_like(fg), dy, dx, False)   # ... that exists
            np.minimum(d2, np.where(other & exists, dd, R * R), out=d2)
    return d2


def squared_distance_separable(mask: np.ndarray, R: int) -> np.ndarray:
    fg = np.asarray(mask) >= 128
    out = np.empty(fg.shape, np.int64)
    h, w = fg.shape
    rows = np.arange(h, dtype=np.int64)[:, None]
    far = 4 * (h + R)
    for kind in (False, True):                       # distance TO the nearest pixel of this kind (0 on such a pixel)
        is_kind = fg == kind
        # column pass: the last row of this kind at or above, the next at or below, capped at R
        above = np.maximum.accumulate(np.where(is_kind, rows, -far), axis=0)
        below = np.minimum.accumulate(np.where(is_kind, rows, far)[::-1], axis=0)[::-1]
        g = np.minimum(np.minimum(rows - above, below - rows), R)
        # row pass: min over |dx| < R of dx^2 + g(x + dx)^2, columns outside the image left out
        gg = g * g
        d2 = gg.copy()
        for dx in range(1, min(R, w)):
            np.minimum(d2[:, dx:], gg[:, :-dx] + dx * dx, out=d2[:, dx:])
            np.minimum(d2[:, :-dx], gg[:, dx:] + dx * dx, out=d2[:, :-dx])
        out[fg != kind] = d2[fg != kind]
    return out


def level(d2, foreground, offset: int, feather: int, border: int):
    check(offset, feather, border)
    R = reach(offset, feather, border)
    d2 = np.minimum(np.asarray(d2, np.int64), R * R)
    table = np.array([q(v) for v in range(R * R + 1)], np.int64)
    S = table[d2] - 128
    T = np.where(np.asarray(foreground), S, -S) + 256 * offset
    if border > 0:
        T = 256 * border - np.abs(T)
    if feather == 0:
        return np.where(T > 0, 255, 0).astype(np.uint8)
    f = feather
    return np.clip((255 * (T + 256 * f) + 256 * f) // (512 * f), 0, 255).astype(np.uint8)


def edge(mask: np.ndarray, offset: int, feather: int = 0, border: int = 0, separable: bool | None = None) -> np.ndarray:
    m = np.asarray(mask)
    assert m.dtype == np.uint8 and m.ndim == 2
    check(offset, feather, border)
    R = reach(offset, feather, border)
    if separable is None:
        separable = (2 * R + 1) ** 2 * m.size > 10 ** 8
    d2 = squared_distance_separable(m, R) if separable else squared_distance(m, R)
    return level(d2, m >= 128, offset, feather, border)
