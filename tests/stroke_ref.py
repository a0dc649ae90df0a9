"""Stroke marks restated in numpy: the cells a scribble switches on, and the clicks sampled from them (kernels.hpp, k::stroke_derive;
csrc/stroke_plan.hpp maps cells to pixels).  Integers throughout, so the GPU's ballots and record are these bytes.

A map is (h, w) uint8 of an image that was encoded at pre_w x pre_h; a pixel belongs to the stroke when its byte is >= 128.
  cells   cell (x, y), x < sw = ceil(pre_w / 4), y < sh = ceil(pre_h / 4), is ON when ANY pixel of its footprint (footprint_lo /
          footprint_hi of kernels/footprint.hpp, both axes) belongs to the stroke
  first   the ON cell nearest the centroid: minimal (n x - Sx)^2 + (n y - Sy)^2, ties to the smallest y, then the smallest x
  more    farthest-point sampling: the ON cell with the largest minimum squared distance to the cells chosen so far, same ties
  pixel   the middle pixel of the cell's footprint
"""
from __future__ import annotations

import numpy as np

LOW = 256
DEFAULT_CLICKS = 3
MAX_CLICKS = 8
RECORD_INTS = 20          # {on_cells, clicks, x0, y0 .. x7, y7, 0, 0}


def pre_extent(w: int, h: int, side: int = 1024) -> tuple:
    """the extent an image w x h is encoded at: longest side -> 1024, as the product rounds it (ResizeLongestSide)"""
    if max(w, h) == side:
        return w, h
    scale = np.float32(side) / np.float32(max(w, h))
    return int(np.float32(w) * scale + np.float32(0.5)), int(np.float32(h) * scale + np.float32(0.5))


def footprint_lo(i, size: int, pre: int):
    return 4 * np.asarray(i, np.int64) * size // pre


def footprint_hi(i, size: int, pre: int):
    e = np.minimum(4 * np.asarray(i, np.int64) + 4, pre)
    return (e * size + pre - 1) // pre


def cells(m: np.ndarray, pre_w: int, pre_h: int) -> np.ndarray:
    """(256, 256) bool [y][x]: the ON cells of map m"""
    h, w = m.shape
    sw, sh = (pre_w + 3) // 4, (pre_h + 3) // 4
    s = np.zeros((h + 1, w + 1), np.int64)
    s[1:, 1:] = np.cumsum(np.cumsum(m >= 128, axis=0, dtype=np.int64), axis=1)
    x0, x1 = footprint_lo(np.arange(sw), w, pre_w), footprint_hi(np.arange(sw), w, pre_w)
    y0, y1 = footprint_lo(np.arange(sh), h, pre_h), footprint_hi(np.arange(sh), h, pre_h)
    inside = s[y1[:, None], x1[None, :]] - s[y0[:, None], x1[None, :]] - s[y1[:, None], x0[None, :]] + s[y0[:, None], x0[None, :]]
    on = np.zeros((LOW, LOW), bool)
    on[:sh, :sw] = inside > 0
    return on


def ballots(on: np.ndarray) -> np.ndarray:
    """(256, 4) uint64: bit b of word [y][w] is cell (64 w + b, y)"""
    bits = on.reshape(LOW, 4, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)
    return np.bitwise_or.reduce(bits, axis=2)


def sample(on: np.ndarray, clicks: int) -> list:
    """the `clicks` cells (x, y) chosen from the ON cells; [] when there is none"""
    n = int(on.sum())
    if n == 0:
        return []
    ys, xs = np.nonzero(on)                  # row-major: y ascending, then x -- argmin / argmax take the first, which is the tie rule
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    key = (n * xs - xs.sum()) ** 2 + (n * ys - ys.sum()) ** 2
    at = int(np.argmin(key))
    chosen = [(int(xs[at]), int(ys[at]))]
    nearest = (xs - xs[at]) ** 2 + (ys - ys[at]) ** 2
    while len(chosen) < clicks:
        at = int(np.argmax(nearest))
        chosen.append((int(xs[at]), int(ys[at])))
        nearest = np.minimum(nearest, (xs - xs[at]) ** 2 + (ys - ys[at]) ** 2)
    return chosen


def record(on: np.ndarray, clicks: int) -> np.ndarray:
    """the 20 int32 k::stroke_derive writes; clicks 0: the default"""
    clicks = clicks or DEFAULT_CLICKS
    out = np.zeros(RECORD_INTS, np.int32)
    chosen = sample(on, clicks)
    if chosen:
        out[0], out[1] = int(on.sum()), clicks
        out[2:2 + 2 * clicks] = np.asarray(chosen, np.int32).reshape(-1)
    return out


def cell_pixel(cell: tuple, w: int, h: int, pre_w: int, pre_h: int) -> tuple:
    x, y = cell
    return (int(footprint_lo(x, w, pre_w) + footprint_hi(x, w, pre_w) - 1) // 2,
            int(footprint_lo(y, h, pre_h) + footprint_hi(y, h, pre_h) - 1) // 2)


def derive(m: np.ndarray, clicks: int = 0, pre: tuple = None) -> list:
    """the pixels (x, y) a stroke mark of `clicks` clicks over map m stands for; [] for an empty stroke"""
    h, w = m.shape
    pre_w, pre_h = pre or pre_extent(w, h)
    return [cell_pixel(c, w, h, pre_w, pre_h) for c in sample(cells(m, pre_w, pre_h), clicks or DEFAULT_CLICKS)]
