"""Numpy restatement of the lasso derivation (csrc/kernels/kernels.hpp K20, csrc/lasso_plan.hpp: fold_lasso_rows): the box of a
selection and its most interior point, from the caller's full-resolution u8 mask.  Integers throughout; numpy alone.

For an image W x H encoded at pre_w x pre_h, with sw = ceil(pre_w / 4), sh = ceil(pre_h / 4) and the footprints lo / hi of
tests/prior_ref.py:

    inside[y, x]  for x < sw, y < sh:  2 * sum(footprint) > 255 * area        (where the prior plane is positive)
                  every other cell of Z^2 is background
    box           {lo(Xmin), lo(Ymin), hi(Xmax), hi(Ymax)} over the inside cells, in image pixels, pixel-edge convention
    d2[y, x]      the exact squared Euclidean distance of inside cell (x, y) to the nearest background cell
    click cell    the inside cell with the largest d2, ties to the smallest y, then the smallest x
    click         ((lo(x) + hi(x) - 1) // 2, (lo(y) + hi(y) - 1) // 2)
    record        int32 [8] = {inside cells, box x0, y0, x1, y1, click x, click y, d2}; all zero when no cell is inside
"""
import numpy as np

import prior_ref

LOW = prior_ref.LOW
BOX, CLICK, MASK = 1, 2, 4


def inside_cells(mask: np.ndarray, pre_w: int, pre_h: int) -> np.ndarray:
    """-> [sh, sw] bool, from integer footprint sums (a summed-area table in int64)."""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim == 2
    H, W = mask.shape
    c0, c1 = prior_ref.footprints(W, pre_w)
    r0, r1 = prior_ref.footprints(H, pre_h)
    sat = np.zeros((H + 1, W + 1), np.int64)
    sat[1:, 1:] = mask.astype(np.int64).cumsum(0).cumsum(1)
    total = sat[r1][:, c1] - sat[r0][:, c1] - sat[r1][:, c0] + sat[r0][:, c0]
    area = (r1 - r0)[:, None] * (c1 - c0)[None, :]
    return 2 * total > 255 * area


def column_distance(inside: np.ndarray) -> np.ndarray:
    """g[y, x]: the vertical distance of cell (x, y) to the nearest background cell of its column, 0 for a background cell; the
    rows above the first and below the last are background."""
    sh, sw = inside.shape
    g = np.zeros((sh, sw), np.int64)
    run = np.zeros(sw, np.int64)
    for y in range(sh):                       # distance to the nearest background row above (row -1 at the latest)
        run = np.where(inside[y], run + 1, 0)
        g[y] = run
    run = np.zeros(sw, np.int64)
    for y in range(sh - 1, -1, -1):           # ... and below (row sh at the latest)
        run = np.where(inside[y], run + 1, 0)
        g[y] = np.minimum(g[y], run)
    return g


def squared_distance(inside: np.ndarray) -> np.ndarray:
    """d2[y, x] of every inside cell (0 for background cells): the separable exact transform -- per column the vertical distance
    g, then per row the minimum over x' of (x - x')^2 + g(x', y)^2, the columns -1 and sw (background throughout) included."""
    sh, sw = inside.shape
    g = column_distance(np.asarray(inside, bool))
    g2 = np.zeros((sh, sw + 2), np.int64)     # columns -1 .. sw
    g2[:, 1:-1] = g * g
    xs = np.arange(sw + 2, dtype=np.int64) - 1
    dx2 = (np.arange(sw, dtype=np.int64)[:, None] - xs[None, :]) ** 2         # [x, x']
    d2 = np.stack([(dx2 + g2[y][None, :]).min(axis=1) for y in range(sh)])
    return np.where(inside, d2, 0)


def brute_force_squared_distance(inside: np.ndarray) -> np.ndarray:
    """The same by an all-pairs minimum over the background cells of the plane with ONE ring of background around it: a
    background cell farther out is never nearer than its projection onto that ring (both coordinate differences shrink)."""
    inside = np.asarray(inside, bool)
    sh, sw = inside.shape
    big = np.zeros((sh + 2, sw + 2), bool)
    big[1:-1, 1:-1] = inside
    by, bx = np.nonzero(~big)
    iy, ix = np.nonzero(big)
    out = np.zeros((sh, sw), np.int64)
    if len(iy):
        out[iy - 1, ix - 1] = ((iy[:, None] - by[None, :]) ** 2 + (ix[:, None] - bx[None, :]) ** 2).min(axis=1)
    return out


def derive_from_inside(inside: np.ndarray, W: int, H: int, pre_w: int, pre_h: int) -> np.ndarray:
    record = np.zeros(8, np.int32)
    inside = np.asarray(inside, bool)
    if not inside.any():
        return record
    c0, c1 = prior_ref.footprints(W, pre_w)
    r0, r1 = prior_ref.footprints(H, pre_h)
    ys, xs = np.nonzero(inside)
    d2 = squared_distance(inside)
    flat = int(np.argmax(d2))                 # the first maximum in raster order: the smallest y, then the smallest x
    cy, cx = divmod(flat, inside.shape[1])
    record[:] = [inside.sum(), c0[xs.min()], r0[ys.min()], c1[xs.max()], r1[ys.max()],
                 (c0[cx] + c1[cx] - 1) // 2, (r0[cy] + r1[cy] - 1) // 2, d2[cy, cx]]
    return record


def derive(mask: np.ndarray, pre_w: int, pre_h: int) -> np.ndarray:
    """-> record int32 [8] of a selection (h, w) uint8 of an image encoded at pre_w x pre_h."""
    H, W = mask.shape
    return derive_from_inside(inside_cells(mask, pre_w, pre_h), W, H, pre_w, pre_h)
