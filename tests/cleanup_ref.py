"""Reference of the mask clean-up (SAM's remove_small_regions as this library states it), pure numpy and Python, nothing from
the library.

    cleanup_ref(mask, max_hole, max_island) -> cleaned mask (uint8, 0 / 255)

mask: (h, w), non-zero = foreground.  Connectivity is 8 for both polarities.
  1. holes (max_hole > 0): every connected component of the background with area < max_hole becomes foreground.
  2. islands (max_island > 0), on the result of 1: every connected component of the foreground with area < max_island becomes
     background -- but when there is a component and ALL are below the threshold, the largest stays; among equal largest the
     one whose first pixel in raster order comes first.
Labelling: the runs of every row, union-find over the runs (a run meets the runs of the row above that it overlaps or touches
diagonally), roots = the smallest run number, so components are numbered by their first pixel in raster order.
"""
from __future__ import annotations

import numpy as np


def label8(m: np.ndarray):
    """m: (h, w) bool.  -> (labels int32 (h, w): 0 where m is False, else 1 .. n in order of the component's first pixel in
    raster order; areas int64 [n + 1], areas[0] = 0)."""
    m = np.ascontiguousarray(m, dtype=bool)
    h, w = m.shape
    padded = np.zeros((h, w + 2), np.int8)
    padded[:, 1:-1] = m
    d = np.diff(padded, axis=1)
    ys, starts = np.nonzero(d == 1)             # raster order: by row, then by column
    _, ends = np.nonzero(d == -1)               # exclusive
    n_runs = len(starts)
    if n_runs == 0:
        return np.zeros((h, w), np.int32), np.zeros(1, np.int64)
    parent = list(range(n_runs))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    row_begin = np.searchsorted(ys, np.arange(h + 1))
    st, en = starts.tolist(), ends.tolist()
    for y in range(1, h):
        a, a_end = row_begin[y], row_begin[y + 1]
        b, b_end = row_begin[y - 1], row_begin[y]
        while a < a_end and b < b_end:
            # run a = [st, en) meets run b of the row above when their columns overlap or touch diagonally
            if st[b] <= en[a] and en[b] >= st[a]:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if en[b] <= en[a]:
                b += 1
            else:
                a += 1
    roots = np.array([find(i) for i in range(n_runs)])
    uniq, comp = np.unique(roots, return_inverse=True)       # sorted by the smallest run of the component
    comp = comp + 1
    lengths = ends - starts
    areas = np.zeros(len(uniq) + 1, np.int64)
    np.add.at(areas, comp, lengths)
    labels = np.zeros(h * w, np.int32)
    labels[m.ravel()] = np.repeat(comp, lengths)
    return labels.reshape(h, w), areas


def cleanup_ref(mask: np.ndarray, max_hole: int, max_island: int) -> np.ndarray:
    m = np.asarray(mask) > 0
    assert m.ndim == 2 and max_hole >= 0 and max_island >= 0
    if max_hole > 0:
        lab, areas = label8(~m)
        small = areas < max_hole
        small[0] = False
        m = m | small[lab]
    if max_island > 0:
        lab, areas = label8(m)
        if len(areas) > 1:
            keep = areas >= max_island
            keep[0] = False
            if not keep.any():
                keep[1 + int(np.argmax(areas[1:]))] = True       # argmax: the first of equal maxima = the first in raster order
            m = keep[lab]
    return np.where(m, 255, 0).astype(np.uint8)
