"""tests/stroke_ref.py against a brute-force farthest-point sampler on small grids, and the values the stroke derivation is pinned
to (no GPU: tests/test_gpu_stroke_kernel.py holds the kernels to stroke_ref, byte for byte)."""
from __future__ import annotations

import numpy as np
import pytest

import stroke_ref


def brute_force(on: np.ndarray, clicks: int) -> list:
    """the rule as written, cell by cell and pair by pair: O(n^2) per click, plain Python integers"""
    pts = [(x, y) for y in range(on.shape[0]) for x in range(on.shape[1]) if on[y, x]]
    if not pts:
        return []
    n, sx, sy = len(pts), sum(p[0] for p in pts), sum(p[1] for p in pts)
    chosen = [min(pts, key=lambda p: ((n * p[0] - sx) ** 2 + (n * p[1] - sy) ** 2, p[1], p[0]))]
    while len(chosen) < clicks:
        def gain(p):
            return min((p[0] - c[0]) ** 2 + (p[1] - c[1]) ** 2 for c in chosen)
        chosen.append(min(pts, key=lambda p: (-gain(p), p[1], p[0])))
    return chosen


@pytest.mark.parametrize("seed", range(12))
def test_sampler_matches_brute_force(seed):
    rng = np.random.default_rng(seed)
    on = np.zeros((stroke_ref.LOW, stroke_ref.LOW), bool)
    side_x, side_y = int(rng.integers(1, 24)), int(rng.integers(1, 24))
    x0, y0 = int(rng.integers(0, stroke_ref.LOW - side_x + 1)), int(rng.integers(0, stroke_ref.LOW - side_y + 1))
    on[y0:y0 + side_y, x0:x0 + side_x] = rng.random((side_y, side_x)) < (0.05, 0.3, 0.9)[seed % 3]
    for clicks in (1, 3, 8):
        assert stroke_ref.sample(on, clicks) == brute_force(on, clicks)


def test_fewer_cells_than_clicks_repeats_a_cell():
    on = np.zeros((stroke_ref.LOW, stroke_ref.LOW), bool)
    on[7, 200] = True
    assert stroke_ref.sample(on, 4) == [(200, 7)] * 4
    assert stroke_ref.sample(np.zeros_like(on), 4) == []
    assert not stroke_ref.record(np.zeros_like(on), 4).any()


def test_cells_are_a_maximum_over_the_footprint():
    # a cell is ON when any pixel of its footprint is, cell by cell, against the definition read literally
    rng = np.random.default_rng(5)
    for w, h in ((37, 23), (300, 1000), (1030, 517)):
        m = np.where(rng.random((h, w)) < 0.002, 255, 0).astype(np.uint8)
        pre_w, pre_h = stroke_ref.pre_extent(w, h)
        on = stroke_ref.cells(m, pre_w, pre_h)
        sw, sh = (pre_w + 3) // 4, (pre_h + 3) // 4
        assert not on[sh:].any() and not on[:, sw:].any()
        for y in range(sh):
            ya, yb = int(stroke_ref.footprint_lo(y, h, pre_h)), int(stroke_ref.footprint_hi(y, h, pre_h))
            for x in range(sw):
                xa, xb = int(stroke_ref.footprint_lo(x, w, pre_w)), int(stroke_ref.footprint_hi(x, w, pre_w))
                assert on[y, x] == bool((m[ya:yb, xa:xb] >= 128).any()), (x, y)


def test_ballots_layout():
    on = np.zeros((stroke_ref.LOW, stroke_ref.LOW), bool)
    on[3, 0] = on[3, 63] = on[3, 64] = on[255, 255] = True
    b = stroke_ref.ballots(on)
    assert b.shape == (256, 4) and b.dtype == np.uint64
    assert int(b[3, 0]) == 1 | 1 << 63 and int(b[3, 1]) == 1 and int(b[255, 3]) == 1 << 63
    assert int(np.count_nonzero(b)) == 3


def diagonal(w: int, h: int) -> np.ndarray:
    """a one-pixel diagonal m[t, t]: bytes alternate 255 and 128; the pixel the diagonal of the map ends in, its last one, is 127.
    (No map here is square, so that pixel lies off the stroke: the pinned counts hold only while 127 stays outside it -- 1419 ON
    cells at 37 x 23 would be 1475 with it, and 1356 if the 127 replaced the stroke's own last pixel.)"""
    m = np.zeros((h, w), np.uint8)
    t = np.arange(min(w, h))
    m[t, t] = np.where(t % 2 == 0, 255, 128)
    m[h - 1, w - 1] = 127
    return m


# (w, h), pre, ON cells, first cells, first pixels
DIAGONALS = [
    ((37, 23), (1024, 637), 1419, [(80, 80), (0, 0), (159, 159), (41, 39)], [(11, 11), (0, 0), (22, 22)]),
    ((1000, 333), (1024, 341), 254, [(42, 42), (85, 85), (0, 0), (63, 64)], [(165, 165), (333, 332), (1, 1)]),
    ((2051, 1537), (1024, 767), 509, [(92, 92), (191, 191), (0, 0), (142, 141)], None),
]


@pytest.mark.parametrize("extent,pre,on_cells,first,pixels", DIAGONALS)
def test_pinned_diagonals(extent, pre, on_cells, first, pixels):
    w, h = extent
    assert stroke_ref.pre_extent(w, h) == pre
    m = diagonal(w, h)
    on = stroke_ref.cells(m, *pre)
    assert int(on.sum()) == on_cells
    assert stroke_ref.sample(on, 4) == first
    rec = stroke_ref.record(on, 4)
    assert rec[0] == on_cells and rec[1] == 4 and [tuple(rec[2 + 2 * i:4 + 2 * i]) for i in range(4)] == first and not rec[10:].any()
    if pixels:
        assert stroke_ref.derive(m, 3) == pixels
        assert stroke_ref.derive(m) == pixels            # the default is 3 clicks


def test_pinned_two_pixels():
    m = np.zeros((512, 512), np.uint8)
    m[100, 100], m[300, 400] = 200, 128
    on = stroke_ref.cells(m, 1024, 1024)
    assert int(on.sum()) == 2
    assert stroke_ref.sample(on, 4) == [(50, 50), (200, 150), (50, 50), (50, 50)]


def test_pinned_centroid_tie():
    m = np.zeros((1024, 1024), np.uint8)
    m[:4, :4] = m[-4:, -4:] = 255
    assert stroke_ref.sample(stroke_ref.cells(m, 1024, 1024), 3) == [(0, 0), (255, 255), (0, 0)]


def test_pinned_full_map():
    m = np.full((64, 64), 255, np.uint8)
    on = stroke_ref.cells(m, 1024, 1024)
    assert on.all()
    assert stroke_ref.sample(on, 5) == [(127, 127), (255, 255), (255, 0), (0, 255), (0, 0)]
