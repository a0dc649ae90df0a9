"""Named cases of the mask clean-up, shared by the CPU test (tests/test_cleanup_oracle.py) and the GPU test of the kernels alone
(tests/test_gpu_cleanup.py).  A case is (name, mask (h, w) uint8 of 0 / 255, max_hole, max_island); expected(case) is the
reference's answer (tests/cleanup_ref.py), computed once per process.

Sizes (w, h): the smallest at which 64 x 64 tiling can go wrong -- 1 x 1, 5 x 3, exactly one tile, one pixel more / less than a
tile, odd sizes of a few tiles, and one of 17 x 9 tiles.  Thresholds that depend on a component's area take it from the
reference's labelling of the INPUT (never from the code under test).
"""
from __future__ import annotations

import numpy as np

from cleanup_ref import cleanup_ref, label8

SIZES = [(1, 1), (5, 3), (64, 64), (65, 63), (91, 37), (257, 130), (1031, 517)]
MULTI_TILE = [(65, 63), (91, 37), (257, 130), (1031, 517)]
UNCHANGED_PATTERNS = ("empty", "full", "checkerboard")       # expected output = input is allowed for these only


def _u8(m) -> np.ndarray:
    return np.where(np.asarray(m, dtype=bool), 255, 0).astype(np.uint8)


def spiral(w: int, h: int, cut: bool = False) -> np.ndarray:
    """A one-pixel-wide foreground spiral with one-pixel gaps over the whole mask: rings at insets 0, 2, 4, ..., each opened
    below its top-left corner and tied to the next ring inside it.  cut: one pixel of the middle ring removed, which leaves an
    outer and an inner part of different areas."""
    m = np.zeros((h, w), bool)
    rings = []
    k = 0
    while w - 4 * k >= 1 and h - 4 * k >= 1:
        a = 2 * k
        m[a, a:w - a] = True
        m[h - 1 - a, a:w - a] = True
        m[a:h - a, a] = True
        m[a:h - a, w - 1 - a] = True
        rings.append(a)
        k += 1
    for a in rings[:-1]:
        if h - 2 * a >= 5 and w - 2 * a >= 5:
            m[a + 1, a] = False              # open the ring
            m[a + 2, a + 1] = True           # tie its end to the next ring's corner
    if cut and len(rings) >= 2:
        a = rings[len(rings) // 2]
        m[a, (a + w - a) // 2] = False
    return m


def checkerboard(w: int, h: int) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx + yy) & 1) == 0


def comb(w: int, h: int) -> np.ndarray:
    """Teeth in every other column that join only in the last row."""
    m = np.zeros((h, w), bool)
    m[:, 0::2] = True
    m[h - 1, :] = True
    return m


def noise(w: int, h: int, density: float, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).random((h, w)) < density


def nested_rings(w: int, h: int) -> np.ndarray:
    """Island in hole in island in hole (filled rectangles at growing insets), plus a foreground speck in the outer background
    and a background speck in the outer ring, so that every threshold above 1 changes something."""
    s = max(2, min(w, h) // 10)
    m = np.zeros((h, w), bool)
    for k, v in ((1, True), (2, False), (3, True), (4, False)):
        m[k * s:h - k * s, k * s:w - k * s] = v
    m[0, 0] = True
    m[s, s + 1] = False
    return m


def corner_diagonal(w: int, h: int, anti: bool = False) -> np.ndarray:
    """Two 3 x 3 blocks that meet only diagonally across the corner of the tiles (0,0), (1,0), (0,1), (1,1), and a 2 x 2 speck."""
    m = np.zeros((h, w), bool)
    m[61:64, 61:64] = True
    m[64:67, 64:67] = True
    if anti:
        m[:, :128] = m[:, 127::-1].copy()
    m[0:2, 0:2] = True
    return m


def specks(w: int, h: int, tie: bool) -> np.ndarray:
    """Three small islands far apart: areas 1, 1, 2 with the largest LAST in raster order (tie = False), or 1, 1, 1."""
    m = np.zeros((h, w), bool)
    m[0, 0] = True
    m[0, w // 2] = True
    m[h - 1, w - 1] = True
    if not tie:
        m[h - 1, w - 2] = True
    return m


def two_blobs(w: int, h: int) -> np.ndarray:
    """Areas 6 and 4, in different tiles where the size allows."""
    m = np.zeros((h, w), bool)
    m[0:2, 0:3] = True
    m[h - 2:h, w - 2:w] = True
    return m


def _areas(m: np.ndarray) -> list:
    return sorted(int(a) for a in label8(m)[1][1:])


def _build() -> list:
    cases = []

    def add(name, m, hole, island):
        cases.append((f"{name}-{m.shape[1]}x{m.shape[0]}-h{hole}-i{island}", _u8(m), int(hole), int(island)))

    for w, h in SIZES:
        tiny = w * h < 4
        for th in ((3, 0), (0, 3), (3, 3)):
            th = (min(th[0], 1), min(th[1], 1)) if tiny else th
            add("empty", np.zeros((h, w), bool), *th)
            add("full", np.ones((h, w), bool), *th)
    for w, h in [(5, 3), (64, 64), (65, 63), (257, 130)]:
        add("checkerboard", checkerboard(w, h), 5, 5)
    for w, h in [(64, 64), (65, 63), (91, 37), (257, 130), (1031, 517)]:
        # the whole background spiral is one hole below the threshold; the cut spiral loses its smaller part, keeps the one
        # whose area EQUALS the threshold
        m = spiral(w, h)
        add("spiral", m, max(_areas(~m)) + 1, 0)
        c = spiral(w, h, cut=True)
        add("spiral_cut", c, 0, max(_areas(c)))
        add("spiral_cut", c, max(_areas(~c)) + 1, max(_areas(c)))
    for w, h in [(5, 3), (64, 64), (65, 63), (91, 37), (257, 130)]:
        add("comb", comb(w, h), h, 0)                      # every gap (area h - 1) is filled
        add("comb_inverted", ~comb(w, h), 0, h)            # every tooth gap an island of h - 1: all below, all equal, the first stays
    # 8-connected sites percolate above a density of about 0.41: at 0.1 only the foreground has small components, at 0.9 only
    # the background, at 0.5 both
    for w, h in [(64, 64), (65, 63), (91, 37), (257, 130)]:
        for di, (density, ths) in enumerate(((0.1, ((0, 8), (8, 8))), (0.5, ((8, 0), (0, 8), (8, 8))), (0.9, ((8, 0), (8, 8))))):
            for th in ths:
                add(f"noise{int(density * 10)}", noise(w, h, density, 100 + di), *th)
    add("noise5", noise(1031, 517, 0.5, 7), 8, 8)
    for w, h in MULTI_TILE:
        m = nested_rings(w, h)
        bg, fg = _areas(~m), _areas(m)
        # background: speck 1, inner hole, hole ring, outside; foreground: speck 1, inner island, outer ring
        inner_hole, hole_ring = bg[1], bg[2]
        inner_island = fg[1]
        for hole in (inner_hole, inner_hole + 1, hole_ring, hole_ring + 1):
            add("nested", m, hole, 0)
        for island in (inner_island, inner_island + 1):
            add("nested", m, 0, island)
        add("nested", m, inner_hole + 1, inner_island + 1)
        add("nested", m, hole_ring + 1, inner_island + 1)
    for w, h in [(257, 130), (1031, 517)]:
        for anti in (False, True):
            m = corner_diagonal(w, h, anti)
            add("corner_anti" if anti else "corner", m, 0, 18)      # 18 = the two blocks together: they stay, the speck goes
            add("corner_anti_bg" if anti else "corner_bg", ~m, 18, 0)
    for w, h in [(5, 3), (64, 64), (65, 63), (257, 130), (1031, 517)]:
        add("largest_unique", specks(w, h, tie=False), 0, 50)
        add("largest_tie", specks(w, h, tie=True), 0, 50)
    for w, h in [(64, 64), (65, 63), (91, 37), (1031, 517)]:
        add("equal_threshold", two_blobs(w, h), 0, 6)       # area 6 is not below 6; area 4 is
        add("equal_threshold_bg", ~two_blobs(w, h), 6, 0)
    return cases


_cases = None
_expected = {}


def cases() -> list:
    global _cases
    if _cases is None:
        _cases = _build()
    return _cases


def expected(case) -> np.ndarray:
    name, mask, hole, island = case
    if name not in _expected:
        out = cleanup_ref(mask, hole, island)
        out.setflags(write=False)
        _expected[name] = out
    return _expected[name]


def pattern_of(case) -> str:
    return case[0].split("-")[0]


def multi_job_call() -> list:
    """Three jobs of different sizes and thresholds for one call."""
    by_name = {c[0]: c for c in cases()}
    pick = [n for n in by_name if n.startswith("noise5-91x37-h8-i8") or n.startswith("spiral_cut-257x130-h0")
            or n.startswith("comb_inverted-65x63")]
    assert len(pick) == 3, pick
    return [by_name[n] for n in sorted(pick)]
