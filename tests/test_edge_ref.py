"""Edge marks on the CPU: the integer definition (tests/edge_ref.py, the numpy restatement of k::mask_edge).

* with feather = border = 0 it is binary dilation (offset > 0) or erosion (offset < 0, nothing eroded from the image's border) by
  the disc {(dx, dy): q(dx^2 + dy^2) < 256 |offset| + 128}, against scipy.ndimage, for offsets 1, 2, 3, 7, 20 and 64;
* the hard border is edge(offset + b) AND NOT edge(offset - b);
* no integer d2 has q(d2) == 256 g + 128 for g in 0 .. 64: T > 0 never sits on a tie, dilation and erosion are exact duals;
* the ramp is 0 from T = -256 f down, 255 from T = 256 f up, and monotone in T; the level is monotone in d2;
* every d2 >= R^2 gives the byte of d2 == R^2, masks of one polarity included;
* the brute-force window and the separable form give the same squared distances;
* dlimgedit.h says DLIMG_EDGE_MARK == 14, and dlimgedit_amd.api mirrors the constant.
"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import edge_ref as ER

ROOT = Path(__file__).resolve().parent.parent

PARAMS = [(1, 0, 0), (-1, 0, 0), (64, 32, 32), (-64, 32, 32), (0, 0, 1), (0, 5, 0), (3, 2, 4)]


def blobs(w, h, rng, cell=9):
    """a 0 / 255 mask of random blobs about `cell` pixels across"""
    coarse = rng.random(((h + cell - 1) // cell + 2, (w + cell - 1) // cell + 2))
    fine = np.kron(coarse, np.ones((cell, cell)))
    fine = (fine + np.roll(fine, cell // 2, 0) + np.roll(fine, cell // 2, 1) + np.roll(fine, -(cell // 3), 0)) / 4
    oy, ox = rng.integers(0, cell, 2)
    return (255 * (fine[oy:oy + h, ox:ox + w] > 0.5)).astype(np.uint8)


def masks(w, h, rng):
    """name -> mask: random blobs, all 0, all 255, a checkerboard"""
    yy, xx = np.mgrid[0:h, 0:w]
    return {"blobs": blobs(w, h, rng), "zeros": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8),
            "checker": (255 * ((xx + yy) & 1)).astype(np.uint8)}


def disc(offset):
    n = abs(offset)
    return np.array([[ER.q(dx * dx + dy * dy) < 256 * n + 128 for dx in range(-n, n + 1)] for dy in range(-n, n + 1)])


def test_the_discs_are_the_familiar_ones():
    assert disc(1).all() and disc(1).shape == (3, 3)
    assert disc(2).sum() == 21
    assert all(disc(n)[n, 0] and disc(n)[0, n] for n in (1, 2, 3, 7, 20, 64))


@pytest.mark.parametrize("offset", [1, 2, 3, 7, 20, 64])
def test_grow_and_shrink_are_dilation_and_erosion_by_the_disc(offset):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(offset)
    m = blobs(150, 110, rng, cell=9 if offset < 20 else 31)
    fg = m >= 128
    grown = ndi.binary_dilation(fg, structure=disc(offset))
    shrunk = ndi.binary_erosion(fg, structure=disc(offset), border_value=1)
    assert np.array_equal(ER.edge(m, offset) == 255, grown) and set(np.unique(ER.edge(m, offset))) <= {0, 255}
    assert np.array_equal(ER.edge(m, -offset) == 255, shrunk)
    assert 0 < grown.sum() < grown.size or offset >= 20


def test_brute_force_and_separable_distances_agree():
    rng = np.random.default_rng(5)
    for (w, h), R in (((40, 31), 2), ((40, 31), 7), ((23, 45), 10), ((30, 20), 40), ((1, 1), 3), ((9, 1), 4), ((1, 9), 4)):
        for name, m in masks(w, h, rng).items():
            assert np.array_equal(ER.squared_distance(m, R), ER.squared_distance_separable(m, R)), (w, h, R, name)
    m = np.zeros((12, 15), np.uint8)
    m[4, 6] = 200                                   # >= 128 is foreground whatever the byte
    d2 = ER.squared_distance(m, 9)
    yy, xx = np.mgrid[0:12, 0:15]
    want = np.minimum((yy - 4) ** 2 + (xx - 6) ** 2, 81)
    want[4, 6] = 1
    assert np.array_equal(d2, want)


def test_the_border_identity():
    rng = np.random.default_rng(9)
    m = blobs(90, 70, rng)
    for offset, b in ((0, 1), (0, 3), (2, 2), (-3, 2), (5, 4), (-1, 6)):
        outer = ER.edge(m, offset + b) if offset + b else m
        inner = ER.edge(m, offset - b) if offset - b else m
        assert np.array_equal(ER.edge(m, offset, 0, b) == 255, (outer >= 128) & ~(inner >= 128)), (offset, b)


def test_no_distance_sits_on_a_tie():
    R = ER.MAX_OFFSET + ER.MAX_FEATHER + ER.MAX_BORDER + 1
    qs = {ER.q(d2) for d2 in range(0, 2 * R * R + 1)}
    assert not qs & {256 * g + 128 for g in range(0, 65)}
    # so growing the background is shrinking the foreground
    rng = np.random.default_rng(2)
    m = blobs(60, 50, rng)
    for n in (1, 2, 5):
        assert np.array_equal(ER.edge(255 - m, n), 255 - ER.edge(m, -n))


def test_ramp_end_points_and_monotonicity():
    for offset, f, b in PARAMS + [(0, 1, 0), (0, 32, 0), (10, 32, 0)]:
        R = ER.reach(offset, f, b)
        d2 = np.arange(R * R + 1)
        for fg in (False, True):
            out = ER.level(d2, fg, offset, f, b).astype(int)
            if b == 0:
                step = np.diff(out)
                assert (step >= 0).all() if fg else (step <= 0).all(), (offset, f, b, fg)
    for f in (1, 5, 32):
        # offset 0, no border: T = S = +-(q - 128); the ramp reaches 0 at T <= -256 f and 255 at T >= 256 f
        R = ER.reach(0, f, 0)
        d2 = np.arange(R * R + 1)
        T = np.array([ER.q(v) for v in d2]) - 128
        inside, outside = ER.level(d2, True, 0, f, 0), ER.level(d2, False, 0, f, 0)
        assert (inside[T >= 256 * f] == 255).all() and (outside[-T <= -256 * f] == 0).all()
        assert inside[1] == (255 * (128 + 256 * f) + 256 * f) // (512 * f) and outside[1] == (255 * (-128 + 256 * f) + 256 * f) // (512 * f)
        assert int(inside[1]) + int(outside[1]) in (254, 255, 256)


@pytest.mark.parametrize("offset,feather,border", PARAMS)
def test_saturation_from_the_reach_on(offset, feather, border):
    R = ER.reach(offset, feather, border)
    at = int(ER.level(R * R, True, offset, feather, border)), int(ER.level(R * R, False, offset, feather, border))
    # the formulas WITHOUT the truncation, at distances past the reach and at the infinite one (a very large q)
    def untruncated(q, fg):
        S = q - 128
        T = (S if fg else -S) + 256 * offset
        if border > 0:
            T = 256 * border - abs(T)
        if feather == 0:
            return 255 if T > 0 else 0
        return min(255, max(0, (255 * (T + 256 * feather) + 256 * feather) // (512 * feather)))
    for d2 in (R * R, R * R + 1, 2 * R * R, 10 ** 6):
        assert (untruncated(ER.q(d2), True), untruncated(ER.q(d2), False)) == at
    assert (untruncated(10 ** 12, True), untruncated(10 ** 12, False)) == at
    assert set(at) <= {0, 255} and (border == 0 or at == (0, 0))
    full, none = np.full((5, 7), 255, np.uint8), np.zeros((5, 7), np.uint8)
    assert (ER.edge(full, offset, feather, border) == at[0]).all() and (ER.edge(none, offset, feather, border) == at[1]).all()


def test_refused_parameters():
    for bad in ((0, 0, 0), (65, 0, 0), (-65, 0, 0), (0, 33, 0), (0, -1, 0), (0, 0, 33), (0, 0, -1)):
        with pytest.raises(AssertionError):
            ER.edge(np.zeros((3, 3), np.uint8), *bad)


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        rocm_clang = Path("/opt/rocm/lib/llvm/bin/clang++")
        cxx = str(rocm_clang) if rocm_clang.exists() else None
    assert cxx, "no host C++ compiler found"
    return cxx


def test_the_header_says_fourteen(tmp_path):
    from dlimgedit_amd import api
    assert api.EDGE_MARK == 14
    src = tmp_path / "consumer.cpp"
    src.write_text("""
#include <dlimgedit/dlimgedit.h>
static_assert(DLIMG_EDGE_MARK == 14, "the edge mark of table slot 14");
int main() { return 0; }
""")
    r = subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
