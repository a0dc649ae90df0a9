"""Matte marks on the CPU: the integer definition (tests/matte_ref.py, the numpy restatement of k::mask_matte).

* it is He et al.'s guided filter: within one grey level of the float64 filter at every pixel, on random, soft and blocky inputs;
* its intermediates A and B fit int32 on the two adversarial inputs (the largest A, the largest B);
* a constant guide gives the twice box-filtered mask; a pixel whose mask is constant over the radius-2r square keeps its value;
* an edge of the mask that lies beside a step of the guide moves to the step; RGBA and BGRA guides give the same matte;
* the C++ wrapper's Matte compiles against DLIMG_MATTE_MARK == 11, and dlimgedit_amd.api mirrors the constant.
"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import matte_ref as MR

ROOT = Path(__file__).resolve().parent.parent


def _inputs(w, h, seed):
    """name -> (mask, grey): random bytes; a soft disc on a smooth image; 0 / 255 blocks on a blocky image that shares some edges"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.hypot(xx - 0.45 * w, yy - 0.55 * h)
    soft = np.clip(255 * (0.3 * min(w, h) - d) / 6.0, 0, 255).astype(np.uint8)
    smooth = np.clip(128 + 90 * np.sin(xx / 17.0) * np.cos(yy / 23.0) + rng.normal(0, 6, (h, w)), 0, 255).astype(np.uint8)
    blocks = np.kron(rng.integers(0, 2, ((h + 15) // 16, (w + 15) // 16)), np.ones((16, 16), np.int64))[:h, :w]
    blocky_g = np.kron(rng.integers(0, 256, ((h + 23) // 24, (w + 23) // 24)), np.ones((24, 24), np.int64))[:h, :w]
    return {"random": (rng.integers(0, 256, (h, w)).astype(np.uint8), rng.integers(0, 256, (h, w)).astype(np.uint8)),
            "soft": (soft, smooth),
            "blocky": ((255 * blocks).astype(np.uint8), blocky_g.astype(np.uint8))}


@pytest.mark.parametrize("w,h,r,eps", [(257, 131, 7, 650), (600, 400, 32, 1)], ids=["257x131-r7-eps650", "600x400-r32-eps1"])
def test_the_integer_matte_is_the_guided_filter(w, h, r, eps):
    for name, (mask, G) in _inputs(w, h, 11).items():
        out, A, B = MR.matte(mask, G, r, eps)
        want = MR.guided_filter_f64(mask, G, r, float(eps))
        diff = np.abs(out.astype(np.int64) - want.astype(np.int64))
        print(f"matte.guided.{w}x{h}.{name}: largest difference {int(diff.max())}, {int((diff > 0).sum())} of {diff.size} pixels differ")
        assert diff.max() <= 1
        assert (diff > 0).mean() < 0.05


def adversarial(w, h):
    """(mask, grey) pairs at eps 1: a G in {0, 2} checkerboard with p = 255 * checkerboard (the largest A, about +63.75 * 2^16), and
    G in {253, 255} with p anti-correlated (the largest B, about 1.07e9)."""
    yy, xx = np.mgrid[0:h, 0:w]
    c = ((xx + yy) & 1).astype(np.uint8)
    return {"largest_A": ((255 * c).astype(np.uint8), (2 * c).astype(np.uint8)),
            "largest_B": ((255 * (1 - c)).astype(np.uint8), (253 + 2 * c).astype(np.uint8))}


def test_a_and_b_fit_int32_on_the_adversarial_inputs():
    pairs = adversarial(200, 150)
    out, A, B = MR.matte(*pairs["largest_A"], 32, 1)
    print(f"matte.bounds.largest_A: A in [{A.min()}, {A.max()}] (63.75 * 2^16 = {63.75 * 65536:.0f}), B in [{B.min()}, {B.max()}]")
    assert 60 * 65536 < A.max() <= 63.75 * 65536 and np.abs(A).max() < 2 ** 31 and np.abs(B).max() < 2 ** 31
    # var G = 1 = eps, so a is half the slope 127.5: the checkerboard comes back at half its contrast
    assert set(np.unique(out[40:-40, 40:-40]).tolist()) <= {63, 64, 191, 192}
    out, A, B = MR.matte(*pairs["largest_B"], 32, 1)
    print(f"matte.bounds.largest_B: A in [{A.min()}, {A.max()}], B in [{B.min()}, {B.max()}]")
    assert 0.9e9 < B.max() < 1.1e9 and np.abs(A).max() <= 63.75 * 65536 and np.abs(B).max() < 2 ** 31
    # every product of the definition stays below 2^63 at radius 32: the largest is 2 cov 2^F
    N = 65 * 65
    assert 2 * (N * N * 255 * 255 // 4) * 2 ** MR.F < 2 ** 63


def test_a_constant_guide_gives_the_twice_box_filtered_mask():
    rng = np.random.default_rng(3)
    mask = rng.integers(0, 256, (90, 140)).astype(np.uint8)
    for level in (0, 77, 255):
        for r in (1, 5, 32):
            out, A, B = MR.matte(mask, np.full(mask.shape, level, np.uint8), r, 650)
            assert not A.any()
            N = MR.window_count(*mask.shape, r)
            once = (2 * MR.box_sum(mask.astype(np.int64), r) * 2 ** MR.F + N) // (2 * N)         # B: the rounded box mean, 16 fraction bits
            assert (B == once).all()
            twice = (2 * MR.box_sum(once, r) + N * 2 ** MR.F) // (2 * N * 2 ** MR.F)
            assert (out == np.clip(twice, 0, 255)).all()
            mean2 = MR.box_sum(MR.box_sum(mask.astype(np.float64), r) / N, r) / N
            assert np.abs(out - mean2).max() <= 0.51


def test_uniform_surroundings_leave_a_pixel_unchanged():
    rng = np.random.default_rng(5)
    h, w, r = 120, 160, 6
    G = rng.integers(0, 256, (h, w)).astype(np.uint8)
    mask = np.zeros((h, w), np.uint8)
    mask[:, 80:] = 255
    mask[40:60, 20:50] = 93                                   # any value is taken as is
    out, _, _ = MR.matte(mask, G, r, 650)
    m = mask.astype(np.int64)
    # constant over the clipped radius-2r square <=> mean == value and mean of squares == value^2 there (zero variance)
    N2 = MR.window_count(h, w, 2 * r)
    const = (MR.box_sum(m, 2 * r) == N2 * m) & (MR.box_sum(m * m, 2 * r) == N2 * m * m)
    assert const.mean() > 0.5 and (~const).any()
    assert (out[const] == mask[const]).all()
    assert (out[~const] != mask[~const]).any()


def test_an_edge_moves_towards_a_step_of_the_guide():
    h, w = 64, 128
    G = np.full((h, w), 40, np.uint8)
    G[:, 64:] = 200                                           # the picture's edge: between columns 63 and 64
    mask = np.zeros((h, w), np.uint8)
    mask[:, 60:] = 255                                        # the mask's edge: 4 columns off, between 59 and 60
    out, _, _ = MR.matte(mask, G, 8, 650)
    edge = (out >= 128).argmax(axis=1)                        # the first column at or above 128, per row
    print(f"matte.edge: thresholded edge at columns {sorted(set(edge.tolist()))} (mask 60, guide 64)")
    assert ((edge > 60) & (edge <= 64)).all()
    # and away from a step it stays where it was: the same mask on a flat guide
    flat, _, _ = MR.matte(mask, np.full((h, w), 40, np.uint8), 8, 650)
    assert ((flat >= 128).argmax(axis=1) == 60).all()


def test_rgba_and_bgra_guides_give_equal_mattes():
    rng = np.random.default_rng(9)
    rgba = rng.integers(0, 256, (50, 70, 4)).astype(np.uint8)
    bgra = rgba[:, :, [2, 1, 0, 3]]
    assert (MR.grey(rgba) == MR.grey(bgra)).all() and (MR.grey(rgba) == MR.grey(rgba[:, :, :3])).all()
    other_alpha = rgba.copy()
    other_alpha[:, :, 3] = 7
    assert (MR.grey(other_alpha) == MR.grey(rgba)).all()
    assert (MR.grey(rgba[:, :, 0]) == rgba[:, :, 0]).all() and (MR.grey(rgba[:, :, :1]) == rgba[:, :, 0]).all()
    c = rgba[3, 4].astype(int)
    assert MR.grey(rgba)[3, 4] == (c[0] + 2 * c[1] + c[2] + 2) // 4
    mask = (255 * (rng.random((50, 70)) < 0.5)).astype(np.uint8)
    assert (MR.matte(mask, MR.grey(rgba), 5, 650)[0] == MR.matte(mask, MR.grey(bgra), 5, 650)[0]).all()


def _cxx():
    rocm_clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    cxx = str(rocm_clang) if rocm_clang.exists() else (shutil.which("c++") or shutil.which("g++") or shutil.which("clang++"))
    assert cxx, "no host C++ compiler found"
    return cxx


def test_cpp_wrapper_compiles_with_a_matte(tmp_path):
    from dlimgedit_amd import api
    assert api.MATTE_MARK == 11 and api.MATTE_DEFAULT_EPS == MR.DEFAULT_EPS
    src = tmp_path / "consumer.cpp"
    src.write_text("""
#include <dlimgedit/dlimgedit.hpp>
static_assert(DLIMG_MATTE_MARK == 11, "the matte mark of table slot 14");
dlimg::Image soft(dlimg::Segmentation const& seg, dlimg::Image const& image, dlimg::Image& selection) {
    dlimg::Matte matte{image.pixels()};
    static_assert(sizeof(matte.guide) == sizeof(void*), "a pointer");
    if (matte.channels != 4 || matte.radius != 8 || matte.eps != 0) return dlimg::Image(dlimg::Extent{1, 1}, dlimg::Channels::mask);
    dlimg::Image clicked = seg.compute_mask({dlimg::Click{dlimg::Point{10, 20}, true}}, std::nullopt, {}, std::nullopt, std::nullopt, std::nullopt, matte);
    dlimg::Image cleaned = seg.compute_mask({dlimg::Click{dlimg::Point{10, 20}, true}}, std::nullopt, {}, dlimg::MaskCleanup{4, 4}, std::nullopt,
                                            std::nullopt, dlimg::Matte{image.pixels(), 3, 16, 100});
    dlimg::Image snapped = seg.snap(dlimg::Lasso{selection.pixels()}, {}, {}, std::nullopt, matte);
    seg.snap(dlimg::Lasso{selection.pixels()}, selection.pixels(), {}, {}, dlimg::MaskCleanup{0, 9}, matte);
    std::vector<std::optional<dlimg::Matte>> mattes{matte, std::nullopt};
    auto both = dlimg::Segmentation::compute_mask_batch({&seg, &seg}, std::vector<std::vector<dlimg::Click>>{{{dlimg::Point{1, 2}}}, {{dlimg::Point{3, 4}}}},
                                                        {}, {}, {}, {}, {}, mattes);
    return std::move(both[0]);
}
int main() { return 0; }
""")
    r = subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", "-DDLIMGEDIT_LOAD_DYNAMIC", f"-I{ROOT / 'include'}", "-fsyntax-only",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
