"""tests/cutout_ref.py, the numpy restatement of the cut-out's definition (kernels.hpp, K22), held to what the definition
promises and to Forte's Blur-Fusion in float64.  No GPU, no library.

The bound against float64: Fh and Bh are rounded to 1 / 256 of a level, so each is off by at most 1 / 512; they enter the result
with the weights (1 - al^2) and al (1 - al), whose sum 1 + al - 2 al^2 is at most 1.125 (at al = 1 / 4); the final rounding adds
1 / 2.  So the result byte lies within 0.5 + 1.125 / 512 < 0.5023 of the unrounded float64 value (clamped), and within one level
of the rounded one."""
import numpy as np
import pytest

import cutout_ref as CR

BOUND = 0.5 + 1.125 / 512 + 1e-9


def soft_edge(w, h, band=10, fg=200, bg=40):
    """Foreground fg left, background bg right, a linear band of `band` columns between: (image (h, w, 3), coverage (h, w))."""
    e0 = w // 2 - band // 2
    al = np.clip((e0 + band - np.arange(w)) / float(band), 0, 1)
    a = np.tile(np.floor(al * 255 + 0.5).astype(np.uint8), (h, 1))
    I = np.floor(a / 255.0 * fg + (1 - a / 255.0) * bg + 0.5).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(I[:, :, None], 3, 2)), a


def coverages(w, h, rng):
    one = np.zeros((h, w), np.uint8)
    one[h // 2, w // 2] = 255
    yy, xx = np.mgrid[0:h, 0:w]
    edge = np.clip(255 * (0.5 + (0.45 * w - xx + 0.3 * (yy - h / 2)) / 12.0), 0, 255).astype(np.uint8)
    return {"zeros": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8),
            "noise": rng.integers(0, 256, (h, w)).astype(np.uint8), "edge": edge, "one": one}


def images(w, h, rng, channels=3):
    return {"noise": rng.integers(0, 256, (h, w, channels)).astype(np.uint8), "white": np.full((h, w, channels), 255, np.uint8)}


SHAPES = [(1, 1), (3, 2), (17, 9), (64, 64), (300, 90)]


@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_consequences_of_the_definition(w, h):
    rng = np.random.default_rng(w * 100 + h)
    for r in (1, 5, 32):
        for iname, img in images(w, h, rng).items():
            for cname, a in coverages(w, h, rng).items():
                out = CR.cutout(img, a, r)
                what = f"{w}x{h} r{r} {iname}/{cname}"
                assert out.shape == (h, w, 4) and out.dtype == np.uint8
                assert (out[:, :, 3] == a).all(), what                          # the alpha byte is the coverage
                opaque = a == 255
                assert (out[opaque][:, :3] == img[opaque][:, :3]).all(), what   # an opaque pixel keeps its colour exactly
                nothing = CR.box_sum(a.astype(np.int64), r) == 0
                assert (out[nothing][:, :3] == img[nothing][:, :3]).all(), what # no coverage in the window: the image's colour
                if iname == "white":
                    assert (out[:, :, :3] == 255).all(), what                   # a constant image stays constant
        flat = np.full((h, w, 3), 77, np.uint8)
        assert (CR.cutout(flat, coverages(w, h, rng)["noise"], r)[:, :, :3] == 77).all()


def test_a_fourth_channel_is_ignored_and_the_order_is_kept():
    rng = np.random.default_rng(3)
    rgba = rng.integers(0, 256, (20, 31, 4)).astype(np.uint8)
    a = coverages(31, 20, rng)["edge"]
    out = CR.cutout(rgba, a, 4)
    assert (out == CR.cutout(np.ascontiguousarray(rgba[:, :, :3]), a, 4)).all()
    bgra = np.ascontiguousarray(rgba[:, :, [2, 1, 0, 3]])
    assert (CR.cutout(bgra, a, 4) == out[:, :, [2, 1, 0, 3]]).all()


def test_a_transparent_pixel_near_the_object_carries_its_colour():
    h, w, r = 12, 80, 8
    img = np.full((h, w, 3), 40, np.uint8)
    img[:, :40] = (200, 150, 90)
    a = np.zeros((h, w), np.uint8)
    a[:, :40] = 255
    out = CR.cutout(img, a, r)
    assert (out[:, 40:40 + r, :3] == (200, 150, 90)).all() and (out[:, 40:40 + r, 3] == 0).all()
    assert (out[:, 40 + r:, :3] == 40).all()                # out of reach of the object: the image's own
    assert (out[:, :40] == np.array([200, 150, 90, 255])).all()


@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_within_one_level_of_float64_blur_fusion(w, h):
    rng = np.random.default_rng(w + 7 * h)
    worst = 0.0
    for r in (1, 2, 7, 16, 32):
        for img in images(w, h, rng).values():
            for cname, a in coverages(w, h, rng).items():
                out = CR.cutout(img, a, r)[:, :, :3].astype(np.float64)
                f = np.clip(CR.blur_fusion_f64(img, a, r), 0.0, 255.0)
                worst = max(worst, float(np.abs(out - f).max()))
                assert np.abs(out - f).max() <= BOUND, (w, h, r, cname, float(np.abs(out - f).max()))
                assert np.abs(out - np.floor(f + 0.5)).max() <= 1, (w, h, r, cname)
    print(f"{w}x{h}: worst distance to the unrounded float64 value {worst:.4f}")


def test_two_colour_edge_loses_its_fringe():
    """200 over 40, a band of 10 columns, radius 32: over the band, weighted by the coverage, the distance of the colour to the
    foreground's.  Measured: 58.7 levels for the image itself, 6.0 for the cut-out (64 x 200 and 90 x 300 alike)."""
    img, a = soft_edge(300, 90)
    out = CR.cutout(img, a, 32)
    band = (a > 0) & (a < 255)
    assert band.sum() == 9 * 90
    wgt = a[band].astype(np.float64)
    own = (wgt * np.abs(img[band][:, 0].astype(np.float64) - 200)).sum() / wgt.sum()
    cut = (wgt * np.abs(out[band][:, 0].astype(np.float64) - 200)).sum() / wgt.sum()
    print(f"coverage-weighted colour error over the band: image {own:.1f}, cut-out {cut:.1f}")
    assert own > 30 and cut <= own / 4


def test_widths_at_the_largest_window():
    h = w = 70
    p = CR.cutout_parts(np.full((h, w, 3), 255, np.uint8), np.full((h, w), 255, np.uint8), 32)
    assert p["N"].max() == 65 * 65
    assert 65 * 255 * 255 < 2 ** 23                                      # a column sum of I a over 65 rows
    assert 256 * 65 * 255 * 255 < 2 ** 31                                # its prefix over 256 columns
    for c in range(3):
        assert p["S_Ia"][c].max() == 65 * 65 * 255 * 255 and p["S_Ia"][c].max() < 2 ** 31
        assert 512 * p["S_Ia"][c].max() >= 2 ** 32                       # why that product is taken in 64 bits
        assert p["Fh"][c].max() <= 65280 and p["Bh"][c].max() <= 65280 and p["Fh"][c].min() >= 0 and p["Bh"][c].min() >= 0
        assert np.abs(2 * p["num"][c] + CR.D).max() < 2 ** 34
    # ... and on noise, where num takes both signs
    rng = np.random.default_rng(5)
    p = CR.cutout_parts(rng.integers(0, 256, (h, w, 3)).astype(np.uint8), rng.integers(0, 256, (h, w)).astype(np.uint8), 32)
    for c in range(3):
        assert p["Fh"][c].max() <= 65280 and p["Bh"][c].max() <= 65280 and np.abs(2 * p["num"][c] + CR.D).max() < 2 ** 34
        assert (p["S_Ib"][c] >= 0).all() and (p["S_Ia"][c] <= 255 * p["S_a"]).all() and (p["S_Ib"][c] <= 255 * p["S_b"]).all()


def test_radius_is_held_to_its_range():
    img, a = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8)
    for r in (0, 33, -1):
        with pytest.raises(AssertionError):
            CR.cutout(img, a, r)
