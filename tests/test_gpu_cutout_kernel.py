"""The cut-out kernels alone (k::mask_cutout through ext.test_cutout) against tests/cutout_ref.py: BYTE FOR BYTE, with guard bytes
around the output, the coverage, the guide and the workspace intact, coverage and guide unchanged -- with the covered-or-bare
shortcut and without it.

Extents are the smallest at which the kernel can go wrong: every window clipped on all four sides (1 x 1, 3 x 2), one, two and
three strips at radius 32 (a strip is 256 - 2 r columns: 192 x 5, 193 x 5, 385 x 3), two bands (a band is 32 rows: 7 x 33; 7 x 129
has five), and several strips, bands and 64 x 64 cells with ragged ends (300 x 131)."""
import numpy as np
import pytest

import cutout_ref as CR
from test_cutout_ref import coverages, images, soft_edge

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 2), (192, 5), (193, 5), (385, 3), (7, 33), (7, 129), (300, 131)]


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


def _check(api, cov, guide, r, what, want=None):
    want = CR.cutout(guide, cov, r) if want is None else want
    for shortcut in (True, False):
        got, ok = api.ext.test_cutout(cov, guide, r, shortcut=shortcut)
        diff = got != want
        assert ok, f"{what}: guard bytes overwritten, or coverage or guide changed (shortcut {shortcut})"
        assert not diff.any(), (f"{what} (shortcut {shortcut}): {int(diff.sum())} of {diff.size} bytes differ, first at "
                                f"{tuple(np.argwhere(diff)[0])}: {got[diff][0]} for {want[diff][0]}")
    return want


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_every_coverage_image_radius_and_channel_count(api, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    pictures = images(w, h, rng, channels=4)
    for r in (1, 5, 32):
        for cname, cov in coverages(w, h, rng).items():
            for iname, rgba in pictures.items():
                want = _check(api, cov, rgba, r, f"{w}x{h} r{r} {cname}/{iname} 4 channels")
                _check(api, cov, np.ascontiguousarray(rgba[:, :, :3]), r, f"{w}x{h} r{r} {cname}/{iname} 3 channels", want)


def test_the_two_colour_edge_and_the_channel_order(api):
    img, cov = soft_edge(300, 90)
    _check(api, cov, img, 32, "soft edge 200 over 40")
    rng = np.random.default_rng(8)
    rgba = rng.integers(0, 256, (90, 300, 4)).astype(np.uint8)
    bgra = np.ascontiguousarray(rgba[:, :, [2, 1, 0, 3]])
    a, b = api.ext.test_cutout(cov, rgba, 16)[0], api.ext.test_cutout(cov, bgra, 16)[0]
    assert np.array_equal(b, a[:, :, [2, 1, 0, 3]]) and np.array_equal(a[:, :, 3], cov)


def test_the_shortcut_takes_whole_blocks_and_changes_nothing(api):
    # an object in the middle of a field of bare pixels, and a covered block beside a soft one: most blocks are copies
    w, h = 700, 300
    rng = np.random.default_rng(12)
    yy, xx = np.mgrid[0:h, 0:w]
    cov = np.clip(255 * (0.5 + (90.0 - np.hypot(xx - 350, yy - 150)) / 16.0), 0, 255).astype(np.uint8)
    cov[:, 560:] = 255
    guide = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    want = _check(api, cov, guide, 8, "disc in a field")
    assert ((cov > 0) & (cov < 255)).sum() > 1000 and (want[:, 600:, :3] == guide[:, 600:]).all()


def test_sixteen_jobs_of_mixed_sizes_and_one_more_than_a_launch_holds(api):
    rng = np.random.default_rng(33)
    shapes = [(1, 1), (3, 2), (97, 260), (300, 40), (193, 5), (7, 129), (64, 64), (65, 65), (5, 3), (200, 131), (31, 17), (256, 2), (2, 256),
              (129, 129), (50, 40), (385, 3)]
    covs, guides, radii = [], [], []
    for k, (w, h) in enumerate(shapes):
        covs.append(list(coverages(w, h, rng).values())[k % 5])
        guides.append(rng.integers(0, 256, (h, w, 3 + k % 2)).astype(np.uint8))
        radii.append((1, 5, 32, 16)[k % 4])
    want = [CR.cutout(g, a, r) for a, g, r in zip(covs, guides, radii)]
    for shortcut in (True, False):
        outs, ok, launches = api.ext.test_cutout(covs, guides, radii, shortcut=shortcut)
        assert ok and launches == 2
        for k in range(16):
            assert np.array_equal(outs[k], want[k]), (k, shapes[k], shortcut)
    # the seventeenth job starts the next pair of launches
    outs, ok, launches = api.ext.test_cutout(covs + covs[2:3], guides + guides[2:3], radii + radii[2:3])
    assert ok and launches == 4
    assert all(np.array_equal(o, q) for o, q in zip(outs, want + want[2:3]))


def test_launcher_refusals_then_one_good_call(api):
    cov, guide = np.zeros((8, 9), np.uint8), np.zeros((8, 9, 3), np.uint8)
    for bad, why in ((dict(radius=0), "radius"), (dict(radius=33), "radius"), (dict(guide=None), "null guide"),
                     (dict(guide=np.zeros((8, 9, 2), np.uint8)), "channels"), (dict(guide=np.zeros((8, 9, 1), np.uint8)), "channels"),
                     (dict(cov=np.zeros((0, 9), np.uint8), guide=np.zeros((0, 9, 3), np.uint8)), "extent")):
        args = dict(cov=cov, guide=guide, radius=4)
        args.update(bad)
        with pytest.raises(api.Error, match=f"mask_cutout: .*{why}"):
            api.ext.test_cutout(args["cov"], args["guide"], args["radius"])
    cov[2:5, 3:7] = 200
    guide[...] = np.arange(9, dtype=np.uint8)[None, :, None] * 20
    got, ok = api.ext.test_cutout(cov, guide, 4)
    assert ok and np.array_equal(got, CR.cutout(guide, cov, 4))
