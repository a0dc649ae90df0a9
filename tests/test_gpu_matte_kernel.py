"""The matte kernels alone (k::mask_matte through ext.test_matte) against tests/matte_ref.py: BYTE FOR BYTE, with guard bytes
around the mask, the guide and the workspace intact -- with the uniform-block shortcut and without it.

Extents are the smallest at which the kernels can go wrong: every window clipped on all four sides (5 x 3 at radius 32), one
block, several strips and bands with ragged ends (a strip is 256 - 2 r columns, a band 128 rows, a cell 64 x 64), and one large
image for index width (guide offsets pass 2^25, the planes' byte offsets 2^27)."""
import numpy as np
import pytest

import matte_ref as MR
from test_matte_ref import adversarial

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


def _masks(w, h, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    corners = np.zeros((h, w), np.uint8)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 255
    return {"zeros": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8),
            "random01": (255 * rng.integers(0, 2, (h, w))).astype(np.uint8), "random": rng.integers(0, 256, (h, w)).astype(np.uint8),
            "checker": (255 * ((xx + yy) & 1)).astype(np.uint8),
            "disc": np.where((xx - 0.4 * w) ** 2 + (yy - 0.6 * h) ** 2 <= (0.3 * min(w, h)) ** 2, 255, 0).astype(np.uint8),
            "corners": corners}


def _guides(w, h, rng):
    step = np.full((h, w), 30, np.uint8)
    step[:, w // 2:] = 220
    return {"random": rng.integers(0, 256, (h, w)).astype(np.uint8), "zero": np.zeros((h, w), np.uint8),
            "white": np.full((h, w), 255, np.uint8), "step": step}


def _check(api, mask, guide, r, eps, what):
    want = MR.matte(mask, MR.grey(guide), r, eps)[0]
    for shortcut in (True, False):
        got, ok = api.ext.test_matte(mask, guide, r, eps, shortcut=shortcut)
        diff = got != want
        assert ok, f"{what}: guard bytes overwritten (shortcut {shortcut})"
        assert not diff.any(), (f"{what} (shortcut {shortcut}): {int(diff.sum())} of {diff.size} bytes differ, first at "
                                f"{tuple(np.argwhere(diff)[0])}: {got[diff][0]} for {want[diff][0]}")


@pytest.mark.parametrize("w,h,r", [(5, 3, 32), (64, 64, 1), (257, 131, 7)], ids=["5x3-r32", "64x64-r1", "257x131-r7"])
def test_every_mask_and_guide_at_the_small_extents(api, w, h, r):
    rng = np.random.default_rng(w * 1000 + h)
    guides = _guides(w, h, rng)
    for mname, mask in _masks(w, h, rng).items():
        for gname, guide in guides.items():
            _check(api, mask, guide, r, 650, f"{w}x{h} r{r} {mname}/{gname}")
    for name, (mask, G) in adversarial(w, h).items():
        _check(api, mask, G, r, 1, f"{w}x{h} r{r} {name}")


@pytest.mark.parametrize("w,h,r", [(600, 400, 16), (600, 400, 32), (1024, 683, 8)], ids=["600x400-r16", "600x400-r32", "1024x683-r8"])
def test_several_strips_and_bands(api, w, h, r):
    rng = np.random.default_rng(w + r)
    masks, guides = _masks(w, h, rng), _guides(w, h, rng)
    for mname, gname, eps in (("disc", "random", 650), ("random01", "step", 1), ("random", "random", 65025), ("checker", "white", 650),
                              ("corners", "random", 650), ("full", "random", 650)):
        _check(api, masks[mname], guides[gname], r, eps, f"{w}x{h} r{r} {mname}/{gname} eps {eps}")
    for name, (mask, G) in adversarial(w, h).items():
        _check(api, mask, G, r, 1, f"{w}x{h} r{r} {name}")


def test_channels_and_eps(api):
    rng = np.random.default_rng(21)
    w, h, r = 257, 131, 7
    mask = _masks(w, h, rng)["disc"]
    rgba = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    for guide in (rgba, np.ascontiguousarray(rgba[:, :, :3]), np.ascontiguousarray(rgba[:, :, 1])):
        for eps in (1, 650, 65025):
            _check(api, mask, guide, r, eps, f"channels {1 if guide.ndim == 2 else guide.shape[2]} eps {eps}")
    bgra = np.ascontiguousarray(rgba[:, :, [2, 1, 0, 3]])
    assert (api.ext.test_matte(mask, bgra, r, 650)[0] == api.ext.test_matte(mask, rgba, r, 650)[0]).all()


def test_two_jobs_of_different_size_in_one_call(api):
    rng = np.random.default_rng(33)
    a, b = _masks(300, 200, rng)["disc"], _masks(97, 260, rng)["random01"]
    ga, gb = rng.integers(0, 256, (200, 300, 3)).astype(np.uint8), rng.integers(0, 256, (260, 97)).astype(np.uint8)
    for shortcut in (True, False):
        outs, ok, launches = api.ext.test_matte([a, b], [ga, gb], [9, 32], [650, 1], shortcut=shortcut)
        assert ok and launches == 3
        assert (outs[0] == MR.matte(a, MR.grey(ga), 9, 650)[0]).all() and (outs[1] == MR.matte(b, MR.grey(gb), 32, 1)[0]).all()
    # sixteen jobs are still three launches, the seventeenth starts the next three
    small = [a[:40, :50]] * 17
    guide = [np.ascontiguousarray(ga[:40, :50])] * 17
    outs, ok, launches = api.ext.test_matte(small[:16], guide[:16], [3] * 16, [650] * 16)
    assert ok and launches == 3
    outs, ok, launches = api.ext.test_matte(small, guide, [3] * 17, [650] * 17)
    want = MR.matte(small[0], MR.grey(guide[0]), 3, 650)[0]
    assert ok and launches == 6 and all((o == want).all() for o in outs)


def test_index_width_at_twelve_megapixels(api):
    w, h, r = 4000, 3000, 32
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:h, 0:w]
    mask = np.where((xx - 2100) ** 2 + (yy - 1400) ** 2 <= 900 ** 2, 255, 0).astype(np.uint8)
    mask[-40:, -300:] = 255                                   # something at the far end of the planes
    mask[2900:2990:2, 100:700:3] = 255
    guide = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    want = MR.matte(mask, MR.grey(guide), r, 650)[0]
    got, ok = api.ext.test_matte(mask, guide, r, 650)
    assert ok and (got == want).all(), int((got != want).sum())
    assert ((want > 0) & (want < 255)).sum() > 100000 and (want[-1, -300:] > 0).all()


def test_launcher_refusals_then_one_good_call(api):
    mask, guide = np.zeros((8, 9), np.uint8), np.zeros((8, 9), np.uint8)
    for bad, why in ((dict(radius=0), "radius"), (dict(radius=33), "radius"), (dict(eps=0), "eps"), (dict(eps=65026), "eps"),
                     (dict(eps=-1), "eps"), (dict(guide=None), "null guide"), (dict(guide=np.zeros((8, 9, 2), np.uint8)), "channels"),
                     (dict(mask=np.zeros((0, 9), np.uint8), guide=np.zeros((0, 9), np.uint8)), "extent")):
        args = dict(mask=mask, guide=guide, radius=4, eps=650)
        args.update(bad)
        with pytest.raises(api.Error, match=f"mask_matte: .*{why}"):
            api.ext.test_matte(args["mask"], args["guide"], args["radius"], args["eps"])
    mask[2:5, 3:7] = 255
    got, ok = api.ext.test_matte(mask, guide, 4, 650)
    assert ok and (got == MR.matte(mask, MR.grey(guide), 4, 650)[0]).all()
