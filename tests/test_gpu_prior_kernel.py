"""k::mask_prior alone on the GPU (kernels/mask_prior.hip, through its hook in lib/libdlimgedit_test.so): a caller's u8 mask
as the 256 x 256 fp32 plane of the prompt encoder's mask branch.  The plane must equal tests/prior_ref.py BIT FOR BIT -- the
definition is integer arithmetic up to one correctly rounded fp32 division and one multiply -- at every extent the kernel takes
another path for: the identity (1024 x 1024), up- and down-scaling, extents that are no multiple of anything, a tiny image whose
footprints are single pixels read several times, a width that is no multiple of the 16-byte loads, and the largest image the
issue names (footprints of 17 x 17).  The guard bytes around the plane and around the mask's device copy stay intact in every
call, and a sum that took in a byte behind the mask's end would take in a guard byte and miss the reference."""
import numpy as np
import pytest

import prior_ref

EXTENTS = [(1024, 1024), (600, 400), (333, 1000), (5, 3), (2047, 1025), (4000, 3000)]       # (width, height)
STRENGTHS = [1, 8000, 100000]
IDS = [f"{w}x{h}" for w, h in EXTENTS]


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


def _shared_columns(w, h, pre_w):
    """255 only in the source columns two neighbouring footprints share (all 0 where the footprints partition the row)."""
    c0, c1 = prior_ref.footprints(w, pre_w)
    m = np.zeros((h, w), np.uint8)
    for x in range(len(c0) - 1):
        m[:, c0[x + 1]:c1[x]] = 255          # empty unless footprint x + 1 starts before footprint x ends
    return m


def _masks(w, h, pre_w, pre_h):
    rng = np.random.default_rng(w * 7919 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    c0, c1 = prior_ref.footprints(w, pre_w)
    r0, r1 = prior_ref.footprints(h, pre_h)
    out = {"zeros": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8),
           "random": rng.integers(0, 256, (h, w), dtype=np.uint8), "checkerboard": (((xx + yy) & 1) * 255).astype(np.uint8),
           "shared_columns": _shared_columns(w, h, pre_w)}
    # single set pixels: the four corners, and the last row and column the scored region reads
    for name, (y, x) in {"corner_tl": (0, 0), "corner_tr": (0, w - 1), "corner_bl": (h - 1, 0), "corner_br": (h - 1, w - 1),
                         "last_read": (int(r1[-1]) - 1, int(c1[-1]) - 1)}.items():
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 255
        out[name] = m
    return out


def _check(api, mask, pre_w, pre_h, strength, what, quotient=None):
    # (the summed-area table of a 12-megapixel mask is the slow part of the reference: once per mask)
    want = prior_ref.plane_from_quotient(prior_ref.coverage_quotient(mask, pre_w, pre_h) if quotient is None else quotient, strength)
    got, guards_ok = api.ext.test_prior_plane(mask, pre_w, pre_h, strength)
    assert guards_ok, f"{what}: guard bytes were written"
    assert got.dtype == np.float32 and got.shape == (256, 256)
    bits, want_bits = got.view(np.uint32), want.view(np.uint32)
    assert not (want_bits == 0x80000000).any() and not (bits == 0x80000000).any(), f"{what}: -0.0 cannot occur"
    bad = np.argwhere(bits != want_bits)
    assert bad.size == 0, f"{what}: {len(bad)} of 65536 values differ, first at (y, x) = {tuple(bad[0])}: " \
                          f"{got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}"
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("extent", EXTENTS, ids=IDS)
def test_plane_is_the_reference_bit_for_bit(api, extent):
    w, h = extent
    pre_w, pre_h = prior_ref.pre_extent(w, h)
    masks = _masks(w, h, pre_w, pre_h)
    if (4 * w) % pre_w:
        assert masks["shared_columns"].any(), "neighbouring footprints share a column at this width"
    for name, mask in masks.items():
        # every mask at the default strength, the random one at the ends of the range too
        quotient = prior_ref.coverage_quotient(mask, pre_w, pre_h)
        for strength in (STRENGTHS if name == "random" else [8000]):
            want = _check(api, mask, pre_w, pre_h, strength, f"{w}x{h} {name} strength {strength}", quotient)
            s = np.float32(strength) / np.float32(1000)
            sw, sh = (pre_w + 3) // 4, (pre_h + 3) // 4
            assert (want[sh:] == -s).all() and (want[:, sw:] == -s).all()          # padding is background
            if name == "full":
                assert (want[:sh, :sw] == s).all()
            if name == "zeros":
                assert (want == -s).all()


@pytest.mark.gpu
def test_launcher_refusals(api):
    mask = np.zeros((3, 5), np.uint8)
    for pre_w, pre_h, strength in ((1024, 614, 0), (1024, 614, -1), (1024, 614, 100001), (0, 614, 8000), (1024, 1025, 8000),
                                   (1028, 614, 8000)):
        with pytest.raises(api.Error, match="mask_prior"):
            api.ext.test_prior_plane(mask, pre_w, pre_h, strength)
    # a mask so much larger than the extent it was encoded at that a footprint's sum would leave 24 bits: 255 * 257 * 257 > 2^24
    with pytest.raises(api.Error, match="mask_prior.*24 bits"):
        api.ext.test_prior_plane(np.zeros((257 * 4, 257 * 4), np.uint8), 16, 16, 8000)
    # ... and the hook still serves
    _check(api, np.full((3, 5), 255, np.uint8), 1024, 614, 8000, "after the refusals")
