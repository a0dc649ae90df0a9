"""The label-map kernels alone (csrc/kernels/mask_grid.hip) through their hook, ext.test_grid_kernels (lib/libdlimgedit_test.so), on
synthetic planes against the numpy reference (tests/grid_ref.py): the harvest's records exactly, the store and the painted map bit for bit.
Both are integer / bit-exact contracts: every comparison is np.array_equal.  Guard bytes around the store, the records and
the map must be untouched in every call.
"""
import numpy as np
import pytest

import grid_ref as G
from dlimgedit_amd import api

pytestmark = pytest.mark.gpu

f32 = np.float32
LOW = G.LOW
# (width, height) of the image: identity second stage; two stages with a padded band below / to the right; a tiny image
EXTENTS = [(1024, 1024), (600, 400), (333, 1000), (5, 3)]
NAMES = ["negative", "positive", "corners", "beyond", "exact", "noise"]


def _planes(width, height):
    """Two prompts whose planes 1..3 are the six named candidates; plane 0 of a prompt is noise the kernels must not read."""
    pre_w, pre_h = G.pre_extent(width, height)
    sw, sh = -(-pre_w // 4), -(-pre_h // 4)
    rng = np.random.default_rng(1000 * width + height)
    c = {}
    c["negative"] = np.full((LOW, LOW), -3.0, f32)
    c["positive"] = np.full((LOW, LOW), 2.5, f32)
    c["corners"] = np.full((LOW, LOW), -3.0, f32)
    for y, x in ((0, 0), (0, sw - 1), (sh - 1, 0), (sh - 1, sw - 1)):
        c["corners"][y, x] = 6.0
    # positives ONLY in the row and the column just beyond the scored region (where there is one)
    # (large against the negatives: the edge pixels weigh that row / column with 1/8 or 3/8 in the first stage)
    c["beyond"] = np.full((LOW, LOW), -1.0, f32)
    if sh < LOW:
        c["beyond"][sh, :] = 1000.0
    if sw < LOW:
        c["beyond"][:, sw] = 1000.0
    c["exact"] = np.tile(np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1.5, -1.5], f32), (LOW, LOW // 8))
    c["exact"][1::2] = np.roll(c["exact"][0], 3)
    c["noise"] = rng.normal(0.0, 1.2, (LOW, LOW)).astype(f32)
    decoy = rng.normal(0.0, 3.0, (2, LOW, LOW)).astype(f32)
    planes4 = np.stack([np.stack([decoy[0], c["negative"], c["positive"], c["corners"]]),
                        np.stack([decoy[1], c["beyond"], c["exact"], c["noise"]])])
    return planes4, (pre_w, pre_h), (sw, sh)


def _same_map(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8
    if not np.array_equal(got, want):
        ys, xs = np.nonzero(got != want)
        raise AssertionError(f"{what}: {len(ys)} pixels differ, the first at (x={xs[0]}, y={ys[0]}): got {got[ys[0], xs[0]]}, want {want[ys[0], xs[0]]}")


@pytest.mark.parametrize("width,height", EXTENTS)
def test_records_store_and_single_masks(width, height):
    planes4, (pre_w, pre_h), _ = _planes(width, height)
    cand = G.candidates_of(planes4)
    want_rec = G.harvest(cand, pre_w, pre_h)
    masks = [G.mask_of(p, width, height) for p in cand]
    for c, name in enumerate(NAMES):
        rec, got, kept, ok, store = api.ext.test_grid_kernels(planes4, width, height, pre_w, pre_h, kept=[c], want_store=(c == 0))
        assert ok, "guard bytes were written"
        assert kept == [c]
        assert np.array_equal(rec.astype(np.int64) & 0xFFFFFFFF, want_rec & 0xFFFFFFFF), (name, rec.tolist(), want_rec.tolist())
        if store is not None:
            assert np.array_equal(store.view(np.uint32), cand.view(np.uint32))            # the bits, -0.0 included
        _same_map(got, (masks[c] == 255).astype(np.uint8), name)
        # without the cull: the same map
        _, plain, _, ok, _ = api.ext.test_grid_kernels(planes4, width, height, pre_w, pre_h, kept=[c], cull=False)
        assert ok
        _same_map(plain, got, name + " without the cull")
    # the cases say what their names say
    assert not masks[0].any() and masks[1].all()
    assert masks[2].any() or width < 64                   # (single low-res pixels do not show in a 5 x 3 image)
    assert list(want_rec[0][:3]) == [0, 0, 0] and want_rec[0][7] == G.CULL_EMPTY
    assert list(want_rec[3][:3]) == [0, 0, 0]                                              # "beyond": nothing in the scored region


@pytest.mark.parametrize("width,height,edge", [(600, 400, "row"), (750, 1000, "column")])
def test_positives_just_beyond_the_scored_region_show_at_the_crops_edge(width, height, edge):
    """The cull trap: the taps of the pixels at the crop's edge reach one low-res row (column) beyond the scored region.  The
    plane is positive ONLY there: the record counts nothing, and the map must still show it."""
    planes4, (pre_w, pre_h), (sw, sh) = _planes(width, height)
    assert (pre_h % 4 in (0, 3) and sh < LOW) if edge == "row" else (pre_w % 4 in (0, 3) and sw < LOW)
    beyond = planes4[1, 1]
    want = (G.mask_of(beyond, width, height) == 255).astype(np.uint8)
    assert (want[-1, :].any() if edge == "row" else want[:, -1].any()) and not want[0, 0]
    rec, got, _, ok, _ = api.ext.test_grid_kernels(planes4, width, height, pre_w, pre_h, kept=[3])
    assert ok and list(rec[3][:7]) == [0, 0, 0, 0, 0, -1, -1]
    _same_map(got, want, "beyond")


@pytest.mark.parametrize("width,height", EXTENTS)
def test_two_nested_segments_the_smallest_on_top(width, height):
    planes4, (pre_w, pre_h), (sw, sh) = _planes(width, height)
    big, small = np.full((LOW, LOW), -2.0, f32), np.full((LOW, LOW), -2.0, f32)
    big[sh // 8: sh - sh // 8, sw // 8: sw - sw // 8] = 3.0
    small[2 * sh // 5: 3 * sh // 5 + 1, 2 * sw // 5: 3 * sw // 5 + 1] = 3.0          # over the centre: a pixel even of the 5 x 3 image
    planes4[0, 1], planes4[1, 3] = big, small
    cand = G.candidates_of(planes4)
    for kept in ([0, 5], [5, 0], [1, 0, 5]):
        _, got, _, ok, _ = api.ext.test_grid_kernels(planes4, width, height, pre_w, pre_h, kept=kept)
        assert ok
        _same_map(got, G.paint(cand, kept, width, height), str(kept))
    _, got, _, _, _ = api.ext.test_grid_kernels(planes4, width, height, pre_w, pre_h, kept=[0, 5])
    assert set(np.unique(got)) == {0, 1, 2}
    _, got, _, _, _ = api.ext.test_grid_kernels(planes4, width, height, pre_w, pre_h, kept=[5, 0])
    assert set(np.unique(got)) == {0, 2}                 # the big one on top hides the small one


def test_255_kept_segments():
    width, height = 96, 288                              # pre 341 x 1024: two stages, a padded band to the right
    pre_w, pre_h = G.pre_extent(width, height)
    assert (pre_w, pre_h) == (341, 1024)
    planes4 = np.full((85, 4, LOW, LOW), -4.0, f32)
    for c in range(255):
        col, row = c % 5, c // 5
        planes4[c // 3, 1 + c % 3, 5 * row: 5 * row + 7, 17 * col: 17 * col + 20] = 2.0       # neighbours overlap
    cand = G.candidates_of(planes4)
    kept = list(range(255))
    rec, got, out_kept, ok, _ = api.ext.test_grid_kernels(planes4, width, height, pre_w, pre_h, kept=kept)
    assert ok and out_kept == kept
    assert np.array_equal(rec.astype(np.int64) & 0xFFFFFFFF, G.harvest(cand, pre_w, pre_h) & 0xFFFFFFFF)
    _same_map(got, G.paint(cand, kept, width, height), "255 kept")
    assert got.max() == 255 and len(np.unique(got)) > 200
    with pytest.raises(api.Error):
        api.ext.test_grid_kernels(planes4, width, height, pre_w, pre_h, kept=kept + [0])       # 256 do not fit a byte


def test_selection_from_the_harvested_records():
    width, height = 600, 400
    pre_w, pre_h = G.pre_extent(width, height)
    rng = np.random.default_rng(5)
    P = 18                                               # two chunks of the harvest
    planes4 = rng.normal(-3.0, 0.6, (P, 4, LOW, LOW)).astype(f32)       # noise that stays negative: the boxes are the blobs'
    for c in range(3 * P):
        x0, y0 = rng.integers(0, 200, 2)
        planes4[c // 3, 1 + c % 3, y0 // 2: y0 // 2 + int(rng.integers(8, 60)), x0: x0 + int(rng.integers(8, 60))] += f32(rng.uniform(2, 6))
    iou4 = rng.uniform(0.3, 1.0, (P, 4)).astype(f32)
    cand = G.candidates_of(planes4)
    want_rec = G.harvest(cand, pre_w, pre_h)
    stab = sorted(int(r[0]) * 1000 // max(int(r[2]), 1) for r in want_rec)[len(want_rec) // 2]
    nms, kept = G.select(want_rec, iou4[:, 1:].reshape(-1), 650, stab)
    assert 2 <= len(kept) < 3 * P
    rec, got, out_kept, ok, _ = api.ext.test_grid_kernels(planes4, width, height, pre_w, pre_h, iou4=iou4, iou_permille=650,
                                                          stability_permille=stab)
    assert ok and out_kept == kept
    assert np.array_equal(rec.astype(np.int64) & 0xFFFFFFFF, want_rec & 0xFFFFFFFF)
    _same_map(got, G.paint(cand, kept, width, height), "selected")


def test_launcher_refusals_leave_the_next_call_working():
    planes4, (pre_w, pre_h), _ = _planes(5, 3)
    for bad in (dict(kept=[6]), dict(kept=[-1])):
        with pytest.raises(api.Error):
            api.ext.test_grid_kernels(planes4, 5, 3, pre_w, pre_h, **bad)
    with pytest.raises(api.Error, match="invalid extent"):
        api.ext.test_grid_kernels(planes4, 5, 3, 1025, pre_h, kept=[0])
    _, got, _, ok, _ = api.ext.test_grid_kernels(planes4, 5, 3, pre_w, pre_h, kept=[1])
    assert ok and got.all()
