"""Edge marks on the GPU, end to end: a continuation entry {14, offset, feather, border} behind the clicks and the clean-up mark of
its prompt and in front of its matte mark makes the prompt deliver its mask grown, shrunk, feathered or bordered.  On the parent
commit 14 is a refused label: every test here that sends the mark fails there.

The delivered bytes EQUAL tests/edge_ref.py applied to the mask the same prompt delivers without the mark: for a click and a box
through slot 14 and through the device form, with a clean-up mark in front (the reference taken on the cleaned mask), with a matte
mark behind (tests/matte_ref.py of the reference's bytes) and a cut-out mark behind that (tests/cutout_ref.py of that coverage),
for a lasso prompt, a stroke prompt and a refined multi-click prompt, with the caller's own buffer and with the result in
create_image memory, in the device form in place and through the lane's staging buffer; the other prompts of a call are
untouched; the entry layout the C++ wrapper sends; the refusals arrive through both forms and nothing is written.

A vit_test model written with the mask branch serves everything.  Images: test_gpu_matte.py's, 1024 x 683 RGBA and 600 x 400 RGB.
"""
import ctypes as C
import os

import numpy as np
import pytest

import cutout_ref as CR
import edge_ref as ER
import matte_ref as MR
from test_gpu_matte import IMAGES, _box, _click, _process, _selection, _table_copy, pictures  # noqa: F401  (pictures: a fixture)

pytestmark = pytest.mark.gpu
EMPTY = (0, 0, -1, -1)
EDGES = [(3, 0, 0), (-2, 0, 0), (0, 4, 0), (1, 2, 3)]


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


@pytest.fixture(scope="module")
def world(api, tmp_path_factory, pictures):
    """a model WITH the prompt encoder's mask branch, for the refinement marks"""
    from dlimgedit_amd import weights as W
    from dlimgedit_amd.sam_config import get_config
    mdir = tmp_path_factory.mktemp("models_vit_test_edge")
    W.write_synthetic_model_dir(mdir, get_config("vit_test"), 7, mask_branch=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    segs = _process(api, env, pictures)
    yield env, segs
    for s in segs.values():
        s.close()
    env.close()


def _same(what, got, want):
    diff = got != want
    assert not diff.any(), (what, int(diff.sum()), tuple(np.argwhere(diff)[0]), int(got[diff][0]), int(want[diff][0]))


def _checked(what, plain, got, p):
    """got == edge_ref(plain); -> the pixels the mark changed"""
    assert set(np.unique(plain)) <= {0, 255}
    _same(what, got, ER.edge(plain, *p))
    changed = int((got != plain).sum())
    print(f"edge.e2e.{what} {p}: mask {float((plain > 0).mean()):.3f} covered, {changed} pixels changed of {plain.size}")
    return changed


def _device_masks(api, env, segs, **how):
    """compute_mask_batch_device into fresh device memory -> the masks, as arrays"""
    sizes = [s.extent().width * s.extent().height for s in segs]
    dev = api.ext.device_alloc(env, sum(sizes))
    try:
        offsets = api.ext.compute_mask_batch_device(segs, dev, **how)
        back = np.zeros(sum(sizes), np.uint8)
        api.ext.copy_to_host(env, back, dev)
    finally:
        api.ext.device_free(env, dev)
    return [back[o:o + n].reshape(s.extent().height, s.extent().width).copy() for o, n, s in zip(offsets, sizes, segs)]


@pytest.mark.parametrize("name", list(IMAGES))
def test_click_and_box_through_slot_14_and_the_device_form(api, world, name):
    env, segs = world
    seg = segs[name]
    calls = {
        "click": dict(clicks=[_click(api, name)]),
        "box": dict(regions=[_box(api, name)]),
        "box+point": dict(points=_click(api, name), regions=[_box(api, name)]),
    }
    changed = 0
    for what, how in calls.items():
        plain = api.Segmentation.compute_mask_batch([seg], **how)[0].copy()
        assert np.array_equal(_device_masks(api, env, [seg], **how)[0], plain)
        for p in EDGES:
            got = api.Segmentation.compute_mask_batch([seg], edge=[p], **how)[0]
            changed += _checked(f"{name}.{what}", plain, got, p)
            _same(f"{name}.{what}.device {p}", _device_masks(api, env, [seg], edge=[p], **how)[0], got)
    assert changed > 0, "no prompt of this image delivered a mask with an edge: the mark was never more than a copy"
    # an int is an offset
    assert np.array_equal(seg.compute_mask_clicks(_click(api, name), edge=3), seg.compute_mask_clicks(_click(api, name), edge=(3, 0, 0)))


def test_the_device_form_through_the_staging_buffer(api, world):
    """DLIMGEDIT_FORCE_PEER_COPY: the mask takes the staging + peer-copy path, where the kernels run in the lane's buffer"""
    env, segs = world
    seg, p = segs["small"], (2, 1, 0)
    want = seg.compute_mask_clicks(_click(api, "small"), clean=(300, 300), edge=p)
    before = os.environ.get("DLIMGEDIT_FORCE_PEER_COPY")
    os.environ["DLIMGEDIT_FORCE_PEER_COPY"] = "1"
    try:
        got = _device_masks(api, env, [seg], clicks=[_click(api, "small")], clean=[(300, 300)], edge=[p])[0]
    finally:
        if before is None:
            del os.environ["DLIMGEDIT_FORCE_PEER_COPY"]
        else:
            os.environ["DLIMGEDIT_FORCE_PEER_COPY"] = before
    _same("small.staged", got, want)


@pytest.mark.parametrize("name", list(IMAGES))
def test_cleanup_in_front_matte_and_cutout_behind(api, world, pictures, name):
    _, segs = world
    seg, picture = segs[name], pictures[name]
    guide = np.array(picture)
    click, clean, p, (mr, eps), cr = _click(api, name), (40, 40), (-2, 0, 0), (5, 100), 6
    cleaned = seg.compute_mask_clicks(click, clean=clean).copy()
    edged = seg.compute_mask_clicks(click, clean=clean, edge=p).copy()
    # (a mask that is neither empty nor the whole image loses a pixel to any erosion; the synthetic model's masks are small
    # islands, of which the clean-up keeps the largest, so no more than that is asked)
    assert 0 < int((cleaned > 0).sum()) < cleaned.size and not np.array_equal(cleaned, seg.compute_mask_clicks(click))
    assert _checked(f"{name}.cleaned", cleaned, edged, p) > 0
    # the matte filters what the edge mark delivered
    want = MR.matte(edged, MR.grey(picture), mr, eps)[0]
    _same(f"{name}.matte", seg.compute_mask_clicks(click, clean=clean, edge=p, matte=(guide, mr, eps)), want)
    assert not np.array_equal(want, MR.matte(cleaned, MR.grey(picture), mr, eps)[0]), "the edge mark made no difference to the matte"
    # ... also a feathered one, any 0 .. 255
    soft = seg.compute_mask_clicks(click, edge=(1, 3, 0)).copy()
    assert ((soft > 0) & (soft < 255)).any()
    _same(f"{name}.matte_of_feather", seg.compute_mask_clicks(click, edge=(1, 3, 0), matte=(guide, mr, eps)),
          MR.matte(soft, MR.grey(picture), mr, eps)[0])
    # ... and the cut-out takes that coverage
    cov, rgba = seg.compute_mask_clicks(click, clean=clean, edge=p, matte=(guide, mr, eps), cutout=cr)
    _same(f"{name}.coverage", cov, want)
    _same(f"{name}.rgba", rgba, CR.cutout(picture, want, cr))
    assert np.array_equal(guide, picture)


def test_lasso_stroke_and_refined_prompts(api, world):
    _, segs = world
    name = "small"
    seg = segs[name]
    two = _click(api, name) + [api.Point(5, 5)]
    calls = {
        "lasso": lambda **k: seg.snap_selection(_selection(name), what=api.LASSO_BOX | api.LASSO_CLICK, **k),
        "scribble": lambda **k: seg.scribble(_selection(name), clicks=2, **k),
        "refined": lambda **k: seg.compute_mask_clicks(two, labels=[1, 0], refine_after="each", **k),
        "everything": lambda **k: seg.compute_mask_clicks(two, labels=[1, 0], refine_after="each", clean=(300, 300),
                                                          strokes=[(_selection(name), 1, 2)], **k),
    }
    for what, call in calls.items():
        plain = call().copy()
        for p in ((2, 0, 0), (-1, 2, 0)):
            _checked(f"{name}.{what}", plain, call(edge=p), p)


def test_other_prompts_of_the_call_are_untouched(api, world):
    env, segs = world
    a, b = segs["wide"], segs["small"]
    clicks = [_click(api, "wide"), _click(api, "small"), _click(api, "small")]
    singles = [a.compute_mask_clicks(clicks[0]).copy(), b.compute_mask_clicks(clicks[1]).copy()]
    edges = [None, (4, 0, 0), (0, 0, 2)]
    got = api.Segmentation.compute_mask_batch([a, b, b], clicks=clicks, edge=edges)
    assert np.array_equal(got[0], singles[0])
    _checked("batch.second", singles[1], got[1], edges[1])
    _checked("batch.third", singles[1], got[2], edges[2])
    # the `points` form, and both through the device form
    got = api.Segmentation.compute_mask_batch([a, b], points=[clicks[0][0], clicks[1][0]], edge=[(-3, 1, 0), None])
    _checked("batch.points_form", singles[0], got[0], (-3, 1, 0))
    assert np.array_equal(got[1], singles[1])
    dev = _device_masks(api, env, [a, b, b], clicks=clicks, edge=edges)
    assert np.array_equal(dev[0], singles[0])
    _same("batch.device.second", dev[1], ER.edge(singles[1], *edges[1]))
    _same("batch.device.third", dev[2], ER.edge(singles[1], *edges[2]))


@pytest.mark.parametrize("name", list(IMAGES))
def test_create_image_memory_equals_the_callers_own_buffer(api, world, name):
    _, segs = world
    seg, p = segs[name], (2, 2, 0)
    plain = seg.compute_mask_clicks(_click(api, name), region=_box(api, name)).copy()
    own = np.full(plain.shape, 7, np.uint8)
    got = seg.compute_mask_clicks(_click(api, name), region=_box(api, name), out=own, edge=p)
    assert got is own
    _checked(f"{name}.own", plain, own, p)
    table = _table_copy(api, np.full(plain.shape, 7, np.uint8))
    seg.compute_mask_clicks(_click(api, name), region=_box(api, name), out=table, edge=p)
    _same(f"{name}.table", table, own)


def _raw(api, seg, handles, points, regions, pointers, written=()):
    """One call of slot 14.  pointers[k]: an array, None, or "head" (a buffer of 7s of a mask's size that must stay as it is
    unless k is in `written`).  -> the arrays the call was given."""
    n = len(handles)
    hs = (C.c_void_p * n)(*[None if h is None else h._handle for h in handles])
    p = None if points is None else (C.c_int * (2 * n))(*[v for q in points for v in q])
    r = (C.c_int * (4 * n))(*[v for q in regions for v in q])
    e = seg.extent()
    arrays = [np.full((e.height, e.width), 7, np.uint8) if isinstance(q, str) else q for q in pointers]
    before = [None if a is None else a.copy() for a in arrays]
    ptrs = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrays])
    try:
        api._check(api.api().get_segmentation_masks(hs, n, p, r, ptrs))
    finally:
        for k, (a, b) in enumerate(zip(arrays, before)):
            assert a is None or k in written or np.array_equal(a, b), f"the call wrote entry {k}'s memory"
    return arrays


def test_the_entry_layout_of_the_cpp_wrapper(api, world, pictures):
    """Segmentation::scribble of dlimgedit.hpp with a region, a clean-up, an Edge and a matte: no `points`; the head with its box,
    the stroke mark, the clean-up mark, the edge mark, the matte mark.  And Segmentation::compute_mask with an Edge alone: the
    head with its click and the empty region, then the mark, whose pointer is NULL."""
    _, segs = world
    name = "small"
    seg, picture = segs[name], pictures[name]
    box, guide, stroke = _box(api, name), np.array(picture), _selection(name)
    region = (box.top_left.x, box.top_left.y, box.bottom_right.x, box.bottom_right.y)
    regions = [region, (12, 2, 1, 0), (6, 0, 20, 0), (14, -2, 1, 0), (11, 5, 100, 3)]
    arrays = _raw(api, seg, [seg, None, None, None, None], None, regions, ["head", stroke, None, None, guide], written=(0,))
    # (islands dropped, no hole filled: the clean-up leaves the mask its background, so the shrink has an edge to move)
    edged = seg.scribble(stroke, clicks=2, region=box, clean=(0, 20), edge=(-2, 1, 0))
    cleaned = seg.scribble(stroke, clicks=2, region=box, clean=(0, 20)).copy()
    assert 0 < int((cleaned > 0).sum()) < cleaned.size and _checked("small.cpp_layout", cleaned, edged, (-2, 1, 0)) > 0
    _same("small.cpp_layout.matte", arrays[0], MR.matte(edged, MR.grey(picture), 5, 100)[0])
    c = _click(api, name)[0]
    arrays = _raw(api, seg, [seg, None], [(c.x, c.y), (0, 0)], [EMPTY, (14, 5, 0, 0)], ["head", None], written=(0,))
    _checked("small.cpp_layout_bare", seg.compute_mask_clicks([c]), arrays[0], (5, 0, 0))


def test_refusals_name_the_mark_and_nothing_is_written(api, world, pictures):
    env, segs = world
    seg = segs["small"]
    guide = np.array(pictures["small"])
    a = (250, 220)
    M, E = (11, 5, 0, 3), (14, 2, 0, 0)
    refused = [
        ([seg, None], [EMPTY, (14, 65, 0, 0)], ["head", None], 1, "offset"),
        ([seg, None], [EMPTY, (14, -65, 0, 0)], ["head", None], 1, "offset"),
        ([seg, None], [EMPTY, (14, 1, 33, 0)], ["head", None], 1, "feather"),
        ([seg, None], [EMPTY, (14, 1, 0, -1)], ["head", None], 1, "border"),
        ([seg, None], [EMPTY, (14, 0, 0, 0)], ["head", None], 1, "all 0"),
        ([seg, None, None], [EMPTY, E, E], ["head", None, None], 2, "second"),
        ([None, seg], [E, EMPTY], [None, "head"], 0, "needs a prompt"),
        ([seg, None, None], [EMPTY, E, (1, 0, 0, 0)], ["head", None, None], 1, "in front of entry 2"),
        ([seg, None, None], [EMPTY, E, (6, 9, 9, 0)], ["head", None, None], 1, "in front of entry 2"),
        ([seg, None, None], [EMPTY, M, E], ["head", guide, None], 2, "behind a matte mark"),
        ([seg, None, None], [EMPTY, (7, 4, 0, 0), E], ["head", None, None], 2, "grid prompt"),
    ]
    for handles, regions, pointers, at, why in refused:
        with pytest.raises(api.Error, match=f"entry {at}:.*edge mark.*{why}"):
            _raw(api, seg, handles, [a] * len(handles), regions, pointers)
    # the device form: the same refusals, and nothing is written
    size = guide.shape[0] * guide.shape[1]
    dev = api.ext.device_alloc(env, size)
    try:
        api.ext.copy_to_device(env, dev, np.full(size, 7, np.uint8))
        for handles, regions, _, at, why in refused:
            n = len(handles)
            hs = (C.c_void_p * n)(*[None if h is None else h._handle for h in handles])
            p = (C.c_int * (2 * n))(*(list(a) * n))
            r = (C.c_int * (4 * n))(*[v for q in regions for v in q])
            offsets = (C.c_size_t * n)()
            with pytest.raises(api.Error, match=f"entry {at}:.*edge mark.*{why}"):
                api._check(api.ext._l().dlimg_amd_get_segmentation_masks_device(hs, n, p, r, 0, dev, offsets))
        back = np.zeros(size, np.uint8)
        api.ext.copy_to_host(env, back, dev)
        assert (back == 7).all(), "a refused device call wrote a mask"
    finally:
        api.ext.device_free(env, dev)
    # the wrapper refuses what it can before anything reaches the library, and the handle still serves
    for bad in (0, (0, 0, 0), 65, (1, 33, 0), (1, 0, 33), (1, 2), "3"):
        with pytest.raises(api.Error, match="edge"):
            seg.compute_mask_clicks(_click(api, "small"), edge=bad)
    with pytest.raises(api.Error, match="grid prompt"):
        api.Segmentation.compute_mask_batch([seg], grid=[(4, 0, 0)], edge=[1])
    plain = seg.compute_mask_clicks(_click(api, "small")).copy()
    _checked("small.after_refusals", plain, seg.compute_mask_clicks(_click(api, "small"), edge=(1, 1, 1)), (1, 1, 1))
