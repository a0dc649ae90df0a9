"""Cut-out marks on the GPU, end to end: a continuation entry {13, radius, 0, 0} directly behind the matte mark of its prompt,
whose out_masks pointer is WRITTEN with height * width * 4 bytes: the image's foreground colours and the coverage.  On the parent
commit 13 is a refused label: every test here that sends the mark fails there.

The head's coverage EQUALS what the same call delivers without the mark, and the RGBA EQUALS tests/cutout_ref.py applied to
(guide, that coverage, radius): for a click, a box, a lasso and a scribble, with clean-up, refinement and stroke marks in front,
with the caller's own buffers and with guide and results in create_image memory, in place on a 4-channel guide, for BGRA input,
two prompts in one call, the entry layout the C++ wrapper sends, and a SAM-HQ model file; radius 0 is radius 16; the refusals
arrive through slot 14 and the device form and nothing is written.

A vit_test model written with the mask branch serves everything but the SAM-HQ case.  Images: test_gpu_matte.py's, 1024 x 683
RGBA and 600 x 400 RGB."""
import ctypes as C

import numpy as np
import pytest

import cutout_ref as CR
from test_gpu_matte import IMAGES, _box, _click, _process, _selection, _table_copy, pictures  # noqa: F401  (pictures: a fixture)

pytestmark = pytest.mark.gpu
EMPTY = (0, 0, -1, -1)
MATTES = {"wide": (8, 0), "small": (5, 100)}          # (radius, eps) of the matte used for the image
CUTS = {"wide": 16, "small": 6}                       # radius of the cut-out


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


@pytest.fixture(scope="module")
def world(api, tmp_path_factory, pictures):
    """a model WITH the prompt encoder's mask branch, for the refinement marks"""
    from dlimgedit_amd import weights as W
    from dlimgedit_amd.sam_config import get_config
    mdir = tmp_path_factory.mktemp("models_vit_test_cutout")
    W.write_synthetic_model_dir(mdir, get_config("vit_test"), 7, mask_branch=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    segs = _process(api, env, pictures)
    yield env, segs
    for s in segs.values():
        s.close()
    env.close()


def _rgba_of(picture):
    """the picture as 4 channels (a fourth of its own when it has three)"""
    if picture.shape[2] == 4:
        return np.array(picture)
    return np.ascontiguousarray(np.dstack([picture, np.full(picture.shape[:2], 99, np.uint8)]))


def _checked(what, picture, coverage, rgba, radius):
    want = CR.cutout(picture, coverage, radius or CR.DEFAULT_RADIUS)
    diff = rgba != want
    assert not diff.any(), (what, int(diff.sum()), tuple(np.argwhere(diff)[0]))
    soft = int(((coverage > 0) & (coverage < 255)).sum())
    changed = int((rgba[:, :, :3] != picture[:, :, :3]).any(axis=2).sum())
    print(f"cutout.e2e.{what}: {soft} soft pixels, {changed} pixels decontaminated of {coverage.size}")
    return changed


@pytest.mark.parametrize("name", list(IMAGES))
def test_click_box_lasso_and_scribble(api, world, pictures, name):
    _, segs = world
    seg, picture, (mr, eps), r = segs[name], pictures[name], MATTES[name], CUTS[name]
    guide = np.array(picture)
    calls = {
        "click": lambda **k: seg.compute_mask_clicks(_click(api, name), **k),
        "box": lambda **k: api.Segmentation.compute_mask_batch([seg], regions=[_box(api, name)], **{a: [v] for a, v in k.items()})[0],
        "lasso": lambda **k: seg.snap_selection(_selection(name), what=api.LASSO_BOX | api.LASSO_CLICK, **k),
        "scribble": lambda **k: seg.scribble(_selection(name), clicks=2, **k),
    }
    soft = 0
    for what, call in calls.items():
        coverage = call(matte=(guide, mr, eps)).copy()
        got, rgba = call(matte=(guide, mr, eps), cutout=r)
        assert np.array_equal(got, coverage), f"{what}: the head's coverage changed with the cut-out mark"
        assert np.array_equal(guide, picture)
        soft += _checked(f"{name}.{what}", picture, coverage, rgba, r)
    assert soft > 0, "no prompt of this image delivered a coverage with a soft edge: the cut-out was never more than a copy"


def test_radius_zero_is_sixteen_and_bgra_keeps_its_order(api, world, pictures):
    _, segs = world
    seg, picture = segs["wide"], pictures["wide"]
    guide = np.array(picture)
    cov, zero = seg.compute_mask_clicks(_click(api, "wide"), matte=(guide, 8, 0), cutout=0)
    _, spelt = seg.compute_mask_clicks(_click(api, "wide"), matte=(guide, 8, 0), cutout=16)
    assert api.CUTOUT_DEFAULT_RADIUS == 16 and np.array_equal(zero, spelt)
    _checked("wide.radius0", picture, cov, zero, 16)
    # the same picture with its first and third channel swapped: the same matte (a grey guide), the colours in the order given
    bgra = np.ascontiguousarray(guide[:, :, [2, 1, 0, 3]])
    cov2, swapped = seg.compute_mask_clicks(_click(api, "wide"), matte=(bgra, 8, 0), cutout=16)
    assert np.array_equal(cov2, cov) and np.array_equal(swapped, spelt[:, :, [2, 1, 0, 3]])


@pytest.mark.parametrize("name", list(IMAGES))
def test_in_place_and_table_memory_equal_the_callers_own_buffer(api, world, pictures, name):
    _, segs = world
    seg, picture, (mr, eps), r = segs[name], pictures[name], MATTES[name], CUTS[name]
    four = _rgba_of(picture)
    guide = four.copy()
    own = np.full(four.shape, 7, np.uint8)
    cov, rgba = seg.compute_mask_clicks(_click(api, name), region=_box(api, name), matte=(guide, mr, eps), cutout=(r, own))
    assert rgba is own and np.array_equal(guide, four)
    _checked(f"{name}.own", four, cov, own, r)
    # in place: the mark's pointer is the guide itself, whose fourth byte becomes the coverage
    cov2, rgba = seg.compute_mask_clicks(_click(api, name), region=_box(api, name), matte=(guide, mr, eps), cutout=(r, guide))
    assert rgba is guide and np.array_equal(cov2, cov) and np.array_equal(guide, own)
    # guide, coverage and RGBA in memory from create_image; then in place there too
    table, out, dst = _table_copy(api, four), api._mask_image(seg.extent()), _table_copy(api, np.zeros_like(four))
    cov3, rgba = seg.compute_mask_clicks(_click(api, name), region=_box(api, name), out=out, matte=(table, mr, eps), cutout=(r, dst))
    assert np.array_equal(cov3, cov) and np.array_equal(dst, own) and np.array_equal(table, four)
    seg.compute_mask_clicks(_click(api, name), region=_box(api, name), out=out, matte=(table, mr, eps), cutout=(r, table))
    assert np.array_equal(out, cov) and np.array_equal(table, own)
    # pinned destination, guide in the caller's own memory, and the other way round
    dst[...] = 0
    seg.compute_mask_clicks(_click(api, name), region=_box(api, name), matte=(four.copy(), mr, eps), cutout=(r, dst))
    assert np.array_equal(dst, own)
    if picture.shape[2] == 3:       # a 3-channel guide: the destination is never the guide
        cov4, rgba = seg.compute_mask_clicks(_click(api, name), region=_box(api, name), matte=(np.array(picture), mr, eps), cutout=r)
        assert np.array_equal(cov4, cov) and np.array_equal(rgba, own)


def test_cleanup_refinement_and_stroke_marks_in_front(api, world, pictures):
    _, segs = world
    name = "small"
    seg, picture, (mr, eps), r = segs[name], pictures[name], MATTES[name], CUTS[name]
    guide = np.array(picture)
    two = _click(api, name) + [api.Point(5, 5)]
    stroke = [(_selection(name), 1, 2)]
    args = dict(labels=[1, 0], refine_after="each", clean=(400, 400), strokes=stroke)
    coverage = seg.compute_mask_clicks(two, matte=(guide, mr, eps), **args).copy()
    got, rgba = seg.compute_mask_clicks(two, matte=(guide, mr, eps), cutout=r, **args)
    assert np.array_equal(got, coverage)
    _checked("small.everything_in_front", picture, coverage, rgba, r)


def test_two_prompts_of_which_one_has_a_cutout(api, world, pictures):
    _, segs = world
    a, b = segs["wide"], segs["small"]
    ga, gb = np.array(pictures["wide"]), np.array(pictures["small"])
    singles = [a.compute_mask_clicks(_click(api, "wide"), matte=(ga, 8, 0)).copy(), b.compute_mask_clicks(_click(api, "small")).copy(),
               b.compute_mask_clicks(_click(api, "small"), matte=(gb, 5, 100)).copy()]
    got = api.Segmentation.compute_mask_batch([a, b, b], clicks=[_click(api, "wide"), _click(api, "small"), _click(api, "small")],
                                              matte=[(ga, 8, 0), None, (gb, 5, 100)], cutout=[None, None, 6])
    assert np.array_equal(got[0], singles[0]) and np.array_equal(got[1], singles[1]) and set(np.unique(got[1])) <= {0, 255}
    assert np.array_equal(got[2][0], singles[2])
    _checked("batch.third", pictures["small"], singles[2], got[2][1], 6)
    # the `points` form, the prompt with the cut-out first
    got = api.Segmentation.compute_mask_batch([a, b], points=[_click(api, "wide")[0], _click(api, "small")[0]],
                                              matte=[(ga, 8, 0), None], cutout=[(16, None), None])
    assert np.array_equal(got[0][0], singles[0]) and np.array_equal(got[1], singles[1])
    _checked("batch.points_form", pictures["wide"], singles[0], got[0][1], 16)


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
    """Segmentation::scribble of dlimgedit.hpp with a region, a clean-up, a matte and a cut-out: no `points`; the head with its
    box, the stroke mark, then the marks that stay last."""
    _, segs = world
    name = "small"
    seg, picture, (mr, eps), r = segs[name], pictures[name], MATTES[name], CUTS[name]
    box, guide, stroke = _box(api, name), np.array(picture), _selection(name)
    region = (box.top_left.x, box.top_left.y, box.bottom_right.x, box.bottom_right.y)
    h, w = guide.shape[:2]
    dst = np.full((h, w, 4), 7, np.uint8)
    regions = [region, (12, 2, 1, 0), (6, 300, 300, 0), (11, mr, eps, 3), (13, r, 0, 0)]
    arrays = _raw(api, seg, [seg, None, None, None, None], None, regions, ["head", stroke, None, guide, dst], written=(0, 4))
    want = seg.scribble(stroke, clicks=2, region=box, clean=(300, 300), matte=(guide, mr, eps))
    assert np.array_equal(arrays[0], want)
    changed = _checked("small.cpp_layout", picture, want, dst, r)
    # ... and without region and clean-up: the head with the empty region, the stroke mark, the matte mark, the cut-out mark
    arrays = _raw(api, seg, [seg, None, None, None], None, [EMPTY, (12, 2, 1, 0), (11, mr, eps, 3), (13, r, 0, 0)],
                  ["head", stroke, guide, dst], written=(0, 3))
    want = seg.scribble(stroke, clicks=2, matte=(guide, mr, eps))
    assert np.array_equal(arrays[0], want)
    changed += _checked("small.cpp_layout_bare", picture, want, dst, r)
    assert changed > 0, "neither call delivered a coverage with a soft edge: the cut-out was never more than a copy"


def test_refusals_name_the_mark_and_nothing_is_written(api, world, pictures):
    env, segs = world
    seg = segs["small"]
    guide = _rgba_of(pictures["small"])
    grey = np.ascontiguousarray(guide[:, :, 1])
    dst = np.full(guide.shape, 7, np.uint8)
    a = (250, 220)
    M, M1, K = (11, 5, 0, 4), (11, 5, 0, 1), (13, 6, 0, 0)
    refused = [
        ([seg, None], [EMPTY, K], ["head", dst], 1),                                           # not directly behind a matte mark
        ([seg, None, None, None], [EMPTY, M, (6, 9, 9, 0), K], ["head", guide, None, dst], 3),
        ([seg, None, None, None], [EMPTY, M, K, (1, 0, 0, 0)], ["head", guide, dst, None], 2),   # not the last entry of its prompt
        ([seg, None, None, None], [EMPTY, M, K, K], ["head", guide, dst, dst.copy()], 3),       # a second one
        ([seg, None, None], [EMPTY, M1, K], ["head", grey, dst], 2),                            # a guide of one channel
        ([seg, None, None], [EMPTY, M, K], ["head", guide, None], 2),                           # a NULL pointer
        ([seg, None, None], [EMPTY, M, (13, 33, 0, 0)], ["head", guide, dst], 2),               # radius
        ([seg, None, None], [EMPTY, M, (13, -1, 0, 0)], ["head", guide, dst], 2),
        ([seg, None, None], [EMPTY, M, (13, 6, 1, 0)], ["head", guide, dst], 2),                # trailing ints
        ([seg, None, None], [EMPTY, M, (13, 6, 0, 1)], ["head", guide, dst], 2),
        ([None, None, seg], [M, K, EMPTY], [guide, dst, "head"], 1),                            # in front of any head
    ]
    for handles, regions, pointers, at in refused:
        with pytest.raises(api.Error, match=f"entry {at}:.*cut-out mark"):
            _raw(api, seg, handles, [a] * len(handles), regions, pointers)
    # a pointer equal to out_masks[head]
    head = np.full(guide.shape, 7, np.uint8)
    with pytest.raises(api.Error, match="entry 2:.*cut-out mark.*head"):
        _raw(api, seg, [seg, None, None], [a] * 3, [EMPTY, M, K], [head, guide, head])
    # a grid prompt is refused through its matte
    with pytest.raises(api.Error, match="entry 2:.*matte mark.*grid"):
        _raw(api, seg, [seg, None, None, None], [a] * 4, [EMPTY, (7, 4, 0, 0), M, K], ["head", None, guide, dst])
    # the device form has no per-entry pointer to write to
    size = guide.shape[0] * guide.shape[1]
    dev = api.ext.device_alloc(env, size)
    try:
        api.ext.copy_to_device(env, dev, np.full(size, 7, np.uint8))
        hs = (C.c_void_p * 3)(seg._handle, None, None)
        p = (C.c_int * 6)(*a, 0, 0, 0, 0)
        r = (C.c_int * 12)(*EMPTY, *M, *K)
        offsets = (C.c_size_t * 3)()
        with pytest.raises(api.Error, match=r"entry 2:.*cut-out mark.*dlimg_amd_get_segmentation_masks_device"):
            api._check(api.ext._l().dlimg_amd_get_segmentation_masks_device(hs, 3, p, r, 0, dev, offsets))
        back = np.zeros(size, np.uint8)
        api.ext.copy_to_host(env, back, dev)
        assert (back == 7).all(), "the refused device call wrote a mask"
    finally:
        api.ext.device_free(env, dev)
    # the wrapper refuses what it can before anything reaches the library, and the handle still serves
    for bad in (dict(cutout=6), dict(matte=(grey, 5, 0), cutout=6), dict(matte=(guide, 5, 0), cutout=33),
                dict(matte=(guide, 5, 0), cutout=(6, np.zeros((3, 3, 4), np.uint8)))):
        with pytest.raises(api.Error, match="cutout"):
            seg.compute_mask_clicks(_click(api, "small"), **bad)
    cov, rgba = seg.compute_mask_clicks(_click(api, "small"), matte=(guide, 5, 100), cutout=6)
    assert np.array_equal(rgba, CR.cutout(guide, cov, 6))


def test_hq_model_serves_a_cutout(api, tmp_path_factory):
    import hq_cases as H
    from dlimgedit_amd import weights as W
    mdir = tmp_path_factory.mktemp("models_hqtest_cutout")
    W.write_synthetic_model_dir(mdir, H.CFG, H.SEED, mask_branch=True, hq=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    img = np.ascontiguousarray(H.image("square"))
    seg = api.Segmentation.process(api.ImageView(img, api.Channels.rgba), env)
    try:
        h, w = img.shape[:2]
        pts = [api.Point(int(0.4 * w), int(0.5 * h))]
        coverage = seg.compute_mask_clicks(pts, matte=(img, 8, 0)).copy()
        got, rgba = seg.compute_mask_clicks(pts, matte=(img, 8, 0), cutout=0)
        assert np.array_equal(got, coverage)
        _checked("hq.click", img, coverage, rgba, 16)
    finally:
        seg.close()
        env.close()
