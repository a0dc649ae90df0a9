"""Matte marks on the GPU, end to end: a continuation entry {11, radius, eps, channels}, the last of its prompt, whose out_masks
pointer is READ as the guide, makes the prompt deliver its mask as coverage 0 .. 255.  On the parent commit 11 is a refused
label: every test here that sends the mark fails there.

The delivered bytes EQUAL tests/matte_ref.py's matte of the mask the same prompt delivers without the mark, guided by the grey
image: for a click, a box, a prompt with a clean-up mark (the reference taken on the cleaned mask), a lasso prompt and a prior
refined in place, each with the caller's own buffers and with guide and result in create_image memory; a batch equals its single
calls; eps 0 is eps 650; the refusals arrive through slot 14 and the device form and nothing is written.

The synthetic ViT-B model of `model_dirs` serves everything but the prior, which needs the mask branch: that runs on a vit_test
model written with it.  Images: 1024 x 683 RGBA and 600 x 400 RGB.
"""
import ctypes as C

import numpy as np
import pytest

import matte_ref as MR
from conftest import synthetic_image

pytestmark = pytest.mark.gpu
EMPTY = (0, 0, -1, -1)
IMAGES = {"wide": (3, 1024, 683, 4), "small": (5, 600, 400, 3)}
MATTES = {"wide": (8, 0), "small": (5, 100)}          # (radius, eps) used for the image


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


@pytest.fixture(scope="module")
def pictures():
    out = {n: synthetic_image(seed, w, h, c) for n, (seed, w, h, c) in IMAGES.items()}
    for a in out.values():
        a.setflags(write=False)
    return out


def _process(api, env, pictures):
    return {n: api.Segmentation.process(api.ImageView(a, api.Channels.rgba if a.shape[2] == 4 else api.Channels.rgb), env)
            for n, a in pictures.items()}


@pytest.fixture(scope="module")
def world(api, model_dirs, pictures):
    mdir, _, _ = model_dirs("vit_b")
    env = api.Environment(api.Options(api.Backend.gpu, mdir))
    segs = _process(api, env, pictures)
    yield env, segs
    for s in segs.values():
        s.close()
    env.close()


@pytest.fixture(scope="module")
def branch_world(api, tmp_path_factory, pictures):
    """a model WITH the prompt encoder's mask branch, for the prior"""
    from dlimgedit_amd import weights as W
    from dlimgedit_amd.sam_config import get_config
    mdir = tmp_path_factory.mktemp("models_vit_test_matte")
    W.write_synthetic_model_dir(mdir, get_config("vit_test"), 7, mask_branch=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    segs = _process(api, env, pictures)
    yield env, segs
    for s in segs.values():
        s.close()
    env.close()


def _click(api, name):
    _, w, h, _ = IMAGES[name]
    return [api.Point(int(0.42 * w), int(0.55 * h))]


def _box(api, name):
    _, w, h, _ = IMAGES[name]
    return api.Region(api.Point(int(0.2 * w), int(0.25 * h)), api.Point(int(0.7 * w), int(0.8 * h)))


def _selection(name):
    _, w, h, _ = IMAGES[name]
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx - 0.5 * w) / (0.25 * w)) ** 2 + ((yy - 0.45 * h) / (0.3 * h)) ** 2 <= 1, 255, 0).astype(np.uint8)


def _table_copy(api, a):
    """the array in memory from create_image, as the reference's wrapper would hold it"""
    h, w = a.shape[:2]
    ch = {1: api.Channels.mask, 3: api.Channels.rgb, 4: api.Channels.rgba}[1 if a.ndim == 2 else a.shape[2]]
    px = api.Image(api.Extent(w, h), ch).pixels()
    px = px.reshape(a.shape)
    px[...] = a
    assert api.ext.image_memory_is_pinned(px)
    return px


def _want(plain, picture, radius, eps):
    return MR.matte(plain, MR.grey(picture), radius, eps or MR.DEFAULT_EPS)[0]


def _report(what, plain, got):
    soft = int(((got > 0) & (got < 255)).sum())
    print(f"matte.e2e.{what}: mask {float((plain > 0).mean()):.3f} covered, {soft} soft pixels of {got.size}")
    return soft


def _both_memories(api, picture, run, plain, what, radius, eps):
    """run(guide, out) -> delivered: with the caller's own buffers, then with guide and result in create_image memory"""
    assert set(np.unique(plain)) <= {0, 255}
    want = _want(plain, picture, radius, eps)
    own = np.full(plain.shape, 7, np.uint8)
    got = run(np.array(picture), own)
    assert got is own and np.array_equal(got, want), (what, int((got != want).sum()))
    guide, out = _table_copy(api, picture), api._mask_image(api.Extent(plain.shape[1], plain.shape[0]))
    got = run(guide, out)
    assert np.array_equal(got, want), (what, "table memory", int((got != want).sum()))
    assert np.array_equal(guide, picture)                     # the call only reads it
    return _report(what, plain, got)


@pytest.mark.parametrize("name", list(IMAGES))
def test_click_box_and_cleaned_prompts(api, world, pictures, name):
    _, segs = world
    seg, picture, (radius, eps) = segs[name], pictures[name], MATTES[name]
    soft = 0
    plain = seg.compute_mask_clicks(_click(api, name)).copy()
    soft += _both_memories(api, picture, lambda g, o: seg.compute_mask_clicks(_click(api, name), out=o, matte=(g, radius, eps)), plain,
                           f"{name}.click", radius, eps)
    plain = api.Segmentation.compute_mask_batch([seg], regions=[_box(api, name)])[0].copy()
    soft += _both_memories(api, picture, lambda g, o: api.Segmentation.compute_mask_batch([seg], regions=[_box(api, name)], out=[o],
                                                                                         matte=[(g, radius, eps)])[0],
                           plain, f"{name}.box", radius, eps)
    clean = (400, 400)
    cleaned = seg.compute_mask_clicks(_click(api, name), region=_box(api, name), clean=clean).copy()
    soft += _both_memories(api, picture, lambda g, o: seg.compute_mask_clicks(_click(api, name), region=_box(api, name), out=o, clean=clean,
                                                                             matte=(g, radius, eps)),
                           cleaned, f"{name}.cleaned", radius, eps)
    assert soft > 0, "no prompt of this image delivered a mask with an edge: the matte was never more than a copy"


@pytest.mark.parametrize("name", list(IMAGES))
def test_lasso_prompt(api, world, pictures, name):
    _, segs = world
    seg, picture, (radius, eps) = segs[name], pictures[name], MATTES[name]
    sel = _selection(name)
    what = api.LASSO_BOX | api.LASSO_CLICK               # (the mask bit needs the mask branch, which this model file lacks)
    plain = seg.snap_selection(sel, what=what).copy()
    soft = _both_memories(api, picture, lambda g, o: seg.snap_selection(sel, what=what, out=o, matte=(g, radius, eps)), plain,
                          f"{name}.lasso", radius, eps)
    assert soft > 0, "the mask has no edge: the matte was no more than a copy"


@pytest.mark.parametrize("name", list(IMAGES))
def test_a_prior_refined_in_place(api, branch_world, pictures, name):
    _, segs = branch_world
    seg, picture, (radius, eps) = segs[name], pictures[name], MATTES[name]
    prior = _selection(name)
    plain = seg.compute_mask_clicks(_click(api, name), prior=prior).copy()
    want = _want(plain, picture, radius, eps)
    own = prior.copy()                                        # the prior is the memory the matte goes to
    got = seg.compute_mask_clicks(_click(api, name), out=own, prior=own, matte=(np.array(picture), radius, eps))
    assert got is own and np.array_equal(own, want), int((own != want).sum())
    table, guide = api._mask_image(seg.extent()), _table_copy(api, picture)
    table[...] = prior
    got = seg.compute_mask_clicks(_click(api, name), out=table, prior=table, matte=(guide, radius, eps))
    assert np.array_equal(got, want), int((got != want).sum())
    assert _report(f"{name}.prior", plain, got) > 0, "the mask has no edge: the matte was no more than a copy"
    # refinement marks in front of it: the matte is that of the last stage's mask
    two = _click(api, name) + [api.Point(5, 5)]
    staged = seg.compute_mask_clicks(two, [1, 0], refine_after="each").copy()
    got = seg.compute_mask_clicks(two, [1, 0], refine_after="each", matte=(np.array(picture), radius, eps))
    assert np.array_equal(got, _want(staged, picture, radius, eps))


def test_a_batch_equals_its_single_calls(api, world, pictures):
    _, segs = world
    a, b = segs["wide"], segs["small"]
    singles = [a.compute_mask_clicks(_click(api, "wide"), matte=(np.array(pictures["wide"]), 8, 0)).copy(),
               b.compute_mask_clicks(_click(api, "small"), matte=(np.array(pictures["small"]), 5, 100)).copy(),
               a.compute_mask_clicks(_click(api, "wide")).copy()]
    got = api.Segmentation.compute_mask_batch([a, b, a], clicks=[_click(api, "wide"), _click(api, "small"), _click(api, "wide")],
                                              matte=[(np.array(pictures["wide"]), 8, 0), (np.array(pictures["small"]), 5, 100), None])
    for j in range(3):
        assert np.array_equal(got[j], singles[j]), j
    assert set(np.unique(got[2])) <= {0, 255}                 # the plain prompt's mask is still 0 / 255
    # the `points` form, the plain prompt first
    got = api.Segmentation.compute_mask_batch([a, b], points=[_click(api, "wide")[0], _click(api, "small")[0]],
                                              matte=[None, (np.array(pictures["small"]), 5, 100)])
    assert np.array_equal(got[0], singles[2]) and np.array_equal(got[1], singles[1])


def test_eps_zero_is_the_default(api, world, pictures):
    _, segs = world
    seg, picture = segs["small"], np.array(pictures["small"])
    zero = seg.compute_mask_clicks(_click(api, "small"), region=_box(api, "small"), matte=(picture, 6, 0)).copy()
    spelt = seg.compute_mask_clicks(_click(api, "small"), region=_box(api, "small"), matte=(picture, 6, api.MATTE_DEFAULT_EPS))
    assert api.MATTE_DEFAULT_EPS == 650 and np.array_equal(zero, spelt)


def _raw(api, seg, handles, points, regions, guide_at=(), guide=None):
    n = len(handles)
    hs = (C.c_void_p * n)(*[None if h is None else h._handle for h in handles])
    p = None if points is None else (C.c_int * (2 * n))(*[v for q in points for v in q])
    r = (C.c_int * (4 * n))(*[v for q in regions for v in q])
    outs = [np.full((seg.extent().height, seg.extent().width), 7, np.uint8) for _ in range(n)]
    ptrs = (C.c_void_p * n)(*[o.ctypes.data if h is not None else (guide.ctypes.data if k in guide_at else None)
                              for k, (o, h) in enumerate(zip(outs, handles))])
    try:
        api._check(api.api().get_segmentation_masks(hs, n, p, r, ptrs))
    finally:
        assert all((o == 7).all() for o in outs), "a refused call wrote a mask"
    return outs


def test_refusals_name_the_mark_and_nothing_is_written(api, world, pictures):
    env, segs = world
    seg, guide = segs["small"], np.array(pictures["small"])
    a = (250, 220)
    M = (11, 5, 0, 3)
    refused = [
        ([None, seg], [a, a], [M, EMPTY], (0,), 0),                                            # in front of any head
        ([seg, None, None], [a, a, a], [EMPTY, M, (1, 0, 0, 0)], (1,), 1),                     # not the last entry of its prompt
        ([seg, None, None], [a, a, a], [EMPTY, M, (6, 9, 9, 0)], (1,), 1),                     # in front of the clean-up mark
        ([seg, None, None], [a, a, a], [EMPTY, M, M], (1, 2), 2),                              # a second one
        ([seg, None], [a, a], [EMPTY, M], (), 1),                                              # a NULL guide
        ([seg, None], [a, a], [EMPTY, (11, 0, 0, 3)], (1,), 1),                                # radius
        ([seg, None], [a, a], [EMPTY, (11, 33, 0, 3)], (1,), 1),
        ([seg, None], [a, a], [EMPTY, (11, 5, -1, 3)], (1,), 1),                               # eps
        ([seg, None], [a, a], [EMPTY, (11, 5, 65026, 3)], (1,), 1),
        ([seg, None], [a, a], [EMPTY, (11, 5, 0, 2)], (1,), 1),                                # channels
        ([seg, None, None], [a, a, a], [EMPTY, (7, 4, 0, 0), M], (2,), 2),                     # a grid prompt
    ]
    for handles, points, regions, guide_at, at in refused:
        with pytest.raises(api.Error, match=f"entry {at}:.*matte mark"):
            _raw(api, seg, handles, points, regions, guide_at, guide)
    # the device form has no per-entry pointer to read a guide from
    size = guide.shape[0] * guide.shape[1]
    dev = api.ext.device_alloc(env, size)
    try:
        api.ext.copy_to_device(env, dev, np.full(size, 7, np.uint8))
        hs = (C.c_void_p * 2)(seg._handle, None)
        p = (C.c_int * 4)(*a, 0, 0)
        r = (C.c_int * 8)(*EMPTY, *M)
        offsets = (C.c_size_t * 2)()
        with pytest.raises(api.Error, match=r"entry 1:.*matte mark.*dlimg_amd_get_segmentation_masks_device"):
            api._check(api.ext._l().dlimg_amd_get_segmentation_masks_device(hs, 2, p, r, 0, dev, offsets))
        back = np.zeros(size, np.uint8)
        api.ext.copy_to_host(env, back, dev)
        assert (back == 7).all(), "the refused device call wrote a mask"
    finally:
        api.ext.device_free(env, dev)
    # the wrapper refuses a guide of another extent before anything reaches the library, and the handle still serves
    with pytest.raises(api.Error, match="matte"):
        seg.compute_mask_clicks(_click(api, "small"), matte=(np.zeros((300, 400, 3), np.uint8), 5, 0))
    plain = seg.compute_mask_clicks(_click(api, "small"))
    got =seg.compute_mask_clicks(_click(api, "small"), matte=(guide, 5, 100))
    assert np.array_equal(got, _want(plain, guide, 5, 100))


def test_hq_model_serves_a_matte(api, tmp_path_factory):
    import hq_cases as H
    from dlimgedit_amd import weights as W
    mdir = tmp_path_factory.mktemp("models_hqtest_matte")
    W.write_synthetic_model_dir(mdir, H.CFG, H.SEED, mask_branch=True, hq=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    img = H.image("square")
    seg = api.Segmentation.process(api.ImageView(img, api.Channels.rgba), env)
    try:
        h, w = img.shape[:2]
        pts = [api.Point(int(0.4 * w), int(0.5 * h))]
        plain = seg.compute_mask_clicks(pts).copy()
        got = seg.compute_mask_clicks(pts, matte=(np.ascontiguousarray(img), 8, 0))
        assert np.array_equal(got, _want(plain, img, 8, 0))
        assert _report("hq.click", plain, got) > 0, "the mask has no edge: the matte was no more than a copy"
    finally:
        seg.close()
        env.close()
