"""Stroke marks on the GPU: a continuation entry {12, clicks, label, 0} stands for `clicks` clicks of its label that are sampled from a
scribble the caller holds -- out_masks[] of the mark is READ -- on the GPU (kernels/mask_stroke.hip).  On the parent commit 12 is
a refused label: every test here that sends the mark fails there.

The yardstick is the library's own explicit path.  The mask delivered for a prompt with stroke marks is BYTE-EQUAL to the mask
delivered for the same call with every mark replaced by explicit click entries at tests/stroke_ref.py's pixels: both run the same
kernels on the same arguments, so there is no tolerance.

* a foreground stroke alone (no points, no box); foreground and background strokes with a box, in both orders; a head point and
  a background stroke; stroke, refinement mark, stroke; a lasso mark followed by a stroke mark; clean-up and matte marks behind
  strokes; a SAM-HQ file at its limit; two stroke prompts on images of different extent beside a plain prompt in one call; the map
  in the table's pinned image memory;
* every refusal says "mark", names the caller's entry and leaves the handle working; the empty stroke names its entry and leaves
  the head's buffer untouched; the device form refuses by name.
"""
import ctypes as C

import numpy as np
import pytest

import lasso_cases as LC
import stroke_ref as SR

pytestmark = pytest.mark.gpu

EMPTY = (0, 0, -1, -1)
BOX = {"square": (257, 264, 580, 567), "wide": (150, 30, 520, 400)}


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


@pytest.fixture(scope="module")
def world(api, tmp_path_factory):
    """(env, {image name: Segmentation}); a model WITH the mask branch"""
    from dlimgedit_amd import weights as W
    from dlimgedit_amd.sam_config import get_config
    mdir = tmp_path_factory.mktemp("models_vit_test_stroke")
    W.write_synthetic_model_dir(mdir, get_config("vit_test"), 7, mask_branch=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    segs = {n: api.Segmentation.process(api.ImageView(LC.image(n), api.Channels.rgba), env) for n in LC.IMAGES}
    yield env, segs
    for s in segs.values():
        s.close()
    env.close()


def scribble(w: int, h: int, path, value: int = 255) -> np.ndarray:
    """a polyline three pixels thick through `path` (fractions of the extent), drawn point by point"""
    m = np.zeros((h, w), np.uint8)
    for (ax, ay), (bx, by) in zip(path, path[1:]):
        for t in np.linspace(0.0, 1.0, 2 * max(w, h)):
            x, y = int((ax + t * (bx - ax)) * (w - 1)), int((ay + t * (by - ay)) * (h - 1))
            m[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = value
    return m


@pytest.fixture(scope="module")
def strokes():
    """image name -> (foreground map, background map), drawn once and never written"""
    out = {}
    for n, (_, w, h) in LC.IMAGES.items():
        fg = scribble(w, h, [(0.25, 0.3), (0.45, 0.55), (0.6, 0.35)])
        bg = scribble(w, h, [(0.05, 0.9), (0.5, 0.95), (0.95, 0.8)], 128)
        fg.setflags(write=False)
        bg.setflags(write=False)
        out[n] = (fg, bg)
    return out


def _pts(api, clicks):
    return [api.Point(int(x), int(y)) for x, y in clicks]


def _region(api, box):
    return None if box is None else api.Region(api.Point(box[0], box[1]), api.Point(box[2], box[3]))


def stood_for(marks, given=(), given_labels=()):
    """(clicks, labels) of the prompt the marks [(map, label, clicks)] stand for behind the clicks given: stroke_ref's pixels in
    the marks' order -- without clicks given, the first foreground one first."""
    clicks, labels = list(given), list(given_labels)
    for m, label, n in marks:
        pixels = SR.derive(m, n)
        assert len(pixels) == (n or 3)
        clicks += pixels
        labels += [label] * len(pixels)
    if not given:
        first = labels.index(1)
        clicks.insert(0, clicks.pop(first))
        labels.insert(0, labels.pop(first))
    return clicks, labels


def _raw(api, seg, handles, points, regions, ptrs, outs=None):
    """Slot 14 with hand-made arrays.  ptrs: per entry None, or the array whose memory is out_masks[i]; a head's None: a new mask."""
    n = len(handles)
    e = seg.extent()
    outs = {} if outs is None else outs
    mem = []
    for k, (h, q) in enumerate(zip(handles, ptrs)):
        if h is not None and q is None:
            q = outs.setdefault(k, np.zeros((e.height, e.width), np.uint8))
        mem.append(q)
    hs = (C.c_void_p * n)(*[None if h is None else h._handle for h in handles])
    p = None if points is None else (C.c_int * (2 * n))(*[int(v) for q in points for v in q])
    r = (C.c_int * (4 * n))(*[int(v) for q in regions for v in q])
    api._check(api.api().get_segmentation_masks(hs, n, p, r, (C.c_void_p * n)(*[None if q is None else q.ctypes.data for q in mem])))
    return [q for h, q in zip(handles, mem) if h is not None]


@pytest.mark.parametrize("name", list(LC.IMAGES))
def test_a_foreground_stroke_alone(api, world, strokes, name):
    _, segs = world
    fg, _ = strokes[name]
    for n in (0, 1, 5):
        clicks, labels = stood_for([(fg, 1, n)])
        want = segs[name].compute_mask_clicks(_pts(api, clicks), labels)
        got = segs[name].scribble(fg, clicks=n)
        print(f"stroke.e2e.{name}.fg{n}: clicks {clicks}, {int((got > 0).sum())} pixels set, {int((got != want).sum())} differ")
        assert set(np.unique(got)) <= {0, 255} and (got > 0).any()
        assert np.array_equal(got, want)
        # slot 14 raw, without `points`: the same bytes
        raw = _raw(api, segs[name], [segs[name], None], None, [EMPTY, (12, n, 1, 0)], [None, fg])[0]
        assert np.array_equal(raw, want)
    assert not np.array_equal(segs[name].scribble(fg, clicks=1), segs[name].scribble(fg, clicks=5))


@pytest.mark.parametrize("name", list(LC.IMAGES))
def test_foreground_and_background_strokes_with_a_box(api, world, strokes, name):
    _, segs = world
    seg = segs[name]
    fg, bg = strokes[name]
    box = _region(api, BOX[name])
    clicks, labels = stood_for([(fg, 1, 2), (bg, 0, 2)])
    assert labels == [1, 1, 0, 0]
    want = seg.compute_mask_clicks(_pts(api, clicks), labels, box)
    assert np.array_equal(seg.scribble(fg, bg, clicks=2, region=box), want)
    assert not np.array_equal(want, seg.compute_mask_clicks(_pts(api, clicks[:2]), labels[:2], box))      # the background clicks count
    # the background stroke first: the head's click is the first FOREGROUND click, the others keep their order
    clicks, labels = stood_for([(bg, 0, 2), (fg, 1, 3)])
    assert labels == [1, 0, 0, 1, 1]
    want = seg.compute_mask_clicks(_pts(api, clicks), labels, box)
    got = _raw(api, seg, [seg, None, None], None, [BOX[name], (12, 2, 0, 0), (12, 3, 1, 0)], [None, bg, fg])[0]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", list(LC.IMAGES))
def test_a_head_point_and_a_background_stroke(api, world, strokes, name):
    _, segs = world
    seg = segs[name]
    _, bg = strokes[name]
    head = [LC.EXTRA_CLICKS[name][0][0]]
    clicks, labels = stood_for([(bg, 0, 0)], head, [1])
    assert labels == [1, 0, 0, 0] and clicks[0] == head[0]
    want = seg.compute_mask_clicks(_pts(api, clicks), labels)
    assert np.array_equal(seg.compute_mask_clicks(_pts(api, head), strokes=[(bg, 0, 0)]), want)
    assert not np.array_equal(want, seg.compute_mask_clicks(_pts(api, head)))
    # the mark's point is not read
    got = _raw(api, seg, [seg, None], [head[0], (-77, 123456)], [EMPTY, (12, 0, 0, 0)], [None, bg])[0]
    assert np.array_equal(got, want)


def test_stroke_refinement_mark_stroke(api, world, strokes):
    _, segs = world
    seg = segs["wide"]
    fg, bg = strokes["wide"]
    head = [LC.EXTRA_CLICKS["wide"][0][0]]
    clicks, labels = stood_for([(fg, 1, 2), (bg, 0, 2)], head, [1])
    staged = seg.compute_mask_clicks(_pts(api, clicks), labels, refine_after=[3])
    got = _raw(api, seg, [seg, None, None, None], [head[0]] + [(0, 0)] * 3, [EMPTY, (12, 2, 1, 0), (4, 0, 0, 0), (12, 2, 0, 0)],
               [None, fg, None, bg])[0]
    assert np.array_equal(got, staged)
    assert not np.array_equal(staged, seg.compute_mask_clicks(_pts(api, clicks), labels))
    # without points: the head's click, the first stroke's first, is in the first stage
    clicks, labels = stood_for([(fg, 1, 2), (bg, 0, 2)])
    staged = seg.compute_mask_clicks(_pts(api, clicks), labels, refine_after=[2])
    got = _raw(api, seg, [seg, None, None, None], None, [EMPTY, (12, 2, 1, 0), (4, 0, 0, 0), (12, 2, 0, 0)], [None, fg, None, bg])[0]
    assert np.array_equal(got, staged)


def test_a_lasso_mark_followed_by_a_stroke_mark(api, world, strokes):
    _, segs = world
    for name in LC.IMAGES:
        seg = segs[name]
        sel = LC.selection(name)
        _, bg = strokes[name]
        fg = strokes[name][0]
        # the lasso's click and box first, then the clicks the strokes stand for
        clicks, labels = stood_for([(fg, 1, 1), (bg, 0, 2)])
        want = seg.compute_mask_clicks(_pts(api, clicks), labels, lasso=sel, lasso_what=7)
        got = seg.compute_mask_clicks(None, strokes=[(fg, 1, 1), (bg, 0, 2)], lasso=sel, lasso_what=7)
        assert np.array_equal(got, want), name
        raw = _raw(api, seg, [seg, None, None, None], None, [EMPTY, (10, 0, 0, 0), (12, 1, 1, 0), (12, 2, 0, 0)], [None, sel, fg, bg])[0]
        assert np.array_equal(raw, want), name
        assert not np.array_equal(want, seg.snap_selection(sel, 7))


def test_clean_up_and_matte_marks_behind_strokes(api, world, strokes):
    _, segs = world
    seg = segs["wide"]
    fg, bg = strokes["wide"]
    guide = LC.image("wide")
    clicks, labels = stood_for([(fg, 1, 0), (bg, 0, 0)])
    for clean, matte in (((64, 64), None), (None, (guide, 8, 0)), ((64, 64), (guide, 4, 100))):
        want = seg.compute_mask_clicks(_pts(api, clicks), labels, clean=clean, matte=matte)
        assert np.array_equal(seg.scribble(fg, bg, clean=clean, matte=matte), want), (clean, matte is not None)
    assert len(np.unique(want)) > 2                              # the matte is a coverage


def test_hq_model_at_its_limit(api, tmp_path_factory):
    import hq_cases as H
    from dlimgedit_amd import weights as W
    mdir = tmp_path_factory.mktemp("models_hqtest_stroke")
    W.write_synthetic_model_dir(mdir, H.CFG, H.SEED, mask_branch=True, hq=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    img = H.image("small")                                       # 640 x 480: the resize path
    seg = api.Segmentation.process(api.ImageView(img, api.Channels.rgba), env)
    try:
        h, w = img.shape[:2]
        fg = scribble(w, h, [(0.2, 0.3), (0.5, 0.6), (0.7, 0.3)])
        box = _region(api, (91, 178, 305, 372))
        head = [(200, 250)]
        # 7 clicks and a box are the file's 9 points: the head's click and 6 derived ones are served, 7 derived ones refused
        clicks, labels = stood_for([(fg, 1, 6)], head, [1])
        want = seg.compute_mask_clicks(_pts(api, clicks), labels, box)
        assert np.array_equal(seg.compute_mask_clicks(_pts(api, head), None, box, strokes=[(fg, 1, 6)]), want)
        with pytest.raises(api.Error, match="entry 1:.*mark"):
            seg.compute_mask_clicks(_pts(api, head), None, box, strokes=[(fg, 1, 7)])
        assert np.array_equal(seg.compute_mask_clicks(_pts(api, head), None, box, strokes=[(fg, 1, 6)]), want)
    finally:
        seg.close()
        env.close()


def test_stroke_prompts_of_two_extents_beside_a_plain_prompt(api, world, strokes):
    _, segs = world
    heads = {n: [LC.EXTRA_CLICKS[n][0][0]] for n in LC.IMAGES}
    marks = {"square": [(strokes["square"][0], 1, 2)], "wide": [(strokes["wide"][0], 1, 0), (strokes["wide"][1], 0, 1)]}
    want = {}
    for n in LC.IMAGES:
        clicks, labels = stood_for(marks[n], heads[n], [1])
        want[n] = segs[n].compute_mask_clicks(_pts(api, clicks), labels).copy()
    plain = segs["square"].compute_mask_clicks(_pts(api, heads["square"])).copy()
    for order in (["square", "wide", None], [None, "wide", "square"]):
        got = api.Segmentation.compute_mask_batch([segs[n or "square"] for n in order], clicks=[_pts(api, heads[n or "square"]) for n in order],
                                                  strokes=[None if n is None else marks[n] for n in order])
        for g, n in zip(got, order):
            assert np.array_equal(g, plain if n is None else want[n]), (order, n)
    # without points: every prompt scribbled
    alone = {n: segs[n].scribble(strokes[n][0]).copy() for n in LC.IMAGES}
    got = api.Segmentation.compute_mask_batch([segs["wide"], segs["square"]], strokes=[[(strokes["wide"][0], 1, 0)], [(strokes["square"][0], 1, 0)]])
    assert np.array_equal(got[0], alone["wide"]) and np.array_equal(got[1], alone["square"])


def test_a_map_in_table_image_memory(api, world, strokes):
    _, segs = world
    for name in LC.IMAGES:
        fg, bg = strokes[name]
        want = segs[name].scribble(fg, bg)
        assert not api.ext.image_memory_is_pinned(fg)
        images = []
        for m in (fg, bg):
            image = api._mask_image(segs[name].extent())
            image[...] = m
            assert api.ext.image_memory_is_pinned(image)
            images.append(image)
        assert np.array_equal(segs[name].scribble(*images), want), name
        assert np.array_equal(images[0], fg) and np.array_equal(images[1], bg)          # the call only reads them
        # the result may go where the foreground map lies
        assert segs[name].scribble(images[0], images[1], out=images[0]) is images[0] and np.array_equal(images[0], want)


def test_refusals_name_the_mark_and_leave_the_handle_working(api, world, strokes):
    _, segs = world
    seg = segs["square"]
    fg, bg = strokes["square"]
    a, b = (523, 454), (816, 511)
    want = seg.scribble(fg).copy()
    FG, BG = (12, 0, 1, 0), (12, 0, 0, 0)
    refused = [
        ([seg, None], [a, a], [EMPTY, (12, 3, 1, 1)], [None, fg], 1),                       # a non-zero fourth int
        ([seg, None], [a, a], [EMPTY, (12, 3, 2, 0)], [None, fg], 1),                       # a label outside {0, 1}
        ([seg, None], [a, a], [EMPTY, (12, 3, -1, 0)], [None, fg], 1),
        ([seg, None], [a, a], [EMPTY, (12, 9, 1, 0)], [None, fg], 1),                       # clicks outside 0 .. 8
        ([seg, None], [a, a], [EMPTY, (12, -1, 1, 0)], [None, fg], 1),
        ([seg, None, None], [a, b, a], [EMPTY, (0, 0, 0, 0), FG], [None, None, None], 2),   # a NULL map
        ([None, seg], [a, a], [FG, EMPTY], [fg, None], 0),                                  # no prompt in front of it
        ([seg, seg, None, None], [a, a, a, a], [EMPTY, EMPTY, FG, (7, 4, 0, 0)], [None, None, fg, None], 2),       # a grid prompt
        ([seg, None], None, [EMPTY, BG], [None, bg], 1),                                    # background strokes alone, no points
        ([seg, None, None], None, [BOX["square"], BG, (12, 2, 0, 0)], [None, bg, bg], 1),
        ([seg, None], [a, a], [EMPTY, (12, 8, 1, 0)], [None, fg], 1),                       # 9 clicks, the derived ones counted
        ([seg, None, None], None, [EMPTY, (12, 8, 1, 0), (12, 1, 0, 0)], [None, fg, bg], 1),
        ([seg, None, None], [a, a, a], [EMPTY, FG, (10, 0, 0, 0)], [None, fg, fg], 1),      # in front of a lasso mark
        ([seg, None, None], [a, a, a], [EMPTY, (6, 8, 8, 0), FG], [None, None, fg], 2),     # behind a clean-up mark
    ]
    for handles, points, regions, ptrs, at in refused:
        with pytest.raises(api.Error, match=f"entry {at}:.*stroke mark"):
            _raw(api, seg, handles, points, regions, ptrs)
        assert np.array_equal(seg.scribble(fg), want)
    # an inner planner's refusal names the caller's entry: three placeholder clicks lie in front of the bad label
    with pytest.raises(api.Error, match="entry 2:.*label"):
        _raw(api, seg, [seg, None, None], [a, a, a], [EMPTY, FG, (5, 0, 0, 0)], [None, fg, None])
    # the wrapper refuses a map of another extent before anything reaches the library
    with pytest.raises(api.Error, match="strokes"):
        seg.scribble(np.zeros((600, 800), np.uint8))
    assert np.array_equal(seg.scribble(fg), want)


def test_the_empty_stroke_is_reported_by_entry(api, world, strokes):
    _, segs = world
    seg = segs["square"]
    fg, _ = strokes["square"]
    e = seg.extent()
    want = seg.scribble(fg).copy()
    for empty in (np.zeros((e.height, e.width), np.uint8), np.full((e.height, e.width), 127, np.uint8)):
        # a box and point prompt in front of it: the empty stroke is the second mark of the prompt of entry 1
        outs = {k: np.full((e.height, e.width), 7, np.uint8) for k in (0, 1)}
        with pytest.raises(api.Error, match=r"entry 3: the stroke mark's map is empty"):
            _raw(api, seg, [seg, seg, None, None], [(312, 487), (523, 454), (0, 0), (0, 0)],
                 [BOX["square"], EMPTY, (12, 2, 1, 0), (12, 0, 0, 0)], [None, None, fg, empty], outs)
        assert (outs[1] == 7).all()                                  # the head's buffer is untouched
        own = np.full((e.height, e.width), 7, np.uint8)
        with pytest.raises(api.Error, match=r"entry 1: the stroke mark's map is empty"):
            seg.scribble(empty, out=own)
        assert (own == 7).all()
        assert np.array_equal(seg.scribble(fg), want)                # the handle works afterwards


def test_the_device_form_refuses_by_name(api, world, strokes):
    env, segs = world
    seg = segs["square"]
    fg, _ = strokes["square"]
    dev = api.ext.device_alloc(env, fg.size)
    try:
        hs = (C.c_void_p * 2)(seg._handle, None)
        r = (C.c_int * 8)(*EMPTY, 12, 0, 1, 0)
        offsets = (C.c_size_t * 2)()
        with pytest.raises(api.Error, match=r"entry 1:.*stroke mark.*dlimg_amd_get_segmentation_masks_device"):
            api._check(api.ext._l().dlimg_amd_get_segmentation_masks_device(hs, 2, None, r, 0, dev, offsets))
    finally:
        api.ext.device_free(env, dev)
    assert np.array_equal(seg.scribble(fg), seg.scribble(fg))
