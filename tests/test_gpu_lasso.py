"""Lasso marks on the GPU: a continuation entry {10, strength_milli, what, 0} directly behind its head makes a prompt of a
selection the caller holds -- out_masks[] of the mark is READ -- whose box and first click are derived on the GPU
(kernels/mask_lasso.hip) and which may be the mask input of the first stage as well.  On the parent commit 10 is a refused
label: every test here that sends the mark fails there.

The yardstick is the library's own explicit path.  The mask delivered for a lasso prompt is BYTE-EQUAL to the mask delivered for
the explicit prompt built from tests/lasso_ref.py's box and click -- with a prior mark on the same buffer when the mask bit is
set, none when it is not: both run the same kernels on the same arguments, so there is no tolerance.

* all six valid `what` values on both images (the second takes the resize path): 7- and 8-row prompts; what = 0 with two further
  clicks (10 rows) and with a refinement mark; a clean-up mark; a SAM-HQ file with the branch; a model without the branch serves
  what = 3 and refuses what = 0 by name;
* slot 14 called raw, the wrapper and a thread give the same bytes; lasso and other prompts share a call in both orders, on one
  handle and on two; a selection snapped in place; a selection in the table's pinned image memory; four threads on one handle;
* every refusal says "mark", names the caller's entry and leaves the handle working; the empty selection names its entry, leaves
  the head's buffer untouched and the handle working; the device form refuses by name; two replicas (on one GPU, and on two
  GPUs where there are two) each derive their own.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import lasso_cases as LC
import lasso_ref
from cleanup_ref import cleanup_ref

EMPTY = (0, 0, -1, -1)
BOX, CLICK, MASK = lasso_ref.BOX, lasso_ref.CLICK, lasso_ref.MASK


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


@pytest.fixture(scope="module")
def world(api, tmp_path_factory):
    """(env, {image name: Segmentation}); a model WITH the branch"""
    from dlimgedit_amd import weights as W
    from dlimgedit_amd.sam_config import get_config
    mdir = tmp_path_factory.mktemp("models_vit_test_lasso")
    W.write_synthetic_model_dir(mdir, get_config("vit_test"), 7, mask_branch=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    segs = {n: api.Segmentation.process(api.ImageView(LC.image(n), api.Channels.rgba), env) for n in LC.IMAGES}
    yield env, segs
    for s in segs.values():
        s.close()
    env.close()


@pytest.fixture(scope="module")
def selections():
    """image name -> (its selection (h, w) uint8, drawn once and never written; the reference's record of it)"""
    out = {}
    for n in LC.IMAGES:
        sel = LC.selection(n)
        sel.setflags(write=False)
        rec = LC.record_of(n, sel)
        assert rec[0] > 0
        out[n] = (sel, rec)
    return out


def _pts(api, clicks):
    return [api.Point(int(x), int(y)) for x, y in clicks]


def _explicit(api, seg, sel, rec, what, strength=0, clicks=(), labels=(), after=None, clean=None, out=None):
    """The prompt a lasso mark stands for, sent explicitly: the reference's click in front of the caller's, the reference's box,
    and a prior mark on the selection when the mask bit is set."""
    what = what or 7
    all_clicks = ([(rec[5], rec[6])] if what & CLICK else []) + list(clicks)
    all_labels = ([1] if what & CLICK else []) + list(labels)
    shift = 1 if what & CLICK else 0
    region = api.Region(api.Point(int(rec[1]), int(rec[2])), api.Point(int(rec[3]), int(rec[4]))) if what & BOX else None
    prior = sel if what & MASK else None
    if all_clicks:
        return seg.compute_mask_clicks(_pts(api, all_clicks), all_labels, region, out=out,
                                       refine_after=None if after is None else [k + shift for k in after], clean=clean, prior=prior,
                                       prior_strength=strength)
    return api.Segmentation.compute_mask_batch([seg], regions=[region], out=None if out is None else [out],
                                               clean=None if clean is None else [clean], prior=None if prior is None else [prior],
                                               prior_strength=strength)[0]


def _snap(api, seg, sel, what, strength=0, clicks=(), labels=(), after=None, clean=None, out=None):
    return seg.snap_selection(sel, what, strength, _pts(api, clicks) or None, list(labels) or None, after, clean, out)


def _raw_lasso(api, seg, sel, what, strength=0, clicks=(), labels=(), after=None, clean=None, out=None):
    """Slot 14 with hand-made arrays: the head with an empty region, the lasso mark directly behind it, then whatever else."""
    e = seg.extent()
    out = np.zeros((e.height, e.width), np.uint8) if out is None else out
    handles, points, regions, ptrs = [seg._handle], [clicks[0] if clicks else (0, 0)], [EMPTY], [out.ctypes.data]
    handles.append(None); points.append((-77, 123456)); regions.append((10, strength, what, 0)); ptrs.append(sel.ctypes.data)
    for k in range(1, len(clicks)):
        if after and k in after:
            handles.append(None); points.append((0, 0)); regions.append((4, 0, 0, 0)); ptrs.append(None)
        handles.append(None); points.append(clicks[k]); regions.append((labels[k], 0, 0, 0)); ptrs.append(None)
    if clean:
        handles.append(None); points.append((0, 0)); regions.append((6, clean[0], clean[1], 0)); ptrs.append(None)
    n = len(handles)
    p = (C.c_int * (2 * n))(*[int(v) for q in points for v in q]) if clicks else None
    r = (C.c_int * (4 * n))(*[int(v) for q in regions for v in q])
    api._check(api.api().get_segmentation_masks((C.c_void_p * n)(*handles), n, p, r, (C.c_void_p * n)(*ptrs)))
    return out


def _extra(name):
    clicks = [c for c, _ in LC.EXTRA_CLICKS[name]]
    labels = [l for _, l in LC.EXTRA_CLICKS[name]]
    return clicks, labels


@pytest.fixture(scope="module")
def explicit(api, world, selections):
    """(image name, what) -> the mask of the explicit prompt, once"""
    _, segs = world
    return {(n, what): _explicit(api, segs[n], *selections[n], what).copy() for n in LC.IMAGES for what in LC.WHATS}


@pytest.mark.gpu
@pytest.mark.parametrize("what", LC.WHATS)
@pytest.mark.parametrize("name", list(LC.IMAGES))
def test_a_lasso_prompt_is_the_explicit_prompt(api, world, selections, explicit, name, what):
    _, segs = world
    sel, rec = selections[name]
    got = _snap(api, segs[name], sel, what)
    want = explicit[(name, what)]
    print(f"lasso.e2e.{name}.what{what}: record {rec.tolist()}, {LC.token_rows(what)} token rows, {int((got > 0).sum())} pixels set, "
          f"{int((got != want).sum())} differ from the explicit prompt")
    assert set(np.unique(got)) <= {0, 255} and (got > 0).any()
    assert np.array_equal(got, want)
    if what == 7:
        assert np.array_equal(_snap(api, segs[name], sel, 0), want)                      # 0 means all three
        assert np.array_equal(_snap(api, segs[name], sel, 7, strength=8000), want)       # the default strength spelt out
        other = _snap(api, segs[name], sel, 7, strength=1000)
        assert np.array_equal(other, _explicit(api, segs[name], sel, rec, 7, strength=1000))
    # the masks of the six prompts are not all one mask
    if what == 3:
        assert not np.array_equal(explicit[(name, 1)], explicit[(name, 2)])
        assert not np.array_equal(explicit[(name, 3)], explicit[(name, 7)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LC.IMAGES))
def test_further_clicks_refinement_and_clean_up(api, world, selections, explicit, name):
    _, segs = world
    seg = segs[name]
    sel, rec = selections[name]
    clicks, labels = _extra(name)
    assert LC.token_rows(0, len(clicks)) == 10
    # two further clicks behind the derived one: 10 token rows
    want = _explicit(api, seg, sel, rec, 0, clicks=clicks, labels=labels)
    assert np.array_equal(_snap(api, seg, sel, 0, clicks=clicks, labels=labels), want)
    assert not np.array_equal(want, explicit[(name, 7)])
    # a refinement mark: the derived click and the first of the caller's in the first stage, the box in both
    staged = _explicit(api, seg, sel, rec, 0, clicks=clicks, labels=labels, after=[1])
    assert np.array_equal(_snap(api, seg, sel, 0, clicks=clicks, labels=labels, after=[1]), staged)
    assert np.array_equal(_raw_lasso(api, seg, sel, 0, clicks=clicks, labels=labels, after=[1]), staged)
    assert not np.array_equal(staged, want)
    # without the mask bit the first stage takes no mask input, the second the first one's logits
    staged3 = _explicit(api, seg, sel, rec, 3, clicks=clicks, labels=labels, after=[1])
    assert np.array_equal(_snap(api, seg, sel, 3, clicks=clicks, labels=labels, after=[1]), staged3)
    # a clean-up mark, on the lasso alone and behind clicks
    clean = (64, 64)
    for what in (3, 7):
        assert np.array_equal(_snap(api, seg, sel, what, clean=clean), cleanup_ref(explicit[(name, what)], *clean))
        assert np.array_equal(_raw_lasso(api, seg, sel, what, clean=clean), cleanup_ref(explicit[(name, what)], *clean))
    assert np.array_equal(_snap(api, seg, sel, 0, clicks=clicks, labels=labels, clean=clean), cleanup_ref(want, *clean))
    # the click alone keeps a box of the caller's
    box = api.Region(api.Point(int(rec[1]) + 8, int(rec[2]) + 8), api.Point(int(rec[3]) - 8, int(rec[4]) - 8))
    got = seg.compute_mask_clicks(_pts(api, clicks[:1]), None, box, lasso=sel, lasso_what=CLICK)
    assert np.array_equal(got, seg.compute_mask_clicks(_pts(api, [(rec[5], rec[6])] + clicks[:1]), None, box))


@pytest.mark.gpu
def test_same_bytes_through_every_route(api, world, selections, explicit):
    _, segs = world
    for name in LC.IMAGES:
        sel, _ = selections[name]
        for what in LC.WHATS:
            want = explicit[(name, what)]
            assert np.array_equal(_raw_lasso(api, segs[name], sel, what), want), (name, what)
            got = api.Segmentation.compute_mask_batch([segs[name]], lasso=[sel], lasso_what=what)[0]
            assert np.array_equal(got, want), (name, what)
            box = {}
            t = threading.Thread(target=lambda: box.update(got=_snap(api, segs[name], sel, what)))
            t.start()
            t.join()
            assert np.array_equal(box["got"], want), (name, what)


@pytest.mark.gpu
def test_lasso_and_other_prompts_share_a_call(api, world, selections, explicit):
    env, segs = world
    second = {n: api.Segmentation.process(api.ImageView(LC.image(n), api.Channels.rgba), env) for n in LC.IMAGES}
    try:
        # prompts with clicks: (image, clicks, labels, lasso what or None), each alone first
        pool = []
        for n in LC.IMAGES:
            sel, rec = selections[n]
            clicks, labels = _extra(n)
            for what in (7, 3, 2):
                pool.append((n, clicks, labels, what, _explicit(api, segs[n], sel, rec, what, clicks=clicks, labels=labels).copy()))
            pool.append((n, clicks, labels, None, segs[n].compute_mask_clicks(_pts(api, clicks), labels).copy()))
            pool.append((n, clicks[:1], labels[:1], None, segs[n].compute_mask_clicks(_pts(api, clicks[:1]), labels[:1]).copy()))
        orders = (list(range(len(pool))), list(range(len(pool)))[::-1], [3, 9, 0, 5, 7, 1, 8, 2, 6, 4])
        for order, handles in zip(orders, ((segs, segs), (segs, second), (second, segs))):
            chosen = [pool[k] for k in order]
            got = api.Segmentation.compute_mask_batch(
                [handles[j % 2][c[0]] for j, c in enumerate(chosen)], clicks=[_pts(api, c[1]) for c in chosen], labels=[c[2] for c in chosen],
                lasso=[None if c[3] is None else selections[c[0]][0] for c in chosen], lasso_what=[c[3] or 0 for c in chosen])
            for j, c in enumerate(chosen):
                assert np.array_equal(got[j], c[4]), (order, j)
        # the form without `points`: a box-only prompt and lasso-only prompts, in both orders, on two handles
        sel, rec = selections["square"]
        box = api.Region(api.Point(257, 264), api.Point(580, 567))
        alone = api.Segmentation.compute_mask_batch([segs["square"]], regions=[box])[0].copy()
        for trio in ([(box, None, 0), (None, sel, 7), (None, sel, 1)], [(None, sel, 2), (box, None, 0), (None, sel, 7)]):
            got = api.Segmentation.compute_mask_batch([second["square"], segs["square"], second["square"]], regions=[t[0] for t in trio],
                                                      lasso=[t[1] for t in trio], lasso_what=[t[2] for t in trio])
            for g, t in zip(got, trio):
                assert np.array_equal(g, alone if t[1] is None else explicit[("square", t[2])])
    finally:
        for s in second.values():
            s.close()


@pytest.mark.gpu
def test_a_selection_snapped_in_place_and_in_table_image_memory(api, world, selections, explicit):
    _, segs = world
    for name, what in (("square", 7), ("wide", 3), ("wide", 6)):
        sel, _ = selections[name]
        want = explicit[(name, what)]
        # the caller's own memory: the selection is packed into staging memory when the call is enqueued
        own = sel.copy()
        assert not api.ext.image_memory_is_pinned(own)
        assert _snap(api, segs[name], own, what, out=own) is own and np.array_equal(own, want), (name, what)
        own = sel.copy()
        assert np.array_equal(_raw_lasso(api, segs[name], own, what, out=own), want)      # out_masks[mark] == out_masks[head]
        # memory of the table: the selection is copied from where it lies
        image = api._mask_image(segs[name].extent())
        image[...] = sel
        assert api.ext.image_memory_is_pinned(image)
        assert np.array_equal(_snap(api, segs[name], image, what), want), (name, what)
        assert np.array_equal(image, sel)                                                   # the call only reads it
        assert np.array_equal(_snap(api, segs[name], image, what, out=image), want), (name, what)


@pytest.mark.gpu
def test_four_threads_on_one_handle(api, world, selections, explicit):
    _, segs = world
    sel, _ = selections["wide"]
    results, errors = {}, []

    def work(t):
        try:
            for rep in range(3):
                what = LC.WHATS[(t + 2 * rep) % len(LC.WHATS)]
                results[(t, rep)] = (what, _snap(api, segs["wide"], sel, what).copy())
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 12
    for (t, rep), (what, got) in results.items():
        assert np.array_equal(got, explicit[("wide", what)]), (t, rep, what)


def _raw(api, seg, handles, points, regions, sel_at=(), sel=None, outs=None):
    n = len(handles)
    hs = (C.c_void_p * n)(*[None if h is None else h._handle for h in handles])
    p = None if points is None else (C.c_int * (2 * n))(*[v for q in points for v in q])
    r = (C.c_int * (4 * n))(*[v for q in regions for v in q])
    outs = [np.zeros((seg.extent().height, seg.extent().width), np.uint8) for _ in range(n)] if outs is None else outs
    ptrs = (C.c_void_p * n)(*[o.ctypes.data if h is not None else (sel.ctypes.data if k in sel_at else None)
                              for k, (o, h) in enumerate(zip(outs, handles))])
    api._check(api.api().get_segmentation_masks(hs, n, p, r, ptrs))
    return outs


@pytest.mark.gpu
def test_refusals_name_the_mark_and_leave_the_handle_working(api, world, selections, explicit):
    _, segs = world
    seg = segs["square"]
    sel, rec = selections["square"]
    a, b = (523, 454), (816, 511)
    LASSO, BOXED = (10, 0, 0, 0), (257, 264, 580, 567)
    refused = [
        ([None, seg], [a, a], [LASSO, EMPTY], (0,), 0),                                     # in front of any head
        ([seg, None, None], [a, b, a], [EMPTY, (0, 0, 0, 0), LASSO], (2,), 2),              # behind a click, not its head
        ([seg, None, None, None], [a, a, a, b], [EMPTY, (4, 0, 0, 0), LASSO, (0, 0, 0, 0)], (2,), 2),      # behind a refinement mark
        ([seg, None, None], [a, a, a], [EMPTY, LASSO, LASSO], (1, 2), 2),                   # a second lasso mark
        ([seg, None, None], [a, a, a], [EMPTY, (8, 0, 0, 0), LASSO], (1, 2), 2),            # a prior mark and a lasso mark
        ([seg, None, None], [a, a, a], [EMPTY, LASSO, (8, 0, 0, 0)], (1, 2), 1),
        ([seg, None], [a, a], [EMPTY, LASSO], (), 1),                                       # a NULL selection
        ([seg, None], [a, a], [EMPTY, (10, 0, 8, 0)], (1,), 1),                             # what outside 0 .. 7
        ([seg, None], [a, a], [EMPTY, (10, 0, -1, 0)], (1,), 1),
        ([seg, None], [a, a], [EMPTY, (10, 0, 4, 0)], (1,), 1),                             # what == 4 derives nothing
        ([seg, None], [a, a], [EMPTY, (10, 0, 0, 3)], (1,), 1),                             # a non-zero fourth int
        ([seg, None], [a, a], [EMPTY, (10, -1, 0, 0)], (1,), 1),                            # strength outside 0 .. 100000
        ([seg, None], [a, a], [EMPTY, (10, 100001, 0, 0)], (1,), 1),
        ([seg, None], [a, a], [EMPTY, (10, 8000, 3, 0)], (1,), 1),                          # a strength without the mask bit
        ([seg, None], [a, a], [BOXED, (10, 0, 1, 0)], (1,), 1),                             # the box bit on a head with a region
        ([seg, None], None, [BOXED, LASSO], (1,), 1),
        ([seg, None, None], [a, a, a], [EMPTY, LASSO, (7, 4, 0, 0)], (1,), 1),              # a grid prompt
        ([seg] + [None] * 8, [a] * 9, [EMPTY, LASSO] + [(1, 0, 0, 0)] * 7, (1,), 1),        # 8 clicks of the caller's and the derived one
    ]
    for handles, points, regions, sel_at, at in refused:
        with pytest.raises(api.Error, match=f"entry {at}:.*mark"):
            _raw(api, seg, handles, points, regions, sel_at, sel)
        assert np.array_equal(_snap(api, seg, sel, 7), explicit[("square", 7)])
    with pytest.raises(api.Error, match="more than 8 clicks"):
        _raw(api, seg, [seg] + [None] * 8, [a] * 9, [EMPTY, LASSO] + [(1, 0, 0, 0)] * 7, (1,), sel)
    # 5 and 9 are still refused labels, and a click without `points` keeps its words
    for label in (5, 9):
        with pytest.raises(api.Error, match="label"):
            _raw(api, seg, [seg, None], [a, a], [EMPTY, (label, 0, 0, 0)])
    with pytest.raises(api.Error, match="is a click and needs `points`"):
        _raw(api, seg, [seg, None, None], None, [EMPTY, LASSO, (1, 0, 0, 0)], (1,), sel)
    # the wrapper refuses a selection of another extent before anything reaches the library
    with pytest.raises(api.Error, match="lasso"):
        _snap(api, seg, np.zeros((600, 800), np.uint8), 7)
    assert np.array_equal(_snap(api, seg, sel, 7), explicit[("square", 7)])


@pytest.mark.gpu
def test_the_empty_selection_is_reported_by_entry(api, world, selections, explicit):
    _, segs = world
    seg = segs["square"]
    sel, _ = selections["square"]
    e = seg.extent()
    for empty in (np.zeros((e.height, e.width), np.uint8), np.full((e.height, e.width), 127, np.uint8)):
        for what in (3, 7):
            outs = [np.full((e.height, e.width), 7, np.uint8) for _ in range(4)]
            # a box-only prompt in front of it: the empty selection is the prompt of entry 1, its mark entry 2
            with pytest.raises(api.Error, match=r"entry 2: the lasso mark's selection is empty"):
                _raw(api, seg, [seg, seg, None], None, [(257, 264, 580, 567), EMPTY, (10, 0, what, 0)], (2,), empty, outs[:3])
            assert (outs[1] == 7).all()                                   # the head's buffer is untouched
            own = np.full((e.height, e.width), 7, np.uint8)
            with pytest.raises(api.Error, match=r"entry 1: the lasso mark's selection is empty"):
                _snap(api, seg, empty, what, out=own)
            assert (own == 7).all()
            assert np.array_equal(_snap(api, seg, sel, what), explicit[("square", what)])     # the handle works afterwards


@pytest.mark.gpu
def test_the_device_form_refuses_by_name(api, world, selections, explicit):
    env, segs = world
    seg = segs["square"]
    sel, _ = selections["square"]
    dev = api.ext.device_alloc(env, sel.size)
    try:
        hs = (C.c_void_p * 2)(seg._handle, None)
        r = (C.c_int * 8)(*EMPTY, 10, 0, 0, 0)
        offsets = (C.c_size_t * 2)()
        with pytest.raises(api.Error, match=r"entry 1:.*lasso mark.*dlimg_amd_get_segmentation_masks_device"):
            api._check(api.ext._l().dlimg_amd_get_segmentation_masks_device(hs, 2, None, r, 0, dev, offsets))
    finally:
        api.ext.device_free(env, dev)
    assert np.array_equal(_snap(api, seg, sel, 7), explicit[("square", 7)])


@pytest.mark.gpu
def test_model_without_the_branch_serves_box_and_click(api, world, selections, explicit, model_dirs):
    mdir, _, _ = model_dirs("vit_test")
    env = api.Environment(api.Options(api.Backend.gpu, mdir))
    bare = api.Segmentation.process(api.ImageView(LC.image("square"), api.Channels.rgba), env)
    sel, rec = selections["square"]
    try:
        # every other tensor of the two files is the same, so the masks without a mask input are those of the model with the branch
        for what in (1, 2, 3):
            got = _snap(api, bare, sel, what)
            assert np.array_equal(got, _explicit(api, bare, sel, rec, what)) and np.array_equal(got, explicit[("square", what)])
        for what in (0, 5, 6, 7):
            with pytest.raises(api.Error, match=r"entry 1:.*lasso mark.*pe\.mask"):
                _snap(api, bare, sel, what)
        assert np.array_equal(_snap(api, bare, sel, 3), explicit[("square", 3)])
    finally:
        bare.close()
        env.close()


@pytest.mark.gpu
def test_hq_model_serves_a_lasso(api, tmp_path_factory):
    import hq_cases as H
    import prior_ref
    from dlimgedit_amd import weights as W
    mdir = tmp_path_factory.mktemp("models_hqtest_lasso")
    W.write_synthetic_model_dir(mdir, H.CFG, H.SEED, mask_branch=True, hq=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    img = H.image("small")                                                     # 640 x 480: the resize path
    seg = api.Segmentation.process(api.ImageView(img, api.Channels.rgba), env)
    try:
        h, w = img.shape[:2]
        yy, xx = np.mgrid[0:h, 0:w]
        sel = np.where(((xx - 0.4 * w) / (0.3 * w)) ** 2 + ((yy - 0.5 * h) / (0.25 * h)) ** 2 <= 1, 255, 0).astype(np.uint8)
        rec = lasso_ref.derive(sel, *prior_ref.pre_extent(w, h))
        for what in (3, 7):
            got = _snap(api, seg, sel, what)
            assert set(np.unique(got)) <= {0, 255} and np.array_equal(got, _explicit(api, seg, sel, rec, what)), what
        # the derived click counts towards the file's point limit: 7 clicks and a box are 9 points, an eighth click is refused
        six = [(100 + 40 * k, 200) for k in range(6)]
        got = _snap(api, seg, sel, 7, clicks=six, labels=[1] * 6)
        assert np.array_equal(got, _explicit(api, seg, sel, rec, 7, clicks=six, labels=[1] * 6))
        with pytest.raises(api.Error):
            _snap(api, seg, sel, 7, clicks=six + [(50, 50)], labels=[1] * 7)
        assert np.array_equal(_snap(api, seg, sel, 7, clicks=six, labels=[1] * 6), got)
    finally:
        seg.close()
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ["0,0", "0,1"], ids=["two_replicas_on_one_gpu", "two_gpus"])
def test_two_replicas_each_derive_their_own(api, tmp_path_factory, monkeypatch, selections, explicit, devices):
    """A lasso prompt is derived on the replica that holds its embedding: GPU 0 listed twice (two replicas on one GPU), and two GPUs."""
    if devices == "0,1" and api.ext.device_count() < 2:
        pytest.skip("one GPU visible")
    from dlimgedit_amd import weights as W
    from dlimgedit_amd.sam_config import get_config
    mdir = tmp_path_factory.mktemp("models_vit_test_lasso_two")
    W.write_synthetic_model_dir(mdir, get_config("vit_test"), 7, mask_branch=True)
    monkeypatch.setenv("DLIMGEDIT_DEVICES", devices)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    monkeypatch.delenv("DLIMGEDIT_DEVICES")
    names = ["square", "wide", "wide", "square"]
    handles = api.Segmentation.process_batch([api.ImageView(LC.image(n), api.Channels.rgba) for n in names], env)
    try:
        assert sorted(api.ext.segmentation_device(s)[0] for s in handles) == [0, 0, 1, 1]
        whats = [7, 3, 6, 1]
        got = api.Segmentation.compute_mask_batch(handles, lasso=[selections[n][0] for n in names], lasso_what=whats)
        for g, n, what in zip(got, names, whats):
            assert np.array_equal(g, explicit[(n, what)]), (n, what)
    finally:
        for s in handles:
            s.close()
        env.close()
