"""Several clicks per prompt through the batch mask calls (table slot 14 and its device-output form): an entry without a
handle is one more click of the prompt in front of it, foreground or background (csrc/prompt_plan.hpp); 1 .. 8 clicks with or
without a box, 7 .. 15 token rows in the decoder, plane 0 out from two clicks on.

* parity: the mask of slot 14 against oracle/decoder_ref.decode_fp64 on the handle's own embedding, the single-mask plane
  through sam_oracle.postprocess_logits: IoU >= IOU_BAR and at most multi_click_cases.DISAGREE_LIMIT of the pixels differ
  (three times what the two-token and three-token prompts of the same cases differ in: multi_click_cases.py);
* every click and its label count: the mask is strictly closer to its own reference than to the reference without the last
  click and to the reference with the last click's label flipped (which differ from it in ten times the limit or more:
  test_multi_click_oracle.py) -- the test that fails when background labels or the token rows above 8 are dropped;
* one click through the new form has the bits of today's point call, one click and a box those of today's box + point call;
* a call that mixes prompts of 7, 8, 9, 12 and 15 token rows over both images, 1 .. 20 prompts (the 8 prompts of a lane's
  chunk, and the per-launch cut of 7 prompts at 15 rows: the 20-prompt call has eight of them; a lane never gets more than
  8 prompts, so through this route the cuts of 12 prompts at 9 rows and 9 at 12 are reached by the planner's CPU tests only;
  on the GPU every cut runs in test_gpu_decoder_prompts.py, through the decoder's test hook), gives every prompt
  the bits of a call of its own; the device-output form gives the host form's bits, offsets tightly packed, also under two
  replicas; a two-token call in between leaves nothing behind;
* 9 clicks, a continuation entry in front and a label other than 0 / 1 are refused, and the handle works afterwards.
"""
import ctypes as C

import numpy as np
import pytest

import multi_click_cases as M
from conftest import IOU_BAR, at_least, iou, within


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


@pytest.fixture(scope="module")
def mc(api, model_dirs):
    """(env, params, {image name: Segmentation}, {image name: its embedding as the GPU computed it})"""
    mdir, params, _ = model_dirs("vit_test")
    env = api.Environment(api.Options(api.Backend.gpu, mdir))
    segs = {n: api.Segmentation.process(api.ImageView(M.image(n), api.Channels.rgba), env) for n in M.IMAGES}
    embs = {n: api.ext.get_embedding(s) for n, s in segs.items()}
    yield env, params, segs, embs
    for s in segs.values():
        s.close()
    env.close()


def _points(api, clicks):
    return [api.Point(*c) for c in clicks]


def _region(api, box):
    return None if box is None else api.Region(api.Point(box[0], box[1]), api.Point(box[2], box[3]))


def _rs(name):
    from oracle import sam_oracle as O
    _, w, h = M.IMAGES[name]
    rs = O.ResizeLongestSide()
    rs.target_extent(w, h)
    return rs, (h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("case", M.CASES, ids=[M.case_id(c) for c in M.CASES])
def test_mask_parity_and_every_click_counts(api, mc, case):
    env, params, segs, embs = mc
    name, clicks, labels, box = case
    rs, hw = _rs(name)
    refs = {}
    for kind, (c, l, b) in M.variants(case).items():
        refs[kind], plane = M.reference_mask(embs[name], rs, c, l, b, params, hw)
        assert plane == 0 or len(c) + (2 if b is not None else 1) == 2
    got = segs[name].compute_mask_clicks(_points(api, clicks), labels, _region(api, box))
    assert set(np.unique(got)) <= {0, 255}
    got = got > 0
    tag = M.case_id(case)
    differing = {kind: int((got != ref).sum()) for kind, ref in refs.items()}
    print(f"multi_click.{tag}: differing pixels {differing} of {got.size}: fraction {differing['full'] / got.size:.3g}")
    at_least(f"multi_click.iou.{tag}", iou(got, refs["full"]), IOU_BAR)
    within(f"multi_click.disagree.{tag}", differing["full"] / got.size, M.DISAGREE_LIMIT)
    # an implementation that drops the last click (a token row above 8, say) answers the mask without it, one that reads
    # every label as foreground the flipped one
    assert differing["full"] < differing["without_last"], differing
    assert differing["full"] < differing["flipped"], differing


@pytest.mark.gpu
def test_one_click_is_todays_call_bit_for_bit(api, mc):
    _, _, segs, _ = mc
    for name, clicks, _, box in M.CASES:
        seg, first = segs[name], api.Point(*clicks[0])
        point_call = api.Segmentation.compute_mask_batch([seg], points=[first])[0]
        assert np.array_equal(seg.compute_mask_clicks([first]), point_call), name
        if box is not None:
            both_call = api.Segmentation.compute_mask_batch([seg], points=[first], regions=[_region(api, box)])[0]
            assert np.array_equal(seg.compute_mask_clicks([first], [1], _region(api, box)), both_call), name
            assert not np.array_equal(both_call, point_call)
    # the same inside a call that has continuation entries: a head with an empty region and no further click is a point
    # prompt, a head with a box and no further click a box + point prompt
    name, clicks, labels, box = M.CASES[1]
    seg = segs[name]
    first, region = api.Point(*clicks[0]), _region(api, box)
    got = api.Segmentation.compute_mask_batch([seg, seg, seg], clicks=[[first], _points(api, clicks), [first]],
                                              labels=[None, labels, None], regions=[None, region, region])
    assert np.array_equal(got[0], api.Segmentation.compute_mask_batch([seg], points=[first])[0])
    assert np.array_equal(got[2], api.Segmentation.compute_mask_batch([seg], points=[first], regions=[region])[0])
    assert np.array_equal(got[1], seg.compute_mask_clicks(_points(api, clicks), labels, region))


def _pool(api, segs, n=20):
    """n prompts of 7, 8, 9, 12 and 15 token rows in irregular order: the cases of multi_click_cases cut to the wanted number
    of clicks (with their box or without), shifted by a few pixels; images alternate, so one handle appears many times."""
    rng = np.random.default_rng(9)
    rows = [15, 7, 9, 12, 8, 15, 9, 15, 12, 7, 15, 12, 8, 9, 15, 15, 12, 9, 15, 15]      # 8 x 15 rows: a lane's chunk of 8 is two launches (7 + 1)
    out = []
    for i in range(n):
        name, clicks, labels, box = M.CASES[(i * 3 + i // 5) % len(M.CASES)]
        _, w, h = M.IMAGES[name]
        t = rows[i % len(rows)]
        with_box = box is not None and t >= 8 and (i % 2 == 0 or t == 15)
        if t == 15 and box is None:
            box, with_box = (w // 8, h // 8, w // 2, h // 2), True
        want = t - (7 if with_box else 6)
        dx, dy = rng.integers(-9, 10, 2)
        pts = [(int(min(max(clicks[k % len(clicks)][0] + dx + 13 * (k // len(clicks)), 0), w - 1)),
                int(min(max(clicks[k % len(clicks)][1] + dy, 0), h - 1))) for k in range(want)]
        labs = [1] + [int(labels[k % len(labels)]) if k % len(labels) else 0 for k in range(1, want)]
        out.append((segs[name], _points(api, pts), labs, _region(api, box) if with_box else None))
        assert 5 + want + (2 if with_box else 1) == t
    return out


def _call(api, entries):
    return api.Segmentation.compute_mask_batch([e[0] for e in entries], clicks=[e[1] for e in entries],
                                               labels=[e[2] for e in entries], regions=[e[3] for e in entries])


@pytest.fixture(scope="module")
def singles(api, mc):
    _, _, segs, _ = mc
    return [_call(api, [e])[0] for e in _pool(api, segs)]


@pytest.mark.gpu
def test_mixed_batch_is_bit_equal_to_one_prompt_per_call(api, mc, singles):
    _, _, segs, _ = mc
    pool = _pool(api, segs)
    assert {5 + len(e[1]) + (2 if e[3] is not None else 1) for e in pool} == {7, 8, 9, 12, 15}
    assert len({id(a) for a in singles}) == len(pool) and any(not np.array_equal(singles[0], s) for s in singles[1:])
    for count in (1, 2, 9, 13, 20):
        start = (7 * count) % len(pool)
        sel = [(start + j) % len(pool) for j in range(count)]
        got = _call(api, [pool[i] for i in sel])
        for j, i in enumerate(sel):
            assert got[j].shape == singles[i].shape
            assert np.array_equal(got[j], singles[i]), f"{count} prompts: prompt {j} (pool {i}) differs from its own call"
    # a two-token call in between leaves nothing behind: the same prompts again
    api.Segmentation.compute_mask_batch([pool[0][0]] * 3, points=[pool[0][1][0]] * 3)
    again = _call(api, pool[:9])
    for i in range(9):
        assert np.array_equal(again[i], singles[i])


def _device_form_equals_host_form(api, env, entries, want):
    extents = [(m.shape[1], m.shape[0]) for m in want]
    total = sum(w * h for w, h in extents)
    dev = api.ext.device_alloc(env, total)
    try:
        api.ext.copy_to_device(env, dev, np.full(total, 7, np.uint8))
        offsets = api.ext.compute_mask_batch_device([e[0] for e in entries], dev, clicks=[e[1] for e in entries],
                                                    labels=[e[2] for e in entries], regions=[e[3] for e in entries], root_device=0)
        got = np.empty(total, np.uint8)
        api.ext.copy_to_host(env, got, dev)
        assert len(offsets) == len(entries) and offsets[0] == 0
        assert all(offsets[k + 1] - offsets[k] == extents[k][0] * extents[k][1] for k in range(len(entries) - 1))
        for k, (w, h) in enumerate(extents):
            assert np.array_equal(got[offsets[k]:offsets[k] + w * h].reshape(h, w), want[k]), k
    finally:
        api.ext.device_free(env, dev)


@pytest.mark.gpu
def test_device_form_is_bit_equal_to_host_form(api, mc, singles):
    env, _, segs, _ = mc
    pool = _pool(api, segs)
    _device_form_equals_host_form(api, env, pool, singles)
    # the raw call: the offset of a continuation entry repeats its prompt's
    seg, clicks, labels, region = pool[0]
    entries = api.click_entries([clicks, clicks[:2]], [labels, labels[:2]], [region, None])
    n, handles, p, r = api._entry_arrays([seg, seg], entries, list(range(len(entries.heads))), True)
    e = seg.extent()
    dev = api.ext.device_alloc(env, 2 * e.width * e.height)
    try:
        offsets = (C.c_size_t * n)()
        api._check(api.ext._l().dlimg_amd_get_segmentation_masks_device(handles, n, p, r, 0, dev, offsets))
        assert list(offsets) == [0] * len(clicks) + [e.width * e.height] * 2
    finally:
        api.ext.device_free(env, dev)


@pytest.mark.gpu
def test_mixed_batch_under_two_replicas(api, model_dirs, monkeypatch):
    """GPU 0 listed twice: two replicas share the prompts of a call, and a prompt -- its head and its continuation entries --
    stays on the replica of its handle.  Host form equal to one prompt per call, device form equal to host form."""
    mdir, _, _ = model_dirs("vit_test")
    monkeypatch.setenv("DLIMGEDIT_DEVICES", "0,0")
    env = api.Environment(api.Options(api.Backend.gpu, mdir))
    monkeypatch.delenv("DLIMGEDIT_DEVICES")
    names = ["square", "wide", "wide", "square"]
    handles = api.Segmentation.process_batch([api.ImageView(M.image(n), api.Channels.rgba) for n in names], env)
    assert sorted(api.ext.segmentation_device(s)[0] for s in handles) == [0, 0, 1, 1]
    by_name = {"square": [handles[0], handles[3]], "wide": [handles[1], handles[2]]}
    try:
        proto = _pool(api, {n: n for n in M.IMAGES})[:13]
        entries = [(by_name[name][k % 2], c, l, r) for k, (name, c, l, r) in enumerate(proto)]
        host = _call(api, entries)
        for k, e in enumerate(entries):
            assert np.array_equal(host[k], _call(api, [e])[0]), k
        _device_form_equals_host_form(api, env, entries, host)
    finally:
        for s in handles:
            s.close()
        env.close()


@pytest.mark.gpu
def test_refusals(api, mc):
    env, _, segs, _ = mc
    name, clicks, labels, box = M.CASES[0]
    seg = segs[name]
    before = seg.compute_mask_clicks(_points(api, clicks), labels)

    def raw(handles, points, regions):
        n = len(handles)
        hs = (C.c_void_p * n)(*[None if h is None else h._handle for h in handles])
        p = (C.c_int * (2 * n))(*[v for q in points for v in q])
        r = None if regions is None else (C.c_int * (4 * n))(*[v for q in regions for v in q])
        outs = [np.zeros((seg.extent().height, seg.extent().width), np.uint8) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        api._check(api.api().get_segmentation_masks(hs, n, p, r, ptrs))
        return outs

    pt = clicks[0]
    # the wrapper's builder refuses before anything reaches the library ...
    with pytest.raises(api.Error):
        seg.compute_mask_clicks(_points(api, [pt] * 9))
    with pytest.raises(api.Error):
        seg.compute_mask_clicks(_points(api, [pt] * 2), [1, 2])
    # ... and the library refuses the same calls made without it: 9 clicks, a continuation entry in front, a bad label
    with pytest.raises(api.Error, match="more than 8 clicks"):
        raw([seg] + [None] * 8, [pt] * 9, None)
    with pytest.raises(api.Error, match="continuation"):
        raw([None, seg], [pt] * 2, None)
    for bad in ((2, 0, 0, 0), (-1, 0, 0, 0), (1, 0, 0, 5)):
        with pytest.raises(api.Error, match="label"):
            raw([seg, None], [pt] * 2, [M_EMPTY, bad])
    # 8 clicks are taken, and the handle works as before
    assert raw([seg] + [None] * 7, [pt] * 8, None)[0].shape == before.shape
    assert np.array_equal(seg.compute_mask_clicks(_points(api, clicks), labels), before)
    assert np.array_equal(raw([seg, None], list(clicks), [M_EMPTY, (0, 0, 0, 0)])[0], before)


M_EMPTY = (0, 0, -1, -1)
