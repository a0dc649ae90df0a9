"""Mask input for click-to-refine on the GPU: a prompt with refinement marks (a continuation entry {4, 0, 0, 0}) is decoded in
stages, every stage from the second on taking the low-res logits of the stage before it through the prompt encoder's mask
branch (kernels/decoder.hip: mask_embed_kernel, the masked decoder_start_kernel); the mask of the last stage is delivered.

* exact stage: the GPU's own stage-1 planes (dlimg_amd_get_logits) fed to the float64 reference of the later stages -- the
  delivered mask differs from it in at most multi_click_cases.DISAGREE_LIMIT of the pixels;
* whole chain: every case against the pure float64 chain, within mask_input_cases.CHAIN_LIMIT, and closer to it than to the
  float64 reference of the same clicks without mask input (on the parent such a call is refused);
* slot 14, the device form and the wrappers give the same bytes; staged and unstaged prompts share a call, on one handle and
  on two, in any order; four threads on one handle reproduce the serial bytes;
* a model file without pe.mask.* serves the multi-click prompts as before and refuses a mark; after every refusal the
  handle works as before.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import mask_input_cases as MI
import multi_click_cases as M
from conftest import within

IDS = [MI.case_id(c) for c in MI.CASES]
EXACT = [c for c in MI.CASES if MI.first_stage_is_two_point_prompt(c)]
EMPTY, MARK = (0, 0, -1, -1), (4, 0, 0, 0)


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


@pytest.fixture(scope="module")
def mi(api, tmp_path_factory):
    """(env, params, {image name: Segmentation}, {image name: its embedding as the GPU computed it}); a model WITH the branch"""
    from dlimgedit_amd import weights as W
    from dlimgedit_amd.sam_config import get_config
    mdir = tmp_path_factory.mktemp("models_vit_test_mask")
    params = W.write_synthetic_model_dir(mdir, get_config("vit_test"), 7, mask_branch=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    segs = {n: api.Segmentation.process(api.ImageView(MI.image(n), api.Channels.rgba), env) for n in MI.IMAGES}
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
    _, w, h = MI.IMAGES[name]
    rs = O.ResizeLongestSide()
    rs.target_extent(w, h)
    return rs, (h, w)


def _staged(api, segs, case):
    name, clicks, labels, box, after = case
    return segs[name].compute_mask_clicks(_points(api, clicks), labels, _region(api, box), refine_after=after)


@pytest.fixture(scope="module")
def delivered(api, mi):
    """case index -> the mask the wrapper delivers, once"""
    _, _, segs, _ = mi
    return [_staged(api, segs, case) for case in MI.CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXACT, ids=[MI.case_id(c) for c in EXACT])
def test_exact_stage(api, mi, delivered, case):
    from conftest import single_mask_index
    _, params, segs, embs = mi
    name, clicks, _, _, _ = case
    rs, hw = _rs(name)
    planes, iou4 = api.ext.get_logits(segs[name], point=api.Point(*clicks[0]))
    plane = single_mask_index(iou4)
    assert plane in (1, 2, 3)
    want, last_plane, _ = MI.staged_reference(embs[name], rs, case, params, hw, first_mask_logits=planes[plane], from_stage=1)
    got = delivered[MI.CASES.index(case)] > 0
    fraction = float((got != want).mean())
    print(f"mask_input.exact.{MI.case_id(case)}: {int((got != want).sum())} of {got.size} pixels differ: fraction {fraction:.3g}")
    assert last_plane == 0
    within(f"mask_input.exact.{MI.case_id(case)}", fraction, MI.EXACT_LIMIT)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MI.CASES, ids=IDS)
def test_whole_chain_and_discrimination(api, mi, delivered, case):
    _, params, segs, embs = mi
    name = case[0]
    rs, hw = _rs(name)
    want, plane, _ = MI.staged_reference(embs[name], rs, case, params, hw)
    without = MI.unstaged_reference(embs[name], rs, case, params, hw)
    got = delivered[MI.CASES.index(case)]
    assert set(np.unique(got)) <= {0, 255} and plane == 0
    got = got > 0
    d_with, d_without = int((got != want).sum()), int((got != without).sum())
    print(f"mask_input.chain.{MI.case_id(case)}: {d_with} of {got.size} pixels differ from the staged reference "
          f"(fraction {d_with / got.size:.3g}), {d_without} from the reference without mask input")
    assert d_with < d_without, (d_with, d_without)
    assert MI.CHAIN_LIMIT <= min(MI.WITHOUT_FRACTION) / 10
    within(f"mask_input.chain.{MI.case_id(case)}", d_with / got.size, MI.CHAIN_LIMIT)


def _raw_entries(api, case):
    name, clicks, labels, box, after = case
    return api.click_entries([_points(api, clicks)], [labels], [_region(api, box)], [after])


def _raw_call(api, seg, entries):
    n, handles, p, r = api._entry_arrays([seg], entries, list(range(len(entries.heads))), True)
    e = seg.extent()
    out = np.zeros((e.height, e.width), np.uint8)
    ptrs = (C.c_void_p * n)(*[out.ctypes.data if h is not None else None for h in entries.heads])
    api._check(api.api().get_segmentation_masks(handles, n, p, r, ptrs))
    return out


@pytest.mark.gpu
def test_same_bytes_through_every_route(api, mi, delivered):
    env, _, segs, _ = mi
    for i, case in enumerate(MI.CASES):
        name, clicks, labels, box, after = case
        seg = segs[name]
        # slot 14 called with hand-made arrays
        assert np.array_equal(_raw_call(api, seg, _raw_entries(api, case)), delivered[i]), MI.case_id(case)
        # the batch wrapper, and "each" spelt out
        spelt = list(range(1, len(clicks))) if after == "each" else list(after)
        got = api.Segmentation.compute_mask_batch([seg], clicks=[_points(api, clicks)], labels=[labels], regions=[_region(api, box)],
                                                  refine_after=[spelt])[0]
        assert np.array_equal(got, delivered[i]), MI.case_id(case)
        # staged is not unstaged
        assert not np.array_equal(seg.compute_mask_clicks(_points(api, clicks), labels, _region(api, box)), delivered[i])
    # the device form, all cases in one call
    extents = [(m.shape[1], m.shape[0]) for m in delivered]
    total = sum(w * h for w, h in extents)
    dev = api.ext.device_alloc(env, total)
    try:
        api.ext.copy_to_device(env, dev, np.full(total, 7, np.uint8))
        offsets = api.ext.compute_mask_batch_device(
            [segs[c[0]] for c in MI.CASES], dev, clicks=[_points(api, c[1]) for c in MI.CASES], labels=[c[2] for c in MI.CASES],
            regions=[_region(api, c[3]) for c in MI.CASES], refine_after=[c[4] for c in MI.CASES], root_device=0)
        got = np.empty(total, np.uint8)
        api.ext.copy_to_host(env, got, dev)
        assert len(offsets) == len(MI.CASES) and offsets[0] == 0
        for k, (w, h) in enumerate(extents):
            assert k == 0 or offsets[k] - offsets[k - 1] == extents[k - 1][0] * extents[k - 1][1]
            assert np.array_equal(got[offsets[k]:offsets[k] + w * h].reshape(h, w), delivered[k]), k
    finally:
        api.ext.device_free(env, dev)


@pytest.mark.gpu
def test_staged_and_unstaged_prompts_share_a_call(api, mi, delivered):
    env, _, segs, _ = mi
    second = {n: api.Segmentation.process(api.ImageView(MI.image(n), api.Channels.rgba), env) for n in MI.IMAGES}
    try:
        plain = [(c[0], c[1], c[2], c[3], None) for c in M.CASES[:4]] + [("square", ((300, 300),), (1,), None, None)]
        alone = [segs[c[0]].compute_mask_clicks(_points(api, c[1]), c[2], _region(api, c[3])) for c in plain]
        pool = [(c, delivered[i]) for i, c in enumerate(MI.CASES)] + list(zip(plain, alone))
        for order, handles in ((list(range(len(pool))), (segs, segs)), (list(range(len(pool)))[::-1], (segs, second)),
                               ([7, 0, 8, 5, 1, 11, 6, 2, 9, 3, 10, 4], (second, segs))):
            sel = [pool[k] for k in order]
            got = api.Segmentation.compute_mask_batch(
                [handles[j % 2][c[0]] for j, (c, _) in enumerate(sel)], clicks=[_points(api, c[1]) for c, _ in sel],
                labels=[c[2] for c, _ in sel], regions=[_region(api, c[3]) for c, _ in sel], refine_after=[c[4] for c, _ in sel])
            for j, (c, want) in enumerate(sel):
                assert np.array_equal(got[j], want), (order, j)
    finally:
        for s in second.values():
            s.close()


@pytest.mark.gpu
def test_four_threads_on_one_handle(api, mi, delivered):
    _, _, segs, _ = mi
    picks = [i for i, c in enumerate(MI.CASES) if c[0] == "wide"]
    results, errors = {}, []

    def work(t):
        try:
            for rep in range(3):
                i = picks[(t + rep) % len(picks)]
                results[(t, rep)] = (i, _staged(api, segs, MI.CASES[i]))
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 12
    for (t, rep), (i, got) in results.items():
        assert np.array_equal(got, delivered[i]), (t, rep, i)


def _raw(api, seg, handles, points, regions):
    n = len(handles)
    hs = (C.c_void_p * n)(*[None if h is None else h._handle for h in handles])
    p = (C.c_int * (2 * n))(*[v for q in points for v in q])
    r = (C.c_int * (4 * n))(*[v for q in regions for v in q])
    outs = [np.zeros((seg.extent().height, seg.extent().width), np.uint8) for _ in range(n)]
    ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    api._check(api.api().get_segmentation_masks(hs, n, p, r, ptrs))
    return outs


@pytest.mark.gpu
def test_refusals_name_the_mark(api, mi, delivered):
    _, _, segs, _ = mi
    case = MI.CASES[0]
    seg = segs[case[0]]
    a, b = case[1]
    refused = [([seg, None, None, None], [a, a, a, b], [EMPTY, MARK, MARK, (0, 0, 0, 0)]),      # a mark directly after a mark
               ([seg, None, None], [a, b, b], [EMPTY, (0, 0, 0, 0), MARK]),                     # a mark as the last entry
               ([seg, None, seg], [a, b, a], [EMPTY, MARK, EMPTY]),                             # ... of its prompt
               ([seg, None, None], [a, a, b], [EMPTY, (4, 0, 0, 5), (0, 0, 0, 0)]),             # trailing ints
               ([seg, None, None], [a, a, b], [EMPTY, (4, 0, 1, 0), (0, 0, 0, 0)])]
    for handles, points, regions in refused:
        with pytest.raises(api.Error, match="mark"):
            _raw(api, seg, handles, points, regions)
        assert np.array_equal(_staged(api, segs, case), delivered[0])
    # the wrapper's builder refuses before anything reaches the library
    with pytest.raises(api.Error):
        seg.compute_mask_clicks(_points(api, case[1]), case[2], refine_after=[2])
    # the point of a mark is not read
    assert np.array_equal(_raw(api, seg, [seg, None, None], [a, (-9999, 123456), b], [EMPTY, MARK, (0, 0, 0, 0)])[0], delivered[0])


@pytest.mark.gpu
def test_model_without_the_branch(api, mi, model_dirs):
    _, _, segs, _ = mi
    mdir, _, _ = model_dirs("vit_test")
    env = api.Environment(api.Options(api.Backend.gpu, mdir))
    bare = {n: api.Segmentation.process(api.ImageView(MI.image(n), api.Channels.rgba), env) for n in MI.IMAGES}
    try:
        def serve():
            # every other tensor of the two files is the same, so the masks are those of the model with the branch
            for name, clicks, labels, box in M.CASES:
                got = bare[name].compute_mask_clicks(_points(api, clicks), labels, _region(api, box))
                assert np.array_equal(got, segs[name].compute_mask_clicks(_points(api, clicks), labels, _region(api, box)))
        serve()
        for case in (MI.CASES[0], MI.CASES[3]):
            with pytest.raises(api.Error, match=r"mark.*pe\.mask"):
                _staged(api, bare, case)
        a, b = MI.CASES[0][1]
        with pytest.raises(api.Error, match="mark"):
            _raw(api, bare["square"], [bare["square"], None, None], [a, a, b], [EMPTY, MARK, MARK])
        serve()
    finally:
        for s in bare.values():
            s.close()
        env.close()
