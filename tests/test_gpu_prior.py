"""Prior marks on the GPU: a continuation entry {8, strength_milli, 0, 0} directly behind its head hands the prompt a mask of the
caller's own -- out_masks[] of the mark is READ -- as SAM's mask input of the prompt's first stage (kernels/mask_prior.hip makes
the plane, kernels/decoder.hip takes it: mask_embed_kernel and the masked decoder_start_kernel, for the first time at 7 token
rows).  On the parent commit 8 is a refused label: every test here that sends the mark fails there.

* exact stage: every case of tests/prior_cases.py against the float64 chain on the GPU's own embedding, started from the plane
  tests/prior_ref.py defines (which the kernel reproduces bit for bit, tests/test_gpu_prior_kernel.py) -- within
  mask_input_cases.EXACT_LIMIT for one stage, CHAIN_LIMIT with a refinement mark -- and closer to it than to the reference
  without the prior;
* slot 14 called raw, the wrappers and a thread give the same bytes; prompts with and without a prior share a call in both orders,
  on one handle and on two; a mask refined in place; a prior in the table's pinned image memory; four threads on one handle;
* every refusal says "mark", names the caller's entry and leaves the handle working; a model without pe.mask.* and the device
  form refuse by name; a SAM-HQ model with the branch serves a prior.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import mask_input_cases as MI
import prior_cases as PC
from cleanup_ref import cleanup_ref
from conftest import within

IDS = [PC.case_id(c) for c in PC.CASES]
EMPTY, PRIOR = (0, 0, -1, -1), (8, 0, 0, 0)


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


@pytest.fixture(scope="module")
def world(api, tmp_path_factory):
    """(env, params, {image name: Segmentation}, {image name: its embedding as the GPU computed it}); a model WITH the branch"""
    from dlimgedit_amd import weights as W
    from dlimgedit_amd.sam_config import get_config
    mdir = tmp_path_factory.mktemp("models_vit_test_prior")
    params = W.write_synthetic_model_dir(mdir, get_config("vit_test"), 7, mask_branch=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    segs = {n: api.Segmentation.process(api.ImageView(PC.image(n), api.Channels.rgba), env) for n in PC.IMAGES}
    embs = {n: api.ext.get_embedding(s) for n, s in segs.items()}
    yield env, params, segs, embs
    for s in segs.values():
        s.close()
    env.close()


@pytest.fixture(scope="module")
def priors():
    """case index -> its prior (h, w) uint8, drawn once and never written"""
    out = [PC.draw_prior(c[0], c[4]) for c in PC.CASES]
    for m in out:
        m.setflags(write=False)
    return out


def _points(api, clicks):
    return [api.Point(*c) for c in clicks]


def _region(api, box):
    return None if box is None else api.Region(api.Point(box[0], box[1]), api.Point(box[2], box[3]))


def _rs(name):
    from oracle import sam_oracle as O
    _, w, h = PC.IMAGES[name]
    rs = O.ResizeLongestSide()
    rs.target_extent(w, h)
    return rs, (h, w)


def _run(api, segs, case, prior, out=None, strength=0):
    """The case through the Python wrapper; prior None: the same prompt without one."""
    name, clicks, labels, box, _, after, clean = case
    seg = segs[name] if isinstance(segs, dict) else segs
    if clicks:
        return seg.compute_mask_clicks(_points(api, clicks), labels, _region(api, box), out=out, refine_after=after, clean=clean,
                                       prior=prior, prior_strength=strength)
    return api.Segmentation.compute_mask_batch([seg], regions=[_region(api, box)], out=None if out is None else [out],
                                               clean=None if clean is None else [clean], prior=None if prior is None else [prior],
                                               prior_strength=strength)[0]


@pytest.fixture(scope="module")
def delivered(api, world, priors):
    """case index -> the mask the wrapper delivers, once"""
    _, _, segs, _ = world
    return [_run(api, segs, case, priors[i]).copy() for i, case in enumerate(PC.CASES)]


def _cleaned(mask_bool, clean):
    m = np.where(mask_bool, 255, 0).astype(np.uint8)
    return (m if clean is None else cleanup_ref(m, *clean)) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(PC.CASES)), ids=IDS)
def test_exact_stage_and_discrimination(api, world, delivered, i):
    _, params, _, embs = world
    case = PC.CASES[i]
    name = case[0]
    rs, hw = _rs(name)
    want, plane, _ = PC.reference(embs[name], rs, case, params, hw)
    without = PC.reference_without(embs[name], rs, case, params, hw)
    want, without = _cleaned(want, case[6]), _cleaned(without, case[6])
    got = delivered[i]
    assert set(np.unique(got)) <= {0, 255}
    got = got > 0
    d_with, d_without = int((got != want).sum()), int((got != without).sum())
    fraction = d_with / got.size
    print(f"prior.exact.{PC.case_id(case)}: {d_with} of {got.size} pixels differ from the reference with the prior (fraction {fraction:.3g}, "
          f"recorded {PC.MEASURED_FRACTION[i]}), {d_without} from the reference without it; plane {plane}")
    assert plane == 0 if PC.token_rows(case)[-1] > 7 else plane in (1, 2, 3)
    assert d_with < d_without, (d_with, d_without)
    within(f"prior.exact.{PC.case_id(case)}", fraction, PC.limit_of(case))


@pytest.mark.gpu
def test_clean_up_mark_cleans_the_mask_of_the_prior_prompt(delivered):
    a, g = delivered[0], delivered[6]
    assert PC.CASES[6][:6] == PC.CASES[0][:6]
    assert np.array_equal(g, cleanup_ref(a, *PC.CASES[6][6]))


def _raw_case(api, seg, case, prior, out=None):
    """Slot 14 with hand-made arrays: the head, the prior mark directly behind it, then whatever else the prompt has."""
    name, clicks, labels, box, _, after, clean = case
    e = seg.extent()
    out = np.zeros((e.height, e.width), np.uint8) if out is None else out
    handles, points, regions, ptrs = [seg._handle], [clicks[0] if clicks else (0, 0)], [EMPTY if box is None else tuple(box)], [out.ctypes.data]
    handles.append(None); points.append((-77, 123456)); regions.append(PRIOR); ptrs.append(prior.ctypes.data)       # its point is not read
    for k in range(1, len(clicks)):
        if after and k in after:
            handles.append(None); points.append((0, 0)); regions.append((4, 0, 0, 0)); ptrs.append(None)
        handles.append(None); points.append(clicks[k]); regions.append((labels[k], 0, 0, 0)); ptrs.append(None)
    if clean:
        handles.append(None); points.append((0, 0)); regions.append((6, clean[0], clean[1], 0)); ptrs.append(None)
    n = len(handles)
    p = (C.c_int * (2 * n))(*[v for q in points for v in q]) if clicks else None
    r = (C.c_int * (4 * n))(*[v for q in regions for v in q])
    api._check(api.api().get_segmentation_masks((C.c_void_p * n)(*handles), n, p, r, (C.c_void_p * n)(*ptrs)))
    return out


@pytest.mark.gpu
def test_same_bytes_through_every_route(api, world, delivered, priors):
    _, _, segs, _ = world
    for i, case in enumerate(PC.CASES):
        seg = segs[case[0]]
        assert np.array_equal(_raw_case(api, seg, case, priors[i]), delivered[i]), PC.case_id(case)
        # the default strength spelt out; the wrapper from another thread
        assert np.array_equal(_run(api, segs, case, priors[i], strength=PC.STRENGTH), delivered[i]), PC.case_id(case)
        box = {}
        t = threading.Thread(target=lambda: box.update(got=_run(api, segs, case, priors[i])))
        t.start()
        t.join()
        assert np.array_equal(box["got"], delivered[i]), PC.case_id(case)
        # with a prior is not without one, and another prior is another mask
        assert not np.array_equal(_run(api, segs, case, None), delivered[i]), PC.case_id(case)
    other = PC.draw_prior("square", PC.OTHER_PRIOR)
    assert (_run(api, segs, PC.CASES[0], other) != delivered[0]).mean() > 10 * PC.EXACT_LIMIT


@pytest.mark.gpu
def test_prior_and_plain_prompts_share_a_call(api, world, delivered, priors):
    env, _, segs, _ = world
    second = {n: api.Segmentation.process(api.ImageView(PC.image(n), api.Channels.rgba), env) for n in PC.IMAGES}
    try:
        with_clicks = [i for i, c in enumerate(PC.CASES) if c[1]]
        pool = [(PC.CASES[i], priors[i], delivered[i]) for i in with_clicks]
        pool += [(PC.CASES[i], None, _run(api, segs, PC.CASES[i], None).copy()) for i in with_clicks[:4]]
        for order, handles in ((list(range(len(pool))), (segs, segs)), (list(range(len(pool)))[::-1], (segs, second)),
                               ([6, 0, 9, 3, 7, 1, 4, 8, 2, 5], (second, segs))):
            sel = [pool[k] for k in order]
            got = api.Segmentation.compute_mask_batch(
                [handles[j % 2][c[0]] for j, (c, _, _) in enumerate(sel)], clicks=[_points(api, c[1]) for c, _, _ in sel],
                labels=[c[2] for c, _, _ in sel], regions=[_region(api, c[3]) for c, _, _ in sel], refine_after=[c[5] for c, _, _ in sel],
                clean=[c[6] for c, _, _ in sel], prior=[p for _, p, _ in sel])
            for j, (_, _, want) in enumerate(sel):
                assert np.array_equal(got[j], want), (order, j)
        # the box-only form: a prior on one prompt of two
        b = PC.CASES[1]
        got = api.Segmentation.compute_mask_batch([second["square"], segs["square"]], regions=[_region(api, b[3])] * 2, prior=[None, priors[1]])
        assert np.array_equal(got[1], delivered[1]) and np.array_equal(got[0], _run(api, segs, b, None))
    finally:
        for s in second.values():
            s.close()


@pytest.mark.gpu
def test_a_mask_refined_in_place(api, world, delivered, priors):
    _, _, segs, _ = world
    for i in (0, 2, 5):
        case = PC.CASES[i]
        # the caller's own memory: the prior is packed into staging memory when the call is enqueued
        own = priors[i].copy()
        assert not api.ext.image_memory_is_pinned(own)
        assert _run(api, segs, case, own, out=own) is own and np.array_equal(own, delivered[i]), PC.case_id(case)
        assert np.array_equal(_raw_case(api, segs[case[0]], case, *(2 * [priors[i].copy()])), delivered[i])
        # memory of the table: the prior is copied from where it lies, in front of the decode on the same stream
        e = segs[case[0]].extent()
        image = api._mask_image(e)
        image[...] = priors[i]
        assert api.ext.image_memory_is_pinned(image)
        assert np.array_equal(_run(api, segs, case, image, out=image), delivered[i]), PC.case_id(case)


@pytest.mark.gpu
def test_a_prior_in_table_image_memory(api, world, delivered, priors):
    _, _, segs, _ = world
    for i in (1, 3):
        case = PC.CASES[i]
        image = api._mask_image(segs[case[0]].extent())
        image[...] = priors[i]
        assert api.ext.image_memory_is_pinned(image)
        assert np.array_equal(_run(api, segs, case, image), delivered[i]), PC.case_id(case)
        assert np.array_equal(image, priors[i])                                    # the call only reads it
        own = np.full(delivered[i].shape, 7, np.uint8)
        assert np.array_equal(_run(api, segs, case, image, out=own), delivered[i])


@pytest.mark.gpu
def test_four_threads_on_one_handle(api, world, delivered, priors):
    _, _, segs, _ = world
    picks = [i for i, c in enumerate(PC.CASES) if c[0] == "wide"]
    results, errors = {}, []

    def work(t):
        try:
            for rep in range(3):
                i = picks[(t + rep) % len(picks)]
                results[(t, rep)] = (i, _run(api, segs, PC.CASES[i], priors[i]).copy())
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


def _raw(api, seg, handles, points, regions, prior_at=(), prior=None):
    n = len(handles)
    hs = (C.c_void_p * n)(*[None if h is None else h._handle for h in handles])
    p = None if points is None else (C.c_int * (2 * n))(*[v for q in points for v in q])
    r = (C.c_int * (4 * n))(*[v for q in regions for v in q])
    outs = [np.zeros((seg.extent().height, seg.extent().width), np.uint8) for _ in range(n)]
    ptrs = (C.c_void_p * n)(*[o.ctypes.data if h is not None else (prior.ctypes.data if k in prior_at else None)
                              for k, (o, h) in enumerate(zip(outs, handles))])
    api._check(api.api().get_segmentation_masks(hs, n, p, r, ptrs))
    return outs


@pytest.mark.gpu
def test_refusals_name_the_mark_and_leave_the_handle_working(api, world, delivered, priors):
    _, _, segs, _ = world
    seg, prior = segs["square"], priors[0]
    a, b = PC.CASES[5][1]
    BOX = tuple(PC.CASES[1][3])
    refused = [
        ([None, seg], [a, a], [PRIOR, EMPTY], (0,), 0),                                     # in front of any head
        ([seg, None, None], [a, b, a], [EMPTY, (0, 0, 0, 0), PRIOR], (2,), 2),              # behind a click, not its head
        ([seg, None, None, None], [a, a, a, b], [EMPTY, (4, 0, 0, 0), PRIOR, (0, 0, 0, 0)], (2,), 2),      # behind a refinement mark
        ([seg, None], [a, a], [EMPTY, PRIOR], (), 1),                                       # a NULL prior
        ([seg, None], [a, a], [EMPTY, (8, -1, 0, 0)], (1,), 1),                             # a negative strength
        ([seg, None], [a, a], [EMPTY, (8, 100001, 0, 0)], (1,), 1),                         # one above 100000
        ([seg, None], [a, a], [EMPTY, (8, 0, 3, 0)], (1,), 1),                              # trailing ints
        ([seg, None], [a, a], [EMPTY, (8, 0, 0, 3)], (1,), 1),
        ([seg, None, None], [a, a, a], [EMPTY, PRIOR, PRIOR], (1, 2), 2),                   # a second prior mark
        ([seg, None, None], [a, a, a], [EMPTY, PRIOR, (7, 4, 0, 0)], (1,), 1),              # a grid prompt
        ([seg, None], None, [EMPTY, PRIOR], (1,), 1),                                       # neither a click nor a box
    ]
    for handles, points, regions, prior_at, at in refused:
        with pytest.raises(api.Error, match=f"entry {at}:.*mark"):
            _raw(api, seg, handles, points, regions, prior_at, prior)
        assert np.array_equal(_run(api, segs, PC.CASES[0], prior), delivered[0])
    # 9 is still a refused label, and a click without `points` keeps its words
    with pytest.raises(api.Error, match="label"):
        _raw(api, seg, [seg, None], [a, a], [EMPTY, (9, 0, 0, 0)])
    with pytest.raises(api.Error, match="is a click and needs `points`"):
        _raw(api, seg, [seg, None, None], None, [BOX, PRIOR, (1, 0, 0, 0)], (1,), prior)
    # the wrapper refuses a prior of another extent before anything reaches the library
    with pytest.raises(api.Error, match="prior"):
        _run(api, segs, PC.CASES[0], np.zeros((600, 800), np.uint8))
    assert np.array_equal(_run(api, segs, PC.CASES[0], prior), delivered[0])


@pytest.mark.gpu
def test_the_device_form_refuses_by_name(api, world, delivered, priors):
    env, _, segs, _ = world
    seg, prior = segs["square"], priors[0]
    dev = api.ext.device_alloc(env, prior.size)
    try:
        hs = (C.c_void_p * 2)(seg._handle, None)
        p = (C.c_int * 4)(*PC.CASES[0][1][0], 0, 0)
        r = (C.c_int * 8)(*EMPTY, *PRIOR)
        offsets = (C.c_size_t * 2)()
        with pytest.raises(api.Error, match=r"entry 1:.*prior mark.*dlimg_amd_get_segmentation_masks_device"):
            api._check(api.ext._l().dlimg_amd_get_segmentation_masks_device(hs, 2, p, r, 0, dev, offsets))
    finally:
        api.ext.device_free(env, dev)
    assert np.array_equal(_run(api, segs, PC.CASES[0], prior), delivered[0])


@pytest.mark.gpu
def test_model_without_the_branch_refuses_by_name(api, world, delivered, priors, model_dirs):
    _, _, segs, _ = world
    mdir, _, _ = model_dirs("vit_test")
    env = api.Environment(api.Options(api.Backend.gpu, mdir))
    bare = api.Segmentation.process(api.ImageView(PC.image("square"), api.Channels.rgba), env)
    try:
        plain = _run(api, bare, PC.CASES[0], None).copy()
        # every other tensor of the two files is the same, so the mask without a prior is that of the model with the branch
        assert np.array_equal(plain, _run(api, segs, PC.CASES[0], None))
        for i in (0, 1, 5):
            with pytest.raises(api.Error, match=r"entry 1:.*prior mark.*pe\.mask"):
                _run(api, bare, PC.CASES[i], priors[i])
        assert np.array_equal(_run(api, bare, PC.CASES[0], None), plain)
    finally:
        bare.close()
        env.close()


@pytest.mark.gpu
def test_hq_model_serves_a_prior(api, tmp_path_factory):
    import hq_cases as H
    from dlimgedit_amd import weights as W
    mdir = tmp_path_factory.mktemp("models_hqtest_prior")
    W.write_synthetic_model_dir(mdir, H.CFG, H.SEED, mask_branch=True, hq=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    img = H.image("square")
    seg = api.Segmentation.process(api.ImageView(img, api.Channels.rgba), env)
    try:
        h, w = img.shape[:2]
        yy, xx = np.mgrid[0:h, 0:w]
        prior = np.where(((xx - 0.4 * w) / (0.3 * w)) ** 2 + ((yy - 0.5 * h) / (0.25 * h)) ** 2 <= 1, 255, 0).astype(np.uint8)
        pts = [api.Point(int(0.4 * w), int(0.5 * h))]
        first = seg.compute_mask_clicks(pts, prior=prior).copy()
        again = seg.compute_mask_clicks(pts, prior=prior)
        plain = seg.compute_mask_clicks(pts)
        print(f"prior.hq: {int((first != plain).sum())} of {first.size} pixels moved by the prior")
        assert set(np.unique(first)) <= {0, 255} and np.array_equal(first, again) and not np.array_equal(first, plain)
    finally:
        seg.close()
        env.close()
