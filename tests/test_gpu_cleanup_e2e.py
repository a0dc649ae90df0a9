"""Clean-up marks through the public calls: a prompt whose last entry is {6, max_hole, max_island, 0} delivers exactly
cleanup_ref(the mask of the same call without the mark) -- bit for bit, the numpy reference of tests/cleanup_ref.py applied to
what the library itself delivers unmarked.

* every prompt kind (a point, a box alone without `points`, box + point, four clicks with a background click, a staged prompt
  with refinement marks) on a 1024 x 1024 and an 1800 x 1200 image, and one case on a SAM-HQ model;
* a mixed call: the unmarked prompts' masks are today's; destinations in the caller's own buffer and in an Image of the table
  (pinned) -- one-prompt calls, which take the direct mode without the mark; the device form with out_offsets, in place and
  through the staging + peer-copy path; four threads; the raw refusals, each followed by a query that still works;
* not vacuous: for at least half of the cases the cleaned mask differs from the raw one (asserted, not skipped).
"""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import hq_cases as H
from cleanup_ref import cleanup_ref
from conftest import synthetic_image

pytestmark = pytest.mark.gpu

EMPTY, MARK = (0, 0, -1, -1), (4, 0, 0, 0)
IMAGES = {"square": (0, 1024, 1024), "big": (3, 1800, 1200)}

# (image, kind, arguments of the kind, (max_hole, max_island)).  Thresholds in pixels of the delivered mask.
CASES = [
    ("square", "point", ((512, 512),), (4096, 4096)),
    ("square", "box", ((257, 264, 580, 567),), (4096, 0)),
    ("square", "box_point", ((257, 264, 580, 567), (312, 487)), (0, 4096)),
    ("square", "clicks", (((300, 300), (700, 650), (512, 200), (150, 820)), (1, 1, 0, 1), None), (4096, 4096)),
    ("square", "staged", (((300, 300), (700, 650), (512, 200)), (1, 0, 1), None, (1,)), (4096, 4096)),
    ("big", "point", ((900, 600),), (4096, 4096)),
    ("big", "box", ((300, 200, 1500, 1000),), (0, 4096)),
    ("big", "box_point", ((300, 200, 1500, 1000), (820, 640)), (4096, 0)),
    ("big", "clicks", (((400, 300), (1400, 900), (900, 100), (200, 1100)), (1, 1, 0, 1), (100, 50, 1700, 1150)), (512, 20000)),
    ("big", "staged", (((400, 300), (1400, 900), (900, 600)), (1, 1, 0), (100, 50, 1700, 1150), "each"), (4096, 4096)),
]
IDS = [f"{c[0]}-{c[1]}-h{c[3][0]}-i{c[3][1]}" for c in CASES]


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


@pytest.fixture(scope="module")
def world(api, tmp_path_factory):
    """(env, {image name: Segmentation}); a vit_test model with the mask branch (the staged cases need it)"""
    from dlimgedit_amd import weights as W
    from dlimgedit_amd.sam_config import get_config
    mdir = tmp_path_factory.mktemp("models_vit_test_cleanup")
    W.write_synthetic_model_dir(mdir, get_config("vit_test"), 7, mask_branch=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    segs = {n: api.Segmentation.process(api.ImageView(synthetic_image(s, width=w, height=h), api.Channels.rgba), env)
            for n, (s, w, h) in IMAGES.items()}
    yield env, segs
    for s in segs.values():
        s.close()
    env.close()


def _region(api, box):
    return None if box is None else api.Region(api.Point(box[0], box[1]), api.Point(box[2], box[3]))


def _run(api, seg, kind, args, clean, out=None):
    outs = None if out is None else [out]
    cl = None if clean is None else [clean]
    if kind == "point":
        return api.Segmentation.compute_mask_batch([seg], points=[api.Point(*args[0])], out=outs, clean=cl)[0]
    if kind == "box":
        return api.Segmentation.compute_mask_batch([seg], regions=[_region(api, args[0])], out=outs, clean=cl)[0]
    if kind == "box_point":
        return api.Segmentation.compute_mask_batch([seg], points=[api.Point(*args[1])], regions=[_region(api, args[0])], out=outs,
                                                   clean=cl)[0]
    clicks, labels, box = args[:3]
    after = args[3] if kind == "staged" else None
    return seg.compute_mask_clicks([api.Point(*c) for c in clicks], labels, _region(api, box), out=out, refine_after=after, clean=clean)


@pytest.fixture(scope="module")
def delivered(api, world):
    """case index -> (the raw mask, the cleaned mask), once"""
    _, segs = world
    out = []
    for name, kind, args, clean in CASES:
        raw = _run(api, segs[name], kind, args, None).copy()
        out.append((raw, _run(api, segs[name], kind, args, clean).copy()))
    return out


@pytest.fixture(scope="module")
def wanted(delivered):
    return [cleanup_ref(raw, *CASES[i][3]) for i, (raw, _) in enumerate(delivered)]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_cleaned_mask_is_the_reference_of_the_raw_mask(delivered, wanted, i):
    raw, got = delivered[i]
    assert got.shape == raw.shape and set(np.unique(got)) <= {0, 255}
    changed = int((got != raw).sum())
    print(f"cleanup.e2e.{IDS[i]}: {changed} of {raw.size} pixels changed by the clean-up")
    assert np.array_equal(got, wanted[i]), f"{int((got != wanted[i]).sum())} pixels differ from the reference"


def test_at_least_half_of_the_cases_change(delivered):
    changed = [bool((got != raw).any()) for raw, got in delivered]
    assert sum(changed) * 2 >= len(CASES), changed


def test_mixed_call_leaves_unmarked_prompts_alone(api, world, delivered, wanted):
    _, segs = world
    picks = [3, 0, 8, 4, 5]                  # multi-click and staged prompts on both images
    marked = [True, False, True, True, False]
    clicks, labels, regions, after, clean, handles = [], [], [], [], [], []
    for i, m in zip(picks, marked):
        name, kind, args, th = CASES[i]
        if kind == "point":
            args = ((args[0],), (1,), None)
        handles.append(segs[name])
        clicks.append([api.Point(*c) for c in args[0]])
        labels.append(args[1])
        regions.append(_region(api, args[2]))
        after.append(args[3] if kind == "staged" else None)
        clean.append(th if m else None)
    got = api.Segmentation.compute_mask_batch(handles, clicks=clicks, labels=labels, regions=regions, refine_after=after, clean=clean)
    for k, (i, m) in enumerate(zip(picks, marked)):
        assert np.array_equal(got[k], wanted[i] if m else delivered[i][0]), (k, i, m)
    # the points / regions form, two prompts, only the second one marked
    got = api.Segmentation.compute_mask_batch([segs["square"], segs["big"]], points=[api.Point(512, 512), api.Point(900, 600)],
                                              clean=[None, CASES[5][3]])
    assert np.array_equal(got[0], delivered[0][0]) and np.array_equal(got[1], wanted[5])


def test_destinations_own_buffer_and_pinned_image(api, world, delivered, wanted):
    """One-prompt calls: without the mark each takes the direct mode (the kernel writes pinned memory), with it the staged one."""
    _, segs = world
    for i in (0, 5):
        name, kind, args, clean = CASES[i]
        own = np.full(delivered[i][0].shape, 7, np.uint8)
        assert not api.ext.image_memory_is_pinned(own)
        assert _run(api, segs[name], kind, args, clean, out=own) is own and np.array_equal(own, wanted[i])
        image = _run(api, segs[name], kind, args, clean)              # an Image of the table: pinned image memory
        assert api.ext.image_memory_is_pinned(image) and np.array_equal(image, wanted[i])
        # ... and the unmarked call into the same buffers is today's
        assert np.array_equal(_run(api, segs[name], kind, args, None, out=own), delivered[i][0])


def test_device_form(api, world, delivered, wanted):
    env, segs = world
    picks = [0, 7, 2]                        # a point, and a box + point on either image
    sizes = [delivered[i][0].size for i in picks]
    total = sum(sizes)
    dev = api.ext.device_alloc(env, total)
    try:
        def call(force_peer, root=0):
            api.ext.copy_to_device(env, dev, np.full(total, 7, np.uint8))
            if force_peer:
                os.environ["DLIMGEDIT_FORCE_PEER_COPY"] = "1"
            try:
                handles = [segs["square"], None, segs["big"], None, segs["square"], None]
                points = [(512, 512), (0, 0), (820, 640), (0, 0), (312, 487), (0, 0)]
                regions = [EMPTY, (6, *CASES[0][3], 0), (300, 200, 1500, 1000), (6, *CASES[7][3], 0),
                           (257, 264, 580, 567), (6, *CASES[2][3], 0)]
                n = len(handles)
                hs = (C.c_void_p * n)(*[None if h is None else h._handle for h in handles])
                p = (C.c_int * (2 * n))(*[v for q in points for v in q])
                r = (C.c_int * (4 * n))(*[v for q in regions for v in q])
                offsets = (C.c_size_t * n)()
                api._check(api.ext._l().dlimg_amd_get_segmentation_masks_device(hs, n, p, r, root, dev, offsets))
            finally:
                os.environ.pop("DLIMGEDIT_FORCE_PEER_COPY", None)
            got = np.empty(total, np.uint8)
            api.ext.copy_to_host(env, got, dev)
            return list(offsets), got

        for force_peer in (False, True):
            offsets, got = call(force_peer)
            # one offset per prompt; a mark repeats its head's
            assert offsets == [0, 0, sizes[0], sizes[0], sizes[0] + sizes[1], sizes[0] + sizes[1]]
            for k, i in enumerate(picks):
                at = offsets[2 * k]
                assert np.array_equal(got[at:at + sizes[k]].reshape(delivered[i][0].shape), wanted[i]), (force_peer, i)
        # the wrapper's device form with `clean`, a box-only call
        api.ext.copy_to_device(env, dev, np.full(total, 7, np.uint8))
        offs = api.ext.compute_mask_batch_device([segs["big"]], dev, regions=[_region(api, CASES[6][2][0])], clean=[CASES[6][3]])
        got = np.empty(sizes[1], np.uint8)
        api.ext.copy_to_host(env, got, dev + offs[0])
        assert offs == [0] and np.array_equal(got.reshape(delivered[6][0].shape), wanted[6])
        if api.ext.device_count() >= 2:
            # masks produced on the embedding's GPU, cleaned there, delivered to another one
            import torch
            other = torch.empty(total, dtype=torch.uint8, device="cuda:1")
            hs = (C.c_void_p * 2)(segs["square"]._handle, None)
            p = (C.c_int * 4)(512, 512, 0, 0)
            r = (C.c_int * 8)(*EMPTY, 6, *CASES[0][3], 0)
            offsets = (C.c_size_t * 2)()
            api._check(api.ext._l().dlimg_amd_get_segmentation_masks_device(hs, 2, p, r, 1, other.data_ptr(), offsets))
            assert np.array_equal(other[:sizes[0]].cpu().numpy().reshape(delivered[0][0].shape), wanted[0])
    finally:
        api.ext.device_free(env, dev)


def test_four_threads_issue_the_same_cleaned_call(api, world, wanted):
    _, segs = world
    name, kind, args, clean = CASES[8]
    results, errors = {}, []

    def work(t):
        try:
            for rep in range(2):
                results[(t, rep)] = _run(api, segs[name], kind, args, clean).copy()
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 8
    for key, got in results.items():
        assert np.array_equal(got, wanted[8]), key


def _raw(api, seg, handles, points, regions):
    n = len(handles)
    hs = (C.c_void_p * n)(*[None if h is None else h._handle for h in handles])
    p = None if points is None else (C.c_int * (2 * n))(*[v for q in points for v in q])
    r = (C.c_int * (4 * n))(*[v for q in regions for v in q])
    outs = [np.zeros((seg.extent().height, seg.extent().width), np.uint8) for _ in range(n)]
    ptrs = (C.c_void_p * n)(*[o.ctypes.data if h is not None else None for o, h in zip(outs, handles)])
    api._check(api.api().get_segmentation_masks(hs, n, p, r, ptrs))
    return outs


def test_raw_refusals_leave_the_handle_working(api, world, delivered, wanted):
    _, segs = world
    seg = segs["square"]
    a, b = (512, 512), (300, 300)
    BOX = (257, 264, 580, 567)
    refused = [
        ([seg, None, None], [a, a, b], [EMPTY, (6, 3, 3, 0), (1, 0, 0, 0)], 1),                 # not the last entry of its prompt
        ([seg, None, None], [a, a, a], [EMPTY, (6, 3, 3, 0), (6, 4, 4, 0)], 1),                 # two marks
        ([None, seg], [a, a], [(6, 3, 3, 0), EMPTY], 0),                                        # in front of any head
        ([seg, None], [a, a], [EMPTY, (6, 0, 0, 0)], 1),                                        # both thresholds 0
        ([seg, None], [a, a], [EMPTY, (6, -1, 5, 0)], 1),                                       # negative
        ([seg, None], [a, a], [EMPTY, (6, 3, 3, 9)], 1),                                        # the fourth int
        ([seg, None, None, None], [a, b, a, a], [EMPTY, (1, 0, 0, 0), MARK, (6, 3, 3, 0)], 2),   # a refinement mark is never last
        ([seg, None], None, [EMPTY, (6, 3, 3, 0)], 0),                                          # neither a click nor a box
    ]
    for handles, points, regions, at in refused:
        with pytest.raises(api.Error, match=f"entry {at}:.*mark"):
            _raw(api, seg, handles, points, regions)
        assert np.array_equal(_run(api, seg, *CASES[0][1:3], CASES[0][3]), wanted[0])
    # a click without `points` keeps its words, and 5 is still a refused label
    with pytest.raises(api.Error, match="is a click and needs `points`"):
        _raw(api, seg, [seg, None, None], None, [BOX, (1, 0, 0, 0), (6, 3, 3, 0)])
    with pytest.raises(api.Error, match="label"):
        _raw(api, seg, [seg, None], [a, a], [EMPTY, (5, 3, 3, 0)])
    # the point of a mark is not read; a box-only call with a mark is served
    got = _raw(api, seg, [seg, None], [a, (-9999, 123456)], [EMPTY, (6, *CASES[0][3], 0)])[0]
    assert np.array_equal(got, wanted[0])
    got = _raw(api, seg, [seg, None], None, [BOX, (6, *CASES[1][3], 0)])[0]
    assert np.array_equal(got, wanted[1])
    assert np.array_equal(_run(api, seg, *CASES[0][1:3], None), delivered[0][0])


def test_hq_model_takes_clean_marks(api, tmp_path_factory):
    from dlimgedit_amd import weights as W
    mdir = tmp_path_factory.mktemp("models_hqtest_cleanup")
    W.write_synthetic_model_dir(mdir, H.CFG, H.SEED, mask_branch=True, hq=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    seg = api.Segmentation.process(api.ImageView(H.image("square"), api.Channels.rgba), env)
    try:
        _, clicks, labels, box, _ = H.CASES[2]                # box plus point
        pts = [api.Point(*c) for c in clicks]
        raw = seg.compute_mask_clicks(pts, labels, _region(api, box)).copy()
        got = seg.compute_mask_clicks(pts, labels, _region(api, box), clean=(4096, 4096))
        print(f"cleanup.e2e.hq: {int((got != raw).sum())} of {raw.size} pixels changed by the clean-up")
        assert np.array_equal(got, cleanup_ref(raw, 4096, 4096))
        # the 9-point limit is what it was: 8 clicks and a box are refused, mark or no mark
        many = [api.Point(10 * k + 5, 20) for k in range(8)]
        for clean in (None, (4096, 4096)):
            with pytest.raises(api.Error, match="more than a SAM-HQ model takes"):
                seg.compute_mask_clicks(many, None, _region(api, box), clean=clean)
    finally:
        seg.close()
        env.close()
