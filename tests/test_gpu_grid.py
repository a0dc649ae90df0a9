"""Grid prompts ("segment everything") through the public calls: a prompt of two entries, a head with an empty region and
{7, side, iou_permille, stability_permille}, delivers a label map that EQUALS the numpy restatement (tests/grid_ref.py) applied
to what the existing single-prompt query (ext.get_logits, the decoder as it stands) returns for every pixel of the grid.

* the comparison is exact because a chunked decode is bit-identical to single decodes: asserted first, on one chunk;
* thresholds come from each case's data (tests/grid_cases.py); the cases are not trivial: at least two segments kept in every
  case, and over the cases each of the three steps (IoU, stability, NMS) rejects a candidate -- on synthetic weights whose
  masks are made sparse for it (grid_cases.sparse_mask_weights);
* the same call through table slot 14, the Python entries, the two entries the C++ wrapper builds, and the device form (in
  place, through the staging + peer-copy path, and with the root on another GPU where there is one);
* a mixed call, two threads on two handles, a SAM-HQ model, and the refusals, each followed by a query that still works.
"""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import grid_cases as GC
import grid_ref as G
import hq_cases as H
from cleanup_ref import cleanup_ref
from conftest import synthetic_image

pytestmark = pytest.mark.gpu

EMPTY = (0, 0, -1, -1)


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


@pytest.fixture(scope="module")
def world(api, tmp_path_factory):
    from dlimgedit_amd.sam_config import get_config
    mdir = tmp_path_factory.mktemp("models_vit_test_grid")
    GC.write_model_dir(mdir, get_config("vit_test"))        # synthetic weights whose masks are sparse (grid_cases.py says why)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    segs = {n: api.Segmentation.process(api.ImageView(synthetic_image(s, width=w, height=h), api.Channels.rgba), env)
            for n, (s, w, h) in GC.IMAGES.items()}
    yield env, segs
    for s in segs.values():
        s.close()
    env.close()


def _reference(api, seg, w, h, side):
    """What the definition gives for one case from the decoder as it stands: one single-prompt query per grid pixel."""
    singles = [api.ext.get_logits(seg, point=api.Point(x, y)) for x, y in G.grid_pixels(w, h, side)]
    planes4 = np.stack([s[0] for s in singles])
    iou4 = np.stack([s[1] for s in singles])
    records = G.harvest(G.candidates_of(planes4), *G.pre_extent(w, h))
    iou = iou4[:, 1:].reshape(-1)
    ip, sp = GC.thresholds(records, iou)
    want, _, nms, kept = G.label_map(planes4, iou4, w, h, ip, sp)
    return dict(planes4=planes4, iou4=iou4, records=records, iou=iou, ip=ip, sp=sp, want=want, nms=nms, kept=kept)


@pytest.fixture(scope="module")
def reference(api, world):
    _, segs = world
    return [_reference(api, segs[name], *GC.IMAGES[name][1:], side) for name, side in GC.CASES]


def _same_map(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.uint8
    if not np.array_equal(got, want):
        ys, xs = np.nonzero(got != want)
        raise AssertionError(f"{what}: {len(ys)} of {got.size} pixels differ, the first at (x={xs[0]}, y={ys[0]}): got {got[ys[0], xs[0]]}, "
                             f"want {want[ys[0], xs[0]]}")


def test_a_chunked_decode_is_bit_identical_to_single_decodes(api, world, reference):
    """What makes the exact comparison below legitimate: the 16 prompts of the first case as ONE decode (the existing hook over
    SamModel::decode, which is what a grid prompt calls per chunk) against the same prompts one by one."""
    from oracle import sam_oracle as O
    env, segs = world
    name, side = GC.CASES[0]
    _, w, h = GC.IMAGES[name]
    rs = O.ResizeLongestSide()
    rs.target_extent(w, h)
    px = G.grid_pixels(w, h, side)
    coords = np.array([[rs.transform(x, y), (0, 0)] for x, y in px], np.float32)
    labels = np.array([[1, -1]] * len(px), np.float32)
    logits, iou = api.ext.test_decode_prompts(env, api.ext.get_embedding(segs[name])[None], [0] * len(px), coords, labels)
    assert np.array_equal(logits.view(np.uint32), reference[0]["planes4"].view(np.uint32))
    assert np.array_equal(iou.view(np.uint32), reference[0]["iou4"].view(np.uint32))


def test_cases_are_not_trivial(reference):
    """At least two segments kept in every case, and over the cases every step rejects a candidate.  The weights are made for
    it (grid_cases.sparse_mask_weights): with plain random weights every candidate's box is the whole image and NMS keeps one."""
    total = np.zeros(3, int)
    for case, ref in zip(GC.IDS, reference):
        by_iou, by_stab, by_nms, kept = GC.rejections(ref["records"], ref["iou"], ref["ip"], ref["sp"])
        print(f"grid.e2e.{case}: thresholds {ref['ip']} / {ref['sp']}, rejected by IoU {by_iou}, stability {by_stab}, NMS {by_nms}, kept {kept}")
        assert kept >= 2, case
        total += (by_iou, by_stab, by_nms)
    assert (total >= 1).all(), total


@pytest.mark.parametrize("i", range(len(GC.CASES)), ids=GC.IDS)
def test_label_map_equals_the_reference(api, world, reference, i):
    _, segs = world
    name, side = GC.CASES[i]
    ref = reference[i]
    got = segs[name].segment_everything(side, ref["ip"], ref["sp"])
    assert api.ext.image_memory_is_pinned(got)                   # an Image of the table, as a mask is
    _same_map(got, ref["want"], GC.IDS[i])
    print(f"grid.e2e.{GC.IDS[i]}: {len(ref['kept'])} kept, {len(np.unique(got)) - 1} of them show in the map, {int((got > 0).sum())} pixels labelled")
    assert int(got.max()) <= len(ref["kept"])


def _raw(api, seg, handles, points, regions, outs=None):
    n = len(handles)
    hs = (C.c_void_p * n)(*[None if h is None else h._handle for h in handles])
    p = None if points is None else (C.c_int * (2 * n))(*[v for q in points for v in q])
    r = (C.c_int * (4 * n))(*[v for q in regions for v in q])
    if outs is None:
        outs = [np.full((h.extent().height, h.extent().width), 9, np.uint8) if h is not None else None for h in handles]
    ptrs = (C.c_void_p * n)(*[None if o is None else o.ctypes.data for o in outs])
    api._check(api.api().get_segmentation_masks(hs, n, p, r, ptrs))
    return outs


def test_every_entry_point_delivers_the_same_map(api, world, reference):
    env, segs = world
    i = 1                                                        # the image with a padded band, a ragged last chunk
    name, side = GC.CASES[i]
    seg, ref = segs[name], reference[i]
    mark = (api.GRID_MARK, side, ref["ip"], ref["sp"])
    # table slot 14: with `points` (not read) and without (what the C++ wrapper's segment_everything passes), the caller's buffer
    _same_map(_raw(api, seg, [seg, None], [(-5, 10 ** 6), (7, 7)], [EMPTY, mark])[0], ref["want"], "slot 14")
    _same_map(_raw(api, seg, [seg, None], None, [EMPTY, mark])[0], ref["want"], "slot 14 without points")
    # Python: the method, its `out` form, the batch call in both forms
    own = np.full(ref["want"].shape, 9, np.uint8)
    assert seg.segment_everything(side, ref["ip"], ref["sp"], out=own) is own
    _same_map(own, ref["want"], "out=")
    _same_map(api.Segmentation.compute_mask_batch([seg], grid=[mark[1:]])[0], ref["want"], "batch")
    _same_map(api.Segmentation.compute_mask_batch([seg], clicks=[None], grid=[mark[1:]])[0], ref["want"], "batch, clicks form")
    # the device form, root on the GPU of the embedding: in place, and through the staging + peer-copy path
    size = ref["want"].size
    dev = api.ext.device_alloc(env, size + 64)
    try:
        for force_peer in (False, True):
            api.ext.copy_to_device(env, dev, np.full(size + 64, 9, np.uint8))
            if force_peer:
                os.environ["DLIMGEDIT_FORCE_PEER_COPY"] = "1"
            try:
                hs = (C.c_void_p * 2)(seg._handle, None)
                r = (C.c_int * 8)(*EMPTY, *mark)
                offsets = (C.c_size_t * 2)(5, 5)
                api._check(api.ext._l().dlimg_amd_get_segmentation_masks_device(hs, 2, None, r, 0, dev, offsets))
            finally:
                os.environ.pop("DLIMGEDIT_FORCE_PEER_COPY", None)
            assert list(offsets) == [0, 0]                       # the mark repeats its head's
            got = np.empty(size + 64, np.uint8)
            api.ext.copy_to_host(env, got, dev)
            _same_map(got[:size].reshape(ref["want"].shape), ref["want"], f"device form, peer {force_peer}")
            assert (got[size:] == 9).all()
        api.ext.copy_to_device(env, dev, np.full(size + 64, 9, np.uint8))
        assert api.ext.compute_mask_batch_device([seg], dev, grid=[mark[1:]]) == [0]
        got = np.empty(size + 64, np.uint8)
        api.ext.copy_to_host(env, got, dev)
        _same_map(got[:size].reshape(ref["want"].shape), ref["want"], "device form, wrapper")
    finally:
        api.ext.device_free(env, dev)


def test_device_form_with_the_root_on_another_gpu(api, world, reference):
    if api.ext.device_count() < 2:
        pytest.skip("one GPU visible")
    import torch
    _, segs = world
    name, side = GC.CASES[1]
    seg, ref = segs[name], reference[1]
    other = torch.full((ref["want"].size,), 9, dtype=torch.uint8, device="cuda:1")
    hs = (C.c_void_p * 2)(seg._handle, None)
    r = (C.c_int * 8)(*EMPTY, api.GRID_MARK, side, ref["ip"], ref["sp"])
    offsets = (C.c_size_t * 2)()
    api._check(api.ext._l().dlimg_amd_get_segmentation_masks_device(hs, 2, None, r, 1, other.data_ptr(), offsets))
    _same_map(other.cpu().numpy().reshape(ref["want"].shape), ref["want"], "root on another GPU")


def test_mixed_call_every_mask_is_what_it_is_alone(api, world, reference):
    """A grid prompt between an 8-click prompt and a cleaned box prompt, in one call."""
    _, segs = world
    sq, band = segs["square"], segs["band"]
    ref = reference[1]                                           # band, side 5
    clicks = [(300, 300), (700, 650), (512, 200), (150, 820), (800, 800), (100, 100), (900, 300), (512, 900)]
    labels = [1, 1, 0, 1, 0, 1, 1, 0]
    box, at, clean = (257, 264, 580, 567), (312, 487), (4096, 4096)
    alone_clicks = sq.compute_mask_clicks([api.Point(*c) for c in clicks], labels).copy()
    alone_box = api.Segmentation.compute_mask_batch([sq], points=[api.Point(*at)], regions=[api.Region(api.Point(*box[:2]), api.Point(*box[2:]))],
                                                    clean=[clean])[0].copy()
    raw_box = api.Segmentation.compute_mask_batch([sq], points=[api.Point(*at)], regions=[api.Region(api.Point(*box[:2]), api.Point(*box[2:]))])[0]
    assert np.array_equal(alone_box, cleanup_ref(raw_box, *clean))
    handles = [sq] + [None] * 7 + [band, None, sq, None]
    points = clicks + [(0, 0), (0, 0), at, (0, 0)]
    regions = [EMPTY] + [(lab, 0, 0, 0) for lab in labels[1:]] + [EMPTY, (api.GRID_MARK, 5, ref["ip"], ref["sp"]), box, (api.CLEAN_MARK, *clean, 0)]
    outs = _raw(api, sq, handles, points, regions)
    assert np.array_equal(outs[0], alone_clicks)
    _same_map(outs[8], ref["want"], "the grid prompt of the mixed call")
    assert np.array_equal(outs[10], alone_box)
    # the wrapper's builder makes the same call
    got = api.Segmentation.compute_mask_batch([sq, band, sq], clicks=[[api.Point(*c) for c in clicks], None, [api.Point(*at)]],
                                              labels=[labels, None, None], regions=[None, None, api.Region(api.Point(*box[:2]), api.Point(*box[2:]))],
                                              clean=[None, None, clean], grid=[None, (5, ref["ip"], ref["sp"]), None])
    assert np.array_equal(got[0], alone_clicks) and np.array_equal(got[2], alone_box)
    _same_map(got[1], ref["want"], "the grid prompt of the wrapper's mixed call")


def test_two_threads_on_two_handles(api, world, reference):
    _, segs = world
    picks = [0, 2]                                               # square side 4, band side 8
    results, errors = {}, []

    def work(t):
        try:
            name, side = GC.CASES[picks[t]]
            ref = reference[picks[t]]
            for rep in range(3):
                results[(t, rep)] = segs[name].segment_everything(side, ref["ip"], ref["sp"]).copy()
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 6
    for (t, rep), got in results.items():
        _same_map(got, reference[picks[t]]["want"], f"thread {t}, call {rep}")


def test_hq_model(api, tmp_path_factory):
    """A SAM-HQ model: 8 token rows per prompt, chunks of 14; its planes are masks_sam + masks_hq already."""
    from dlimgedit_amd import weights as W
    mdir = tmp_path_factory.mktemp("models_hqtest_grid")
    W.write_synthetic_model_dir(mdir, H.CFG, H.SEED, mask_branch=True, hq=True)
    env = api.Environment(api.Options(api.Backend.gpu, str(mdir)))
    seg = api.Segmentation.process(api.ImageView(H.image("small"), api.Channels.rgba), env)
    try:
        _, w, h = H.IMAGES["small"]
        ref = _reference(api, seg, w, h, 4)                      # 16 prompts: a chunk of 14 and one of 2
        got = seg.segment_everything(4, ref["ip"], ref["sp"])
        print(f"grid.e2e.hq: thresholds {ref['ip']} / {ref['sp']}, kept {len(ref['kept'])}")
        _same_map(got, ref["want"], "SAM-HQ")
        assert len(ref["kept"]) >= 1 and int(got.max()) <= len(ref["kept"])
    finally:
        seg.close()
        env.close()


def test_raw_refusals_leave_the_handle_working(api, world, reference):
    _, segs = world
    seg = segs["square"]
    a, b = (512, 512), (300, 300)
    BOX = (257, 264, 580, 567)
    before = seg.compute_mask(api.Point(*a)).copy()
    refused = [
        ([seg, None], [a, a], [EMPTY, (7, 0, 0, 0)], 1),                             # side out of range
        ([seg, None], [a, a], [EMPTY, (7, 33, 0, 0)], 1),
        ([seg, None], [a, a], [BOX, (7, 4, 0, 0)], 1),                               # a non-empty head region
        ([seg, None, None], [a, a, b], [EMPTY, (7, 4, 0, 0), (1, 0, 0, 0)], 2),      # a click in the prompt
        ([seg, None, None], [a, b, a], [EMPTY, (1, 0, 0, 0), (7, 4, 0, 0)], 2),
        ([seg, None, None], [a, a, a], [EMPTY, (7, 4, 0, 0), (6, 8, 8, 0)], 2),      # a clean-up mark on a grid prompt
        ([seg, None, None, None], [a, a, a, b], [EMPTY, (7, 4, 0, 0), (4, 0, 0, 0), (1, 0, 0, 0)], 2),      # a refinement mark
        ([seg, None, None], [a, a, a], [EMPTY, (7, 4, 0, 0), (7, 4, 0, 0)], 2),      # two grid marks
        ([None, seg], [a, a], [(7, 4, 0, 0), EMPTY], 0),                             # in front of any head
        ([seg, None], None, [EMPTY, (7, 40, 0, 0)], 1),                              # ... and without `points`
    ]
    for handles, points, regions, at in refused:
        with pytest.raises(api.Error, match=f"entry {at}:.*mark"):
            _raw(api, seg, handles, points, regions)
        assert np.array_equal(seg.compute_mask(api.Point(*a)), before)
    # a refusal about another prompt of the call names the caller's entry; 5 is still a refused label
    with pytest.raises(api.Error, match="entry 3:.*label"):
        _raw(api, seg, [seg, None, seg, None], [a, a, a, a], [EMPTY, (7, 4, 0, 0), EMPTY, (5, 0, 0, 0)])
    ref = reference[0]
    _same_map(seg.segment_everything(GC.CASES[0][1], ref["ip"], ref["sp"]), ref["want"], "after the refusals")
    # the wrapper refuses what the library refuses, before anything reaches it
    with pytest.raises(api.Error, match="grid"):
        seg.segment_everything(0)
    with pytest.raises(api.Error, match="grid"):
        seg.segment_everything(33)
