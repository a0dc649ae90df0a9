"""A box and a point in one prompt through the batch mask calls (table slot 14 and its device-output form): when `points`
and `regions` are both given, entry i is the box regions[i] refined by the foreground point points[i] -- three prompt
tokens (point, top-left, bottom-right; labels 1, 2, 3; no padding point), eight token rows in the decoder, plane 0 out.

* parity: the mask of slot 14 against oracle/decoder_ref.decode_fp64 on the handle's own embedding, plane 0 through
  sam_oracle.postprocess_logits: IoU >= IOU_BAR and at most box_point_cases.DISAGREE_LIMIT of the pixels differ.
  Measured on MI355X with the two-token decoder this change started from (same images, boxes, points and route): box alone
  differs in at most 3.38e-4 of the pixels, point alone in at most 2.00e-4 (box_point_cases.py has all twelve figures); the
  limit is three times the larger, 1.01e-3;
* both parts of the prompt count: the mask is strictly closer to the reference of box + point than to the references of
  the box alone and of the point alone (which differ from it in ten times the limit or more: test_box_point_oracle.py);
* a call with 1 .. 33 entries (chunks of 8 per lane, mixed image sizes, one handle repeated) gives every entry the bits of a
  call of its own; the device-output form gives the host form's bits, offsets tightly packed, also under two replicas;
* unchanged: slot 4 given both still lets the point win; slot 14 given neither is still an error.
"""
import numpy as np
import pytest

import box_point_cases as B
from conftest import IOU_BAR, at_least, iou, within


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


@pytest.fixture(scope="module")
def bp(api, model_dirs):
    """(env, params, {image name: Segmentation}, {image name: its embedding as the GPU computed it})"""
    mdir, params, _ = model_dirs("vit_test")
    env = api.Environment(api.Options(api.Backend.gpu, mdir))
    segs = {n: api.Segmentation.process(api.ImageView(B.image(n), api.Channels.rgba), env) for n in B.IMAGES}
    embs = {n: api.ext.get_embedding(s) for n, s in segs.items()}
    yield env, params, segs, embs
    for s in segs.values():
        s.close()
    env.close()


def _region(api, box):
    return api.Region(api.Point(box[0], box[1]), api.Point(box[2], box[3]))


def _references(name, box, pt, emb, params):
    """{"both" | "box" | "point": boolean reference mask} of one pair, float64 decoder on the given embedding."""
    from oracle import sam_oracle as O
    _, w, h = B.IMAGES[name]
    rs = O.ResizeLongestSide()
    rs.target_extent(w, h)
    packed, counts = B.prompts(rs, box, pt)
    out = {}
    for kind in packed:
        out[kind], plane = B.reference_mask(emb, *packed[kind], counts[kind], params, (h, w))
        assert (plane == 0) == (kind == "both")
    return out


def _ids():
    return [f"{n}-{b[0]}_{b[1]}_{b[2]}_{b[3]}-{p[0]}_{p[1]}" for n, b, p in B.PAIRS]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", B.PAIRS, ids=_ids())
def test_mask_parity_and_both_parts_count(api, bp, pair):
    env, params, segs, embs = bp
    name, box, pt = pair
    refs = _references(name, box, pt, embs[name], params)
    got = api.Segmentation.compute_mask_batch([segs[name]], points=[api.Point(*pt)], regions=[_region(api, box)])[0]
    assert set(np.unique(got)) <= {0, 255}
    got = got > 0
    tag = f"{name}.{box[0]}_{box[1]}.{pt[0]}_{pt[1]}"
    differing = {kind: int((got != ref).sum()) for kind, ref in refs.items()}
    print(f"box_point.{tag}: differing pixels {differing} of {got.size}")
    at_least(f"box_point.iou.{tag}", iou(got, refs["both"]), IOU_BAR)
    within(f"box_point.disagree.{tag}", differing["both"] / got.size, B.DISAGREE_LIMIT)
    # an implementation that drops the point answers the box's mask, one that drops the box the point's
    assert differing["both"] < differing["box"], differing
    assert differing["both"] < differing["point"], differing


def _pool(api, segs, n=33):
    """n entries: the pairs of box_point_cases in turn and shifted copies of them; images alternate irregularly, so one
    handle appears many times and neighbours in a chunk have different sizes."""
    rng = np.random.default_rng(5)
    out = []
    for i in range(n):
        name, box, pt = B.PAIRS[(i * 5 + i // 6) % len(B.PAIRS)]
        _, w, h = B.IMAGES[name]
        dx, dy = (0, 0) if i < len(B.PAIRS) else rng.integers(-15, 16, 2)
        clip = lambda x, y: (int(min(max(x + dx, 0), w - 1)), int(min(max(y + dy, 0), h - 1)))  # noqa: E731
        b = clip(box[0], box[1]) + clip(box[2], box[3])
        out.append((segs[name], api.Point(*clip(*pt)), _region(api, b)))
    return out


@pytest.fixture(scope="module")
def singles(api, bp):
    _, _, segs, _ = bp
    return [api.Segmentation.compute_mask_batch([s], points=[p], regions=[r])[0] for s, p, r in _pool(api, segs)]


@pytest.mark.gpu
def test_batch_is_bit_equal_to_one_entry_per_call(api, bp, singles):
    _, _, segs, _ = bp
    pool = _pool(api, segs)
    for count in (1, 13, 14, 15, 28, 29, 33):
        start = (7 * count) % len(pool)
        sel = [(start + j) % len(pool) for j in range(count)]
        got = api.Segmentation.compute_mask_batch([pool[i][0] for i in sel], points=[pool[i][1] for i in sel],
                                                  regions=[pool[i][2] for i in sel])
        for j, i in enumerate(sel):
            assert got[j].shape == singles[i].shape
            assert np.array_equal(got[j], singles[i]), f"{count} entries: entry {j} (pool {i}) differs from its own call"
    # a two-token call in between leaves nothing behind: the same entries again
    api.Segmentation.compute_mask_batch([pool[0][0]] * 3, points=[pool[0][1]] * 3)
    again = api.Segmentation.compute_mask_batch([pool[i][0] for i in range(9)], points=[pool[i][1] for i in range(9)],
                                                regions=[pool[i][2] for i in range(9)])
    for i in range(9):
        assert np.array_equal(again[i], singles[i])


def _device_form_equals_host_form(api, env, entries, want):
    extents = [(m.shape[1], m.shape[0]) for m in want]
    total = sum(w * h for w, h in extents)
    dev = api.ext.device_alloc(env, total)
    try:
        api.ext.copy_to_device(env, dev, np.full(total, 7, np.uint8))
        offsets = api.ext.compute_mask_batch_device([e[0] for e in entries], dev, points=[e[1] for e in entries],
                                                    regions=[e[2] for e in entries], root_device=0)
        got = np.empty(total, np.uint8)
        api.ext.copy_to_host(env, got, dev)
        assert offsets[0] == 0
        assert all(offsets[k + 1] - offsets[k] == extents[k][0] * extents[k][1] for k in range(len(entries) - 1))
        for k, (w, h) in enumerate(extents):
            assert np.array_equal(got[offsets[k]:offsets[k] + w * h].reshape(h, w), want[k]), k
    finally:
        api.ext.device_free(env, dev)


@pytest.mark.gpu
def test_device_form_is_bit_equal_to_host_form(api, bp, singles):
    env, _, segs, _ = bp
    pool = _pool(api, segs)[:19]
    _device_form_equals_host_form(api, env, pool, singles[:19])


@pytest.mark.gpu
def test_device_form_under_two_replicas(api, model_dirs, monkeypatch):
    """GPU 0 listed twice: two replicas share the entries of a call (the per-replica split of both batch forms), once with
    the peer-copy branch forced.  Host form equal to one entry per call, device form equal to host form, bit for bit."""
    mdir, _, _ = model_dirs("vit_test")
    monkeypatch.setenv("DLIMGEDIT_DEVICES", "0,0")
    env = api.Environment(api.Options(api.Backend.gpu, mdir))
    monkeypatch.delenv("DLIMGEDIT_DEVICES")
    names = ["square", "wide", "wide", "square"]
    handles = api.Segmentation.process_batch([api.ImageView(B.image(n), api.Channels.rgba) for n in names], env)
    assert sorted(api.ext.segmentation_device(s)[0] for s in handles) == [0, 0, 1, 1]
    by_name = {"square": [handles[0], handles[3]], "wide": [handles[1], handles[2]]}
    try:
        # the pool of the module's environment, each entry on a handle of this one (alternating between the replicas)
        proto = _pool(api, {n: n for n in B.IMAGES})[:21]
        entries = [(by_name[name][k % 2], p, r) for k, (name, p, r) in enumerate(proto)]
        host = api.Segmentation.compute_mask_batch([e[0] for e in entries], points=[e[1] for e in entries],
                                                   regions=[e[2] for e in entries])
        for k, e in enumerate(entries):
            own = api.Segmentation.compute_mask_batch([e[0]], points=[e[1]], regions=[e[2]])[0]
            assert np.array_equal(host[k], own), k
        for forced in ("0", "1"):
            monkeypatch.setenv("DLIMGEDIT_FORCE_PEER_COPY", forced)
            _device_form_equals_host_form(api, env, entries, host)
        monkeypatch.delenv("DLIMGEDIT_FORCE_PEER_COPY")
    finally:
        for s in handles:
            s.close()
        env.close()


@pytest.mark.gpu
def test_existing_rules_are_unchanged(api, bp):
    env, _, segs, _ = bp
    name, box, pt = B.PAIRS[0]
    seg = segs[name]
    # slot 4 given both: the point wins, the region is ignored (the reference's rule)
    out_both = seg._query(api.Point(*pt), _region(api, box), 1)[0][0]
    out_point = seg._query(api.Point(*pt), None, 1)[0][0]
    assert np.array_equal(out_both, out_point)
    assert np.array_equal(out_point, api.Segmentation.compute_mask_batch([seg], points=[api.Point(*pt)])[0])
    three = api.Segmentation.compute_mask_batch([seg], points=[api.Point(*pt)], regions=[_region(api, box)])[0]
    assert not np.array_equal(three, out_point)
    # slot 14 and its device form given neither array: an error, and the handle still works afterwards
    with pytest.raises(api.Error):
        api.Segmentation.compute_mask_batch([seg])
    dev = api.ext.device_alloc(env, seg.extent().width * seg.extent().height)
    try:
        with pytest.raises(api.Error):
            api.ext.compute_mask_batch_device([seg], dev)
    finally:
        api.ext.device_free(env, dev)
    assert np.array_equal(api.Segmentation.compute_mask_batch([seg], points=[api.Point(*pt)])[0], out_point)
