"""SAM-HQ models on the GPU: a model file with the dec.hq.* group is served as SAM-HQ -- the HQ token as one more trailing token
row, the per-image HQ features from the early ViT feature and the embedding, the 3x3 mask path on MFMA (kernels/decoder_hq.hip)
and the HQ plane added to all four logits planes.

* parity with the float64 reference (tests/hq_ref.py, HQ token at row 5 as Hugging Face has it) on the handle's own embedding:
  every value of every plane where dlimg_amd_get_logits can express the prompt, the delivered mask for every case;
* against the Hugging Face fixture with no reference code in the loop;
* one result through every door; 15 prompts across a launch; mixed prompt sizes; a batched pass equals one image at a time;
* the encoder is untouched (embedding bit-equal to the plain twin's, the twin's logits do not care about an HQ environment);
* what an HQ model refuses, by name, the handle working afterwards; the fed-back plane of a marked prompt carries the HQ plane.

On the parent commit the file is served as plain SAM: every parity test fails there (the HQ masks differ from the plain ones in
a third of the pixels and more, tests/test_hq_oracle.py), and nothing is refused.
"""
import numpy as np
import pytest

import box_point_cases as B
import hq_cases as H
import hq_ref as Q
import multi_click_cases as M
from conftest import EMB_TOL, IOU_PRED_TOL, LOGIT_TOL, single_mask_index, within

IDS = [H.case_id(c) for c in H.CASES]
# the mask-level floor: the convention of DISAGREE_LIMIT in the case files, three times the largest fraction measured there
FLOOR = 3 * max(M.PARENT_TWO_TOKEN_FRACTION, M.PARENT_THREE_TOKEN_FRACTION, B.PARENT_BOX_FRACTION, B.PARENT_POINT_FRACTION)
EMB_STRIDE, LOW_STRIDE, FEAT_STRIDE = 257, 61, 509


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


def _process(api, env, name):
    return api.Segmentation.process(api.ImageView(H.image(name), api.Channels.rgba), env)


def _early(name, params):
    """The numpy encoder's stream after the first global block, on the image as the library encodes it."""
    from oracle import sam_oracle as O
    from oracle import stb_resize
    img = H.image(name)
    _, w, h = H.IMAGES[name]
    rs, _ = H.resize_geometry(name)
    rw, rh = rs.target_extent(w, h)
    if (rw, rh) != (w, h):
        x = O.preprocess(O.create_image_tensor(stb_resize.resize_srgb(img[:, :, :3].copy(), rw, rh), O.CH_RGB))
    else:
        x = O.preprocess(O.create_image_tensor(img, O.CH_RGBA))
    return Q.encoder_stream(x, params, H.CFG, Q.first_global_block(H.CFG))


@pytest.fixture(scope="module")
def hq(api, tmp_path_factory):
    """The HQ model and its plain twin (the same file without dec.hq.*): environments, handles, embeddings, reference features."""
    from dlimgedit_amd import weights as W
    twin_dir, hq_dir = tmp_path_factory.mktemp("models_hqtest_plain"), tmp_path_factory.mktemp("models_hqtest_hq")
    W.write_synthetic_model_dir(twin_dir, H.CFG, H.SEED, mask_branch=True)
    params = W.write_synthetic_model_dir(hq_dir, H.CFG, H.SEED, mask_branch=True, hq=True)
    twin_env = api.Environment(api.Options(api.Backend.gpu, str(twin_dir)))
    twin = {n: _process(api, twin_env, n) for n in H.IMAGES}
    point = api.Point(*H.CASES[0][1][0])
    twin_before = api.ext.get_logits(twin["square"], point=point)       # before any HQ environment exists in the process
    env = api.Environment(api.Options(api.Backend.gpu, str(hq_dir)))
    segs = {n: _process(api, env, n) for n in H.IMAGES}
    embs = {n: api.ext.get_embedding(s) for n, s in segs.items()}
    feats = {n: Q.hq_features(_early(n, params), embs[n], params) for n in H.IMAGES}
    s = dict(env=env, params=params, segs=segs, embs=embs, feats=feats, twin_env=twin_env, twin=twin,
             twin_embs={n: api.ext.get_embedding(t) for n, t in twin.items()}, twin_before=twin_before, point=point)
    yield s
    for h in list(segs.values()) + list(twin.values()):
        h.close()
    env.close()
    twin_env.close()


def _points(api, clicks):
    return [api.Point(*c) for c in clicks]


def _region(api, box):
    return None if box is None else api.Region(api.Point(box[0], box[1]), api.Point(box[2], box[3]))


def _deliver(api, segs, case):
    """The mask the wrappers deliver for a case (a box alone goes through compute_mask, the others through the click form)."""
    name, clicks, labels, box, after = case
    if not clicks:
        return segs[name].compute_mask(_region(api, box))
    return segs[name].compute_mask_clicks(_points(api, clicks), labels, _region(api, box), refine_after=after)


@pytest.fixture(scope="module")
def delivered(api, hq):
    return [_deliver(api, hq["segs"], c) for c in H.CASES]


@pytest.fixture(scope="module")
def reference(hq):
    """case index -> (mask, plane, delivered logits, iou) of the float64 HQ reference on the handle's own embedding"""
    out = []
    for case in H.CASES:
        rs, hw = H.resize_geometry(case[0])
        out.append(Q.staged(hq["embs"][case[0]], hq["feats"][case[0]], rs, case, hq["params"], hw))
    return out


@pytest.fixture(scope="module")
def twin_fraction(api, hq):
    """case index -> share of pixels in which the plain twin's delivered mask differs from decode_fp64's, in this run"""
    out = []
    for case in H.CASES:
        rs, hw = H.resize_geometry(case[0])
        want = Q.plain_mask(hq["twin_embs"][case[0]], rs, case, hq["params"], hw)
        out.append(float(((_deliver(api, hq["twin"], case) > 0) != want).mean()))
    return out


def _logit_bound(ref_logits):
    return LOGIT_TOL * max(1.0, float(np.std(ref_logits)) / 1.3)


@pytest.mark.gpu
@pytest.mark.parametrize("index", [0, 1], ids=IDS[:2])
def test_logits_parity(api, hq, reference, index):
    """All 65,536 values of all four planes, tile seams and the image border included."""
    name, clicks, _, box, _ = H.CASES[index]
    got, iou = api.ext.get_logits(hq["segs"][name], point=api.Point(*clicks[0])) if clicks else \
        api.ext.get_logits(hq["segs"][name], region=_region(api, box))
    _, _, want, want_iou = reference[index]
    print(f"hq.logits.{IDS[index]}: reference std {np.std(want):.3g}, max-abs per plane "
          f"{[float(np.abs(got[m] - want[m]).max()) for m in range(4)]}")
    within(f"hq.logits.{IDS[index]}", np.abs(got - want).max(), _logit_bound(want))
    within(f"hq.iou.{IDS[index]}", np.abs(iou - want_iou).max(), IOU_PRED_TOL)
    # the border rows and columns and the seams of the 16 x 16 tiles on their own
    edge = np.zeros((256, 256), bool)
    edge[[0, 255], :] = edge[:, [0, 255]] = True
    edge[15::16, :] = edge[16::16, :] = edge[:, 15::16] = edge[:, 16::16] = True
    within(f"hq.logits.seams.{IDS[index]}", np.abs(got - want)[:, edge].max(), _logit_bound(want))


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(H.CASES)), ids=IDS)
def test_mask_parity(api, hq, delivered, reference, twin_fraction, index):
    case = H.CASES[index]
    rs, hw = H.resize_geometry(case[0])
    want = reference[index][0]
    got = delivered[index]
    assert set(np.unique(got)) <= {0, 255}
    fraction = float(((got > 0) != want).mean())
    plain = Q.plain_mask(hq["embs"][case[0]], rs, case, hq["params"], hw)
    from_plain = float(((got > 0) != plain).mean())
    limit = max(3 * twin_fraction[index], FLOOR)
    print(f"hq.mask.{IDS[index]}: differs from the HQ reference in {fraction:.3g} of the pixels, from the plain reference in "
          f"{from_plain:.3g}; plain twin against its reference {twin_fraction[index]:.3g}; limit {limit:.3g}")
    within(f"hq.mask.{IDS[index]}", fraction, limit)
    assert from_plain > 10 * limit, "the delivered mask is the plain mask"


@pytest.mark.gpu
def test_against_hugging_face(api, hq, delivered):
    gold = np.load(Q.__file__.replace("hq_ref.py", "golden/sam_vit_hqtest.npz"))
    seg = hq["segs"]["square"]
    within("hq.hf.embedding", np.abs(hq["embs"]["square"].reshape(-1)[::EMB_STRIDE] - gold["emb_samples"]).max(), EMB_TOL)
    state = api.ext.decoder_state(seg, hq["point"])
    feat = state["hq_features"]
    assert feat.size == 256 * 256 * 32 and state["hyper_hq"].size == 32
    # the embedding's bound, scaled to the spread of the features (the embedding is LayerNorm'ed: std 1)
    want = gold["feat_samples"]
    within("hq.hf.features", np.abs(feat[::FEAT_STRIDE] - want).max(), EMB_TOL * max(1.0, float(np.std(want))))
    for k, i in enumerate(gold["cases"]):
        case = H.CASES[int(i)]
        name = f"hq.hf.{H.case_id(case)}"
        if int(i) == 0:
            low, iou = api.ext.get_logits(seg, point=hq["point"])
            want_low = gold["low_samples"][k]
            within(name + ".logits", np.abs(low.reshape(4, -1)[:, ::LOW_STRIDE] - want_low).max(), _logit_bound(want_low))
            within(name + ".iou", np.abs(iou - gold["iou"][k]).max(), IOU_PRED_TOL)
            assert single_mask_index(iou) == int(gold["plane"][k])
        bits = np.unpackbits(gold["mask_bits"][k]).reshape(-1, 1024).astype(bool)
        within(name + ".mask", ((delivered[int(i)] > 0)[::2] != bits).mean(), FLOOR)


@pytest.mark.gpu
def test_one_result_every_door(api, hq, delivered, reference):
    env, segs = hq["env"], hq["segs"]
    seg, point = segs["square"], hq["point"]
    want = delivered[0]
    # slot 4 (single mask), slot 14, the device form, the wrappers
    assert np.array_equal(seg.compute_mask(point), want)
    assert np.array_equal(api.Segmentation.compute_mask_batch([seg], points=[point])[0], want)
    assert np.array_equal(seg.compute_mask_clicks([point]), want)
    dev = api.ext.device_alloc(env, want.size)
    try:
        offsets = api.ext.compute_mask_batch_device([seg], dev, points=[point], root_device=0)
        got = np.empty(want.size, np.uint8)
        api.ext.copy_to_host(env, got, dev)
        assert offsets[0] == 0 and np.array_equal(got.reshape(want.shape), want)
    finally:
        api.ext.device_free(env, dev)
    # the three-mask form of slot 4: planes 1..3, each with the HQ plane added
    from oracle import sam_oracle as O
    _, _, low, _ = reference[0]
    for m, mask in enumerate(seg.compute_masks(point)):
        ref = O.postprocess_logits(np.asarray(low[1 + m], np.float32), want.shape) > 0
        within(f"hq.doors.three_mask.{m}", ((np.asarray(mask.image) > 0) != ref).mean(), FLOOR)


@pytest.mark.gpu
def test_many_prompts_and_mixed_sizes(api, hq, delivered):
    segs = hq["segs"]
    seg = segs["square"]
    # 15 one-point prompts: 8 token rows each with the HQ token, 14 per launch
    pts = [api.Point(40 + 60 * i, 900 - 50 * i) for i in range(15)]
    alone = [seg.compute_mask(p) for p in pts]
    together = api.Segmentation.compute_mask_batch([seg] * 15, points=pts)
    for i in range(15):
        assert np.array_equal(together[i], alone[i]), i
    # prompts of different sizes (and a marked one) in one call, on both images
    order = [4, 0, 6, 3, 2, 5]
    cases = [H.CASES[i] for i in order]
    got = api.Segmentation.compute_mask_batch([segs[c[0]] for c in cases], clicks=[_points(api, c[1]) for c in cases],
                                              labels=[c[2] for c in cases], regions=[_region(api, c[3]) for c in cases],
                                              refine_after=[c[4] for c in cases])
    for i, g in zip(order, got):
        assert np.array_equal(g, delivered[i]), IDS[i]


@pytest.mark.gpu
def test_batched_pass_equals_one_image_at_a_time(api, hq, delivered):
    env = hq["env"]
    names = list(H.IMAGES)
    both = api.Segmentation.process_batch([api.ImageView(H.image(n), api.Channels.rgba) for n in names], env)
    try:
        for n, s in zip(names, both):
            assert np.array_equal(api.ext.get_embedding(s), hq["embs"][n]), n
            p = api.Point(100, 100)
            assert np.array_equal(api.ext.decoder_state(s, p)["hq_features"], api.ext.decoder_state(hq["segs"][n], p)["hq_features"]), n
        for i, case in enumerate(H.CASES):
            assert np.array_equal(_deliver(api, dict(zip(names, both)), case), delivered[i]), IDS[i]
    finally:
        for s in both:
            s.close()


@pytest.mark.gpu
def test_encoder_untouched(api, hq):
    for n in H.IMAGES:
        assert np.array_equal(hq["embs"][n], hq["twin_embs"][n]), n
    low, iou = api.ext.get_logits(hq["twin"]["square"], point=hq["point"])
    assert np.array_equal(low, hq["twin_before"][0]) and np.array_equal(iou, hq["twin_before"][1])
    # and the twin is plain SAM: its logits are not the HQ model's
    assert np.abs(low - api.ext.get_logits(hq["segs"]["square"], point=hq["point"])[0]).max() > 1.0


@pytest.mark.gpu
def test_refusals_leave_the_handle_usable(api, hq, delivered):
    env, segs = hq["env"], hq["segs"]

    def still_works():
        assert np.array_equal(_deliver(api, segs, H.CASES[0]), delivered[0])
        assert np.array_equal(_deliver(api, segs, H.CASES[4]), delivered[4])

    # 8 clicks and a box: 10 points, one more than an HQ model takes
    name, clicks, labels, box, _ = H.TOO_MANY
    with pytest.raises(api.Error, match=r"at most 9 points.*SAM-HQ|SAM-HQ.*at most 9 points"):
        segs[name].compute_mask_clicks(_points(api, clicks), labels, _region(api, box))
    still_works()
    # ... also when it shares a call with prompts the model takes: nothing of the call is decoded
    with pytest.raises(api.Error, match="at most 9 points"):
        api.Segmentation.compute_mask_batch([segs[name]] * 2, clicks=[_points(api, clicks[:1]), _points(api, clicks)],
                                            labels=[labels[:1], labels], regions=[None, _region(api, box)])
    still_works()
    # the asynchronous path
    img = H.image("square")
    src, mask = api.ext.device_alloc(env, img.size), api.ext.device_alloc(env, 1024 * 1024)
    try:
        api.ext.copy_to_device(env, src, img)
        with pytest.raises(api.Error, match=r"encode_and_mask.*SAM-HQ"):
            api.ext.encode_and_mask(env, api.ext.device_views([src], 1024, 1024), [api.Point(512, 512)], [mask])
        api.ext.synchronize(env)
        api.ext.encode_only(env, api.ext.device_views([src], 1024, 1024))      # stays served
        api.ext.synchronize(env)
    finally:
        api.ext.device_free(env, src)
        api.ext.device_free(env, mask)
    still_works()
    # the hooks that decode bare embeddings
    emb = hq["embs"]["square"][None]
    coords, labs = np.array([[[512, 512], [0, 0]]], np.float32), np.array([[1, -1]], np.float32)
    with pytest.raises(api.Error, match=r"SAM-HQ.*bare embeddings"):
        api.ext.test_decode(env, emb, [0], coords, labs)
    with pytest.raises(api.Error, match=r"SAM-HQ.*bare embeddings"):
        api.ext.test_decode_prompts(env, emb, [0], coords, labs)
    still_works()


@pytest.mark.gpu
def test_fed_back_plane_carries_the_hq_plane(api, hq, delivered, twin_fraction):
    """The marked case by hand: the GPU's own stage-1 planes (dlimg_amd_get_logits) through the float64 reference of stage 2."""
    index = 6
    case = H.CASES[index]
    name, clicks, _, box, after = case
    assert after == (1,) and box is None
    rs, hw = H.resize_geometry(name)
    planes, iou4 = api.ext.get_logits(hq["segs"][name], point=api.Point(*clicks[0]))
    plane = single_mask_index(iou4)
    want, _, _, _ = Q.staged(hq["embs"][name], hq["feats"][name], rs, case, hq["params"], hw,
                             first_mask_logits=planes[plane], from_stage=1)
    fraction = float(((delivered[index] > 0) != want).mean())
    within(f"hq.staging.{IDS[index]}", fraction, max(3 * twin_fraction[index], FLOOR))
    # fed back WITHOUT the HQ plane the second stage gives another mask: the stage-1 plane of the plain twin as mask input
    plain_planes, plain_iou = api.ext.get_logits(hq["twin"][name], point=api.Point(*clicks[0]))
    other, _, _, _ = Q.staged(hq["embs"][name], hq["feats"][name], rs, case, hq["params"], hw,
                              first_mask_logits=plain_planes[single_mask_index(plain_iou)], from_stage=1)
    assert float(((delivered[index] > 0) != other).mean()) > 10 * max(3 * twin_fraction[index], FLOOR)
