"""The box + point prompt on the CPU: what the three-token form IS, pinned against an independent implementation.

* semantics: oracle/sam_oracle.decode_masks and oracle/decoder_ref.decode_fp64, called with coords [3, 2] = (point,
  top-left, bottom-right) and labels (1, 2, 3), against tests/golden/sam_vit_test_box_point.npz -- Hugging Face SamModel
  given input_points AND input_boxes (tests/golden/make_box_point_golden.py).  This pins the token order, the labels and
  the absence of a padding point; each of the three wrong forms is shown to miss the fixture;
* selection: with three prompt points SamOnnxModel.select_masks always returns plane 0;
* the inputs of the GPU tests: the reference masks of box + point, box alone and point alone differ pairwise by at least
  ten times what the GPU parity test lets a mask disagree in, from the oracle alone.
"""
from pathlib import Path

import numpy as np
import pytest

import box_point_cases as B
from conftest import IOU_PRED_TOL, LOGIT_TOL
from dlimgedit_amd import weights as W
from dlimgedit_amd.sam_config import get_config
from oracle import decoder_ref as R
from oracle import sam_oracle as O

GOLD = Path(__file__).resolve().parent / "golden" / "sam_vit_test_box_point.npz"
EMB_STRIDE, LOW_STRIDE = 257, 61


@pytest.fixture(scope="module")
def oracle_segs():
    """name -> (OracleSegmentation with its embedding, params) for the images of box_point_cases, reduced variant."""
    cfg = get_config("vit_test")
    params = W.synthetic_weights(cfg, 7)
    return {name: O.OracleSegmentation(params, cfg).process(B.image(name), O.CH_RGBA) for name in B.IMAGES}, params


def _samples(low):
    return np.asarray(low, np.float64).reshape(4, -1)[:, ::LOW_STRIDE]


def test_three_token_prompt_matches_hugging_face(oracle_segs):
    segs, params = oracle_segs
    g = np.load(GOLD)
    assert int(g["seed"]) == 7
    seg = segs["square"]
    assert np.abs(seg.embedding.reshape(-1)[::EMB_STRIDE] - g["emb_samples"]).max() < 2e-4
    want_pairs = [(box, pt) for name, box, pt in B.PAIRS if name == "square"]
    assert [tuple(b) for b in g["boxes"]] == [b for b, _ in want_pairs]
    assert [tuple(p) for p in g["points"]] == [p for _, p in want_pairs]
    for i, (box, pt) in enumerate(want_pairs):
        packed, _ = B.prompts(seg.rs, box, pt)
        coords, labels = packed["both"]
        assert coords.shape == (3, 2) and labels.tolist() == [1, 2, 3]
        for name, decode in (("sam_oracle", O.decode_masks), ("decoder_ref", R.decode_fp64)):
            low, iou = decode(seg.embedding, coords, labels, params)
            d_low = np.abs(_samples(low) - g["low_samples"][i]).max()
            d_iou = np.abs(np.asarray(iou, np.float64) - g["iou"][i]).max()
            print(f"box_point.hf.{name}.pair{i}: logits {d_low:.3g} (< {LOGIT_TOL}), iou {d_iou:.3g} (< {IOU_PRED_TOL})")
            assert d_low < LOGIT_TOL, (name, i, d_low)
            assert d_iou < IOU_PRED_TOL, (name, i, d_iou)
        # plane 0 is the single mask; the oracle's post-processing against torch's on HF's plane
        low, iou = R.decode_fp64(seg.embedding, coords, labels, params)
        assert O.select_single(np.asarray(iou, np.float32), 3) == 0
        mask = O.postprocess_logits(np.asarray(low[0], np.float32), (1024, 1024)) > 0
        want = np.unpackbits(g["mask0_bits"][i]).reshape(1024, 1024).astype(bool)
        assert (mask != want).mean() < 2e-5


def test_other_token_orders_and_a_pad_token_miss_the_fixture(oracle_segs):
    """The fixture tells the forms apart: corners in front of the point, a pad token behind the box, and the point's label
    on a corner each move the logits by far more than the tolerance the right form is held to."""
    segs, params = oracle_segs
    g = np.load(GOLD)
    seg = segs["square"]
    _, box, pt = B.PAIRS[0]
    packed, _ = B.prompts(seg.rs, box, pt)
    (coords, labels) = packed["both"]
    wrong = {
        "box first": (coords[[1, 2, 0]], labels[[1, 2, 0]]),
        "with pad token": (np.concatenate([coords, np.zeros((1, 2), np.float32)]), np.array([1, 2, 3, -1], np.float32)),
        "labels shifted": (coords, np.array([2, 3, 1], np.float32)),
    }
    for name, (c, l) in wrong.items():
        low, _ = R.decode_fp64(seg.embedding, c, l, params)
        d = np.abs(_samples(low) - g["low_samples"][0]).max()
        if name == "box first":
            # attention over a set of tokens: the order of the prompt rows alone does not move the output planes
            assert d < LOGIT_TOL, (name, d)
        else:
            assert d > 10 * LOGIT_TOL, (name, d)


@pytest.mark.parametrize("seed", range(8))
def test_three_points_always_select_plane_zero(seed):
    rng = np.random.default_rng(seed)
    cases = [rng.uniform(-1, 2, 4), rng.standard_normal(4) * 100, np.array([-400.0, 99.0, 99.0, 99.0]),
             np.array([0.0, 0.0, 0.0, 0.0]), np.array([-499.0, 0.5, 0.9, 1.0])]
    for iou in cases:
        assert O.select_single(iou.astype(np.float32), 3) == 0
    # ... and with two it never does, for predictions in any plausible range
    assert O.select_single(np.array([0.99, 0.1, 0.2, 0.15], np.float32), 2) == 2


def test_the_pairs_tell_box_point_and_both_apart(oracle_segs):
    """Inputs of tests/test_gpu_box_point.py, confirmed from the oracle alone: for every pair the reference masks of
    box + point, box alone and point alone differ pairwise by at least ten times the number of pixels the GPU parity test
    lets a mask disagree with its reference in."""
    assert B.DISAGREE_LIMIT == 3 * max(B.PARENT_BOX_FRACTION, B.PARENT_POINT_FRACTION) > 0
    segs, params = oracle_segs
    for name, box, pt in B.PAIRS:
        seg = segs[name]
        w, h = seg.rs.original
        packed, counts = B.prompts(seg.rs, box, pt)
        masks = {k: B.reference_mask(seg.embedding, *packed[k], counts[k], params, (h, w))[0] for k in packed}
        allowed = B.DISAGREE_LIMIT * w * h
        for a, b in (("both", "box"), ("both", "point"), ("box", "point")):
            differing = int((masks[a] != masks[b]).sum())
            assert differing >= 10 * allowed, (name, box, pt, a, b, differing, allowed)
