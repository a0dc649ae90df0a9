"""The float64 decoder reference (oracle/decoder_ref.py) against the fp32 oracle, and its f16-storage emulation: what
tests/test_gpu_decoder.py compares the HIP decoder with.  CPU only."""
import numpy as np
import pytest

from oracle import decoder_ref as R
from oracle import sam_oracle as O

POINT = (np.array([[512, 512], [0, 0]], np.float32), np.array([1, -1], np.float32))
BOX = (np.array([[200, 300], [700, 800]], np.float32), np.array([2, 3], np.float32))


@pytest.fixture(scope="module")
def params(model_dirs):
    return model_dirs("vit_test")[1]


@pytest.fixture(scope="module")
def emb():
    return np.random.default_rng(7).standard_normal((4096, 256)).astype(np.float32)


@pytest.mark.parametrize("prompt", ["point", "box"])
def test_fp64_reference_agrees_with_the_fp32_oracle(params, emb, prompt):
    coords, labels = POINT if prompt == "point" else BOX
    want, want_iou = O.decode_masks(emb, coords, labels, params)
    taps = {}
    got, got_iou = R.decode_fp64(emb, coords, labels, params, taps)
    assert got.dtype == np.float64 and got.shape == (4, 256, 256) and got_iou.shape == (4,)
    assert np.abs(got - want).max() < 1e-4
    assert np.abs(got_iou - want_iou).max() < 1e-4
    # the taps are the oracle's intermediates
    otaps = {}
    O.decode_masks(emb, coords, labels, params, otaps)
    assert np.abs(taps["tokens"] - otaps["tokens"]).max() < 1e-5
    assert np.abs(taps["keys_head"] - otaps["keys"][:16]).max() < 1e-4
    assert np.abs(taps["hyper"] - otaps["hyper"]).max() < 1e-4
    assert taps["queries"].shape == (7, 256)


def test_emulation_without_rounding_points_is_the_fp64_reference(params, emb):
    coords, labels = POINT
    a, ai = R.decode_fp64(emb, coords, labels, params)
    b, bi = R.decode(emb, coords, labels, params, round_at=())
    assert np.array_equal(a, b) and np.array_equal(ai, bi)
    with pytest.raises(ValueError):
        R.decode(emb, coords, labels, params, round_at=("no_such_point",))


@pytest.mark.parametrize("point", R.F16_POINTS)
def test_every_rounding_point_changes_the_result(params, emb, point):
    """Each rounding point is wired to something: enabling it alone moves the logits, by far less than all of them."""
    coords, labels = POINT
    a, _ = R.decode_fp64(emb, coords, labels, params)
    b, _ = R.decode(emb, coords, labels, params, round_at=(point,))
    assert 1e-7 < np.abs(a - b).max() < 2e-2, point


@pytest.mark.parametrize("scale", [1.0, 4.0])
def test_emulation_floor(params, emb, scale):
    """The f16 storage of the HIP decoder costs 1e-4 .. 2e-2 in the logits on a random embedding: the emulation does
    something, and not more than the decoder's precision can explain."""
    coords, labels = POINT
    a, ai = R.decode_fp64(scale * emb, coords, labels, params)
    b, bi = R.decode_f16(scale * emb, coords, labels, params)
    assert 1e-4 <= np.abs(a - b).max() <= 2e-2
    assert np.abs(ai - bi).max() < 2e-3


def test_perturbed_weights_touch_two_tensors_only(params):
    q = R.perturbed(params)
    changed = sorted(k for k in params if not np.array_equal(params[k], q[k]))
    assert changed == ["dec.iou.2.b", "pe.no_mask"]
    assert all(q[k].dtype == np.float32 for k in changed)
    assert np.allclose(q["pe.no_mask"], params["pe.no_mask"] * 0.99, rtol=1e-6)
    assert np.allclose(q["dec.iou.2.b"] - params["dec.iou.2.b"], 0.002, atol=1e-7)
