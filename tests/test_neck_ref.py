"""tests/neck_ref.py on the CPU: its float64 neck against the fp32 oracle's (an independent implementation: per-tap matrix
products over a padded map, weights in [co, ci, ky, kx] layout), and its check() against three models that are wrong in
exactly the ways an implicit 3x3 operand or a fused LayerNorm2d can be wrong."""
import numpy as np
import pytest

import neck_ref as R

f16, f32, f64 = np.float16, np.float32, np.float64


@pytest.fixture(scope="module")
def case():
    """One image, encoder width 64.  Everything f16-representable, so the oracle and the reference see the same operands.  The
    map between the two convolutions has rows of standard deviation ~0.1 (small gamma): the 3x3 result's variance is ~1e-2,
    where an eps of 1e-5 instead of 1e-6 shows."""
    rng = np.random.default_rng(3)
    D = 64
    x = rng.normal(0, 1, (R.TOKENS, D)).astype(f16)
    w1 = (rng.normal(0, 1, (R.C, D)) / np.sqrt(D)).astype(f16)
    g1 = rng.uniform(0.05, 0.15, R.C).astype(f32)
    b1 = rng.normal(0, 0.02, R.C).astype(f32)
    w2 = R.conv3x3_weights(4)
    g2, b2 = R.affine(5)
    return {"x": x, "w1": w1, "g1": g1, "b1": b1, "w2": w2, "g2": g2, "b2": b2}


def test_reference_against_the_fp32_oracle(case):
    """Bound 1e-4 on outputs of unit scale.  The oracle works in fp32: a dot product of K <= 2304 terms carries a relative error
    of about sqrt(K) 2^-24 = 3e-6 of its terms' scale (worst case K 2^-24 = 1.4e-4), the two LayerNorms divide by standard
    deviations the sums dominate, so a few 1e-6 are expected and 1e-4 leaves the worst case room -- while a tap in the wrong
    place, a wrong border or a wrong eps moves values by 1e-3 to 1 (test_check_rejects_modified_models)."""
    from conftest import within
    from oracle import sam_oracle as O
    c = case
    w2_oihw = c["w2"].astype(f32).reshape(R.C, 3, 3, R.C).transpose(0, 3, 1, 2)         # [co, (ky, kx), ci] -> [co, ci, ky, kx]
    p = {"enc.neck.conv1.w": c["w1"].astype(f32), "enc.neck.ln1.w": c["g1"], "enc.neck.ln1.b": c["b1"],
         "enc.neck.conv2.w": np.ascontiguousarray(w2_oihw), "enc.neck.ln2.w": c["g2"], "enc.neck.ln2.b": c["b2"]}
    want = O.neck(c["x"].astype(f32).reshape(R.GRID, R.GRID, -1), p, None).reshape(R.TOKENS, R.C)
    got = R.neck(c["x"], c["w1"], c["g1"], c["b1"], c["w2"], c["g2"], c["b2"], round_map=False)
    assert R.rms(want) > 0.5
    within("neck_ref vs fp32 oracle max abs", np.abs(got - want).max(), 1e-4)


@pytest.fixture(scope="module")
def stage2(case):
    """The second launch on its own: the f16 map the first one would store, the float64 reference, its fp32 rounding model,
    and an fp32 emulation of the launches it replaces (f16 operands, fp32 products and sums, fp32 LayerNorm) as `parent`."""
    c = case
    fmap = R.round_f16(R.conv1x1_ln(c["x"], c["w1"], c["g1"], c["b1"])).astype(f16).reshape(1, R.GRID, R.GRID, R.C)
    ref = R.conv3x3_ln(fmap, c["w2"], c["g2"], c["b2"])
    v = R.im2col3x3(fmap).astype(f32) @ c["w2"].astype(f32).T
    mean = v.mean(axis=1, keepdims=True, dtype=f32)
    d = v - mean
    rstd = f32(1) / np.sqrt((d * d).mean(axis=1, keepdims=True, dtype=f32) + f32(R.EPS))
    parent = d * rstd * c["g2"] + c["b2"]
    assert parent.dtype == f32
    return {"map": fmap, "ref": ref, "model": R.output_model(ref, "f32"), "parent": parent}


def test_check_accepts_the_contract(case, stage2):
    s = stage2
    R.check("neck_ref self-check: parent", s["parent"], s["parent"], s["ref"], s["model"])
    R.check("neck_ref self-check: model", s["model"], s["parent"], s["ref"], s["model"])


@pytest.mark.parametrize("variant", [{"tap_order": "xy"}, {"pad": "clamp"}, {"eps": 1e-5}], ids=["taps-transposed", "clamped-border", "eps-1e-5"])
def test_check_rejects_modified_models(case, stage2, variant):
    """Each modified model is computed in float64 and rounded like the contract's: only the modelling error is left."""
    c, s = case, stage2
    wrong = R.round_f32(R.conv3x3_ln(s["map"], c["w2"], c["g2"], c["b2"], **variant))
    with pytest.raises(AssertionError):
        R.check("neck_ref modified model " + "/".join(variant), wrong, s["parent"], s["ref"], s["model"])


def test_im2col_layout_and_probes():
    """Column (ky * 3 + kx) * C + c of row (y, x) is map[y + ky - 1, x + kx - 1, c], zeros outside; the probe neighbourhoods
    cover every tap at corners, edges and in the interior."""
    fmap = np.arange(2 * 64 * 64 * 2, dtype=f32).reshape(2, 64, 64, 2) + 1
    cols = R.im2col3x3(fmap).reshape(2, 64, 64, 9, 2)
    assert np.array_equal(cols[1, 10, 20, 0 * 3 + 2], fmap[1, 9, 21])
    assert np.array_equal(cols[0, 10, 20, 2 * 3 + 0], fmap[0, 11, 19])
    assert not cols[1, 0, :, 0:3].any() and not cols[0, 63, :, 6:9].any()          # nothing from the other image
    assert not cols[:, :, 0, 0::3].any() and not cols[:, :, 63, 2::3].any()
    assert len(R.probe_neighbourhood()) == 4 * 4 + 4 * 6 + 9
