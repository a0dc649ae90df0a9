"""The measures of tests/test_gpu_hq_features.py, shown to work before they judge a kernel (no GPU).

* The free-running emulation of hq_feature_ref with unrounded weights and an unrounded H is hq_ref.hq_features on the same raw
  tensors to 1e-9 relative: that ties the new reference, the loader's permutation and the pixel order to the independent one.
* On the Gaussian input of the D = 128 model, with the float64 results rounded to fp32 standing in for what a device delivers,
  the yardsticks pass every stage's check, and every stand-in -- each a mistake the chain could make that the end-to-end bounds of
  tests/test_gpu_hq.py (0.015 std on a strided sample of the features, 0.03 on the logits) let through -- reaches at least 3
  times the allowance of the stage that is there to see it (ViT branch / embedding branch):

      stand-in                               stage      times the allowance
      sub-pixel s = kx * 2 + ky              A          3.6e6 / 1.9e6
      conv1 bias on sub-pixel 0 only         A          8.9e4 / 4.8e4
      tanh-form GELU                         H          118 / 181
      unbiased variance                      H          38 / 288
      LayerNorm over 4 C columns             H          4.2e4 / 1.5e5
      conv2 bias added in the GEMM as well   Y          7.9e4 / 2.4e5
      conv2 bias added twice                 features   69 (one branch's alone: 39 / 38)

  Every figure is printed by the tests and asserted to be 3 or more.

* What no measure of this file can see is listed in BLIND with its figure, and asserted to stay below 3, instead of being dropped:

      eps = 1e-5                             H          1.02 / 1.03   (it would fail the check, but not by a factor 3)
      H not rounded to f16                   features   0.81
"""
import numpy as np
import pytest

import gemm_ref as G
import hq_cases as H
import hq_feature_ref as F
import hq_ref as Q

f16, f32, f64 = np.float16, np.float32, np.float64

REJECT = 3.0

# Stand-ins the measures cannot see on the Gaussian input, with the larger figure of the two branches (times the allowance) and why.
# eps 1e-5: eps only matters where a row's variance is within a few orders of it; the Gaussian input's rows have a variance of
#   0.3, so 1e-5 instead of 1e-6 moves the normalised values by 1.5e-5 relative, a thirtieth of half an f16 spacing: it tips a few
#   roundings of H and no more.  The row kernel's own eps is held on rows whose variance is near eps
#   (tests/test_gpu_row_kernels.py: test_layernorm_hard_rows, and the two launches of this branch exactly in
#   test_layernorm_product_shapes_of_the_hq_branch); what is held nowhere is that SamModel::hq_branch passes kLnEps = 1e-6.
# H not rounded to f16: H is an f16 buffer, so a kernel cannot fail to round it; the free-running comparison is the only place the
#   rounding shows, and there it is of the size of the allowance itself (boundary flips of H between two precisions).
BLIND = {"eps 1e-5": 1.03, "H not rounded to f16": 0.81}


@pytest.fixture(scope="module")
def params():
    from dlimgedit_amd import weights as W
    return W.synthetic_weights(H.CFG, H.SEED, hq=True)


@pytest.fixture(scope="module")
def gaussian(params):
    """Per branch: the loader's operands, the GPU test's Gaussian input, float64 A, the fp32 A a device would deliver (the
    reference rounded once), float64 H and the LayerNorm yardsticks."""
    out = {}
    for i, branch in enumerate(("vit", "emb")):
        ops = F.loader_operands(params, branch)
        a = F.branch_input("gaussian", 900 + 10 * i, ops)
        A = F.stage_a(a, ops)
        A32 = A.astype(f32)
        out[branch] = dict(ops=ops, a=a, A=A, A32=A32, H=F.stage_h(A32, ops), yard_h=F.stage_h_yardsticks(A32, ops))
    return out


def test_emulation_is_the_independent_reference(params):
    rng = np.random.default_rng(5)
    early, emb = rng.standard_normal((F.TOKENS, H.CFG.embed_dim)), rng.standard_normal((F.TOKENS, 256))
    raw = {b: F.loader_operands(params, b, round_weights=False) for b in ("vit", "emb")}
    got = F.emulate(early, emb, raw["vit"], raw["emb"], round_h=False)
    want = Q.hq_features(early, emb, params)
    assert got.shape == want.shape == (256, 256, 32)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    # and it is not blind to the order of the sub-pixels or to the pixel mapping
    swapped = {b: F.loader_operands(params, b, round_weights=False, order="xy") for b in ("vit", "emb")}
    assert np.abs(F.emulate(early, emb, swapped["vit"], swapped["emb"], round_h=False) - want).max() > 0.1 * np.abs(want).max()


def test_input_conditions_hold(params):
    for i, branch in enumerate(("vit", "emb")):
        for kind in F.KINDS:
            p = F.offset_params(params) if kind == "offset" else params
            ops = F.loader_operands(p, branch)
            a = F.branch_input(kind, 900 + 10 * i + F.KINDS.index(kind), ops)
            F.input_conditions(kind, F.stage_a(a, ops), ops)
    ops = F.loader_operands(params, "vit")
    with pytest.raises(AssertionError):
        F.input_conditions("offset", F.stage_a(F.branch_input("gaussian", 1, ops), ops), ops)


def _gemm_excess(got, ref, yard) -> float:
    """How many times its allowance a GEMM result needs: rms or max, whichever is worse, over ALLOW * the larger yardstick."""
    model = G.output_model(ref)
    g = G.ratios(got, ref, model)
    bound = {k: max(G.ratios(y, ref, model)[k] for y in yard.values()) for k in g}
    return max(g[k] / (G.ALLOW * bound[k]) for k in g)


@pytest.mark.parametrize("branch", ["vit", "emb"])
def test_stage_a_measure(params, gaussian, branch):
    g = gaussian[branch]
    ops, a, ref = g["ops"], g["a"], g["A"]
    yard = F.gemm_yardsticks(a, ops["w1"], ops["b1"])
    for name, y in yard.items():
        G.check(f"hq feature ref {branch} A {name}", y, ref, G.output_model(ref), yard)
    stand_ins = {"s = kx * 2 + ky": F.loader_operands(params, branch, order="xy"),
                 "conv1 bias on sub-pixel 0 only": F.loader_operands(params, branch, bias1="first")}
    for name, bad in stand_ins.items():
        excess = _gemm_excess(F.stage_a(a, bad).astype(f32), ref, yard)
        print(f"hq feature ref stand-in: {name}, {branch} branch, stage A: {excess:.3g} times the allowance")
        assert excess >= REJECT, (name, excess)


@pytest.mark.parametrize("branch", ["vit", "emb"])
def test_stage_h_measure(gaussian, branch):
    g = gaussian[branch]
    ops, A32, ref, yard = g["ops"], g["A32"], g["H"], g["yard_h"]
    for name, y in yard.items():
        G.check_f16(f"hq feature ref {branch} H {name}", y.astype(f16), ref, yard)
    bound = G.f16_bound(ref, yard)
    stand_ins = {"tanh-form GELU": dict(gelu="tanh"), "unbiased variance": dict(unbiased=True),
                 "LayerNorm over 4 C columns": dict(over_4c=True), "eps 1e-5": dict(eps=1e-5)}
    for name, kw in stand_ins.items():
        bad = F.stage_h(A32, ops, **kw).astype(f16).astype(f64)
        excess = float((np.abs(bad - ref) / bound).max())
        print(f"hq feature ref stand-in: {name}, {branch} branch, stage H: {excess:.3g} times the allowance")
        if name in BLIND:
            assert excess < REJECT and excess <= 1.5 * BLIND[name] + 1.0, (name, excess)
        else:
            assert excess >= REJECT, (name, excess)


def test_stage_y_measure(gaussian):
    for branch in ("vit", "emb"):
        g = gaussian[branch]
        H16 = g["yard_h"]["tree"].astype(f16)
        ref, yard = F.stage_y(H16, g["ops"]), F.gemm_yardsticks(H16, g["ops"]["w2"])
        for name, y in yard.items():
            G.check(f"hq feature ref {branch} Y {name}", y, ref, G.output_model(ref), yard)
        # a second GEMM that added its bias here as well (hq_features_finish adds it): stage Y sees it at once
        excess = _gemm_excess(G.plain(H16, g["ops"]["w2"], g["ops"]["b2"]).astype(f32), ref, yard)
        print(f"hq feature ref stand-in: conv2 bias added in the GEMM too, {branch} branch, stage Y: {excess:.3g} times the allowance")
        assert excess >= REJECT, excess


def test_free_running_measure(params, gaussian):
    """The float32 emulation is inside its own allowance by construction (a third of it); conv2's bias added twice and an H that
    is not rounded to f16 are at least 3 times outside."""
    v, e = gaussian["vit"], gaussian["emb"]
    e64 = F.emulate(v["a"], e["a"], v["ops"], e["ops"])
    e32 = F.emulate(v["a"], e["a"], v["ops"], e["ops"], ft=f32)
    allowance = 3 * float(np.abs(e64 - e32).max())
    print(f"hq feature ref free-running: float64 vs float32 emulation {allowance / 3:.3g}, allowance {allowance:.3g}")
    doubled = {b: F.loader_operands(params, b, bias2_scale=2.0) for b in ("vit", "emb")}
    stand_ins = {"conv2 bias added twice": F.emulate(v["a"], e["a"], doubled["vit"], doubled["emb"]),
                 "conv2 bias of the ViT branch added twice": F.emulate(v["a"], e["a"], doubled["vit"], e["ops"]),
                 "conv2 bias of the embedding branch added twice": F.emulate(v["a"], e["a"], v["ops"], doubled["emb"]),
                 "H not rounded to f16": F.emulate(v["a"], e["a"], v["ops"], e["ops"], round_h=False)}
    for name, bad in stand_ins.items():
        excess = float(np.abs(bad - e64).max()) / allowance
        print(f"hq feature ref stand-in: {name}, features: {excess:.3g} times the allowance")
        if name in BLIND:
            assert excess < REJECT and excess <= 1.5 * BLIND[name] + 1.0, (name, excess)
        else:
            assert excess >= REJECT, (name, excess)
