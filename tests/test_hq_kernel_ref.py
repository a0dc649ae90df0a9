"""The measure of tests/test_gpu_hq_kernels.py, shown to work before it judges a kernel (no GPU): on the inputs the GPU tests use,
the fp32 yardsticks of tests/hq_kernel_ref.py pass check / check_f16 against the float64 reference, and every modified model
-- each a mistake the kernels could make, that the end-to-end bound of 0.03 on the finished logits lets through -- fails the
same call.  Also: the conditions the inputs promise, and that the absolute bounds of the probe test sit at least 100 times
below what a misrouted tap does to the probes' neighbourhoods."""
import numpy as np
import pytest

import hq_kernel_ref as R

f16, f32, f64 = np.float16, np.float32, np.float64


def _fails(call) -> bool:
    try:
        call()
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------ hq_mask_path

@pytest.fixture(scope="module")
def stage1():
    """The GPU test's main case: operands, float64 H, both yardsticks."""
    p = R.hq_params(101)
    U, feat, hyper = R.hq_inputs(102)
    return {"p": p, "U": U, "feat": feat, "hyper": hyper, "ref": R.conv1(U, p), "yard": R.conv1_yardsticks(U, p)}


@pytest.fixture(scope="module")
def stage2(stage1):
    """Stage 2 on a stand-in for the delivered H: the chain yardstick of stage 1 rounded to f16."""
    p, feat, hyper = stage1["p"], stage1["feat"], stage1["hyper"]
    H = stage1["yard"]["chain"].astype(f16)
    ref = R.conv2_plane(H, p, feat, hyper)
    return {"H": H, "ref": ref, "yard": R.conv2_yardsticks(H, p, feat, hyper)}


def test_inputs_keep_their_promises(stage1):
    R.hq_input_conditions(stage1["U"], stage1["p"])
    assert np.abs(stage1["ref"]).max() < R.F16_LIMIT
    p = R.hq_params(111, flat=True)
    U, _, _ = R.hq_inputs(112, spike=False, flat=True)
    R.hq_input_conditions(U, p, flat=True, spike=False)
    assert np.abs(R.conv1(U, p)).max() < R.F16_LIMIT
    # the flat pixels' H is GELU(ln_b) in every channel: the deviations are exactly zero, eps keeps the division finite
    y, x = R.FLAT_PIXEL
    flat = R.conv1(U, p).reshape(R.RES, R.RES, R.C_H)[y - 1:y + 2, x - 1:x + 2]
    assert np.array_equal(flat, np.broadcast_to(R.gelu64(p["ln_b"].astype(f64)), flat.shape))
    # the weights differ per tap
    for w in (stage1["p"]["w1"], stage1["p"]["w2"]):
        norms = np.sqrt((w.astype(f64) ** 2).sum(axis=(1, 2)))
        assert np.diff(norms).min() > 0.1 * norms[0]


def test_stage1_yardsticks_pass_and_wrong_models_fail(stage1):
    p, U, ref, yard = stage1["p"], stage1["U"], stage1["ref"], stage1["yard"]
    for name, y in yard.items():
        R.check_f16(f"hq ref conv1 {name}", y.astype(f16), ref, yard)
    wrong = {"tanh-form GELU": R.conv1(U, p, gelu="tanh"),
             "ky and kx swapped": R.conv1(U, p, tap_order="xy"),
             "unbiased variance": R.conv1(U, p, unbiased=True)}
    for name, model in wrong.items():
        assert _fails(lambda: R.check_f16(f"hq ref conv1 wrong: {name}", model.astype(f16), ref, yard)), name


def test_stage2_yardsticks_pass_and_wrong_models_fail(stage1, stage2):
    p, feat, hyper = stage1["p"], stage1["feat"], stage1["hyper"]
    H, ref, yard = stage2["H"], stage2["ref"], stage2["yard"]
    model = R.output_model(ref)
    for name, y in yard.items():
        R.check(f"hq ref conv2 {name}", y, ref, model, yard)
    edge = R.seam_mask()
    seam_yard = {k: y[edge] for k, y in yard.items()}
    R.check("hq ref conv2 seams chain", yard["chain"][edge], ref[edge], model[edge], seam_yard)
    wrong = {"H padded with GELU(LN(bias))": R.conv2_plane(H, p, feat, hyper, pad=R.outside_value(p)),
             "ky and kx swapped": R.conv2_plane(H, p, feat, hyper, tap_order="xy"),
             "weight read as [tap][in][out]": R.conv2_plane(H, p, feat, hyper, layout="tio")}
    for name, plane in wrong.items():
        assert _fails(lambda: R.check(f"hq ref conv2 wrong: {name}", plane.astype(f32), ref, model, yard)), name
    # the padding mistake touches the border only: the seam comparison is the one that is sure to see it
    pad = wrong["H padded with GELU(LN(bias))"].astype(f32)
    assert np.array_equal(pad[1:-1, 1:-1], ref.astype(f32)[1:-1, 1:-1])
    assert _fails(lambda: R.check("hq ref conv2 seams wrong: padding", pad[edge], ref[edge], model[edge], seam_yard))
    # the plane goes to all four logits planes
    rng = np.random.default_rng(7)
    logits_in = rng.standard_normal((4, R.RES, R.RES)).astype(f32)
    want = R.add_plane(logits_in, ref)
    yard4 = {k: (logits_in + y[None]).astype(f32) for k, y in yard.items()}
    R.check("hq ref logits chain", yard4["chain"], want, R.output_model(want), yard4)
    only0 = R.add_plane(logits_in, ref, planes=(0,)).astype(f32)
    assert _fails(lambda: R.check("hq ref logits wrong: plane 0 only", only0, want, R.output_model(want), yard4))


def test_probe_bounds_sit_far_below_a_misrouted_tap():
    """The absolute bounds of the probe test (hq_kernel_ref.probe_bounds) against what exchanging ky and kx does to the probes'
    neighbourhoods, in H and in the plane: at least 100 times apart, and the yardsticks are inside the bounds."""
    p = R.hq_params(121)
    U, feat, hyper = R.probe_inputs(122)
    nb = R.probe_neighbourhood()
    assert nb.sum() == 4 * 4 + 4 * 6 + 9 + 2 * 12
    ref = R.conv1(U, p).reshape(R.RES, R.RES, R.C_H)
    H = R.conv1_yardsticks(U, p)["chain"].astype(f16).reshape(R.RES, R.RES, R.C_H)
    plane = R.conv2_plane(H, p, feat, hyper)
    bound_h, bound_plane = R.probe_bounds(U, H, p, feat, hyper)
    print(f"probe bounds: H {bound_h:.3g}, plane {bound_plane:.3g}")
    assert np.abs(H.astype(f64) - ref)[nb].max() <= bound_h
    assert np.abs(R.conv2_yardsticks(H, p, feat, hyper)["trunc16"] - plane)[nb].max() <= bound_plane
    wrong_h = R.conv1(U, p, tap_order="xy").reshape(R.RES, R.RES, R.C_H)
    wrong_plane = R.conv2_plane(H, p, feat, hyper, tap_order="xy")
    effect_h, effect_plane = np.abs(wrong_h - ref)[nb].max(), np.abs(wrong_plane - plane)[nb].max()
    print(f"misrouted taps: H {effect_h:.3g}, plane {effect_plane:.3g}")
    assert effect_h >= 100 * bound_h and effect_plane >= 100 * bound_plane
    # and each probe on its own: no neighbourhood is blind to the exchange
    for y, x in R.PROBES:
        own = np.zeros_like(nb)
        own[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
        assert np.abs(wrong_h - ref)[own].max() >= 100 * bound_h, (y, x)
        assert np.abs(wrong_plane - plane)[own].max() >= 100 * bound_plane, (y, x)


# ------------------------------------------------------------------------------------------ upscale_logits

def test_upscale_yardsticks_pass_and_exchanged_sub_pixels_fail():
    q = R.upscale_params(131)
    keys, hyper = R.upscale_inputs(132, 1)
    u_ref, l_ref = R.upscale(keys, q, hyper[0])
    assert np.abs(u_ref).max() < R.F16_LIMIT
    yard = R.upscale_yardsticks(keys, q, hyper[0])
    yard_u, yard_l = {k: v[0] for k, v in yard.items()}, {k: v[1] for k, v in yard.items()}
    for name in yard:
        R.check_f16(f"hq ref upscale U {name}", yard_u[name].astype(f16), u_ref, yard_u)
        R.check(f"hq ref upscale logits {name}", yard_l[name], l_ref, R.output_model(l_ref), yard_l)
        # the tie between the logits and the stored U holds for a product taken with the un-rounded fp32 u
        tie = np.abs(yard_l[name].astype(f64) - np.einsum("mc,yxc->myx", hyper[0].astype(f64), yard_u[name].astype(f16).astype(f64)))
        assert (tie <= R.tie_bound(yard_u[name].astype(f16), hyper[0])).all()
    u_bad, l_bad = R.upscale(keys, q, hyper[0], exchanged=True)
    assert _fails(lambda: R.check_f16("hq ref upscale U wrong: s1 and s2 exchanged", u_bad.astype(f16), u_ref, yard_u))
    assert _fails(lambda: R.check("hq ref upscale logits wrong: s1 and s2 exchanged", l_bad.astype(f32), l_ref,
                                  R.output_model(l_ref), yard_l))


# ------------------------------------------------------------------------------------------ hq_features_finish

def test_finish_mapping_and_bound():
    vit, emb, b_vit, b_emb = R.finish_index_case()
    want = R.finish(vit, emb, b_vit, b_emb)
    assert np.array_equal(want, want.astype(f32).astype(f64)) and want.max() < 2 ** 24
    # every output names the place it came from: value = 3 (128 row + column) + 101 channel
    Y, X, c = np.meshgrid(np.arange(256), np.arange(256), np.arange(32), indexing="ij")
    row = ((Y >> 2) * 64 + (X >> 2)) * 4 + ((Y >> 1) & 1) * 2 + ((X >> 1) & 1)
    col = ((Y & 1) * 2 + (X & 1)) * 32 + c
    assert np.array_equal(want, 3.0 * (128 * row + col) + 101 * c)
    bad = R.finish(vit, emb, b_vit, b_emb, exchanged=True)
    assert not np.array_equal(bad, want) and (bad != want).mean() > 0.4
    g = R.finish_gaussian_case(141)
    ref, bound = R.finish(*g), R.finish_bound(*g)
    in_order = (g[0] + g[1]).reshape(4096, 4, 4, 32) + (g[2] + g[3])
    assert (np.abs(R.to_raster(in_order).astype(f64) - ref) <= bound).all()
    assert (np.abs(R.finish(*g, exchanged=True) - ref) > bound).mean() > 0.4
