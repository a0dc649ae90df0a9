"""The SAM-HQ kernels alone, and the kernel that feeds them (kernels.hpp: k::hq_mask_path, k::upscale_logits,
k::hq_features_finish), through their hooks in lib/libdlimgedit_test.so: one launcher call on given operands, guard bytes
around every device buffer.

Accuracy is measured against the float64 references of tests/hq_kernel_ref.py in units of the rounding model, and the allowance
is ALLOW = 1.25 times what the larger of two numpy fp32 yardsticks needs on the same inputs (tests/test_hq_kernel_ref.py shows
what that measure rejects); every ratio goes to parity_margins.txt.  Everything else is exact: the four planes among each other,
the += into the logits, a batch against its prompts one at a time, the two forms of upscale_logits, the pixel mapping of
hq_features_finish.  All float64 comparisons run at one prompt, the smallest launch: the grid is 256 x 256 whatever the input."""
import numpy as np
import pytest

import hq_kernel_ref as R
from conftest import within

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64


@pytest.fixture(scope="module")
def ext():
    from dlimgedit_amd import api
    assert api.ext.device_count() >= 1, "no HIP device visible"
    return api.ext


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == f16 else np.uint32)


def _run(ext, U, p, feat, hyper, logits_in=None, feat_index=None):
    """One k::hq_mask_path call; features [256, 256, 32] of one image or [n, 256, 256, 32]; guards asserted."""
    feat = np.asarray(feat, f32).reshape(-1, R.RES, R.RES, R.C_OUT)
    U = np.asarray(U).reshape(-1, R.RES, R.RES, R.C_U)
    index = [0] * len(U) if feat_index is None else feat_index
    logits, H, ok = ext.test_hq_mask_path(U, R.weights_tuple(p), p["eps"], feat, index, np.asarray(hyper, f32).reshape(-1, R.C_OUT),
                                          logits_in)
    assert ok, "a guard byte around a device buffer was overwritten"
    return logits, H


# ------------------------------------------------------------------------------------------ hq_mask_path: float64

@pytest.fixture(scope="module")
def main(ext):
    """The main case (a GELU of Gaussians with one spike pixel), ONE launch with logits_in = 0, and stage 1's reference."""
    p = R.hq_params(101)
    U, feat, hyper = R.hq_inputs(102)
    logits, H = _run(ext, U, p, feat, hyper)
    return {"p": p, "U": U, "feat": feat, "hyper": hyper, "logits": logits[0], "H": H[0]}


def test_stage1_h_against_float64(main):
    """H as the launch left it against float64 from U: half an f16 spacing plus 1.25 times the larger yardstick's error."""
    ref = R.conv1(main["U"], main["p"])
    R.check_f16("hq kernel conv1 H", main["H"].reshape(R.PIXELS, R.C_H), ref, R.conv1_yardsticks(main["U"], main["p"]))


def test_stage2_planes_against_float64_of_the_delivered_h(main):
    """logits_in = 0: each plane is hyper_hq . (conv2(H delivered) + b2 + features), the four planes the same bits; all pixels, and
    the image border with both sides of every tile seam on their own, in the same units."""
    planes = main["logits"]
    for m in range(1, 4):
        assert np.array_equal(_bits(planes[m]), _bits(planes[0])), m
    ref = R.conv2_plane(main["H"], main["p"], main["feat"], main["hyper"])
    yard = R.conv2_yardsticks(main["H"], main["p"], main["feat"], main["hyper"])
    model = R.output_model(ref)
    R.check("hq kernel conv2 plane", planes[0], ref, model, yard)
    edge = R.seam_mask()
    R.check("hq kernel conv2 border and seams", planes[0][edge], ref[edge], model[edge], {k: y[edge] for k, y in yard.items()})


def test_plane_is_added_to_what_the_logits_held(ext, main):
    """A non-zero logits_in whose four planes differ: the result is float32(logits_in + d) bit for bit, d from the zero run."""
    rng = np.random.default_rng(103)
    logits_in = (rng.standard_normal((1, 4, R.RES, R.RES)) * np.array([1, 2, 3, 4])[None, :, None, None]).astype(f32)
    got, H = _run(ext, main["U"], main["p"], main["feat"], main["hyper"], logits_in)
    assert np.array_equal(_bits(got[0]), _bits(logits_in[0] + main["logits"][0][None]))
    assert np.array_equal(_bits(H[0]), _bits(main["H"]))


def test_probes_taps_borders_seams(ext):
    """Impulses of height 8 in channels of their own at the four corners, four edges, one interior pixel and both sides of a tile
    seam in x (15 | 16) and in y, on noise of sigma 0.05; weights that differ per tap (scale 1 + tap / 4).  Every pixel within
    one step of a probe sees its impulse through exactly one tap, and at the border the missing taps read zeros.

    The neighbourhoods (73 pixels) are held to an absolute bound as well, computed from the operands by
    hq_kernel_ref.probe_bounds.  H: the fp32 sum of K = 288 products is within K u S of the exact one (u = 2^-24, S = sum |U| |W1|
    <= 8 * 0.5 + noise), three times that for the bias and the statistics, over the pixel's sigma (>= 0.3: an impulse of 8 times
    weights of 0.06 .. 0.18), times max ln_w = 1.5 and GELU's slope 1.13: 4e-4, plus half an f16 spacing at the largest |H|
    (sqrt 63 * 1.5 + |ln_b| < 16: 2^-8 = 3.9e-3), 4.3e-3 in all.  Plane: (K + 34) u with K = 576 times sum_c |hyper_c| (sum |H| |W2|
    + |b2| + |features|) = 1.4e-2.  A misrouted tap moves H by 5 and the plane by 17 on these inputs, at every probe more than
    100 times either bound: tests/test_hq_kernel_ref.py asserts that."""
    p = R.hq_params(121)
    U, feat, hyper = R.probe_inputs(122)
    logits, H = _run(ext, U, p, feat, hyper)
    nb = R.probe_neighbourhood()
    ref_h = R.conv1(U, p).reshape(R.RES, R.RES, R.C_H)
    ref_plane = R.conv2_plane(H[0], p, feat, hyper)
    bound_h, bound_plane = R.probe_bounds(U, H[0], p, feat, hyper)
    assert bound_h < 5e-3 and bound_plane < 2e-2
    within("hq kernel probes H max abs", np.abs(H[0].astype(f64) - ref_h)[nb].max(), bound_h)
    within("hq kernel probes plane max abs", np.abs(logits[0, 0] - ref_plane)[nb].max(), bound_plane)
    # and all pixels in rounding units: the measure of the main case on these inputs
    yard = R.conv2_yardsticks(H[0], p, feat, hyper)
    R.check("hq kernel probes conv2 plane", logits[0, 0], ref_plane, R.output_model(ref_plane), yard)
    R.check_f16("hq kernel probes conv1 H", H[0].reshape(R.PIXELS, R.C_H), ref_h.reshape(R.PIXELS, R.C_H), R.conv1_yardsticks(U, p))


def test_flat_pixel_needs_eps(ext):
    """A parameter set of its own with the constant b1 = 0.5 and a 5 x 5 block of zeros in U: the central 3 x 3 pixels have 64
    equal channels, a variance of exactly zero, and H = f16(GELU(ln_b)) there -- 0 / sqrt(0 + eps).  Without eps it is a NaN."""
    p = R.hq_params(111, flat=True)
    U, feat, hyper = R.hq_inputs(112, spike=False, flat=True)
    logits, H = _run(ext, U, p, feat, hyper)
    y, x = R.FLAT_PIXEL
    rows = np.zeros((R.RES, R.RES), bool)
    rows[y - 1:y + 2, x - 1:x + 2] = True
    rows = rows.reshape(-1)
    want = np.broadcast_to(R.gelu64(p["ln_b"].astype(f64)), (9, R.C_H))
    assert np.array_equal(R.conv1(U, p, rows=rows), want)
    R.check_f16("hq kernel flat pixel H", H[0].reshape(R.PIXELS, R.C_H)[rows], want, R.conv1_yardsticks(U, p, rows=rows))
    assert np.isfinite(logits).all() and np.isfinite(H.astype(f32)).all()


# ------------------------------------------------------------------------------------------ hq_mask_path: batches, refusals

@pytest.fixture(scope="module")
def batch():
    """16 prompts with U, hyper_hq and logits_in of their own, and the features of two images."""
    rng = np.random.default_rng(151)
    U = (np.abs(rng.standard_normal((16, R.RES, R.RES, R.C_U), f32)) * f32(0.6)).astype(f16)
    feat = rng.standard_normal((2, R.RES, R.RES, R.C_OUT), f32)
    hyper = rng.standard_normal((16, R.C_OUT), f32)
    logits_in = rng.standard_normal((16, 4, R.RES, R.RES), f32)
    return {"p": R.hq_params(152), "U": U, "feat": feat, "hyper": hyper, "logits_in": logits_in}


@pytest.mark.parametrize("P,index,alone", [(3, [1, 0, 1], [0, 1, 2]), (16, [i % 2 for i in range(16)], [0, 7, 15])],
                         ids=["P3_shared_features", "P16"])
def test_batch_equals_each_prompt_alone(ext, batch, P, index, alone):
    """Two prompts share one image's features (P = 3: feat_index 1, 0, 1); the largest launch (P = 16).  Logits and H of a prompt
    are the bits of that prompt alone, and no guard byte is touched."""
    b = batch
    logits, H = _run(ext, b["U"][:P], b["p"], b["feat"], b["hyper"][:P], b["logits_in"][:P], index)
    for i in alone:
        one, one_h = _run(ext, b["U"][i:i + 1], b["p"], b["feat"], b["hyper"][i:i + 1], b["logits_in"][i:i + 1], [index[i]])
        assert np.array_equal(_bits(logits[i]), _bits(one[0])), i
        assert np.array_equal(_bits(H[i]), _bits(one_h[0])), i
        assert not np.array_equal(one[0], b["logits_in"][i])


def test_refusals_launch_nothing(ext, batch):
    from dlimgedit_amd import api
    b = batch
    w = R.weights_tuple(b["p"])
    # 17 prompts: one more than a launch takes
    with pytest.raises(api.Error, match="too many prompts"):
        ext.test_hq_mask_path(np.zeros((17, R.RES, R.RES, R.C_U), f16), w, R.EPS, b["feat"], [0] * 17, np.zeros((17, R.C_OUT), f32),
                              want_h=False)
    # a prompt without features
    logits_in = b["logits_in"][:2].copy()
    with pytest.raises(api.Error, match="needs its image's"):
        ext.test_hq_mask_path(b["U"][:2], w, R.EPS, b["feat"], [0, -1], b["hyper"][:2], logits_in, want_h=False)
    # no prompt: no error, and the logits stay what they were
    logits, _, ok = ext.test_hq_mask_path(b["U"][:1], w, R.EPS, b["feat"], [0], b["hyper"][:1], b["logits_in"][:1], prompts=0)
    assert ok and np.array_equal(_bits(logits), _bits(b["logits_in"][:1]))
    # the device is as usable as before
    one, _ = _run(ext, b["U"][:1], b["p"], b["feat"], b["hyper"][:1], b["logits_in"][:1], [0])
    assert np.isfinite(one).all()


# ------------------------------------------------------------------------------------------ upscale_logits

@pytest.fixture(scope="module")
def up(ext):
    """Five prompts' keys and hyper vectors, and every prompt alone in the storing form (the 64-row path)."""
    q = R.upscale_params(131)
    keys, hyper = R.upscale_inputs(132, 5)
    alone = []
    for i in range(5):
        logits, U, ok = ext.test_upscale_logits(keys[i * 4096:(i + 1) * 4096], *R.upscale_args(q), hyper[i:i + 1], True)
        assert ok
        alone.append((logits[0], U[0]))
    return {"q": q, "keys": keys, "hyper": hyper, "alone": alone}


def test_upscale_against_float64(ext, up):
    """One prompt.  U against the float64 chain (erf-form GELU, no rounding between the stages) with check_f16, the logits with
    check in fp32 units; the yardsticks apply the fitted GELU and round the intermediate to f16.  The two instantiations give
    the same logits bit for bit.  And the tie between the two results: the logits are the product with the fp32 u, U its f16
    rounding, so |logits[m] - hyper[m] . float(U)| <= sum_c |hyper[m][c]| ulp16(U[c]) / 2 + ALLOW * 32 * 2^-24 * sum |hyper| |U|."""
    q, keys, hyper = up["q"], up["keys"][:4096], up["hyper"][0]
    logits, U = up["alone"][0]
    plain, none, ok = ext.test_upscale_logits(keys, *R.upscale_args(q), hyper[None], False)
    assert ok and none is None
    assert np.array_equal(_bits(plain[0]), _bits(logits))
    u_ref, l_ref = R.upscale(keys, q, hyper)
    yard = R.upscale_yardsticks(keys, q, hyper)
    R.check_f16("hq kernel upscale U", U, u_ref, {k: v[0] for k, v in yard.items()})
    R.check("hq kernel upscale logits", logits, l_ref, R.output_model(l_ref), {k: v[1] for k, v in yard.items()})
    tie = np.abs(logits.astype(f64) - np.einsum("mc,yxc->myx", hyper.astype(f64), U.astype(f64)))
    worst = float((tie / R.tie_bound(U, hyper)).max())
    print(f"hq kernel upscale: largest |logits - hyper . U| / bound {worst:.4f}")
    within("hq kernel upscale logits-U tie/bound", worst, np.nextafter(1.0, np.inf))


@pytest.mark.parametrize("P", [3, 5], ids=["P3_128_rows", "P5_256_rows"])
@pytest.mark.parametrize("store_u", [True, False], ids=["store_u", "logits_only"])
def test_upscale_batch_equals_each_prompt_alone(ext, up, P, store_u):
    """P = 3 takes the 128-row path, P = 5 the 256-row path (one prompt: 64 rows), in both forms: the bits of each prompt alone."""
    logits, U, ok = ext.test_upscale_logits(up["keys"][:P * 4096], *R.upscale_args(up["q"]), up["hyper"][:P], store_u)
    assert ok, "a guard byte around a device buffer was overwritten"
    assert (U is not None) == store_u
    for i in range(P):
        assert np.array_equal(_bits(logits[i]), _bits(up["alone"][i][0])), i
        if store_u:
            assert np.array_equal(_bits(U[i]), _bits(up["alone"][i][1])), i


# ------------------------------------------------------------------------------------------ hq_features_finish

def test_finish_pixel_mapping_is_exact(ext):
    """Integer inputs that encode their own (row, column), every sum below 2^24: each add is exact whatever the order, so the
    result is the contract's mapping bit for bit."""
    case = R.finish_index_case()
    out, ok = ext.test_hq_features_finish(*case)
    assert ok
    assert np.array_equal(out.astype(f64), R.finish(*case))


def test_finish_rounding(ext):
    """Gaussian inputs: three fp32 adds, |out - float64 sum| <= 3 * 2^-24 * (|vit| + |emb| + |b_vit| + |b_emb|) element by element."""
    case = R.finish_gaussian_case(141)
    out, ok = ext.test_hq_features_finish(*case)
    assert ok
    worst = float((np.abs(out.astype(f64) - R.finish(*case)) / R.finish_bound(*case)).max())
    print(f"hq kernel finish: largest |out - ref| / bound {worst:.4f}")
    within("hq kernel finish err/bound", worst, np.nextafter(1.0, np.inf))
