"""The two launches of the encoder neck (kernels.hpp: neck_conv1x1_ln, neck_conv3x3_ln -- convolution + LayerNorm2d in one
kernel, the 3x3 operand read straight from the map) through their hooks in lib/libdlimgedit_test.so, on the smallest shapes at
which they can go wrong.

Accuracy is measured against tests/neck_ref.py's float64 reference in units of its rounding model, and the allowance is 1.25
times what the FIVE launches they replace need on the same inputs (GEMM and LayerNorm through their own hooks, the im2col copy
done here): both ratios go to parity_margins.txt.  Everything else is exact: a batch against its images one at a time, the
per-image destinations, the image border, the f16 copy."""
import numpy as np
import pytest

import neck_ref as R

pytestmark = pytest.mark.gpu

f16, f32 = np.float16, np.float32


@pytest.fixture(scope="module")
def ext():
    from dlimgedit_amd import api
    assert api.ext.device_count() >= 1, "no HIP device visible"
    return api.ext


@pytest.fixture(scope="module")
def env(model_dirs):
    """Device memory comes from an environment (dlimg_amd_device_alloc); the smallest model will do."""
    from dlimgedit_amd import api
    e = api.Environment(api.Options(api.Backend.gpu, model_dirs("vit_test")[0]))
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == f16 else np.uint32)


def _parent(ext, a16, w16, gamma, beta):
    """The launches the fused one replaces: the planner's GEMM with an fp32 result, then the row LayerNorm kernel."""
    v = ext.test_gemm(a16, w16)
    return ext.test_layernorm(v, gamma, beta, R.EPS)          # (fp32, f16)


# ------------------------------------------------------------------------------------------ 1x1 + LN

@pytest.mark.parametrize("B,K", [(1, 256), (2, 768)])
def test_conv1x1_ln_against_float64(ext, env, B, K):
    """K = 256 is four K tiles, the shortest that runs the steady loop; K = 768 with two images is the workload's own shape
    at ViT-B.  Non-trivial scale and shift; row 1234 has one channel about 300 times the rest."""
    x, w = R.conv1x1_case(11 + K, B, K, spike_row=1234)
    gamma, beta = R.affine(5)
    got16, got32, flag, _ = ext.test_neck_conv_ln(env, x, w, gamma, beta, R.EPS)
    par32, par16 = _parent(ext, x, w, gamma, beta)
    ref = R.conv1x1_ln(x, w, gamma, beta)
    spike = np.sort(np.abs(x[1234].astype(np.float64) @ w.astype(np.float64).T))
    assert spike[-1] > 250 * R.rms(spike[:-1]), "the planted row lost its outlier channel"
    assert flag == 0
    R.check(f"neck 1x1 B{B} K{K} fp32", got32, par32, ref, R.output_model(ref, "f32"))
    R.check(f"neck 1x1 B{B} K{K} f16", got16, par16, ref, R.output_model(ref, "f16"))


# ------------------------------------------------------------------------------------------ 3x3 + LN

@pytest.fixture(scope="module")
def conv3(ext, env):
    """Four images of impulses + noise, weights distinct per tap, and the result of ONE launch over all four (everything into
    the shared workspace): what the batch, destination and border tests compare with."""
    fmap = R.impulse_map(21, 4)
    w = R.conv3x3_weights(22)
    gamma, beta = R.affine(6)
    out16, out32, flag, _ = ext.test_neck_conv_ln(env, fmap, w, gamma, beta, R.EPS)
    assert flag == 0
    return {"map": fmap, "w": w, "gamma": gamma, "beta": beta, "f16": out16, "f32": out32}


def test_conv3x3_ln_taps_borders_against_float64(ext, env, conv3):
    """B = 2.  Every probe token (four corners, four edges, one interior) carries an impulse in a channel of its own, the
    weights differ per tap: each of the up to nine output tokens around a probe receives the impulse through exactly one tap,
    and at the borders the missing taps must read zeros.

    The neighbourhood rows are held to an absolute bound as well, 1e-2: a misrouted or missing tap moves an impulse of height 8
    times a weight of 0.02-0.06 in rows of standard deviation ~0.1, i.e. changes normalised values by O(1), while fp32
    accumulation is bounded by K u sum|a||w| / sigma = 2304 * 6e-8 * 2.8 / 0.1 = 4e-3 (times gamma <= 1.5) in the worst case."""
    fmap, w, gamma, beta = conv3["map"][:2], conv3["w"], conv3["gamma"], conv3["beta"]
    got16, got32, flag, _ = ext.test_neck_conv_ln(env, fmap, w, gamma, beta, R.EPS)
    assert flag == 0
    par32, par16 = _parent(ext, R.im2col3x3(fmap), w, gamma, beta)
    ref = R.conv3x3_ln(fmap, w, gamma, beta)
    rows = np.concatenate([R.probe_neighbourhood() + b * R.TOKENS for b in range(2)])
    assert len(rows) == 2 * 49          # 4 corners x 4, 4 edges x 6, 1 interior x 9
    from conftest import within
    within("neck 3x3 probe neighbourhoods max abs", np.abs(got32[rows] - ref[rows]).max(), 1e-2)
    R.check("neck 3x3 B2 fp32", got32, par32, ref, R.output_model(ref, "f32"))
    R.check("neck 3x3 B2 f16", got16, par16, ref, R.output_model(ref, "f16"))


def test_conv3x3_images_do_not_see_each_other(ext, env, conv3):
    """Tokens 4095 of image 0 and 4096 of image 1 are neighbours in memory and not in any image.  A large value planted all
    along image 1's first row must leave image 0 (its last row above all) exactly what it is on its own, and image 1's
    first row must not see image 0's last."""
    fmap = conv3["map"][:2].copy()
    fmap[1, 0] += f16(1000.0)
    w, gamma, beta = conv3["w"], conv3["gamma"], conv3["beta"]
    _, both, flag, _ = ext.test_neck_conv_ln(env, fmap, w, gamma, beta, R.EPS, want_f16=False)
    _, alone0, _, _ = ext.test_neck_conv_ln(env, fmap[:1], w, gamma, beta, R.EPS, want_f16=False)
    _, alone1, _, _ = ext.test_neck_conv_ln(env, fmap[1:], w, gamma, beta, R.EPS, want_f16=False)
    assert flag == 0
    last_row = slice(63 * 64, 4096)
    assert np.array_equal(_bits(both[:4096][last_row]), _bits(alone0[last_row]))
    assert np.array_equal(_bits(both[:4096]), _bits(alone0))
    assert np.array_equal(_bits(both[4096:]), _bits(alone1))
    assert np.array_equal(_bits(alone0), _bits(conv3["f32"][:4096])), "image 0 itself was not changed"


# ------------------------------------------------------------------------------------------ batches, destinations

def test_batch_equals_single_launches(ext, env, conv3):
    """The tile is fixed whatever the batch: four images in one launch against four launches of one, bit for bit, both entry
    points."""
    fmap, w, gamma, beta = conv3["map"], conv3["w"], conv3["gamma"], conv3["beta"]
    for i in range(4):
        one16, one32, _, _ = ext.test_neck_conv_ln(env, fmap[i:i + 1], w, gamma, beta, R.EPS)
        rows = slice(i * 4096, (i + 1) * 4096)
        assert np.array_equal(_bits(one32), _bits(conv3["f32"][rows])), i
        assert np.array_equal(_bits(one16), _bits(conv3["f16"][rows])), i
    x, w1 = R.conv1x1_case(31, 4, 256)
    all16, all32, _, _ = ext.test_neck_conv_ln(env, x, w1, gamma, beta, R.EPS)
    for i in range(4):
        rows = slice(i * 4096, (i + 1) * 4096)
        one16, one32, _, _ = ext.test_neck_conv_ln(env, x[rows], w1, gamma, beta, R.EPS)
        assert np.array_equal(_bits(one32), _bits(all32[rows])), i
        assert np.array_equal(_bits(one16), _bits(all16[rows])), i


def test_per_image_destinations_and_guards(ext, env, conv3):
    """Three images into buffers of their own, one (no destination given) into the workspace: the same bits as the launch
    that wrote everything into the workspace, and the guard bytes in front of and behind every buffer untouched."""
    from dlimgedit_amd import api
    fmap, w, gamma, beta = conv3["map"], conv3["w"], conv3["gamma"], conv3["beta"]
    own = [True, True, False, True]
    out16, out32, flag, guards = ext.test_neck_conv_ln(env, fmap, w, gamma, beta, R.EPS, own_buffer=own)
    assert flag == 0
    assert np.array_equal(_bits(out32), _bits(conv3["f32"]))
    assert np.array_equal(_bits(out16), _bits(conv3["f16"]))
    for i, g in enumerate(guards):
        assert (g is not None) == own[i]
        if g is not None:
            assert len(g[0]) == len(g[1]) == api.ext.NECK_GUARD
            assert (g[0] == api.ext.NECK_GUARD_BYTE).all() and (g[1] == api.ext.NECK_GUARD_BYTE).all(), i
    x, w1 = R.conv1x1_case(31, 4, 256)
    ws16, ws32, _, _ = ext.test_neck_conv_ln(env, x, w1, gamma, beta, R.EPS)
    own16, own32, _, guards = ext.test_neck_conv_ln(env, x, w1, gamma, beta, R.EPS, own_buffer=own)
    assert np.array_equal(_bits(own32), _bits(ws32)) and np.array_equal(_bits(own16), _bits(ws16))
    for g in guards:
        assert g is None or ((g[0] == api.ext.NECK_GUARD_BYTE).all() and (g[1] == api.ext.NECK_GUARD_BYTE).all())


# ------------------------------------------------------------------------------------------ report, f16 copy

def test_non_finite_input_sets_the_flag(ext, env, conv3):
    """An infinity in one token of the input is an input VALUE: the launch completes, the rows it reaches have no finite
    statistics, and the flag says so.  Clean inputs leave it 0 (the conv3 fixture and the tests above assert that)."""
    w, gamma, beta = conv3["w"], conv3["gamma"], conv3["beta"]
    fmap = conv3["map"][:1].copy()
    fmap[0, 40, 17, 3] = f16(np.inf)
    _, out32, flag, _ = ext.test_neck_conv_ln(env, fmap, w, gamma, beta, R.EPS, want_f16=False)
    assert flag == 1
    touched = np.zeros((64, 64), bool)
    touched[39:42, 16:19] = True
    assert not np.isfinite(out32.reshape(64, 64, 256)[touched]).any()
    clean = conv3["f32"][:4096].reshape(64, 64, 256)
    assert np.array_equal(_bits(out32.reshape(64, 64, 256)[~touched]), _bits(clean[~touched])), "rows the infinity cannot reach"
    x, w1 = R.conv1x1_case(33, 1, 256)
    _, good, flag, _ = ext.test_neck_conv_ln(env, x, w1, gamma, beta, R.EPS, want_f16=False)
    assert flag == 0
    x[2049, 100] = f16(-np.inf)
    _, out32, flag, _ = ext.test_neck_conv_ln(env, x, w1, gamma, beta, R.EPS, want_f16=False)
    assert flag == 1
    assert not np.isfinite(out32[2049]).any()
    keep = np.arange(4096) != 2049
    assert np.array_equal(_bits(out32[keep]), _bits(good[keep]))


def test_f16_copy_is_the_rounded_fp32_result(ext, env, conv3):
    """SAM-HQ's f16 copy of the embedding: f16(fp32 output), element for element, of both entry points."""
    assert np.array_equal(_bits(conv3["f16"]), _bits(conv3["f32"].astype(f16)))
    x, w1 = R.conv1x1_case(35, 1, 256, spike_row=7)
    out16, out32, _, _ = ext.test_neck_conv_ln(env, x, w1, conv3["gamma"], conv3["beta"], R.EPS)
    assert np.array_equal(_bits(out16), _bits(out32.astype(f16)))
