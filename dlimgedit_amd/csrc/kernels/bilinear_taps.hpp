// The two-stage bilinear sample of the mask post-processing as device functions: what postprocess.hip (masks) and
// mask_grid.hip (label maps) both evaluate, so that a label map's "mask" is bit for bit the mask k::postprocess_masks delivers.
//
// Every multiply/add is an explicitly rounded fp32 operation (__fmul_rn/__fadd_rn, no fma contraction) in the order of
// oracle/sam_oracle.py:bilinear_resize.  A file that includes this header is compiled with -ffp-contract=off (build.py).
#pragma once

#include "device_common.hpp"

// bit-exactness contract with the oracle: no mul+add contraction in anything that includes this header
#pragma clang fp contract(off)

namespace dlimg {
namespace taps {

constexpr int LOW = 256;
constexpr int FULL = 1024;

struct Tap { int i0, i1; float w0, w1; };

// half-pixel bilinear source coordinates, align_corners=False (oracle: _lin_coeffs)
DLIMG_DEVICE Tap make_tap(int dst, float scale, int in_size) {
    float src = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    src = fmaxf(src, 0.f);
    Tap t;
    t.i0 = min((int)src, in_size - 1);
    t.i1 = min(t.i0 + 1, in_size - 1);
    float l1 = __fsub_rn(src, (float)t.i0);
    l1 = fminf(fmaxf(l1, 0.f), 1.f);
    t.w1 = l1;
    t.w0 = __fsub_rn(1.0f, l1);
    return t;
}

DLIMG_DEVICE float lerp2(float a00, float a01, float a10, float a11, const Tap& ty, const Tap& tx) {
    const float top = __fadd_rn(__fmul_rn(a00, tx.w0), __fmul_rn(a01, tx.w1));
    const float bot = __fadd_rn(__fmul_rn(a10, tx.w0), __fmul_rn(a11, tx.w1));
    return __fadd_rn(__fmul_rn(ty.w0, top), __fmul_rn(ty.w1, bot));
}

// value of the 1024x1024 upsampled plane at (Y, X)
DLIMG_DEVICE float stage1(const float* __restrict__ low, int Y, int X) {
    const Tap ty = make_tap(Y, 0.25f, LOW), tx = make_tap(X, 0.25f, LOW);
    const float* r0 = low + ty.i0 * LOW;
    const float* r1 = low + ty.i1 * LOW;
    return lerp2(r0[tx.i0], r0[tx.i1], r1[tx.i0], r1[tx.i1], ty, tx);
}

// second stage: the crop of the upsampled plane (pre_h x pre_w) resampled to the output; t2y / t2x are the output pixel's
// taps into the crop (make_tap(oy, pre_h / H, pre_h), make_tap(ox, pre_w / W, pre_w))
DLIMG_DEVICE float stage2(const float* __restrict__ low, const Tap& t2y, const Tap& t2x) {
    return lerp2(stage1(low, t2y.i0, t2x.i0), stage1(low, t2y.i0, t2x.i1), stage1(low, t2y.i1, t2x.i0),
                 stage1(low, t2y.i1, t2x.i1), t2y, t2x);
}

}  // namespace taps
}  // namespace dlimg
