// K19  prior marks: a caller's full-resolution u8 mask as the 256 x 256 fp32 plane the prompt encoder's mask branch takes
// (kernels.hpp, k::mask_prior).
//
// Low-res pixel (x, y) of the scored region (x < ceil(pre_w / 4), y < ceil(pre_h / 4)) covers the pixels 4x .. 4x + 3 of the
// image as it was encoded, and those come from the source columns c0 .. c1 - 1 (rows likewise): its value is the mean coverage
// of that footprint, mapped from 0 .. 255 to -1 .. +1 and multiplied by the strength.  Everything up to the one division is
// integer arithmetic, so the plane is the same bits wherever it is computed (tests/prior_ref.py restates it in numpy).
// Footprints of neighbouring low-res columns may share a source column (whenever 4 x W is not a multiple of pre_w), so the
// footprints do not partition a row and a running sum over the row would not do.
//
// One wave per low-res row and segment of 64 low-res columns.  The wave sums the source rows r0 .. r1 - 1 of its segment's
// source columns vertically: a lane owns 16 consecutive columns, loads them as one 16-byte access per row (the address is
// whatever the image's width makes it: unaligned accesses are left to the compiler through memcpy) and keeps 16 int32 column
// sums in registers, which go to LDS once.  After the barrier every lane sums the columns of its own pixel out of LDS.  No
// atomics, no waiting on other workgroups; the plane is written with plain (vector) stores, 256 bytes per wave.  Memory-bound
// on paper: the mask is read once (a source row of a footprint border twice), 256 KB are written.
#include "device_common.hpp"
#include "footprint.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace dlimg {
namespace {

constexpr int LOW = 256;
constexpr int kSeg = 64;             // low-res columns of one workgroup, one per lane
constexpr int kSpanMax = 8192;       // source columns of one segment the LDS holds (a multiple of 16): 32 KB

// footprint_lo / footprint_hi: footprint.hpp (shared with the lasso derivation)

struct PriorArgs { const uint8_t* mask; float* plane; int W, H, pre_w, pre_h, sw, sh; float s; };

__global__ __launch_bounds__(kSeg) void mask_prior_kernel(PriorArgs a) {
    __shared__ int col[kSpanMax];
    const int y = blockIdx.y, x_first = blockIdx.x * kSeg, x = x_first + threadIdx.x;
    float out = -1.f * a.s;                                      // padding is background
    if (y < a.sh && x_first < a.sw) {                            // (uniform over the workgroup)
        const int x_last = min(x_first + kSeg, a.sw) - 1;
        const int c_lo = footprint_lo(x_first, a.W, a.pre_w), c_hi = footprint_hi(x_last, a.W, a.pre_w);
        const int r0 = footprint_lo(y, a.H, a.pre_h), r1 = footprint_hi(y, a.H, a.pre_h);
        const int chunks = (c_hi - c_lo + 15) >> 4;              // 16 * chunks <= kSpanMax: checked by the launcher
        const size_t total = (size_t)a.W * a.H;
        for (int k = threadIdx.x; k < chunks; k += kSeg) {
            int acc[16];
#pragma unroll
            for (int b = 0; b < 16; ++b) acc[b] = 0;
#pragma unroll 4
            for (int r = r0; r < r1; ++r) {
                const size_t at = (size_t)r * a.W + c_lo + 16 * k;
                if (at + 16 <= total) {
                    uint4_t v;
                    __builtin_memcpy(&v, a.mask + at, 16);
#pragma unroll
                    for (int b = 0; b < 16; ++b) acc[b] += (int)((v[b >> 2] >> (8 * (b & 3))) & 255u);
                } else {
                    // the last bytes of the mask: nothing is read behind them (columns past c_hi are never summed)
#pragma unroll
                    for (int b = 0; b < 16; ++b)
                        if (at + b < total) acc[b] += a.mask[at + b];
                }
            }
#pragma unroll
            for (int b = 0; b < 16; ++b) col[16 * k + b] = acc[b];
        }
        __syncthreads();
        if (x < a.sw) {
            const int c0 = footprint_lo(x, a.W, a.pre_w), c1 = footprint_hi(x, a.W, a.pre_w);
            int sum = 0;
            for (int c = c0; c < c1; ++c) sum += col[c - c_lo];
            const int area = (r1 - r0) * (c1 - c0);
            // both numerators are below 2^24 (launcher): the conversions are exact, the division is the one rounding
            out = ((float)(2 * sum - 255 * area) / (float)(255 * area)) * a.s;
        }
    }
    a.plane[y * LOW + x] = out;
}

}  // namespace

namespace k {

void mask_prior(const uint8_t* mask, int W, int H, int pre_w, int pre_h, int strength_milli, float* plane, hipStream_t s) {
    if (!mask || !plane) throw_error("mask_prior: null buffer");
    if (((uintptr_t)plane) & 15) throw_error("mask_prior: the plane is 16-byte aligned");
    if (W <= 0 || H <= 0 || pre_w <= 0 || pre_h <= 0 || pre_w > 4 * LOW || pre_h > 4 * LOW) throw_error("mask_prior: invalid extent");
    if ((int64_t)W * H > (int64_t)1 << 31) throw_error("mask_prior: the mask is too large");
    if (strength_milli < 1 || strength_milli > kPriorMaxStrength) throw_error("mask_prior: strength_milli is 1..100000");
    const int sw = (pre_w + 3) / 4, sh = (pre_h + 3) / 4;
    // what the kernel assumes: every footprint lies in the mask, its numerators convert exactly, a segment's columns fit the LDS
    int widest = 0, tallest = 0;
    for (int x = 0; x < sw; ++x) {
        const int c0 = footprint_lo(x, W, pre_w), c1 = footprint_hi(x, W, pre_w);
        if (!(0 <= c0 && c0 < c1 && c1 <= W)) throw_error("mask_prior: a footprint leaves the mask");
        widest = c1 - c0 > widest ? c1 - c0 : widest;
    }
    for (int y = 0; y < sh; ++y) {
        const int r0 = footprint_lo(y, H, pre_h), r1 = footprint_hi(y, H, pre_h);
        if (!(0 <= r0 && r0 < r1 && r1 <= H)) throw_error("mask_prior: a footprint leaves the mask");
        tallest = r1 - r0 > tallest ? r1 - r0 : tallest;
    }
    if ((int64_t)255 * widest * tallest >= (int64_t)1 << 24)
        throw_error("mask_prior: the mask is too large for the extent the image was encoded at (a footprint's sum leaves 24 bits)");
    for (int x0 = 0; x0 < sw; x0 += kSeg) {
        const int x1 = (x0 + kSeg < sw ? x0 + kSeg : sw) - 1;
        if (footprint_hi(x1, W, pre_w) - footprint_lo(x0, W, pre_w) > kSpanMax)
            throw_error("mask_prior: the mask is too wide for the extent the image was encoded at");
    }
    const PriorArgs a{mask, plane, W, H, pre_w, pre_h, sw, sh, (float)strength_milli / 1000.f};
    hipLaunchKernelGGL(mask_prior_kernel, dim3(LOW / kSeg, LOW), dim3(kSeg), 0, s, a);
}

}  // namespace k
}  // namespace dlimg
