// K17  longest-side resize: the stb_image_resize-equivalent resampler on the device
// (reference: dlimg::resize -> stbir_resize_uint8_generic, /root/reference/src/image.cpp:37-51).
// Two separable passes over host-built contributor tables (csrc/resize_tables.cpp):
//   horizontal: u8 --sRGB table--> linear float, weighted gather along x into fp32 rows of the output width
//   vertical  : weighted gather along y, float --Giesen table--> sRGB u8
// The same two passes with a linear decode table and no encode table are dlimg::resize_mask (image.cpp:53-62).
// Every multiply and add is explicitly rounded (no fma) and runs in increasing source order, so the
// result is bit-identical to oracle/stb_resize.py.  Edges clamp.
#include "device_common.hpp"
#include "kernels.hpp"

// bit-exactness contract with the oracle: no mul+add contraction anywhere in this file
#pragma clang fp contract(off)

namespace dlimg {
namespace {

__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t* __restrict__ src, int w, int h, int stride, int C,
                                                       const int* __restrict__ first, const int* __restrict__ count,
                                                       const float* __restrict__ coef, int taps, int ow,
                                                       const float* __restrict__ decode, float* __restrict__ tmp) {
    __shared__ float lut[256];
    lut[threadIdx.x] = decode[threadIdx.x];
    __syncthreads();
    const long total = (long)h * ow;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int y = (int)(i / ow), ox = (int)(i % ow);
        const uint8_t* row = src + (size_t)y * stride;
        const int f = first[ox], n = count[ox];
        const float* cf = coef + (size_t)ox * taps;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < n; ++t) {
            const int j = min(max(f + t, 0), w - 1);
            const float wgt = cf[t];
            const uint8_t* px = row + (size_t)j * C;
            for (int c = 0; c < C; ++c) acc[c] = __fadd_rn(acc[c], __fmul_rn(lut[px[c]], wgt));
        }
        float* dst = tmp + (size_t)i * C;
        for (int c = 0; c < C; ++c) dst[c] = acc[c];
    }
}

DLIMG_DEVICE uint8_t linear_to_srgb_uchar(float in, const uint32_t* tab4) {
    const float minval = __uint_as_float((127u - 13u) << 23);
    const float almost_one = __uint_as_float(0x3f7fffffu);
    if (!(in > minval)) in = minval;
    if (in > almost_one) in = almost_one;
    const uint32_t u = __float_as_uint(in);
    const uint32_t tab = tab4[(u - ((127u - 13u) << 23)) >> 20];
    const uint32_t bias = (tab >> 16) << 9;
    const uint32_t scale = tab & 0xffffu;
    const uint32_t t = (u >> 12) & 0xffu;
    return (uint8_t)((bias + scale * t) >> 16);
}

// STBIR_COLORSPACE_LINEAR encode: (int)(saturate(v) * 255 + 0.5)
DLIMG_DEVICE uint8_t linear_to_uchar(float v) {
    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    return (uint8_t)(int)__fadd_rn(__fmul_rn(v, 255.0f), 0.5f);
}

template <bool SRGB>
__global__ __launch_bounds__(256) void resize_v_kernel(const float* __restrict__ tmp, int h, int ow, int C,
                                                       const int* __restrict__ first, const int* __restrict__ count,
                                                       const float* __restrict__ coef, int taps, int oh,
                                                       const uint32_t* __restrict__ encode, uint8_t* __restrict__ dst) {
    __shared__ uint32_t tab4[104];
    if (SRGB && threadIdx.x < 104) tab4[threadIdx.x] = encode[threadIdx.x];
    __syncthreads();
    const long total = (long)oh * ow;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int oy = (int)(i / ow), ox = (int)(i % ow);
        const int f = first[oy], n = count[oy];
        const float* cf = coef + (size_t)oy * taps;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < n; ++t) {
            const int j = min(max(f + t, 0), h - 1);
            const float wgt = cf[t];
            const float* px = tmp + ((size_t)j * ow + ox) * C;
            for (int c = 0; c < C; ++c) acc[c] = __fadd_rn(acc[c], __fmul_rn(px[c], wgt));
        }
        uint8_t* out = dst + (size_t)i * C;
        for (int c = 0; c < C; ++c) out[c] = SRGB ? linear_to_srgb_uchar(acc[c], tab4) : linear_to_uchar(acc[c]);
    }
}

// ---------------------------------------------------------------------------------------------
// K18  longest-side resize fused with pixel pre-processing, for all images of one encoder pass.
//
// The arithmetic is that of resize_h_kernel / resize_v_kernel above followed by preprocess_kernel (elementwise.hip):
// every colour channel is resampled on its own, so dropping the channels the encoder never reads (alpha) and keeping
// the resampled sRGB byte in a register instead of a 1024 x 1024 u8 image changes no bit of the patch matrix.
//   stage 1  resize_rows_kernel: u8 rows -> fp32 rows of the target width, R / G / B (or the one mask channel) as planes
//            [nc][h][pitch], pitch = rw rounded up to 8 floats.  A workgroup takes 256 neighbouring outputs of RZ_ROWS
//            source rows; the bytes those outputs draw on are brought into LDS as aligned 16-byte pieces (their taps
//            overlap: every source byte is fetched once per workgroup instead of once per tap).
//   stage 2  resize_cols_preprocess_kernel: the lane mapping of preprocess_kernel (a lane owns 8 pixels of one patch row);
//            the taps of a row are 32-byte reads of the planes, four lanes to a 128-byte line; then the Giesen encode,
//            (u8 - mean) / std, zero padding and the 16-byte patch-major stores.
// One launch per stage for up to RZ_MAX_JOBS images (the job list travels in the kernel arguments).

constexpr int RZ_MAX_JOBS = 16;
constexpr int RZ_ROWS = 4;                   // source rows per stage 1 workgroup
constexpr int RZ_SPAN_BYTES = 32 * 1024;     // LDS for the source bytes of 256 outputs: RGBA shrunk up to ~32 x

struct RzJob {
    const uint8_t* src;
    const int *xfirst, *xcount, *yfirst, *ycount;
    const float *xcoef, *ycoef;
    float* tmp;
    half_t* patches;
    int w, h, stride, channels, xtaps, ytaps, rw, rh, pitch;
    int block_begin;                         // stage 1: first workgroup of this image
};
struct RzJobs { RzJob j[RZ_MAX_JOBS]; int n; };

__global__ __launch_bounds__(256) void resize_rows_kernel(RzJobs jobs, const float* __restrict__ decode) {
    __shared__ float lut[256];
    __shared__ __attribute__((aligned(16))) uint8_t span[RZ_SPAN_BYTES];
    __shared__ int range[2];
    const int tid = threadIdx.x;
    lut[tid] = decode[tid];
    if (tid == 0) { range[0] = 0x7fffffff; range[1] = -1; }
    int ji = 0;
    while (ji + 1 < jobs.n && (int)blockIdx.x >= jobs.j[ji + 1].block_begin) ++ji;
    const RzJob job = jobs.j[ji];
    const int w = job.w, h = job.h, rw = job.rw;
    const ChannelMap cm = channel_map(job.channels);
    const int C = cm.bytes, nc = C == 1 ? 1 : 3;
    const int chunks = (rw + 255) / 256;
    const int local = (int)blockIdx.x - job.block_begin;
    const int ox = (local % chunks) * 256 + tid;
    const int y0 = (local / chunks) * RZ_ROWS;
    const bool active = ox < rw;
    int f = 0, n = 0;
    __syncthreads();
    if (active) {
        f = job.xfirst[ox];
        n = job.xcount[ox];
        if (n > 0) {       // the clamped taps of this output lie in [clamp(f), clamp(f + n - 1)]
            atomicMin(&range[0], min(max(f, 0), w - 1));
            atomicMax(&range[1], min(max(f + n - 1, 0), w - 1));
        }
    }
    __syncthreads();
    const int lo = range[0], hi = range[1];
    if (hi < lo) {                               // no output of this chunk has a tap (uniform): sums of nothing, as resize_h_kernel
        if (active)
            for (int y = y0; y < min(y0 + RZ_ROWS, h); ++y)
                for (int c = 0; c < nc; ++c)
                    job.tmp[((size_t)c * h + y) * job.pitch + ox] = 0.f;
        return;
    }
    const float* cf = job.xcoef + (size_t)ox * job.xtaps;
    const size_t row_bytes = (size_t)w * C;
    const size_t need = (size_t)(hi - lo + 1) * C;
    // In LDS the bytes lie as in memory from the 16-byte boundary at or below the first one (at most 15 bytes of slack).
    // A chunk whose source bytes do not fit (an image shrunk more than ~32 x) reads its taps from memory instead.
    const bool staged = need + 15 <= (size_t)RZ_SPAN_BYTES;
    for (int y = y0; y < min(y0 + RZ_ROWS, h); ++y) {
        const uint8_t* row = job.src + (size_t)y * job.stride;
        const uint8_t* g0 = row + (size_t)lo * C;
        const uint8_t* a0 = g0 - ((uintptr_t)g0 & 15);
        const int shift = (int)(g0 - a0);
        if (staged) {
            const int pieces = (int)((shift + need + 15) / 16);
            for (int p = tid; p < pieces; p += 256) {
                const uint8_t* a = a0 + (size_t)p * 16;
                if (a >= row && a + 16 <= row + row_bytes) {          // a whole piece inside this row of the view
                    *reinterpret_cast<uint4*>(span + p * 16) = *reinterpret_cast<const uint4*>(a);
                } else {                                              // the pieces at the ends of the row: byte by byte
                    for (int b = 0; b < 16; ++b) span[p * 16 + b] = (a + b >= row && a + b < row + row_bytes) ? a[b] : (uint8_t)0;
                }
            }
            __syncthreads();
        }
        if (active) {
            float acc[3] = {0.f, 0.f, 0.f};
            const bool word = staged && C == 4 && (((uintptr_t)g0 & 3) == 0);
            for (int t = 0; t < n; ++t) {
                const int j = min(max(f + t, 0), w - 1);
                const float wgt = cf[t];
                if (word) {
                    const uint32_t px = *reinterpret_cast<const uint32_t*>(span + shift + (j - lo) * 4);
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        acc[c] = __fadd_rn(acc[c], __fmul_rn(lut[(px >> (8 * cm.idx[c])) & 0xffu], wgt));
                } else if (staged) {
                    const uint8_t* px = span + shift + (j - lo) * C;
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (c < nc) acc[c] = __fadd_rn(acc[c], __fmul_rn(lut[px[cm.idx[c]]], wgt));
                } else {
                    const uint8_t* px = row + (size_t)j * C;
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (c < nc) acc[c] = __fadd_rn(acc[c], __fmul_rn(lut[px[cm.idx[c]]], wgt));
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (c < nc) job.tmp[((size_t)c * h + y) * job.pitch + ox] = acc[c];
        }
        if (staged) __syncthreads();                                  // the next row overwrites the span
    }
}

__global__ __launch_bounds__(256) void resize_cols_preprocess_kernel(RzJobs jobs, const uint32_t* __restrict__ encode) {
    __shared__ uint32_t tab4[104];
    if (threadIdx.x < 104) tab4[threadIdx.x] = encode[threadIdx.x];
    __syncthreads();
    const RzJob job = jobs.j[blockIdx.y];
    const int h = job.h, rw = job.rw, rh = job.rh, pitch = job.pitch;
    const int nc = channel_map(job.channels).bytes == 1 ? 1 : 3;
    const PatchLane pl = patch_lane();                          // as preprocess_kernel
    const int y = pl.y, x0 = pl.x0;

    float v[3][8];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 8; ++i) v[c][i] = 0.f;

    if (y < rh && x0 < rw) {
        const int f = job.yfirst[y], n = job.ycount[y];
        const float* cf = job.ycoef + (size_t)y * job.ytaps;
        const float* col = job.tmp + x0;                        // x0 + 8 <= pitch; what lies beyond rw is never used
        float acc[3][8];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[c][i] = 0.f;
        for (int t = 0; t < n; ++t) {
            const int j = min(max(f + t, 0), h - 1);
            const float wgt = cf[t];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c < nc) {
                    const float4_t* src = reinterpret_cast<const float4_t*>(col + ((size_t)c * h + j) * pitch);
                    const float4_t a = src[0], b = src[1];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        acc[c][i] = __fadd_rn(acc[c][i], __fmul_rn(a[i], wgt));
                        acc[c][4 + i] = __fadd_rn(acc[c][4 + i], __fmul_rn(b[i], wgt));
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (x0 + i < rw) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float u = (float)linear_to_srgb_uchar(acc[c < nc ? c : 0][i], tab4);
                    v[c][i] = normalise_pixel(u, c);
                }
            }
        }
    }
    store_patch_pixels(job.patches, pl, v);
}

}  // namespace

namespace k {

void resize_srgb(const uint8_t* src, int w, int h, int stride, int C, const ResizeAxis& ax, const ResizeAxis& ay,
                 const float* decode_lut, const uint32_t* encode_tab, float* tmp, uint8_t* dst, hipStream_t s) {
    if (w <= 0 || h <= 0 || C < 1 || C > 4 || stride < w * C) throw_error("resize_srgb: invalid source image");
    if (ax.out <= 0 || ay.out <= 0 || ax.taps <= 0 || ay.taps <= 0) throw_error("resize_srgb: invalid tables");
    const long n1 = (long)h * ax.out, n2 = (long)ay.out * ax.out;
    auto grid = [](long n) { long g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); };
    hipLaunchKernelGGL(resize_h_kernel, dim3(grid(n1)), dim3(256), 0, s, src, w, h, stride, C, ax.first, ax.count, ax.coef,
                       ax.taps, ax.out, decode_lut, tmp);
    if (encode_tab)
        hipLaunchKernelGGL(resize_v_kernel<true>, dim3(grid(n2)), dim3(256), 0, s, tmp, h, ax.out, C, ay.first, ay.count,
                           ay.coef, ay.taps, ay.out, encode_tab, dst);
    else        // linear colour space (resize_mask): decode_lut holds i / 255
        hipLaunchKernelGGL(resize_v_kernel<false>, dim3(grid(n2)), dim3(256), 0, s, tmp, h, ax.out, C, ay.first, ay.count,
                           ay.coef, ay.taps, ay.out, encode_tab, dst);
}

size_t resize_preprocess_tmp_floats(int h, int rw, int channels) {
    const size_t pitch = ((size_t)rw + 7) & ~(size_t)7;
    const size_t n = (size_t)(channels == 1 ? 1 : 3) * h * pitch;
    return (n + 63) & ~(size_t)63;               // a multiple of 256 bytes: areas carved one after the other stay aligned
}

void resize_preprocess_batch(const ResizeJob* list, int count, const float* decode_lut, const uint32_t* encode_tab,
                             hipStream_t s) {
    if (!decode_lut || !encode_tab) throw_error("resize_preprocess: the colour space tables are missing");
    for (int base = 0; base < count; base += RZ_MAX_JOBS) {
        const int n = count - base < RZ_MAX_JOBS ? count - base : RZ_MAX_JOBS;
        RzJobs jobs{};
        long blocks = 0;
        for (int i = 0; i < n; ++i) {
            const ResizeJob& r = list[base + i];
            if (!r.src || !r.tmp || !r.patches) throw_error("resize_preprocess: null buffer");
            if (!(r.channels == 1 || r.channels == 3 || r.channels == 4 || r.channels == 5 || r.channels == 6))
                throw_error("resize_preprocess: unsupported channel order");
            const int bytes = channel_map(r.channels).bytes;
            if (r.w <= 0 || r.h <= 0 || r.stride < r.w * bytes) throw_error("resize_preprocess: invalid source image");
            if (r.ax.out <= 0 || r.ay.out <= 0 || r.ax.out > 1024 || r.ay.out > 1024 || r.ax.taps <= 0 || r.ay.taps <= 0 ||
                !r.ax.first || !r.ax.count || !r.ax.coef || !r.ay.first || !r.ay.count || !r.ay.coef)
                throw_error("resize_preprocess: invalid tables");
            if (((uintptr_t)r.tmp & 31) != 0) throw_error("resize_preprocess: the scratch area must be 32-byte aligned");
            RzJob& j = jobs.j[i];
            j.src = r.src;
            j.xfirst = r.ax.first; j.xcount = r.ax.count; j.xcoef = r.ax.coef; j.xtaps = r.ax.taps;
            j.yfirst = r.ay.first; j.ycount = r.ay.count; j.ycoef = r.ay.coef; j.ytaps = r.ay.taps;
            j.tmp = r.tmp;
            j.patches = r.patches;
            j.w = r.w; j.h = r.h; j.stride = r.stride; j.channels = r.channels;
            j.rw = r.ax.out; j.rh = r.ay.out;
            j.pitch = (r.ax.out + 7) & ~7;
            j.block_begin = (int)blocks;
            blocks += (long)((r.ax.out + 255) / 256) * ((r.h + RZ_ROWS - 1) / RZ_ROWS);
            if (blocks > 0x7fffffffL) throw_error("resize_preprocess: the images of one pass have too many rows");
        }
        jobs.n = n;
        hipLaunchKernelGGL(resize_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, jobs, decode_lut);
        hipLaunchKernelGGL(resize_cols_preprocess_kernel, dim3(512, n), dim3(256), 0, s, jobs, encode_tab);
    }
}

}  // namespace k
}  // namespace dlimg
