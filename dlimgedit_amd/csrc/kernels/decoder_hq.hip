// SAM-HQ's per-prompt mask path (sam-hq: MaskDecoderHQ.embedding_maskfeature and the HQ mask product) and the kernel that
// finishes the per-image HQ features:
//
//   hqplane[p][Y][X] = hyper_hq[p] . ( conv2_3x3( GELU( LN2d_64( conv1_3x3(U[p]) ) ) ) + hq_features[image of p] )[Y][X]
//   logits[p][m][Y][X] += hqplane[p][Y][X]   for the four planes m
//
// U[p] is the up-scaled embedding [256][256][32] f16 that upscale_logits leaves (its STORE_U form).  Both 3x3 convolutions
// (zero padding 1) are implicit GEMMs on v_mfma_f32_16x16x32_f16: a workgroup takes a 16 x 16 tile of pixels, stages the
// 18 x 18 halo of its input in LDS and walks the nine taps; for one tap the B operand of a tile row is 16 neighbouring pixels
// of the halo (lane l: pixel l % 16, channels 8 (l / 16) .. + 7, one 16-byte LDS read) and the A operand 16 output channels of
// the tap's weight slice (lane l: channel l % 16, the same eight input channels).  No im2col matrix exists anywhere.  The
// accumulator then holds, in lane (pixel j = l % 16, group g = l / 16), output channels 16 ct + 4 g + r of pixel j: a pixel's
// channels sit in the four lanes l, l ^ 16, l ^ 32, l ^ 48, so LayerNorm2d and the final dot product fold over the registers
// and two lane exchanges, and the intermediate is stored as 8-byte channel runs.  Accumulation, the LayerNorm statistics
// (two-pass), GELU (erf form) and the dot product are fp32.
//
// Two launches, with the 64-channel f16 intermediate H[p][256][256][64] in HBM between them (8 MB per prompt): the second
// convolution pads ITS input with zeros at the image border, which a fused kernel has to restate for the ring of intermediate
// pixels outside the image; the two-launch form gets it from the halo load and was the one finished.
//
// LDS layout of a halo: [18][18] pixels, a pixel's channels contiguous, pixel stride padded to 80 bytes (32 channels) / 144
// bytes (64 channels): the 16 pixels of a fragment read then start 20 / 36 banks apart, which are 16 different multiples of 4
// mod 64 -- a 16-byte read per lane without bank conflicts inside each group of 16 lanes.
#include "device_common.hpp"
#include "kernels.hpp"

namespace dlimg {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
DLIMG_DEVICE f32x4 mfma16(half8_t a, half8_t b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
DLIMG_DEVICE float sum_over_groups(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

constexpr int RES = 256;              // the low-res grid
constexpr int TILE = 16, HALO = TILE + 2;
constexpr int C_IN1 = 32, C_MID = 64, C_OUT = 32;
constexpr int PIX1 = C_IN1 + 8;       // halves per halo pixel in LDS, first convolution (80 bytes)
constexpr int PIX2 = C_MID + 8;       // ... second convolution (144 bytes)
constexpr size_t LDS1 = (size_t)HALO * HALO * PIX1 * 2;      // 25.3 KB
constexpr size_t LDS2 = (size_t)HALO * HALO * PIX2 * 2;      // 45.6 KB
static_assert(LDS1 <= 64 * 1024 && LDS2 <= 64 * 1024, "below the default dynamic-LDS limit");

// halo of tile (ty, tx) of a [256][256][C] f16 map -> LDS, zeros outside the map; C / 8 chunks of 16 bytes per pixel
template <int C, int PIX>
DLIMG_DEVICE void load_halo(const half_t* __restrict__ map, int ty, int tx, half_t* lds) {
    constexpr int CH = C / 8;
    for (int i = threadIdx.x; i < HALO * HALO * CH; i += 256) {
        const int pix = i / CH, ch = i % CH;
        const int y = ty * TILE - 1 + pix / HALO, x = tx * TILE - 1 + pix % HALO;
        half8_t v = zero_h8();
        if (y >= 0 && y < RES && x >= 0 && x < RES) v = *reinterpret_cast<const half8_t*>(map + ((size_t)y * RES + x) * C + ch * 8);
        *reinterpret_cast<half8_t*>(lds + pix * PIX + ch * 8) = v;
    }
}

struct HqConv1 {
    const half_t* U;                  // [P][256][256][32]
    const half_t* W;                  // [9][64][32]: tap, output channel, input channel
    const float* b; const float* ln_w; const float* ln_b; float eps;
    half_t* H;                        // [P][256][256][64]
};

// grid (256 tiles, P); wave w takes tile rows 4 w .. 4 w + 3, all 64 output channels
__global__ __launch_bounds__(256) void hq_conv1_kernel(HqConv1 a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* halo = reinterpret_cast<half_t*>(smem);
    const int p = blockIdx.y, ty = blockIdx.x >> 4, tx = blockIdx.x & 15;
    const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
    load_halo<C_IN1, PIX1>(a.U + (size_t)p * RES * RES * C_IN1, ty, tx, halo);
    __syncthreads();
    f32x4 acc[4][4];                  // [row of the wave][channel tile]
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[r][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap % 3;
        half8_t w[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
            w[ct] = *reinterpret_cast<const half8_t*>(a.W + ((size_t)tap * C_MID + ct * 16 + j) * C_IN1 + 8 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int hy = wave * 4 + r + ky, hx = j + kx;
            const half8_t px = *reinterpret_cast<const half8_t*>(halo + (hy * HALO + hx) * PIX1 + 8 * g);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[r][ct] = mfma16(w[ct], px, acc[r][ct]);
        }
    }
    // + bias, LayerNorm2d over the 64 channels of a pixel, GELU, f16
    float4_t bias[4], lw[4], lb[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        bias[ct] = reinterpret_cast<const float4_t*>(a.b)[ct * 4 + g];
        lw[ct] = reinterpret_cast<const float4_t*>(a.ln_w)[ct * 4 + g];
        lb[ct] = reinterpret_cast<const float4_t*>(a.ln_b)[ct * 4 + g];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float sum = 0.f;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[r][ct][e] += bias[ct][e];
                sum += acc[r][ct][e];
            }
        const float mean = sum_over_groups(sum) * (1.0f / C_MID);
        float sq = 0.f;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[r][ct][e] -= mean;
                sq = fmaf(acc[r][ct][e], acc[r][ct][e], sq);
            }
        const float rstd = 1.0f / sqrtf(sum_over_groups(sq) * (1.0f / C_MID) + a.eps);
        const int Y = ty * TILE + wave * 4 + r, X = tx * TILE + j;
        half_t* dst = a.H + (((size_t)p * RES + Y) * RES + X) * C_MID + 4 * g;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            half4_t h;
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = (half_t)gelu_erf(acc[r][ct][e] * rstd * lw[ct][e] + lb[ct][e]);
            *reinterpret_cast<half4_t*>(dst + ct * 16) = h;
        }
    }
}

struct HqConv2 {
    const half_t* H;                  // [P][256][256][64]
    const half_t* W;                  // [9][32][64]: tap, output channel, input channel
    const float* b;                   // [32]
    const float* feat[k::kDecoderMaxPrompts];       // per prompt: hq_features of its image, [256][256][32] fp32
    const float* hyper_hq;            // [P][32]
    float* logits;                    // [P][4][256][256]
};

__global__ __launch_bounds__(256) void hq_conv2_kernel(HqConv2 a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* halo = reinterpret_cast<half_t*>(smem);
    const int p = blockIdx.y, ty = blockIdx.x >> 4, tx = blockIdx.x & 15;
    const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
    load_halo<C_MID, PIX2>(a.H + (size_t)p * RES * RES * C_MID, ty, tx, halo);
    __syncthreads();
    f32x4 acc[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[r][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap % 3;
        half8_t w[2][2];              // [channel tile][k half]
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int kh = 0; kh < 2; ++kh)
                w[ct][kh] = *reinterpret_cast<const half8_t*>(a.W + ((size_t)tap * C_OUT + ct * 16 + j) * C_MID + 32 * kh + 8 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int hy = wave * 4 + r + ky, hx = j + kx;
            const half_t* src = halo + (hy * HALO + hx) * PIX2 + 8 * g;
#pragma unroll
            for (int kh = 0; kh < 2; ++kh) {
                const half8_t px = *reinterpret_cast<const half8_t*>(src + 32 * kh);
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) acc[r][ct] = mfma16(w[ct][kh], px, acc[r][ct]);
            }
        }
    }
    float4_t bias[2], hy4[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        bias[ct] = reinterpret_cast<const float4_t*>(a.b)[ct * 4 + g];
        hy4[ct] = reinterpret_cast<const float4_t*>(a.hyper_hq + (size_t)p * C_OUT)[ct * 4 + g];
    }
    const float* __restrict__ feat = a.feat[p];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int Y = ty * TILE + wave * 4 + r, X = tx * TILE + j;
        const float4_t* f = reinterpret_cast<const float4_t*>(feat + ((size_t)Y * RES + X) * C_OUT);
        float d = 0.f;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const float4_t fv = f[ct * 4 + g];
#pragma unroll
            for (int e = 0; e < 4; ++e) d = fmaf((acc[r][ct][e] + bias[ct][e]) + fv[e], hy4[ct][e], d);
        }
        d = sum_over_groups(d);
        // group g of the pixel's four lanes adds the plane to logits plane g
        float* out = a.logits + (((size_t)p * 4 + g) * RES + Y) * RES + X;
        *out += d;
    }
}

struct HqFinish {
    const float* vit;                 // [4096 * 4][128]: row = token * 4 + first sub-pixel, column = second sub-pixel * 32 + c
    const float* emb;                 // the same of the embedding branch
    const float* b_vit; const float* b_emb;          // [32] each
    float* out;                       // [256][256][32]
};

// one thread per (pixel, four channels): out = vit + emb + both biases, in raster order
__global__ __launch_bounds__(256) void hq_finish_kernel(HqFinish a) {
    const int i = blockIdx.x * 256 + threadIdx.x;            // < 65536 * 8
    const int c4 = i & 7, pix = i >> 3, X = pix & 255, Y = pix >> 8;
    const int tok = (Y >> 2) * 64 + (X >> 2), s1 = ((Y >> 1) & 1) * 2 + ((X >> 1) & 1), s2 = (Y & 1) * 2 + (X & 1);
    const size_t src = ((size_t)tok * 4 + s1) * 128 + s2 * 32 + c4 * 4;
    const float4_t v = *reinterpret_cast<const float4_t*>(a.vit + src) + *reinterpret_cast<const float4_t*>(a.emb + src) +
                       (reinterpret_cast<const float4_t*>(a.b_vit)[c4] + reinterpret_cast<const float4_t*>(a.b_emb)[c4]);
    reinterpret_cast<float4_t*>(a.out)[i] = v;
}

}  // namespace

namespace k {

void hq_features_finish(const float* vit, const float* emb, const float* b_vit, const float* b_emb, float* out, hipStream_t s) {
    if (!vit || !emb || !b_vit || !b_emb || !out) throw_error("hq_features_finish: null operand");
    if (((uintptr_t)vit | (uintptr_t)emb | (uintptr_t)b_vit | (uintptr_t)b_emb | (uintptr_t)out) & 15)
        throw_error("hq_features_finish: operands must be 16-byte aligned");
    HqFinish a{vit, emb, b_vit, b_emb, out};
    hipLaunchKernelGGL(hq_finish_kernel, dim3(RES * RES * 8 / 256), dim3(256), 0, s, a);
}

bool hq_mask_path_prompts(const float* const* features, int P) {
    if (P <= 0) return false;
    if (P > kDecoderMaxPrompts) throw_error("hq_mask_path: too many prompts for one launch");
    for (int i = 0; features && i < P; ++i)
        if (!features[i] || ((uintptr_t)features[i] & 15)) throw_error("hq_mask_path: every prompt needs its image's 16-byte aligned HQ features");
    return true;
}

void hq_mask_path(const half_t* U, const HqMaskWeights& w, float eps, half_t* H, const float* const* features,
                  const float* hyper_hq, float* logits, int P, hipStream_t s) {
    if (!hq_mask_path_prompts(features, P)) return;
    if (!U || !H || !features || !hyper_hq || !logits || !w.conv1_w || !w.conv1_b || !w.ln_w || !w.ln_b || !w.conv2_w || !w.conv2_b)
        throw_error("hq_mask_path: the model has no SAM-HQ group (dec.hq.*)");
    if (((uintptr_t)U | (uintptr_t)H | (uintptr_t)hyper_hq | (uintptr_t)w.conv1_w | (uintptr_t)w.conv1_b | (uintptr_t)w.ln_w |
         (uintptr_t)w.ln_b | (uintptr_t)w.conv2_w | (uintptr_t)w.conv2_b) & 15)
        throw_error("hq_mask_path: operands must be 16-byte aligned");
    HqConv2 b{H, w.conv2_w, w.conv2_b, {}, hyper_hq, logits};
    for (int i = 0; i < P; ++i) b.feat[i] = features[i];
    // both kernels stay below the 64 KB every kernel may ask for; the opt-in is made all the same, so that a device that
    // grants less is reported by name instead of by a failed launch
    static k::LdsOptIn opt_in1, opt_in2;
    opt_in1.ensure((const void*)hq_conv1_kernel, LDS1, "hq_mask_path: the device refuses the first convolution's LDS size");
    opt_in2.ensure((const void*)hq_conv2_kernel, LDS2, "hq_mask_path: the device refuses the second convolution's LDS size");
    HqConv1 a{U, w.conv1_w, w.conv1_b, w.ln_w, w.ln_b, eps, H};
    const dim3 grid((RES / TILE) * (RES / TILE), P);
    hipLaunchKernelGGL(hq_conv1_kernel, grid, dim3(256), LDS1, s, a);
    hipLaunchKernelGGL(hq_conv2_kernel, grid, dim3(256), LDS2, s, b);
}

}  // namespace k
}  // namespace dlimg
