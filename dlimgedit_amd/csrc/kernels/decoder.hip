// Token-side kernels of the SAM prompt encoder / mask decoder (everything that is NOT a big GEMM).
// In the reference all of this runs inside the decoder ONNX graph behind Session::operator()
// (/root/reference/src/segmentation.cpp:154-158); the published definition is SAM's PromptEncoder,
// TwoWayTransformer and MaskDecoder.  The token side is 7 or 8 tokens per prompt: latency-bound fp32
// VALU work, kept in fp32 end to end.
#include "device_common.hpp"
#include "kernels.hpp"
#include "gemm_plan.hpp"      // kStatRegs of gemm_f16_tile.inc

#include <cstring>
#include <mutex>
#include <type_traits>

namespace dlimg {
namespace {

#include "gemm_f16_tile.inc"

// Tokens per prompt: iou token + 4 mask tokens + the prompt's points -- 7 (a point and its pad token, or the two corners of
// a box), 8 (a point and a box), and up to 15 for several clicks (n clicks and the pad token: 6 + n, n clicks and a box:
// 7 + n, n <= 8).  It is the template parameter TOK of everything below that depends on it: the launchers pick the
// instantiation -- one per count, so a kernel sees exactly the packed token list and no attention has a key to mask --
// the 7-token code is what it was when TOK was a constant of this file, and a launch never mixes counts.
constexpr int OUT_TOK = 5;    // iou token + 4 mask tokens: the rows the heads read
constexpr int DIM = 256;
constexpr int INNER = 128;    // cross-attention width (downsample 2)
constexpr int HEADS = 8;
constexpr int NTOK_IMG = 4096;

// ---------------------------------------------------------------------------------------------
// Prompt encoder: SamOnnxModel._embed_points applied to the TOK - 5 packed points
// (segmentation.cpp:135-152 packs two; labels 1/-1 for a point, 2/3 for a box; SAM's PromptEncoder.forward puts the point
// in front of the box corners and sends no pad token with a box: labels 1, 2, 3).
// Column c of the TOK token rows of prompt p: iou token, 4 mask tokens, the prompt points.
// HQ (SAM-HQ models): the last packed point is the pseudo-point of the HQ token (kernels.hpp, kDecoderHqLabel): its row is
// hq_token[c] alone.
template <int TOK, bool HQ = false, typename Prompts>
DLIMG_DEVICE void prompt_token_column(const Prompts& pr, int p, int c, const float* __restrict__ gauss,
                                      const float* __restrict__ point_embed, const float* __restrict__ not_a_point,
                                      const float* __restrict__ iou_token, const float* __restrict__ mask_tokens,
                                      float (&out)[TOK], const float* __restrict__ hq_token = nullptr) {
    constexpr int NPTS = TOK - OUT_TOK;
    out[0] = iou_token[c];
#pragma unroll
    for (int m = 0; m < 4; ++m) out[1 + m] = mask_tokens[m * DIM + c];
    const int kf = c & 127;
#pragma unroll
    for (int i = 0; i < NPTS; ++i) {
        if constexpr (HQ) {
            if (i == NPTS - 1) {
                out[OUT_TOK + i] = hq_token[c];
                continue;
            }
        }
        const float x = (pr.coords[(p * NPTS + i) * 2 + 0] + 0.5f) / 1024.0f;
        const float y = (pr.coords[(p * NPTS + i) * 2 + 1] + 0.5f) / 1024.0f;
        float v = __fadd_rn(__fmul_rn(2.0f * x - 1.0f, gauss[kf]), __fmul_rn(2.0f * y - 1.0f, gauss[128 + kf]));
        v = 6.283185307179586f * v;
        float e = c < 128 ? sinf(v) : cosf(v);
        const float lab = pr.labels[p * NPTS + i];
        if (lab == -1.0f) e = not_a_point[c];
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4)
            if (lab == (float)k4) e += point_embed[k4 * DIM + c];
        out[OUT_TOK + i] = e;
    }
}



// ---------------------------------------------------------------------------------------------
// Token-side linear layers, several per launch, with the LayerNorm in front of them applied on the fly.
//
// The token side is a chain of tiny dependent steps (7 tokens per prompt); each launch costs 5-9 us whatever it computes
// (dispatch + a cold weight row per wave), so what matters is how few launches the chain takes.  Every LayerNorm of the
// two-way blocks is therefore evaluated by its CONSUMERS: a linear layer (or a residual read) names the un-normalised
// rows and the LayerNorm's parameters, every workgroup computes the rows' statistics itself (two-pass, fp32, as
// layernorm_vec_kernel) and normalises while it reads.  Layers that consume the same step run in one launch (q / k / v).
// (A lane-per-row form with the rows staged in LDS and wave-uniform weight loads was built as well: 18.8 us per launch
// at one prompt against 9.4 us for this one, 27 against 35 us at five prompts -- scalar weight loads and LDS reads
// share one counter and serialise.  Not kept.)
constexpr int RCHUNK = 8;               // rows a wave accumulates at a time in the token linears
constexpr int TL_MAX_ROWS = k::kDecoderMaxRows;   // 16 prompts x 7 tokens, or 14 prompts x 8 tokens, per launch
constexpr int TL_MAX_OPS = 5;
constexpr int TL_MAX_ROW_SLICE = 16;         // lane L of a wave finishes row L of a slice
// prompts per workgroup of the token linears and the fused attention-output kernels: two while two fit the 16 rows of a
// slice, one from 9 token rows on (k::decoder_prompt_slice is the launchers' copy)
template <int TOK> constexpr int TL_PROMPT_SLICE = k::decoder_prompt_slice(TOK);
// rows per workgroup of token_linears_kernel (whole prompts)
template <int TOK> constexpr int TL_ROW_SLICE = TL_PROMPT_SLICE<TOK> * TOK;

struct LinJob { k::TokenLinear op[TL_MAX_OPS]; int count; int rows; };

// (mean, rstd) of every row of a TokenRows matrix with a LayerNorm: rows dealt to the four waves
DLIMG_DEVICE void token_row_stats(const k::TokenRows& m, int rows, float2_t* stat /*LDS [rows]*/, int row0 = 0) {
    const int lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int r = row0 + wave; r < rows; r += nw) {
        const float4_t v = reinterpret_cast<const float4_t*>(m.x + (size_t)r * DIM)[lane];
        const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / DIM);
        const float4_t d = v - mean;
        const float var = wave_sum((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) * (1.0f / DIM);
        if (lane == 0) stat[r] = float2_t{mean, 1.0f / sqrtf(var + m.eps)};
    }
}
// 4 consecutive columns (4 * c4 ..) of row r
DLIMG_DEVICE float4_t token_row_load4(const k::TokenRows& m, const float2_t* stat, int r, int c4) {
    float4_t v = reinterpret_cast<const float4_t*>(m.x + (size_t)r * DIM)[c4];
    if (m.ln_w) {
        const float2_t st = stat[r];
        v = (v - st[0]) * st[1] * reinterpret_cast<const float4_t*>(m.ln_w)[c4] + reinterpret_cast<const float4_t*>(m.ln_b)[c4];
    }
    if (m.add) v += reinterpret_cast<const float4_t*>(m.add + (size_t)r * DIM)[c4];
    return v;
}
DLIMG_DEVICE float token_row_load1(const k::TokenRows& m, const float2_t* stat, int r, int c) {
    float v = m.x[(size_t)r * DIM + c];
    if (m.ln_w) v = (v - stat[r][0]) * stat[r][1] * m.ln_w[c] + m.ln_b[c];
    if (m.add) v += m.add[(size_t)r * DIM + c];
    return v;
}

// Rows [row0, row0 + rows) of a token matrix as its consumers see them (LayerNorm, addend) into LDS [rows][256].  What a
// launch of the token side costs is its chain of dependent round trips to L2 (1-2 us each), so every load of the step is
// issued before the first wait.  blockDim.x == 256: thread = column; statistics a wave per row (token_row_stats' arithmetic).
template <int MAXR>
DLIMG_DEVICE void stage_token_rows(const k::TokenRows& m, int row0, int rows, float* x_lds, float2_t* stat_lds) {
    const int c = threadIdx.x, lane = lane_id(), wave = c >> 6;
    float xv[MAXR], av[MAXR];
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        xv[r] = r < rows ? m.x[(size_t)(row0 + r) * DIM + c] : 0.f;
        av[r] = (m.add && r < rows) ? m.add[(size_t)(row0 + r) * DIM + c] : 0.f;
    }
    const float lw = m.ln_w ? m.ln_w[c] : 1.f, lb = m.ln_w ? m.ln_b[c] : 0.f;
    if (m.ln_w) {
        constexpr int PER_WAVE = (MAXR + 3) / 4;
        float4_t sv[PER_WAVE];
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) {
            const int r = wave + 4 * i;
            sv[i] = r < rows ? reinterpret_cast<const float4_t*>(m.x + (size_t)(row0 + r) * DIM)[lane] : float4_t{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) {
            const int r = wave + 4 * i;
            const float4_t v = sv[i];
            const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / DIM);
            const float4_t d = v - mean;
            const float var = wave_sum((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) * (1.0f / DIM);
            if (lane == 0 && r < rows) stat_lds[r] = float2_t{mean, 1.0f / sqrtf(var + m.eps)};
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < MAXR; ++r)
        if (r < rows) {
            float v = xv[r];
            if (m.ln_w) v = (v - stat_lds[r][0]) * stat_lds[r][1] * lw + lb;
            x_lds[r * DIM + c] = v + av[r];
        }
    __syncthreads();
}

// One output column per wave: Y[r][n] = act(in[r] . W[n] + b[n]) + resid[r][n] for all rows of a slice (<= 16).
// lds_in: rows of the input already in LDS ([rows][K] fp32; K <= 256) or null (then `op.in` is read from memory).
// TokenColumn: what the wave needs from memory for its column, requested by the caller BEFORE its own prologue so that the
// latency runs behind the statistics / attention work instead of after it: the first 64 float4 of the weight row (cold in
// the caches), the bias, and -- lane L for row row0 + L, which is the lane that finishes and stores that row -- the
// residual entry with its LayerNorm scale / shift.  [Before r03 lane 0 fetched bias and residual after the sums: one more
// round trip to L2 per call, which a workgroup that runs several columns per wave pays several times over.]
struct TokenColumn { float4_t w; float bias, rx, radd, rlw, rlb; };
static_assert(TL_ROW_SLICE<7> <= TL_MAX_ROW_SLICE && TL_ROW_SLICE<8> <= TL_MAX_ROW_SLICE && TL_ROW_SLICE<9> <= TL_MAX_ROW_SLICE &&
              TL_ROW_SLICE<k::kDecoderMaxTokens> <= TL_MAX_ROW_SLICE, "lane L of a wave finishes row L of the slice");
DLIMG_DEVICE TokenColumn token_column_prefetch(const k::TokenLinear& op, int first_col, int row0, int row1) {
    const int lane = lane_id();
    const int n = first_col + (threadIdx.x >> 6);
    TokenColumn c{float4_t{0.f, 0.f, 0.f, 0.f}, 0.f, 0.f, 0.f, 1.f, 0.f};
    if (n >= op.N) return c;
    if (lane < (op.K >> 2)) c.w = reinterpret_cast<const float4_t*>(op.W + (size_t)n * op.K)[lane];
    if (op.b) c.bias = op.b[n];
    if (op.resid.x) {
        const int r = min(row0 + lane, row1 - 1);
        c.rx = op.resid.x[(size_t)r * DIM + n];
        if (op.resid.add) c.radd = op.resid.add[(size_t)r * DIM + n];
        if (op.resid.ln_w) { c.rlw = op.resid.ln_w[n]; c.rlb = op.resid.ln_b[n]; }
    }
    return c;
}
// NR = rows of the slice: one or two whole prompts of TOK rows.
// The accumulate loop keeps the round-2 shape -- a run-time row bound, one guarded step per row, chunks of 8 -- and the whole
// library is built with -fno-slp-vectorize (dlimgedit_amd/build.py).  With the row count a compile-time constant and the
// seven rows' loads in straight-line code, the SLP vectoriser paired the rows (2,1), (4,3), (6,5) into chains of
// v_pk_fma_f32 with op_sel between v_mov shuffles, and THAT code got ONE output element in about 10^4 decodes wrong (error
// 0.02-0.5, always the low half of a pair: token row 2, 4 or 6) as soon as four host threads kept the execution lanes busy,
// and never from one thread.  Found by tools/decoder_stress.py (every workspace of the token side compared bit for bit with
// the serial answer); bisected in a second build by swapping single pieces: the epilogue, system-scope loads of the rows,
// a second barrier, lane-0 stores and lower occupancy made no difference, the loop shape did (0 in 320 000 decodes), and so
// did the compiler pass alone: the straight-line source built with -fno-slp-vectorize is clean too (0 in 240 000, the
// vectorised build of the same source 7 in 60 000 on the same box).  Every wait the ISA manual asks for is in the failing
// code; whether it is a gap in the compiler's hazard table for packed fp32 on gfx950 or an erratum is not known.  The
// tuning build keeps the failing form (-DDLIMG_STRAIGHT_ROWS, build it WITHOUT -fno-slp-vectorize to see it fail);
// tests/test_gpu_concurrency.py keeps the stress in the suite.
template <int TOK, int NR>
DLIMG_DEVICE void token_linear_columns(const k::TokenLinear& op, int first_col, const float* lds_in, const float2_t* stat_in,
                                       const float2_t* stat_res, const TokenColumn& col, int row0) {
    static_assert(NR % TOK == 0 && NR <= TL_MAX_ROW_SLICE, "slices are whole prompts");
    const int lane = lane_id();
    const int n = first_col + (threadIdx.x >> 6);
    if (n >= op.N) return;
    const int K4 = op.K >> 2;
    const float4_t* wr = reinterpret_cast<const float4_t*>(op.W + (size_t)n * op.K);
    float mine = 0.f;                       // the finished sum of row row0 + lane
#if defined(DLIMG_TUNING) && defined(DLIMG_STRAIGHT_ROWS)
    // the failing form, kept in the tuning build for the hunt (tools/decoder_stress.py with DLIMGEDIT_TUNING_LIB)
#pragma unroll
    for (int c0 = 0; c0 < NR; c0 += TOK) {
        float acc[TOK];
#pragma unroll
        for (int r = 0; r < TOK; ++r) acc[r] = 0.f;
        for (int k4 = lane; k4 < K4; k4 += 64) {
            const float4_t w = k4 == lane ? col.w : wr[k4];
            float4_t x[TOK];
#pragma unroll
            for (int r = 0; r < TOK; ++r) {
                if (lds_in) x[r] = reinterpret_cast<const float4_t*>(lds_in + (size_t)(c0 + r) * op.K)[k4];
                else if (op.K == DIM) x[r] = token_row_load4(op.in, stat_in, row0 + c0 + r, k4);
                else x[r] = reinterpret_cast<const float4_t*>(op.in.x + (size_t)(row0 + c0 + r) * op.K)[k4];
            }
#pragma unroll
            for (int r = 0; r < TOK; ++r)
                acc[r] = fmaf(x[r][0], w[0], fmaf(x[r][1], w[1], fmaf(x[r][2], w[2], fmaf(x[r][3], w[3], acc[r]))));
        }
#pragma unroll
        for (int r = 0; r < TOK; ++r) {
            const float v = wave_sum(acc[r]);
            if (lane == c0 + r) mine = v;
        }
    }
#else
    const int rows = row0 + NR;
    for (int r0 = row0; r0 < rows; r0 += RCHUNK) {
        float acc[RCHUNK];
#pragma unroll
        for (int r = 0; r < RCHUNK; ++r) acc[r] = 0.f;
        for (int k4 = lane; k4 < K4; k4 += 64) {
            const float4_t w = k4 == lane ? col.w : wr[k4];
#pragma unroll
            for (int r = 0; r < RCHUNK; ++r) {
                if (r0 + r < rows) {
                    float4_t x;
                    if (lds_in) x = reinterpret_cast<const float4_t*>(lds_in + (size_t)(r0 + r - row0) * op.K)[k4];
                    else if (op.K == DIM) x = token_row_load4(op.in, stat_in, r0 + r, k4);
                    else x = reinterpret_cast<const float4_t*>(op.in.x + (size_t)(r0 + r) * op.K)[k4];
                    acc[r] = fmaf(x[0], w[0], fmaf(x[1], w[1], fmaf(x[2], w[2], fmaf(x[3], w[3], acc[r]))));
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RCHUNK; ++r) {
            const float v = wave_sum(acc[r]);
            if (lane == r0 - row0 + r) mine = v;
        }
    }
#endif
    if (lane < NR) {
        const int r = row0 + lane;
        float v = mine + col.bias;
        if (op.relu) v = fmaxf(v, 0.f);
        if (op.resid.x) {
            float x = col.rx;
            if (op.resid.ln_w) x = (x - stat_res[r][0]) * stat_res[r][1] * col.rlw + col.rlb;
            v += x + col.radd;
        }
        op.Y[(size_t)r * op.N + n] = v;
    }
}
// the body once for each slice size
#define DLIMG_FOR_SLICE_ROWS(count, ...)                                   \
    if ((count) == TL_ROW_SLICE<TOK>) { constexpr int NR = TL_ROW_SLICE<TOK>; __VA_ARGS__ } \
    else { constexpr int NR = TOK; __VA_ARGS__ }

#if defined(DLIMG_TUNING) && defined(DLIMG_LOW_OCCUPANCY)
__attribute__((amdgpu_waves_per_eu(1, 4)))
#endif
template <int TOK>
__global__ __launch_bounds__(256) void token_linears_kernel(LinJob job) {
    __shared__ float2_t stat_in[TL_MAX_ROWS], stat_res[TL_MAX_ROWS];
    int o = 0, first = blockIdx.x * 4;
    while (o + 1 < job.count && first >= job.op[o].N) { first -= job.op[o].N; ++o; }      // N is a multiple of 4
    const k::TokenLinear& op = job.op[o];
    // rows are dealt to blockIdx.y in slices of TL_ROW_SLICE: more prompts are more workgroups, not longer ones
    const int row0 = blockIdx.y * TL_ROW_SLICE<TOK>, row1 = min(job.rows, row0 + TL_ROW_SLICE<TOK>);
    const TokenColumn w_first = token_column_prefetch(op, first, row0, row1);
    const bool ln_in = op.in.ln_w && op.K == DIM, ln_res = op.resid.x && op.resid.ln_w;
    if (ln_in) token_row_stats(op.in, row1, stat_in, row0);
    if (ln_res) token_row_stats(op.resid, row1, stat_res, row0);
    if (ln_in || ln_res) __syncthreads();
    DLIMG_FOR_SLICE_ROWS(row1 - row0, token_linear_columns<TOK, NR>(op, first, nullptr, stat_in, stat_res, w_first, row0);)
}

// Deep layers (the token MLP's second linear, K = 2048): one column per wave like token_linears_kernel, but the input
// rows are staged in LDS by the whole workgroup and the wave's weight row is requested in full before that, so no
// load sits inside the accumulation loop (that loop, 8 dependent trips to L2, made this launch 20.5 us for one prompt).
// Same order of additions as token_linear_columns: results are bit-identical.
constexpr int TLD_MAX_K = 2048;
template <int TOK>
__global__ __launch_bounds__(256) void token_linear_deep_kernel(k::TokenLinear op, int rows) {
    constexpr int row_slice = TL_ROW_SLICE<TOK>;
    extern __shared__ __attribute__((aligned(16))) float lds[];        // [row slice][K]
    __shared__ float2_t stat_res[TL_MAX_ROWS];
    const int lane = lane_id();
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int K4 = op.K >> 2, trips = K4 >> 6;
    const int row0 = blockIdx.y * row_slice, row1 = min(rows, row0 + row_slice);
    float4_t w[TLD_MAX_K / 256];
#pragma unroll
    for (int t = 0; t < TLD_MAX_K / 256; ++t)
        w[t] = (t < trips && n < op.N) ? reinterpret_cast<const float4_t*>(op.W + (size_t)n * op.K)[lane + 64 * t]
                                       : float4_t{0.f, 0.f, 0.f, 0.f};
    k::TokenLinear tail = op;          // bias and residual of the wave's column, requested with the weights (TokenColumn)
    tail.K = 0;
    const TokenColumn col = token_column_prefetch(tail, blockIdx.x * 4, row0, row1);
    const float4_t* src = reinterpret_cast<const float4_t*>(op.in.x + (size_t)row0 * op.K);
    float4_t* dst = reinterpret_cast<float4_t*>(lds);
    for (int i = threadIdx.x; i < (row1 - row0) * K4; i += 256) dst[i] = src[i];
    if (op.resid.x && op.resid.ln_w) token_row_stats(op.resid, row1, stat_res, row0);
    __syncthreads();
    if (n >= op.N) return;
    float mine = 0.f;
    for (int r = row0; r < row1; ++r) {
        const float4_t* xr = dst + (size_t)(r - row0) * K4;
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < TLD_MAX_K / 256; ++t)
            if (t < trips) {
                const float4_t x = xr[lane + 64 * t];
                acc = fmaf(x[0], w[t][0], fmaf(x[1], w[t][1], fmaf(x[2], w[t][2], fmaf(x[3], w[t][3], acc))));
            }
        const float v = wave_sum(acc);
        if (lane == r - row0) mine = v;
    }
    const int r = row0 + lane;
    if (r < row1) {
        float v = mine + col.bias;
        if (op.relu) v = fmaxf(v, 0.f);
        if (op.resid.x) {
            float x = col.rx;
            if (op.resid.ln_w) x = (x - stat_res[r][0]) * stat_res[r][1] * col.rlw + col.rlb;
            v += x + col.radd;
        }
        op.Y[(size_t)r * op.N + n] = v;
    }
}

// Tokens attend to the 4096 image positions (8 heads x 16), in two steps so that the 4096 keys of a head are spread
// over 8 workgroups (one workgroup per head streams 0.5 MB through a single CU and takes 44 us):
//   partial: workgroup = (prompt, head, key group of 512); a thread takes 2 keys (requested up front), then query
//            by query scores them, does the softmax against the wave's maximum (one exponential per score, no
//            rescale) and its part of P.V; butterfly inside each wave -> per-wave (max, sum, output[16]) in `part`
//   merge  : the consumers (token_merge_linear_kernel, output_heads_kernel) fold the 8 group partials in a fixed order
//            and apply the output projection themselves
// The query projection (LayerNorm + positional part on the fly, 256 -> 128) can ride in this launch: a workgroup needs
// the 16 columns of its head for the prompt's tokens only and computes them with the code (and bits) of token_linears_kernel.
constexpr int T2I_GROUPS = 8;                                  // key groups per head
constexpr int T2I_THREADS = 256;
constexpr int T2I_KEYS = NTOK_IMG / T2I_GROUPS / T2I_THREADS;  // keys per thread
constexpr int T2I_WAVES = T2I_THREADS / 64;
constexpr int T2I_PARTS = T2I_GROUPS;                          // partial triples per (prompt, head, query)

template <int TOK>
__global__ __launch_bounds__(T2I_THREADS) void token_to_image_partial_kernel(const float* __restrict__ q, k::TokenLinear qp,
                                                                             const half_t* __restrict__ K, int ldk,
                                                                             const half_t* __restrict__ V, int ldv,
                                                                             float* __restrict__ part) {
    __shared__ float sq[TOK * 16];
    __shared__ float qrows[TOK * INNER];
    __shared__ __attribute__((aligned(16))) float xrows[TOK * DIM];
    __shared__ float2_t qstat[TOK];
    __shared__ float wpart[TOK][T2I_WAVES][18];
    const int grp = blockIdx.x % T2I_GROUPS, h = (blockIdx.x / T2I_GROUPS) % HEADS, p = blockIdx.x / (T2I_GROUPS * HEADS);
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const size_t key0 = (size_t)p * NTOK_IMG + (size_t)grp * (NTOK_IMG / T2I_GROUPS);
    const half_t* kb = K + key0 * ldk + h * 16;
    const half_t* vb = V + key0 * ldv + h * 16;
    half8_t kreg[T2I_KEYS][2], vreg[T2I_KEYS][2];
#pragma unroll
    for (int i = 0; i < T2I_KEYS; ++i) {
        const size_t j = (size_t)i * T2I_THREADS + tid;
        kreg[i][0] = *reinterpret_cast<const half8_t*>(kb + j * ldk);
        kreg[i][1] = *reinterpret_cast<const half8_t*>(kb + j * ldk + 8);
        vreg[i][0] = *reinterpret_cast<const half8_t*>(vb + j * ldv);
        vreg[i][1] = *reinterpret_cast<const half8_t*>(vb + j * ldv + 8);
    }
    if (qp.W) {
        // q = qp(rows of prompt p) for the 16 columns of head h, 4 columns (one per wave) at a time
        const int row0 = p * TOK;
        TokenColumn wf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) wf[i] = token_column_prefetch(qp, h * 16 + 4 * i, row0, row0 + TOK);
        stage_token_rows<TOK>(qp.in, row0, TOK, xrows, qstat);
        qp.Y = qrows - (size_t)row0 * INNER;
#pragma unroll
        for (int i = 0; i < 4; ++i) token_linear_columns<TOK, TOK>(qp, h * 16 + 4 * i, xrows, nullptr, nullptr, wf[i], row0);
        __syncthreads();
        if (tid < TOK * 16) sq[tid] = qrows[(tid / 16) * INNER + h * 16 + (tid & 15)] * 0.25f;               // 16^-0.5
    } else if (tid < TOK * 16) {
        sq[tid] = q[((size_t)p * TOK + tid / 16) * INNER + h * 16 + (tid & 15)] * 0.25f;
    }
    __syncthreads();
    float* dst = part + ((((size_t)p * HEADS + h) * TOK) * T2I_PARTS + grp) * 18;
#pragma unroll 1
    for (int t = 0; t < TOK; ++t) {
        // keep K / V as the f16 they arrived in: otherwise the conversions to float are hoisted out of the query loop
#pragma unroll
        for (int i = 0; i < T2I_KEYS; ++i)
            asm volatile("" : "+v"(kreg[i][0]), "+v"(kreg[i][1]), "+v"(vreg[i][0]), "+v"(vreg[i][1]));
        float sc[T2I_KEYS];
#pragma unroll
        for (int i = 0; i < T2I_KEYS; ++i) {
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) s = fmaf(sq[t * 16 + e], (float)kreg[i][e >> 3][e & 7], s);
            sc[i] = s;
        }
        float m = sc[0];
#pragma unroll
        for (int i = 1; i < T2I_KEYS; ++i) m = fmaxf(m, sc[i]);
        const float M = wave_max(m);
        float l = 0.f, o[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e] = 0.f;
#pragma unroll
        for (int i = 0; i < T2I_KEYS; ++i) {
            const float pj = __expf(sc[i] - M);
            l += pj;
#pragma unroll
            for (int e = 0; e < 16; ++e) o[e] = fmaf(pj, (float)vreg[i][e >> 3][e & 7], o[e]);
        }
        const float ls = wave_sum(l);
        float* d = wpart[t][wave];
        if (lane == 0) { d[0] = M; d[1] = ls; }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float x = wave_sum(o[e]);
            if (lane == 0) d[2 + e] = x;
        }
    }
    // the four waves' partials of every query are folded here, in wave order: one triple per workgroup leaves
    __syncthreads();
    if constexpr (TOK * 18 <= T2I_THREADS) {
        if (tid < TOK * 18) {
            const int t = tid / 18, e = tid % 18;
            float M = wpart[t][0][0];
#pragma unroll
            for (int w = 1; w < T2I_WAVES; ++w) M = fmaxf(M, wpart[t][w][0]);
            float acc = 0.f;
#pragma unroll
            for (int w = 0; w < T2I_WAVES; ++w) acc += (e == 0 ? 0.f : wpart[t][w][e]) * __expf(wpart[t][w][0] - M);
            dst[(size_t)t * T2I_PARTS * 18 + e] = e == 0 ? M : acc;
        }
    } else {
        // 15 token rows: 270 values, a second trip for the last few (the same arithmetic)
        for (int i = tid; i < TOK * 18; i += T2I_THREADS) {
            const int t = i / 18, e = i % 18;
            float M = wpart[t][0][0];
#pragma unroll
            for (int w = 1; w < T2I_WAVES; ++w) M = fmaxf(M, wpart[t][w][0]);
            float acc = 0.f;
#pragma unroll
            for (int w = 0; w < T2I_WAVES; ++w) acc += (e == 0 ? 0.f : wpart[t][w][e]) * __expf(wpart[t][w][0] - M);
            dst[(size_t)t * T2I_PARTS * 18 + e] = e == 0 ? M : acc;
        }
    }
}


// Self-attention among the TOK tokens of every prompt (8 heads x 32), recomputed by every workgroup into LDS, followed by
// the output projection (one column per wave) with bias and residual: one launch instead of two.
// Thread c owns channel c of q, k and v of a prompt (3 TOK registers); a head is 32 adjacent lanes, so a score is one product
// per lane summed over the half wave (DPP inside the rows of 16, one lane exchange across them).  [The first version had
// every lane walk all 32 channels of its head out of LDS: 3136 LDS reads per thread and prompt, 12-14 us per launch.]
DLIMG_DEVICE float sum_over_32_lanes(float v) {
    v += dpp_move<0xB1>(v);
    v += dpp_move<0x4E>(v);
    v += dpp_move<0x141>(v);
    v += dpp_move<0x140>(v);
    return v + __shfl_xor(v, 16, 64);
}
template <int TOK>
DLIMG_DEVICE void token_self_attn_out_body(const float* __restrict__ q, const float* __restrict__ kx, const float* __restrict__ v,
                                           const k::TokenLinear& op, int P, const int block_x, const int block_y, float* lds) {
    // prompts are dealt to block_y in pairs (rows row0 .. row1 of the token matrix; LDS rows are local)
    const int p0 = block_y * TL_PROMPT_SLICE<TOK>, p1 = min(P, p0 + TL_PROMPT_SLICE<TOK>);
    const int row0 = p0 * TOK, row1 = p1 * TOK;
    float* att = lds;                                   // [rows of this slice][256]
    float2_t* stat_res = reinterpret_cast<float2_t*>(att + (size_t)TL_PROMPT_SLICE<TOK> * TOK * DIM) - row0;     // indexed by global row
    const TokenColumn w_first = token_column_prefetch(op, block_x * 4, row0, row1);
    const int c = threadIdx.x;
    const float scale = 0.17677669529663687f;           // 32^-0.5
    for (int p = p0; p < p1; ++p) {
        float rq[TOK], rk[TOK], rv[TOK];
#pragma unroll
        for (int t = 0; t < TOK; ++t) {
            rq[t] = q[((size_t)p * TOK + t) * DIM + c] * scale;
            rk[t] = kx[((size_t)p * TOK + t) * DIM + c];
            rv[t] = v[((size_t)p * TOK + t) * DIM + c];
        }
#pragma unroll
        for (int t = 0; t < TOK; ++t) {
            float s[TOK];
            float m = -INFINITY;
#pragma unroll
            for (int j = 0; j < TOK; ++j) {
                s[j] = sum_over_32_lanes(rq[t] * rk[j]);
                m = fmaxf(m, s[j]);
            }
            float l = 0.f, o = 0.f;
#pragma unroll
            for (int j = 0; j < TOK; ++j) {
                const float pj = expf(s[j] - m);
                l += pj;
                o = fmaf(pj, rv[j], o);
            }
            att[((size_t)(p - p0) * TOK + t) * DIM + c] = o / l;
        }
    }
    if (op.resid.x && op.resid.ln_w) token_row_stats(op.resid, row1, stat_res, row0);
    __syncthreads();
    DLIMG_FOR_SLICE_ROWS(row1 - row0, token_linear_columns<TOK, NR>(op, block_x * 4, att, nullptr, stat_res, w_first, row0);)
}
template <int TOK>
__global__ __launch_bounds__(256) void token_self_attn_out_kernel(const float* __restrict__ q, const float* __restrict__ kx,
                                                                  const float* __restrict__ v, k::TokenLinear op, int P) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    token_self_attn_out_body<TOK>(q, kx, v, op, P, blockIdx.x, blockIdx.y, lds);
}

// The same launch with the layer's image-side projection riding along: [K | Q | V] = keys . W^T (decoder_image side, an MFMA
// GEMM of 64 x 64 tiles, gemm_f16_tile) does not depend on the token self-attention and the self-attention not on it, and
// on their own they are 14 and 19 us one after the other, twice per decode (the stream is in order; a second stream costs
// more in cross-queue waits than it hides, and hipExtAnyOrderLaunch is not honoured on gfx950: LABNOTES r06).  The last
// `gemm_tiles` workgroups take one GEMM tile each -- the same code, tile shape and K order as the launch of its own, so the
// same bits -- in front of them the self-attention's workgroups.  Both parts use 256 threads.
constexpr int SAG_BM = 64, SAG_BN = 64;
constexpr size_t SAG_GEMM_LDS = (size_t)2 * (SAG_BM + SAG_BN) * 64 * 2 + aux_bytes(SAG_BM, SAG_BN);
template <int TOK> constexpr size_t SA_TOKEN_LDS = (size_t)TL_PROMPT_SLICE<TOK> * TOK * (DIM * 4 + 8);
template <int TOK> constexpr size_t SAG_LDS = SAG_GEMM_LDS > SA_TOKEN_LDS<TOK> ? SAG_GEMM_LDS : SA_TOKEN_LDS<TOK>;
static_assert(SAG_LDS<7> <= 48 * 1024 && SAG_LDS<8> <= 48 * 1024 && SAG_LDS<k::kDecoderMaxTokens> <= 48 * 1024,
              "below the default dynamic-LDS limit: no opt-in needed");
template <int TOK>
__global__ __launch_bounds__(256, 4) void self_attn_out_and_gemm_kernel(k::GemmArgs g, int gemm_tiles, const float* __restrict__ q,
                                                                        const float* __restrict__ kx, const float* __restrict__ v,
                                                                        k::TokenLinear op, int P, int token_blocks_x) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // the self-attention's workgroups come first: with many prompts the GEMM has thousands of tiles, and workgroups are
    // dispatched in index order -- behind them the long chain of the token part would start when the GEMM is all but done
    const int token_blocks = (int)gridDim.x - gemm_tiles;        // a multiple of 8: the tiles keep their XCDs
    if ((int)blockIdx.x < token_blocks) {
        token_self_attn_out_body<TOK>(q, kx, v, op, P, blockIdx.x % token_blocks_x, blockIdx.x / token_blocks_x, reinterpret_cast<float*>(smem));
        return;
    }
    gemm_f16_tile<SAG_BM, SAG_BN, 2, 2, 64, 2, 4, k::ACT_NONE, EPI_PLAIN>(g, xcd_remap((int)blockIdx.x - token_blocks, gemm_tiles), smem);
}

// The rest of the token-to-image attention, done by its CONSUMERS (a launch of its own cost 9-16 us for 0.2 MFLOP):
//   merge_partials         folds the 8 key-group partials of (prompt, head, token) in a fixed order -> att [rows][128] in LDS
//   output projection      thread c = output column c: y[r][c] = att[r] . Wo[c] + b[c] + resid[r][c] with Wo TRANSPOSED
//                          ([128][256], prepared at load) so that a wave reads 256 contiguous bytes per k
// Every workgroup of the consumer repeats both for the rows it needs (TOK x 256 x 128 FMAs at most per prompt, the 128 KB of
// Wo come out of L2), so the result is the same bits wherever it is computed and nothing has to be exchanged.
// NR rows starting at token t0 of prompt p0 (wrapping into the next prompts); blockDim.x >= 128.  Thread = (head, element)
// for the rows r = (tid / 128) + i * (blockDim.x / 128); the 24 values of up to 4 rows are requested before the first is
// used (one round trip to L2 for 4 rows, not four).
template <int TOK, int NR>
DLIMG_DEVICE void merge_partials(const float* __restrict__ part, int p0, int t0, float* att /*LDS [NR][128]*/) {
    const int e = threadIdx.x & 15, h = (threadIdx.x >> 4) & (HEADS - 1);
    const int rstep = blockDim.x >> 7, rfirst = threadIdx.x >> 7;
    constexpr int GROUP = 4;
    for (int base = 0; base < NR; base += GROUP * rstep) {
        float M[GROUP][T2I_PARTS], L[GROUP][T2I_PARTS], O[GROUP][T2I_PARTS];
#pragma unroll
        for (int i = 0; i < GROUP; ++i) {
            const int r = min(base + rfirst + i * rstep, NR - 1);
            const int p = p0 + (t0 + r) / TOK, t = (t0 + r) % TOK;
            const float* src = part + ((((size_t)p * HEADS + h) * TOK + t) * T2I_PARTS) * 18;
#pragma unroll
            for (int w = 0; w < T2I_PARTS; ++w) {
                M[i][w] = src[w * 18];
                L[i][w] = src[w * 18 + 1];
                O[i][w] = src[w * 18 + 2 + e];
            }
        }
#pragma unroll
        for (int i = 0; i < GROUP; ++i) {
            const int r = base + rfirst + i * rstep;
            float mx = M[i][0];
#pragma unroll
            for (int w = 1; w < T2I_PARTS; ++w) mx = fmaxf(mx, M[i][w]);
            float ls = 0.f, os = 0.f;
#pragma unroll
            for (int w = 0; w < T2I_PARTS; ++w) {
                const float f = __expf(M[i][w] - mx);
                ls += L[i][w] * f;
                os += O[i][w] * f;
            }
            if (r < NR) att[r * INNER + h * 16 + e] = os / ls;
        }
    }
}
// one row (the heads kernel): threads 0..127
DLIMG_DEVICE void merge_partials_one(const float* __restrict__ part, int p, int t, int TOK, float* att /*LDS [128]*/) {
    const int e = threadIdx.x & 15, h = (threadIdx.x >> 4) & (HEADS - 1);
    const float* src = part + ((((size_t)p * HEADS + h) * TOK + t) * T2I_PARTS) * 18;
    float M[T2I_PARTS], L[T2I_PARTS], O[T2I_PARTS];
#pragma unroll
    for (int w = 0; w < T2I_PARTS; ++w) {
        M[w] = src[w * 18];
        L[w] = src[w * 18 + 1];
        O[w] = src[w * 18 + 2 + e];
    }
    float mx = M[0];
#pragma unroll
    for (int w = 1; w < T2I_PARTS; ++w) mx = fmaxf(mx, M[w]);
    float ls = 0.f, os = 0.f;
#pragma unroll
    for (int w = 0; w < T2I_PARTS; ++w) {
        const float f = __expf(M[w] - mx);
        ls += L[w] * f;
        os += O[w] * f;
    }
    att[h * 16 + e] = os / ls;
}
// (mean, rstd) of rows held in LDS ([rows][256]); the arithmetic of token_row_stats
DLIMG_DEVICE void lds_row_stats(const float* y, int rows, float eps, float2_t* stat) {
    const int lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int r = wave; r < rows; r += nw) {
        const float4_t v = reinterpret_cast<const float4_t*>(y + (size_t)r * DIM)[lane];
        const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / DIM);
        const float4_t d = v - mean;
        const float var = wave_sum((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) * (1.0f / DIM);
        if (lane == 0) stat[r] = float2_t{mean, 1.0f / sqrtf(var + eps)};
    }
}

// Token-to-image attention finished (merge + output projection + residual -> out.Y, written by the first column block) and
// the NEXT linear (`next`, K = 256, whose input is the LayerNorm of those rows) applied to it: a workgroup = COLS columns
// of `next` for the rows of one prompt.  COLS = 16, 32 or 64: the smallest workgroups that still fit the chip in one round (16 for one or two prompts, 64
// from five) (every workgroup pays the fold, the 128 KB of Wo and the projection before its columns: at five prompts 640
// workgroups of 16 columns took 53 us, two and a half rounds on 256 CUs).  The arithmetic of a column does not depend on COLS.  [Kept small on purpose: code that runs once is fetched cold, and a 43 KB body --
// 32 columns, two prompts, everything unrolled -- took 24 us where this one takes half.]
template <int TOK>
constexpr size_t TML_LDS = (size_t)(INNER * DIM + TL_ROW_SLICE<TOK> * INNER + TL_ROW_SLICE<TOK> * DIM) * 4 + 2 * TL_ROW_SLICE<TOK> * 8;
template <int TOK, int NR, int COLS>
DLIMG_DEVICE void token_merge_linear_body(const float* __restrict__ part, const k::TokenLinear& out,
                                          const float* __restrict__ out_wt, const k::TokenLinear& next, int p0, float* lds) {
    float* wt = lds;                                     // [128][256]: the whole transposed output projection (128 KB)
    float* att = wt + INNER * DIM;                       // [rows][128]
    float* y = att + TL_ROW_SLICE<TOK> * INNER;          // [rows][256]
    float2_t* stat_res = reinterpret_cast<float2_t*>(y + TL_ROW_SLICE<TOK> * DIM);
    float2_t* stat_in = stat_res + TL_ROW_SLICE<TOK>;
    const int row0 = p0 * TOK, row1 = row0 + NR;
    const int first = blockIdx.x * COLS;
    const int c = threadIdx.x, lane = lane_id(), wave = c >> 6;
    // everything this workgroup reads is requested here: Wo as DMA into LDS (no registers), the wave's columns of `next`,
    // the residual rows; the partials follow in merge_partials
    for (int k = wave; k < INNER; k += 4) glds16(out_wt + (size_t)k * DIM + lane * 4, wt + k * DIM);
    TokenColumn col = token_column_prefetch(next, first, row0, row1);      // the later columns are requested one step ahead
    float res[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) res[r] = out.resid.x ? out.resid.x[(size_t)(row0 + r) * DIM + c] : 0.f;
    const bool res_ln = out.resid.x && out.resid.ln_w;
    const float rw = res_ln ? out.resid.ln_w[c] : 1.f, rb = res_ln ? out.resid.ln_b[c] : 0.f;
    const float ob = out.b ? out.b[c] : 0.f;
    const float nw = next.in.ln_w ? next.in.ln_w[c] : 1.f, nb = next.in.ln_w ? next.in.ln_b[c] : 0.f;
    float nadd[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) nadd[r] = next.in.add ? next.in.add[(size_t)(row0 + r) * DIM + c] : 0.f;
    merge_partials<TOK, NR>(part, p0, 0, att);
    if (res_ln) token_row_stats(out.resid, row1, stat_res - row0, row0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // output projection: thread = column, k in order
    float acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.f;
#pragma unroll 2
    for (int k4 = 0; k4 < INNER / 4; ++k4) {
        float w[4];
        float4_t a[NR];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = wt[(4 * k4 + i) * DIM + c];
#pragma unroll
        for (int r = 0; r < NR; ++r) a[r] = reinterpret_cast<const float4_t*>(att)[r * (INNER / 4) + k4];
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[r] = fmaf(a[r][i], w[i], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        float v = acc[r] + ob;
        if (out.resid.x) v += res_ln ? (res[r] - stat_res[r][0]) * stat_res[r][1] * rw + rb : res[r];
        y[r * DIM + c] = v;
        if (blockIdx.x == 0) out.Y[(size_t)(row0 + r) * DIM + c] = v;
    }
    __syncthreads();
    if (next.in.ln_w) {
        lds_row_stats(y, NR, next.in.eps, stat_in);
        __syncthreads();
    }
    if (next.in.ln_w || next.in.add) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            float v = y[r * DIM + c];
            if (next.in.ln_w) v = (v - stat_in[r][0]) * stat_in[r][1] * nw + nb;
            y[r * DIM + c] = v + nadd[r];
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int i = 0; i < COLS / 4; ++i) {
        const TokenColumn following = token_column_prefetch(next, first + 4 * min(i + 1, COLS / 4 - 1), row0, row1);
        token_linear_columns<TOK, NR>(next, first + 4 * i, y, nullptr, nullptr, col, row0);
        col = following;
    }
}
template <int TOK, int COLS>
__global__ __launch_bounds__(256) void token_merge_linear_kernel(const float* __restrict__ part, k::TokenLinear out,
                                                                 const float* __restrict__ out_wt, k::TokenLinear next, int P) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    token_merge_linear_body<TOK, TOK, COLS>(part, out, out_wt, next, blockIdx.y, lds);
}

// ---------------------------------------------------------------------------------------------
// Hyper-network MLPs + IoU head.  grid (P, 5): y = 0..3 mask token MLPs (-> 32), y = 4 IoU head (-> 4).
// One wave per output neuron at a time: the 64 lanes read one 1-KB weight row with a single 16-byte load each
// (a thread per neuron reads 64 rows per instruction, one line each), multiply with the activations in LDS and fold
// with the DPP wave sum; 16 waves share the 256 neurons of a layer.
constexpr int HEAD_THREADS = 1024;
static_assert(DIM == 64 * 4, "one float4 of the weight row per lane");

template <int N_OUT>
DLIMG_DEVICE void head_layer(const float* x /*LDS*/, const float* __restrict__ w, const float* __restrict__ b, int n_out,
                             bool relu, float* y) {
    constexpr int WAVES = HEAD_THREADS / 64, ROWS = (N_OUT + WAVES - 1) / WAVES;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const float4_t v = reinterpret_cast<const float4_t*>(x)[lane];
    float4_t wr[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {             // every row of this wave is requested before the first is used
        const int n = wave + r * WAVES;
        wr[r] = float4_t{0.f, 0.f, 0.f, 0.f};
        if (n < n_out) wr[r] = reinterpret_cast<const float4_t*>(w + (size_t)n * DIM)[lane];
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int n = wave + r * WAVES;
        const float acc = wave_sum((v[0] * wr[r][0] + v[1] * wr[r][1]) + (v[2] * wr[r][2] + v[3] * wr[r][3]));
        if (lane == 0 && n < n_out) {
            const float out = acc + b[n];
            y[n] = relu ? fmaxf(out, 0.f) : out;
        }
    }
}

// The workgroup first finishes the final token-to-image attention for ITS token (merge of the partials, output projection,
// residual: see merge_partials) and applies norm_final_attn to it.
// HQ (SAM-HQ models): grid row 5 does the same for the HQ token, row TOK - 1, with SAM-HQ's MLP, and writes hyper_hq [P][32].
struct HeadWeightsHq : k::HeadWeights { k::HqHead hq; };
template <int TOK /*rows per prompt*/, bool HQ = false>
__global__ __launch_bounds__(HEAD_THREADS) void output_heads_kernel(const float* __restrict__ part, k::TokenLinear out,
                                                                    const float* __restrict__ out_wt, k::TokenRows norm,
                                                                    std::conditional_t<HQ, HeadWeightsHq, k::HeadWeights> hw,
                                                                    float* __restrict__ hyper, float* __restrict__ iou) {
    __shared__ __attribute__((aligned(16))) float x0[DIM], x1[DIM], x2[DIM], att[INNER];
    __shared__ float opart[4][DIM];
    __shared__ float2_t stat[1], stat_res[1];
    const int p = blockIdx.x, mi = blockIdx.y;
    const int tok = mi < 4 ? 1 + mi : (HQ && mi == 5 ? TOK - 1 : 0);
    const int row = p * TOK + tok;
    // one round trip: this thread's 32 weights of the output projection (column c, k quarter kq), the partials, the residual
    const int c = threadIdx.x & (DIM - 1), kq = threadIdx.x >> 8;
    float w[INNER / 4];
#pragma unroll
    for (int k = 0; k < INNER / 4; ++k) w[k] = out_wt[(size_t)(kq * (INNER / 4) + k) * DIM + c];
    float res = 0.f, rw = 1.f, rb = 0.f;
    if (out.resid.x && kq == 0) {
        res = out.resid.x[(size_t)row * DIM + c];
        if (out.resid.ln_w) { rw = out.resid.ln_w[c]; rb = out.resid.ln_b[c]; }
    }
    const float ob = (out.b && kq == 0) ? out.b[c] : 0.f;
    if (threadIdx.x < INNER) merge_partials_one(part, p, tok, TOK, att);
    if (out.resid.x && out.resid.ln_w && (threadIdx.x >> 6) == 15) {       // statistics of the residual row: the last wave
        const int lane = lane_id();
        const float4_t v = reinterpret_cast<const float4_t*>(out.resid.x + (size_t)row * DIM)[lane];
        const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / DIM);
        const float4_t d = v - mean;
        const float var = wave_sum((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) * (1.0f / DIM);
        if (lane == 0) stat_res[0] = float2_t{mean, 1.0f / sqrtf(var + out.resid.eps)};
    }
    __syncthreads();
    {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < INNER / 4; ++k) acc = fmaf(att[kq * (INNER / 4) + k], w[k], acc);
        opart[kq][c] = acc;
    }
    __syncthreads();
    if (kq == 0) {
        float v = ((opart[0][c] + opart[1][c]) + (opart[2][c] + opart[3][c])) + ob;
        if (out.resid.x) v += out.resid.ln_w ? (res - stat_res[0][0]) * stat_res[0][1] * rw + rb : res;
        x1[c] = v;
    }
    __syncthreads();
    // the token after norm_final_attn: statistics of its row by wave 0, normalised while it is staged
    if (threadIdx.x < 64) lds_row_stats(x1, 1, norm.eps, stat);
    __syncthreads();
    if (threadIdx.x < DIM)
        x0[threadIdx.x] = (x1[threadIdx.x] - stat[0][0]) * stat[0][1] * norm.ln_w[threadIdx.x] + norm.ln_b[threadIdx.x];
    __syncthreads();
    if constexpr (HQ) {
        if (mi == 5) {
            head_layer<DIM>(x0, hw.hq.w[0], hw.hq.b[0], DIM, true, x1);
            __syncthreads();
            head_layer<DIM>(x1, hw.hq.w[1], hw.hq.b[1], DIM, true, x2);
            __syncthreads();
            head_layer<32>(x2, hw.hq.w[2], hw.hq.b[2], 32, false, hw.hq.hyper_hq + (size_t)p * 32);
            return;
        }
    }
    head_layer<DIM>(x0, hw.w[mi][0], hw.b[mi][0], DIM, true, x1);
    __syncthreads();
    head_layer<DIM>(x1, hw.w[mi][1], hw.b[mi][1], DIM, true, x2);
    __syncthreads();
    float* dst = mi < 4 ? hyper + ((size_t)p * 4 + mi) * 32 : iou + (size_t)p * 4;
    head_layer<32>(x2, hw.w[mi][2], hw.b[mi][2], mi < 4 ? 32 : 4, false, dst);
}

// ---------------------------------------------------------------------------------------------
// Image side, start of a decode: keys = embedding + no_mask_embed (has_mask_input == 0, segmentation.cpp:43-45) as fp32
// and f16 (the A operand of the image-side projections), for all prompts.
// One launch starts a decode: workgroups 0 .. P-1 write the prompts' tokens (the positional part every later step adds),
// the next `lin_blocks` apply the first linears of the token side (q / k / v of the first self-attention) to those same
// rows, which they rebuild in LDS instead of waiting for them, and the rest initialise the keys.  The three have nothing
// to do with each other except that all are the first step of their chain -- and every launch of the decoder costs its
// 5-9 us of dependent latency.  The prompts travel as kernel arguments: no host-to-device copy in front of a decode.
// They travel at the size of the launch's own token count (k::DecoderPrompts holds the largest): a two-point launch carries
// the 512 bytes it always did.
// Up to 8 token rows the arrays hold kDecoderMaxPrompts prompts, as they always did; from 9 on the prompts one launch of that
// count can hold (decoder_max_prompts: 12 at 9 rows, 7 at 15), so the block stays under 1 KB at every count.
template <int TOK>
struct StartPrompts {
    static constexpr int NPTS = TOK - OUT_TOK;
    static constexpr int MAXP = TOK <= 8 ? k::kDecoderMaxPrompts : k::decoder_max_prompts(TOK);
    float coords[MAXP * NPTS * 2];
    float labels[MAXP * NPTS];
    const float* emb[MAXP];
};
template <int TOK>
struct DecoderStart {
    StartPrompts<TOK> prompts;
    const float* gauss; const float* point_embed; const float* not_a_point; const float* iou_token; const float* mask_tokens;
    float* tokens;
    LinJob first;
    int lin_blocks, lin_cols;
    const float* no_mask; float* keys; half_t* keys_h; size_t n4_per_prompt; int P;
};
// kernel arguments are limited to 4 KB; the largest prompt block is the one of 14 token rows (8 prompts x 9 points, 928 bytes)
static_assert(sizeof(DecoderStart<7>) <= 2048 && sizeof(DecoderStart<8>) <= 2048 && sizeof(DecoderStart<9>) <= 2048 &&
              sizeof(DecoderStart<10>) <= 2048 && sizeof(DecoderStart<11>) <= 2048 && sizeof(DecoderStart<12>) <= 2048 &&
              sizeof(DecoderStart<13>) <= 2048 && sizeof(DecoderStart<14>) <= 2048 && sizeof(DecoderStart<15>) <= 2048,
              "the prompts travel as kernel arguments");
// A masked launch (SAM's mask_input: the previous step's low-res logits through the prompt encoder's mask branch,
// mask_embed_kernel below) initialises the keys as  emb + proj.b + h[token] . proj.w  instead of  emb + no_mask : the dense
// embedding SAM adds to the image embedding is the last 1x1 convolution of the branch (16 -> 256), applied here to the 16
// values of the token, so it never exists as a [4096][256] tensor.  Same single f16 rounding of the sum as the unmasked
// form.  MASKED is a template parameter: the unmasked instantiations take DecoderStart<TOK> and keep their code; a launch
// never mixes masked and unmasked prompts.
constexpr int MASK_HID = k::kMaskHidden;
template <int TOK>
struct DecoderStartMasked : DecoderStart<TOK> {
    const float* h[StartPrompts<TOK>::MAXP];     // per prompt: [4096][16] fp32
    const float* proj_w;                         // [256][16]
    const float* proj_b;                         // [256]
};
static_assert(sizeof(DecoderStartMasked<7>) <= 2560 && sizeof(DecoderStartMasked<8>) <= 2560 && sizeof(DecoderStartMasked<9>) <= 2560 &&
              sizeof(DecoderStartMasked<10>) <= 2560 && sizeof(DecoderStartMasked<11>) <= 2560 && sizeof(DecoderStartMasked<12>) <= 2560 &&
              sizeof(DecoderStartMasked<13>) <= 2560 && sizeof(DecoderStartMasked<14>) <= 2560 && sizeof(DecoderStartMasked<15>) <= 2560,
              "the prompts travel as kernel arguments");
// HQ (SAM-HQ models) is a template parameter like MASKED: the other instantiations keep their arguments and their code.
template <typename Base> struct WithHqToken : Base { const float* hq_token; };
template <int TOK, bool MASKED, bool HQ = false>
using DecoderStartArgs = std::conditional_t<HQ, WithHqToken<std::conditional_t<MASKED, DecoderStartMasked<TOK>, DecoderStart<TOK>>>,
                                            std::conditional_t<MASKED, DecoderStartMasked<TOK>, DecoderStart<TOK>>>;
static_assert(sizeof(WithHqToken<DecoderStartMasked<15>>) <= 2568 && sizeof(WithHqToken<DecoderStartMasked<8>>) <= 2568,
              "the prompts travel as kernel arguments");

template <int TOK, bool MASKED = false, bool HQ = false>
__global__ __launch_bounds__(256) void decoder_start_kernel(DecoderStartArgs<TOK, MASKED, HQ> a) {
    __shared__ __attribute__((aligned(16))) float rows[TL_ROW_SLICE<TOK> * DIM];
    const int c = threadIdx.x;
    if ((int)blockIdx.x < a.P) {
        float v[TOK];
        if constexpr (HQ)
            prompt_token_column<TOK, true>(a.prompts, blockIdx.x, c, a.gauss, a.point_embed, a.not_a_point, a.iou_token, a.mask_tokens, v,
                                           a.hq_token);
        else
        prompt_token_column<TOK>(a.prompts, blockIdx.x, c, a.gauss, a.point_embed, a.not_a_point, a.iou_token, a.mask_tokens, v);
#pragma unroll
        for (int t = 0; t < TOK; ++t) a.tokens[((size_t)blockIdx.x * TOK + t) * DIM + c] = v[t];
        return;
    }
    if ((int)blockIdx.x < a.P + a.lin_blocks) {
        const int bid = blockIdx.x - a.P;
        int o = 0, first = (bid % a.lin_cols) * 4;
        while (o + 1 < a.first.count && first >= a.first.op[o].N) { first -= a.first.op[o].N; ++o; }
        const k::TokenLinear& op = a.first.op[o];
        const int row0 = (bid / a.lin_cols) * TL_ROW_SLICE<TOK>, row1 = min(a.first.rows, row0 + TL_ROW_SLICE<TOK>);
        const TokenColumn w_first = token_column_prefetch(op, first, row0, row1);
        for (int p = row0 / TOK; p * TOK < row1; ++p) {
            float v[TOK];
            if constexpr (HQ)
                prompt_token_column<TOK, true>(a.prompts, p, c, a.gauss, a.point_embed, a.not_a_point, a.iou_token, a.mask_tokens, v,
                                               a.hq_token);
            else
            prompt_token_column<TOK>(a.prompts, p, c, a.gauss, a.point_embed, a.not_a_point, a.iou_token, a.mask_tokens, v);
#pragma unroll
            for (int t = 0; t < TOK; ++t) rows[(p * TOK + t - row0) * DIM + c] = v[t];
        }
        __syncthreads();
        DLIMG_FOR_SLICE_ROWS(row1 - row0, token_linear_columns<TOK, NR>(op, first, rows, nullptr, nullptr, w_first, row0);)
        return;
    }
    const float* __restrict__ no_mask = a.no_mask;
    float* __restrict__ keys = a.keys;
    half_t* __restrict__ keys_h = a.keys_h;
    const size_t n4_per_prompt = a.n4_per_prompt;
    const int P = a.P, skip = a.P + a.lin_blocks;
    const size_t total = n4_per_prompt * P;
    const size_t nblk = gridDim.x - skip;
    if constexpr (MASKED) {
        // element i is columns 4 (i % 64) .. + 3 of token (i / 64) % 4096; the stride of the loop and n4_per_prompt are
        // multiples of 64, so a thread keeps its four columns -- and their 4 x 16 weights -- for all of its elements
        const int c4 = threadIdx.x & (DIM / 4 - 1);
        float4_t w[4][MASK_HID / 4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < MASK_HID / 4; ++q)
                w[e][q] = reinterpret_cast<const float4_t*>(a.proj_w)[(c4 * 4 + e) * (MASK_HID / 4) + q];
        const float4_t bias = reinterpret_cast<const float4_t*>(a.proj_b)[c4];
        for (size_t i = (blockIdx.x - skip) * (size_t)blockDim.x + threadIdx.x; i < total; i += nblk * blockDim.x) {
            const size_t p = i / n4_per_prompt, j = i % n4_per_prompt;
            const float4_t* __restrict__ hrow = reinterpret_cast<const float4_t*>(a.h[p]) + (j / (DIM / 4)) * (MASK_HID / 4);
            float4_t d = bias;
#pragma unroll
            for (int q = 0; q < MASK_HID / 4; ++q) {
                const float4_t hv = hrow[q];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    d[e] = fmaf(hv[0], w[e][q][0], fmaf(hv[1], w[e][q][1], fmaf(hv[2], w[e][q][2], fmaf(hv[3], w[e][q][3], d[e]))));
            }
            const float4_t v = reinterpret_cast<const float4_t*>(a.prompts.emb[p])[j] + d;
            reinterpret_cast<float4_t*>(keys)[i] = v;
            reinterpret_cast<half4_t*>(keys_h)[i] = half4_t{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
        }
        return;
    }
    for (size_t i = (blockIdx.x - skip) * (size_t)blockDim.x + threadIdx.x; i < total; i += nblk * blockDim.x) {
        const size_t p = i / n4_per_prompt, j = i % n4_per_prompt;
        float4_t v = reinterpret_cast<const float4_t*>(a.prompts.emb[p])[j];
        v += reinterpret_cast<const float4_t*>(no_mask)[j % (DIM / 4)];
        reinterpret_cast<float4_t*>(keys)[i] = v;
        reinterpret_cast<half4_t*>(keys_h)[i] = half4_t{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
    }
}

// ---------------------------------------------------------------------------------------------
// The prompt encoder's mask branch up to its last convolution (SAM: mask_downscaling[0..5]): low-res logits [256][256] ->
// conv 2x2 / 2 (1 -> 4) -> LayerNorm2d -> GELU -> conv 2x2 / 2 (4 -> 16) -> LayerNorm2d -> GELU, one value set h[token][16]
// per token of the 64 x 64 grid.  The last convolution (1x1, 16 -> 256) is applied by the masked decoder_start_kernel.
// One thread per token, 16 workgroups of 256 per prompt: a token's receptive field is its own 4 x 4 block of logits, read as
// four aligned 16-byte loads; the 332 weights go through LDS (broadcast reads); everything else lives in registers.  The
// plane is chosen here from the IoU predictions with post-processing's rule (postprocess.hip), so the logits are read
// where the decode left them.  fp32 throughout, exact (erf) GELU.
struct MaskEmbedArgs {
    k::MaskSource src[k::kDecoderMaxPrompts];
    k::MaskBranch w;
    float* h;                                    // [P][4096][16]
};
constexpr int ME_W1 = 0, ME_B1 = 16, ME_G1 = 20, ME_H1 = 24, ME_W2 = 28, ME_B2 = ME_W2 + 256, ME_G2 = ME_B2 + 16, ME_H2 = ME_G2 + 16,
              ME_WEIGHTS = ME_H2 + 16;
__global__ __launch_bounds__(256) void mask_embed_kernel(MaskEmbedArgs a) {
    __shared__ __attribute__((aligned(16))) float w[ME_WEIGHTS];
    {
        const int t = threadIdx.x;
        w[ME_W2 + t] = a.w.w2[t];
        if (t < 16) {
            w[ME_W1 + t] = a.w.w1[t];
            w[ME_B2 + t] = a.w.b2[t];
            w[ME_G2 + t] = a.w.ln2_w[t];
            w[ME_H2 + t] = a.w.ln2_b[t];
        }
        if (t < 4) {
            w[ME_B1 + t] = a.w.b1[t];
            w[ME_G1 + t] = a.w.ln1_w[t];
            w[ME_H1 + t] = a.w.ln1_b[t];
        }
    }
    const int p = blockIdx.y;
    const k::MaskSource src = a.src[p];
    const float* low = src.logits4;
    if (src.iou4) {
        // SamOnnxModel.select_masks with two prompt points, as postprocess_kernel chooses
        float best = __fadd_rn(src.iou4[0], __fmul_rn(-0.5f, 1000.0f));
        int bi = 0;
#pragma unroll
        for (int i = 1; i < 4; ++i)
            if (src.iou4[i] > best) { best = src.iou4[i]; bi = i; }
        low += (size_t)bi * 256 * 256;
    }
    const int token = blockIdx.x * 256 + threadIdx.x;            // 16 x 256 = 4096: no tail
    const int ty = token >> 6, tx = token & 63;
    float4_t rows[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) rows[r] = *reinterpret_cast<const float4_t*>(low + (size_t)(4 * ty + r) * 256 + 4 * tx);
    __syncthreads();
    float acc[MASK_HID];
#pragma unroll
    for (int o = 0; o < MASK_HID; ++o) acc[o] = w[ME_B2 + o];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            // first convolution at (2 ty + dy, 2 tx + dx): the 2 x 2 logits at rows 2 dy, 2 dy + 1, columns 2 dx, 2 dx + 1
            const float x00 = rows[2 * dy][2 * dx], x01 = rows[2 * dy][2 * dx + 1], x10 = rows[2 * dy + 1][2 * dx],
                        x11 = rows[2 * dy + 1][2 * dx + 1];
            float y[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                y[c] = fmaf(x00, w[ME_W1 + 4 * c], fmaf(x01, w[ME_W1 + 4 * c + 1], fmaf(x10, w[ME_W1 + 4 * c + 2],
                       fmaf(x11, w[ME_W1 + 4 * c + 3], w[ME_B1 + c]))));
            const float mean = ((y[0] + y[1]) + (y[2] + y[3])) * 0.25f;
            float var = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) { y[c] -= mean; var = fmaf(y[c], y[c], var); }
            const float rstd = 1.0f / sqrtf(var * 0.25f + 1e-6f);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float g = gelu_erf(fmaf(y[c] * rstd, w[ME_G1 + c], w[ME_H1 + c]));
#pragma unroll
                for (int o = 0; o < MASK_HID; ++o) acc[o] = fmaf(g, w[ME_W2 + ((o * 4 + c) * 2 + dy) * 2 + dx], acc[o]);
            }
        }
    float mean = 0.f;
#pragma unroll
    for (int o = 0; o < MASK_HID; ++o) mean += acc[o];
    mean *= 1.0f / MASK_HID;
    float var = 0.f;
#pragma unroll
    for (int o = 0; o < MASK_HID; ++o) { acc[o] -= mean; var = fmaf(acc[o], acc[o], var); }
    const float rstd = 1.0f / sqrtf(var * (1.0f / MASK_HID) + 1e-6f);
    float4_t* dst = reinterpret_cast<float4_t*>(a.h + ((size_t)p * NTOK_IMG + token) * MASK_HID);
#pragma unroll
    for (int q = 0; q < MASK_HID / 4; ++q) {
        float4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = gelu_erf(fmaf(acc[4 * q + e] * rstd, w[ME_G2 + 4 * q + e], w[ME_H2 + 4 * q + e]));
        dst[q] = v;
    }
}

}  // namespace

// the body once for each supported token count (k::decoder_tokens_supported)
#define DLIMG_TOKENS_CASE(N, ...) else if (tokens_ == N) { constexpr int TOK = N; __VA_ARGS__ }
#define DLIMG_FOR_TOKENS(T, who, ...)                                        \
    if (const int tokens_ = (T); tokens_ == 7) { constexpr int TOK = 7; __VA_ARGS__ } \
    DLIMG_TOKENS_CASE(8, __VA_ARGS__) DLIMG_TOKENS_CASE(9, __VA_ARGS__) DLIMG_TOKENS_CASE(10, __VA_ARGS__)  \
    DLIMG_TOKENS_CASE(11, __VA_ARGS__) DLIMG_TOKENS_CASE(12, __VA_ARGS__) DLIMG_TOKENS_CASE(13, __VA_ARGS__) \
    DLIMG_TOKENS_CASE(14, __VA_ARGS__) DLIMG_TOKENS_CASE(15, __VA_ARGS__)    \
    else { throw_error(who ": 7 to 15 tokens per prompt"); }
static_assert(k::kDecoderMaxTokens == 15, "DLIMG_FOR_TOKENS names every supported count");

namespace k {

void decoder_start(const DecoderStartInputs& in, int P, int T, hipStream_t s) {
    const DecoderPrompts& prompts = in.prompts;
    const TokenLinear* first = in.first;
    const int n_first = in.n_first;
    const bool masked = in.mask_h || in.mask;
    if (P <= 0) return;
    if (!decoder_tokens_supported(T)) throw_error("decoder_start: 7 to 15 tokens per prompt");
    if (in.hq_token) {
        if (T < 8) throw_error("decoder_start: a SAM-HQ prompt has at least 8 token rows (the HQ token travels as the last one)");
        for (int i = 0; i < P && i < decoder_max_prompts(T); ++i)
            if (prompts.labels[(size_t)i * (T - 5) + (T - 6)] != kDecoderHqLabel)
                throw_error("decoder_start: the last point of a SAM-HQ prompt is the HQ token's pseudo-point");
    }
    if (P > decoder_max_prompts(T) || n_first < 0 || n_first > TL_MAX_OPS) throw_error("decoder_start: too many prompts or layers");
    if (masked) {
        if (!in.mask_h || !in.mask || !in.mask->proj_w || !in.mask->proj_b)
            throw_error("decoder_start: a masked launch needs the mask branch's rows and weights");
        for (int i = 0; i < P; ++i)
            if (!in.mask_h[i]) throw_error("decoder_start: a launch never mixes masked and unmasked prompts");
    }
    const size_t n4 = (size_t)NTOK_IMG * DIM / 4;
    const size_t total = n4 * P;
    const int key_blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    int cols = 0;
    for (int i = 0; i < n_first; ++i) {
        if (first[i].K != DIM || first[i].N <= 0 || first[i].N % 4 || first[i].in.ln_w || first[i].in.add || first[i].resid.x)
            throw_error("decoder_start: the first linears take the plain 256-wide token rows");
        cols += first[i].N / 4;
    }
    // one argument block and one launch for every (TOK, MASKED, HQ): the tags pick the kernel and the fields it has
    auto launch = [&](auto tok_tag, auto masked_tag, auto hq_tag) {
        constexpr int TOK = decltype(tok_tag)::value;
        constexpr bool MASKED = decltype(masked_tag)::value, HQ = decltype(hq_tag)::value;
        static_assert(TL_PROMPT_SLICE<TOK> == decoder_prompt_slice(TOK), "the first linears are cut as the kernel cuts them");
        if constexpr (!HQ || TOK >= 8) {             // a SAM-HQ prompt of 7 token rows was refused above: no such kernel
            DecoderStartArgs<TOK, MASKED, HQ> a{};
            constexpr int NPTS = StartPrompts<TOK>::NPTS;
            std::memcpy(a.prompts.coords, prompts.coords, (size_t)P * NPTS * 2 * sizeof(float));
            std::memcpy(a.prompts.labels, prompts.labels, (size_t)P * NPTS * sizeof(float));
            for (int i = 0; i < P; ++i) a.prompts.emb[i] = prompts.emb[i];
            a.gauss = in.pe.gauss; a.point_embed = in.pe.point_embed; a.not_a_point = in.pe.not_a_point;
            a.iou_token = in.pe.iou_token; a.mask_tokens = in.pe.mask_tokens;
            a.tokens = in.tokens;
            a.first.count = n_first;
            a.first.rows = P * T;
            for (int i = 0; i < n_first; ++i) a.first.op[i] = first[i];
            a.lin_cols = cols > 0 ? cols : 1;
            a.lin_blocks = cols * ((P + decoder_prompt_slice(T) - 1) / decoder_prompt_slice(T));
            a.keys = in.keys; a.keys_h = in.keys_h; a.n4_per_prompt = n4; a.P = P;
            if constexpr (MASKED) {
                for (int i = 0; i < P; ++i) a.h[i] = in.mask_h[i];
                a.proj_w = in.mask->proj_w; a.proj_b = in.mask->proj_b;
            } else {
                a.no_mask = in.no_mask;
            }
            if constexpr (HQ) a.hq_token = in.hq_token;
            hipLaunchKernelGGL((decoder_start_kernel<TOK, MASKED, HQ>), dim3(P + a.lin_blocks + key_blocks), dim3(256), 0, s, a);
        }
    };
    constexpr std::true_type yes;
    constexpr std::false_type no;
    DLIMG_FOR_TOKENS(T, "decoder_start",
        const std::integral_constant<int, TOK> tok;
        if (in.hq_token) masked ? launch(tok, yes, yes) : launch(tok, no, yes);
        else masked ? launch(tok, yes, no) : launch(tok, no, no);)
}

void mask_embed(const MaskSource* src, const MaskBranch& branch, float* h, int P, hipStream_t s) {
    if (P <= 0) return;
    if (P > kDecoderMaxPrompts) throw_error("mask_embed: too many prompts for one launch");
    if (!h || !branch.w1 || !branch.b1 || !branch.ln1_w || !branch.ln1_b || !branch.w2 || !branch.b2 || !branch.ln2_w || !branch.ln2_b)
        throw_error("mask_embed: the model has no mask branch (pe.mask.*)");
    MaskEmbedArgs a{};
    for (int i = 0; i < P; ++i) {
        if (!src[i].logits4 || ((uintptr_t)src[i].logits4 & 15)) throw_error("mask_embed: every prompt needs 16-byte aligned logits");
        a.src[i] = src[i];
    }
    a.w = branch;
    a.h = h;
    hipLaunchKernelGGL(mask_embed_kernel, dim3(NTOK_IMG / 256, P), dim3(256), 0, s, a);
}

size_t token_to_image_scratch_floats(int P, int T) { return (size_t)P * HEADS * T * T2I_PARTS * 18; }

void token_linears(const TokenLinear* ops, int count, int rows, int T, hipStream_t s) {
    if (count <= 0 || rows <= 0) return;
    if (!decoder_tokens_supported(T) || rows % T) throw_error("token_linears: whole prompts of 7 to 15 token rows");
    if (count > TL_MAX_OPS || rows > TL_MAX_ROWS) throw_error("token_linears: too many layers or rows for one launch");
    LinJob job;
    job.count = count;
    job.rows = rows;
    int blocks = 0;
    for (int i = 0; i < count; ++i) {
        if (ops[i].K <= 0 || ops[i].K % 4 || ops[i].N <= 0 || ops[i].N % 4)
            throw_error("token_linears: K and N must be positive multiples of 4");
        if ((ops[i].in.ln_w || ops[i].in.add) && ops[i].K != DIM)
            throw_error("token_linears: on-the-fly LayerNorm / addition needs 256-wide input rows");
        job.op[i] = ops[i];
        blocks += ops[i].N / 4;
    }
    const int row_slice = decoder_prompt_slice(T) * T;
    const int slices = (rows + row_slice - 1) / row_slice;
    if (count == 1 && ops[0].K > DIM && ops[0].K % 256 == 0 && ops[0].K <= TLD_MAX_K && !ops[0].in.ln_w && !ops[0].in.add) {
        const size_t lds = (size_t)std::min(rows, row_slice) * ops[0].K * 4;
        DLIMG_FOR_TOKENS(T, "token_linears",
            static k::LdsOptIn opt_in;          // one per token count
            opt_in.ensure((const void*)token_linear_deep_kernel<TOK>, (size_t)TL_ROW_SLICE<TOK> * TLD_MAX_K * 4,
                          "token_linears: the device refuses the kernel's LDS size");
            hipLaunchKernelGGL(token_linear_deep_kernel<TOK>, dim3(ops[0].N / 4, slices), dim3(256), lds, s, ops[0], rows);)
        return;
    }
    DLIMG_FOR_TOKENS(T, "token_linears", hipLaunchKernelGGL(token_linears_kernel<TOK>, dim3(blocks, slices), dim3(256), 0, s, job);)
}

void token_self_attention_out(const float* q, const float* kx, const float* v, const TokenLinear& out, int P, int T, hipStream_t s) {
    if (P <= 0) return;
    if (!decoder_tokens_supported(T) || P * T > TL_MAX_ROWS || out.K != DIM || out.N % 4)
        throw_error("token_self_attention_out: unsupported shape");
    static_assert(SA_TOKEN_LDS<7> <= 64 * 1024 && SA_TOKEN_LDS<8> <= 64 * 1024 && SA_TOKEN_LDS<kDecoderMaxTokens> <= 64 * 1024,
                  "below the default dynamic-LDS limit: no opt-in needed");
    const int slice = decoder_prompt_slice(T);
    DLIMG_FOR_TOKENS(T, "token_self_attention_out",
        hipLaunchKernelGGL(token_self_attn_out_kernel<TOK>, dim3(out.N / 4, (P + slice - 1) / slice), dim3(256),
                           SA_TOKEN_LDS<TOK>, s, q, kx, v, out, P);)
}

bool token_self_attention_out_with_gemm(const float* q, const float* kx, const float* v, const TokenLinear& out, int P, int T,
                                        const GemmArgs& g, hipStream_t s) {
    if (P <= 0) return true;
    if (!decoder_tokens_supported(T) || P * T > TL_MAX_ROWS || out.K != DIM || out.N % 4)
        throw_error("token_self_attention_out: unsupported shape");
    // what the 64 x 64 plain tile computes, and nothing else: otherwise the caller launches the two on their own
    if (const char* err = gemm_check(g)) throw_error(err);
    const bool plain = !g.out_l && !g.resid_h && !g.ln_stats && !g.stats_out && g.act == ACT_NONE && g.M % SAG_BM == 0 &&
                       g.N % SAG_BN == 0 && g.K % 64 == 0 && !(g.resid && g.resid_mod % SAG_BM != 0);
    if (!plain) return false;
    const int tiles = (g.M / SAG_BM) * (g.N / SAG_BN);
    const int slice = decoder_prompt_slice(T);
    const int bx = out.N / 4, by = (P + slice - 1) / slice;
    // the tiles sit behind the self-attention's workgroups and find their XCD by their own index (xcd_remap): that is the
    // XCD the hardware gave them only if a multiple of 8 workgroups stands in front
    if ((bx * by) % 8) return false;
    DLIMG_FOR_TOKENS(T, "token_self_attention_out",
        hipLaunchKernelGGL(self_attn_out_and_gemm_kernel<TOK>, dim3(tiles + bx * by), dim3(256), SAG_LDS<TOK>, s, g, tiles, q, kx, v,
                           out, P, bx);)
    return true;
}

void token_merge_linear(const float* scratch, const TokenLinear& out, const float* out_wt, const TokenLinear& next, int P,
                        int T, hipStream_t s) {
    if (P <= 0) return;
    if (!decoder_tokens_supported(T) || P * T > TL_MAX_ROWS || out.K != INNER || out.N != DIM || out.resid.add || next.K != DIM ||
        next.N % 64 || next.resid.x)
        throw_error("token_merge_linear: unsupported shape");
    auto launch = [&](auto tok_tag, auto cols_tag) {
        constexpr int TOK = decltype(tok_tag)::value, COLS = decltype(cols_tag)::value;
        static k::LdsOptIn opt_in;          // one per instantiation of this lambda's call operator: per (TOK, COLS)
        opt_in.ensure((const void*)token_merge_linear_kernel<TOK, COLS>, TML_LDS<TOK>, "token_merge_linear: the device refuses the kernel's LDS size");
        hipLaunchKernelGGL((token_merge_linear_kernel<TOK, COLS>), dim3(next.N / COLS, P), dim3(256), TML_LDS<TOK>, s, scratch, out, out_wt,
                           next, P);
    };
    // the smallest workgroups that still fit the chip in one round (256 CUs, one workgroup each: 150 KB of LDS)
    DLIMG_FOR_TOKENS(T, "token_merge_linear",
        const std::integral_constant<int, TOK> tok;
        if ((next.N / 16) * P <= 256) launch(tok, std::integral_constant<int, 16>{});
        else if ((next.N / 32) * P <= 256) launch(tok, std::integral_constant<int, 32>{});
        else launch(tok, std::integral_constant<int, 64>{});)
}

void token_to_image_partials(const float* q, const TokenLinear* q_proj, const half_t* K, int ldk, const half_t* V, int ldv,
                             float* scratch, int P, int T, hipStream_t s) {
    if (P <= 0) return;
    if (ldk % 8 || ldv % 8 || (((uintptr_t)K | (uintptr_t)V) & 15))
        throw_error("token_to_image_attention: K/V rows must be 16-byte aligned");
    TokenLinear qp{};
    if (q_proj) {
        if (q_proj->K != DIM || q_proj->N != INNER || q_proj->resid.x || q_proj->relu)
            throw_error("token_to_image_attention: the query projection is 256 -> 128 without residual");
        qp = *q_proj;
    } else if (!q) {
        throw_error("token_to_image_attention: neither queries nor their projection given");
    }
    DLIMG_FOR_TOKENS(T, "token_to_image_attention",
        hipLaunchKernelGGL(token_to_image_partial_kernel<TOK>, dim3(P * HEADS * T2I_GROUPS), dim3(T2I_THREADS), 0, s, q, qp, K, ldk, V,
                           ldv, scratch);)
}

void output_heads(const float* scratch, const TokenLinear& out, const float* out_wt, const TokenRows& norm,
                  const HeadWeights& hw, float* hyper, float* iou, int P, int T, hipStream_t s, const HqHead* hq) {
    if (P <= 0) return;
    if (out.K != INNER || out.N != DIM || !norm.ln_w) throw_error("output_heads: unsupported shape");
    if (hq) {
        if (T < 8 || !hq->hyper_hq || !hq->w[0] || !hq->w[1] || !hq->w[2] || !hq->b[0] || !hq->b[1] || !hq->b[2] ||
            (((uintptr_t)hq->w[0] | (uintptr_t)hq->w[1] | (uintptr_t)hq->w[2]) & 15))
            throw_error("output_heads: the SAM-HQ head needs its MLP, its output and a prompt of at least 8 token rows");
        HeadWeightsHq hwq;
        static_cast<HeadWeights&>(hwq) = hw;
        hwq.hq = *hq;
        DLIMG_FOR_TOKENS(T, "output_heads",
            hipLaunchKernelGGL((output_heads_kernel<TOK, true>), dim3(P, 6), dim3(HEAD_THREADS), 0, s, scratch, out, out_wt, norm, hwq, hyper, iou);)
        return;
    }
    DLIMG_FOR_TOKENS(T, "output_heads",
        hipLaunchKernelGGL(output_heads_kernel<TOK>, dim3(P, 5), dim3(HEAD_THREADS), 0, s, scratch, out, out_wt, norm, hw, hyper, iou);)
}

}  // namespace k
}  // namespace dlimg
