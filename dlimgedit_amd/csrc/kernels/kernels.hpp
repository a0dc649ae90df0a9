// Host-callable launchers of the gfx950 kernels.  All pointers are device pointers unless noted;
// every launcher validates the shapes its grid assumes and throws dlimg::Exception on mismatch
// (a faulting kernel can take the whole node down, so nothing is launched on unchecked shapes).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dlimg {

typedef _Float16 half_t;

[[noreturn]] void throw_error(const char* msg);   // defined in common.cpp

namespace k {

// Opt-in of one kernel to more than 64 KB of dynamic LDS.  hipFuncAttributeMaxDynamicSharedMemorySize belongs to the
// function ON THE CURRENT DEVICE, and an environment may hold one replica per GPU (DLIMGEDIT_DEVICES), so the state is
// kept per device: the first launcher on each GPU sets the attribute, every later one only reads the outcome.  A refused
// opt-in is remembered and reported by every caller (launching anyway would fail with an invalid-configuration error
// or, worse, run with less LDS than the kernel addresses).  One static instance per kernel at its launch site.
class LdsOptIn {
  public:
    static constexpr int kMaxDevices = 64;
    void ensure(const void* kernel, size_t bytes, const char* refused_message) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) throw_error("kernel launch: no current HIP device");
        int st = __atomic_load_n(&state_[dev], __ATOMIC_ACQUIRE);
        if (st == 0) {
            // several lanes may arrive together: setting the same value twice is harmless, the outcome is the same
            st = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess ? 1 : -1;
            if (st < 0) (void)hipGetLastError();
            __atomic_store_n(&state_[dev], st, __ATOMIC_RELEASE);
        }
        if (st < 0) throw_error(refused_message);
    }

  private:
    int state_[kMaxDevices] = {};        // 0 = not tried on this device, 1 = granted, -1 = refused
};

enum Act { ACT_NONE = 0, ACT_GELU = 1 };

// ---- GEMM ------------------------------------------------------------------------------------
struct GemmArgs {
    const half_t* A = nullptr;  int lda = 0;     // [M,K] row-major f16
    const half_t* W = nullptr;  int ldw = 0;     // [N,K] row-major f16 (nn.Linear layout)
    const float* bias = nullptr;                 // [N] or null
    const float* resid = nullptr; int ldr = 0; int resid_mod = 1;   // added after activation: resid[m % resid_mod][n]
    float* out_f32 = nullptr;   int ldc32 = 0;
    half_t* out_h = nullptr;    int ldc16 = 0;
    // The residual stream as an f16 PAIR (r04): value = hi + lo, hi = f16(value) -- which is also the A operand of the GEMM
    // that consumes the stream -- and lo = f16(value - hi): 22 significant bits in 4 bytes.  A stream writer then moves 8 bytes
    // per element (pair in, pair out) instead of 10 (fp32 in, fp32 + f16 copy out).  resid_h / resid_l: the residual as a
    // pair (instead of `resid`; rows m % resid_mod, leading dimension ldrs); out_l with out_h: the result as a pair (instead
    // of out_f32; both with leading dimension ldc16).  Ping-pong tiles (9, 10, 11) only.
    const half_t* resid_h = nullptr; const half_t* resid_l = nullptr; int ldrs = 0;
    half_t* out_l = nullptr;
    int M = 0, N = 0, K = 0;
    int act = ACT_NONE;
    // LayerNorm folded into the GEMMs around it (gemm.hip).  Producer: stats_out receives, per tile column block and
    // row, the (sum, sum of squared deviations) of the fp32 result -- [N / BN][M][2] (BN from gemm_choose_tile).  Consumer: A is
    // the raw, un-normalised input, W carries the LayerNorm scale (W * diag(gamma)), bias carries b + W.beta; ln_stats
    // are the producer's partials ([ln_groups][M][2], groups of K / ln_groups columns) and the epilogue applies
    // rstd_m * (acc - mean_m * ln_colsum[n]) + bias[n].
    float* stats_out = nullptr;
    const float* ln_stats = nullptr;
    int ln_groups = 0;
    const float* ln_colsum = nullptr;            // [N] sum over k of the (f16-rounded) scaled weight
    float ln_eps = 0.f;
    // Tile selection.  shared_gpu: kernels of several execution lanes share the device (prefer tiles that can share a
    // CU).  tile: -1 = let gemm() choose; gemm_choose_tile() fixes the choice in the arguments so that a caller who
    // needs the tile width beforehand (stats_out layout) and the launch agree by construction.
    bool shared_gpu = false;
    // alone: the pass this GEMM belongs to has the GPU to itself (no other lane has work in flight: a synchronous caller).
    // A one-image launch may then use tiles that double its workgroups at a worse cost per FLOP (gemm_plan.hpp, tile 11);
    // the bits do not depend on it.
    bool alone = false;
    int tile = -1;
    // Rows of ONE independent unit (an image: 4096 tokens) when M stacks several of them.  The tile is chosen for the
    // unit's shape, so a batch runs the same tiles -- and produces the same bits -- as its images one at a time.
    int unit_rows = 0;
    // Diagnostics (tuning builds of the benchmark hook only; null in the product): per workgroup 4 x u64 =
    // { shader cycles, 100 MHz ticks } of the main loop and of the whole kernel, written by wave 0.
    unsigned long long* stamps = nullptr;
    // The neck launches only (neck_conv1x1_ln / neck_conv3x3_ln below; k::gemm ignores them): LayerNorm2d scale and shift
    // [256] applied in the epilogue (eps in ln_eps), the fp32 result per image (entry i: rows 4096 i .. of the launch, or null),
    // the host-visible non-finite report, and the 128-byte line of zeros the implicit 3x3 operand reads for taps outside
    // the image.
    const float* ln2d_w = nullptr;
    const float* ln2d_b = nullptr;
    float* out_img[8] = {};
    int* nonfinite = nullptr;
    const half_t* zeros = nullptr;
};
const char* gemm_check(const GemmArgs&);
bool gemm_tile_fits(const GemmArgs&, int tile);   // may `tile` (index into k::kGemmTiles, gemm_plan.hpp) run this problem?
int gemm_pick_tile(const GemmArgs&);          // the tile gemm() launches: a.tile if set (-1 unless it fits), else the choice; -1: none fits
int gemm_choose_tile(GemmArgs&);              // sets a.tile; returns BN (columns per tile) of that configuration
// start/stop (both or neither): events attached to the kernel's own dispatch (hipExtLaunchKernelGGL): their elapsed time
// is the kernel's execution time as a profiler reports it, without the marker packets an hipEventRecord pair adds.
void gemm(const GemmArgs&, hipStream_t, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// ---- encoder neck: convolution + LayerNorm2d in one launch -------------------------------------
// Both neck convolutions have 256 output channels, one column tile of the ping-pong kernels, so a whole output row lies in
// one workgroup and LayerNorm2d over the channels is an epilogue: y = gamma (v - mean) rstd + beta with the row statistics of
// the fp32 accumulators.  Fixed 64 x 256 tiles whatever the batch (B * 64 workgroups, no planner): a batch computes the bits of
// its images one at a time.  No bias (the neck's convolutions have none).
struct NeckOutputs {
    half_t* out_h = nullptr;             // [B * 4096][256] f16, or null
    float* const* out_f32 = nullptr;     // HOST array of B device pointers, [4096][256] fp32 per image (null entries: not
                                         // written), or null
    int* nonfinite = nullptr;            // as layernorm(): set to 1 when a row's statistics are not finite
};
// 1x1: in [B * 4096][K] f16 (K a multiple of 64), w [256][K] f16
void neck_conv1x1_ln(const half_t* in, int B, int K, const half_t* w, const float* gamma, const float* beta, float eps,
                     const NeckOutputs& out, hipStream_t, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// 3x3, zero pad 1, over the f16 map in [B][64][64][256]; w [256][9 * 256] f16, column = (ky * 3 + kx) * 256 + c (im2col3x3's
// order).  The A operand is read straight from the map: no im2col matrix.  zeros: 128 bytes of zeros, 16-byte aligned.
void neck_conv3x3_ln(const half_t* in, int B, const half_t* w, const half_t* zeros, const float* gamma, const float* beta,
                     float eps, const NeckOutputs& out, hipStream_t, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// ---- row LayerNorm ---------------------------------------------------------------------------
// y = (x-mean)/sqrt(var+eps)*w+b over rows of length D (<= 1280); optional GELU; f32 and/or f16 out.
// x and out_f32 may alias.  nonfinite (optional; D a multiple of 256 AND x, w, b, out_f32 16-byte, out_h 8-byte aligned, i.e.
// the 16-byte kernel: refused otherwise): an int in memory the kernel can write (pinned host memory) that is set to 1 when a
// row holds an infinity or a NaN; never cleared by the kernel.
void layernorm(const float* x, const float* w, const float* b, float eps, int rows, int D, int act,
               float* out_f32, half_t* out_h, hipStream_t, int* nonfinite = nullptr);

// ---- pixel pre-processing (K1) ---------------------------------------------------------------
// u8 image [h,w,C] (row stride `stride` bytes; dlimg::Channels code `channels`) -> f16 patch-major
// matrix [4096, 768]: row = patch (py*64+px), column = c*256 + iy*16 + ix, value
// (float(u8) - mean[c]) / std[c]; pixels outside h x w (zero padding of the graph) are 0.
void preprocess(const uint8_t* img, int w, int h, int stride, int channels, half_t* patches, hipStream_t);
// the same for several images in one launch (the images of a batched pass)
struct PreImage { const uint8_t* img; int w, h, stride, channels; half_t* patches; };
void preprocess_batch(const PreImage* images, int count, hipStream_t);

// ---- K17 longest-side resize (stb_image_resize equivalent; tables from csrc/resize_tables.cpp) ------------
struct ResizeAxis { const int* first; const int* count; const float* coef; int taps; int out; };   // device pointers
// src u8 [h][stride] with C bytes per pixel -> dst u8 [ay.out][ax.out*C] packed; tmp: fp32 [h][ax.out][C] scratch
void resize_srgb(const uint8_t* src, int w, int h, int stride, int C, const ResizeAxis& ax, const ResizeAxis& ay,
                 const float* decode_lut, const uint32_t* encode_tab, float* tmp, uint8_t* dst, hipStream_t);

// ---- K18 longest-side resize fused with pre-processing, for the images of one pass ---------------------------
// src u8 [h][stride] (dlimg::Channels code `channels`) -> resampled to ax.out x ay.out exactly as resize_srgb does and
// written as preprocess writes it: f16 patch-major [4096, 768] with zero padding outside ax.out x ay.out.  The resampled
// u8 image is never stored.  tmp: fp32 scratch of resize_preprocess_tmp_floats(h, ax.out, channels) floats, 32-byte
// aligned, one area per image.  Two launches for up to 16 images.
struct ResizeJob { const uint8_t* src; int w, h, stride, channels; ResizeAxis ax, ay; float* tmp; half_t* patches; };
size_t resize_preprocess_tmp_floats(int h, int rw, int channels);
void resize_preprocess_batch(const ResizeJob* jobs, int count, const float* decode_lut, const uint32_t* encode_tab,
                             hipStream_t);

// ---- elementwise -----------------------------------------------------------------------------
// out_h[i] = f16(a[i] + (b ? b[i % b_mod] : 0)); out_f32 likewise (either may be null); n % 4 == 0 and, with b, b_mod % 4 == 0
// and b_mod > 0 (refused otherwise); every pointer 16-byte aligned (out_h: 8)
void add_cast(const float* a, const float* b, size_t b_mod, size_t n, float* out_f32, half_t* out_h, hipStream_t);
// 3x3 im2col over a [B,64,64,C] f16 map (zero pad 1): out [B*4096, 9*C], column = (ky*3+kx)*C + c
void im2col3x3(const half_t* in, int B, int C, half_t* out, hipStream_t);
// f32 -> f16 conversion of a weight tensor
void cast_f16(const float* in, half_t* out, size_t n, hipStream_t);

// ---- encoder attention -----------------------------------------------------------------------
// qkv: [B*4096, 3*D] f16 token-major (q | k | v, head-major inside each), out: [B*4096, D] f16.
// qkv_pad: f16 [3*D], the qkv bias (keys / values of a window's zero-padding tokens equal it).
// rel_h/rel_w: f16 [2*S-1, hd] with S = 14 (windowed) or 64 (global); converted once when the weights are loaded.
void attention_window(const half_t* qkv, const half_t* qkv_pad, const half_t* rel_h, const half_t* rel_w,
                      half_t* out, int B, int heads, int hd, hipStream_t);
// attention_global works in units of log2 and leaves the scaling to whoever produces its operands: the q columns of qkv
// must arrive multiplied by attention_global_q_scale(hd) = log2(e) / sqrt(hd) and both rel-pos tables by
// attention_global_rel_scale(hd) = sqrt(hd), so that q'.k is the scaled score and q'.R' the bias q.R, both times
// log2(e).  SamModel folds the factors into the qkv weights / bias and the tables of the global blocks when it loads them.
float attention_global_q_scale(int hd);
float attention_global_rel_scale(int hd);
void attention_global(const half_t* qkv, const half_t* rel_h, const half_t* rel_w, half_t* out, int B,
                      int heads, int hd, hipStream_t);

// ---- mask decoder (token side is tiny: fp32 VALU kernels) ------------------------------------
// Every launcher of the token side takes T, the token rows per prompt: 5 output tokens (iou + 4 mask tokens) + the prompt's
// points, 7 (a point and its pad token, or a box), 8 (a point and a box), up to 15 (8 clicks and a box).  Every count has
// its own instantiation of every kernel, a launch never mixes counts, and one launch holds at most 112 token rows:
// decoder_max_prompts(T) prompts.
constexpr int kDecoderMaxRows = 112;
constexpr int kDecoderMaxPoints = 10;                       // 8 clicks + the two corners of a box
constexpr int kDecoderMaxTokens = 5 + kDecoderMaxPoints;
constexpr bool decoder_tokens_supported(int T) { return T >= 7 && T <= kDecoderMaxTokens; }
constexpr int decoder_max_prompts(int T) { return kDecoderMaxRows / T; }
// prompts per workgroup of the token-side kernels that take whole prompts (their slice of rows is at most 16)
constexpr int decoder_prompt_slice(int T) { return T <= 8 ? 2 : 1; }
// floats of workspace for the per-key-group partial results of token_to_image_partials
size_t token_to_image_scratch_floats(int P, int T);
// A [rows][256] fp32 token matrix as a consumer sees it: optionally LayerNorm'ed (over the 256 columns) and with another
// matrix added behind the LayerNorm (the query positional encoding), both applied while the rows are read.
struct TokenRows {
    const float* x = nullptr;
    const float* ln_w = nullptr;
    const float* ln_b = nullptr;
    float eps = 0.f;
    const float* add = nullptr;
};
// Y[r][n] = act(in[r] . W[n] + b[n]) + resid[r][n]; W is [N][K] fp32.  K = 256: `in` with TokenRows semantics; any other
// K: in.x is a plain [rows][K] matrix.  resid.x == nullptr: no residual.
struct TokenLinear {
    TokenRows in;
    int K = 0;
    const float* W = nullptr;
    const float* b = nullptr;
    TokenRows resid;
    float* Y = nullptr;
    int N = 0;
    int relu = 0;
};
// The prompts of one decode (at most 16 per launch); the part a launch uses travels in the first kernel's arguments.  With
// n = T - 5 points per prompt (2 .. 10): coords [P][n][2] in the 1024-pixel frame, labels [P][n], both tightly packed, and per prompt the DEVICE address
// of its image embedding ([4096][256] fp32).
constexpr int kDecoderMaxPrompts = 16;
struct DecoderPrompts {
    float coords[kDecoderMaxPrompts * kDecoderMaxPoints * 2];
    float labels[kDecoderMaxPrompts * kDecoderMaxPoints];
    const float* emb[kDecoderMaxPrompts];
};
// Mask input (SAM's click-to-refine loop: the low-res logits of the previous step through the prompt encoder's mask branch).
// MaskBranch: the branch's tensors as the model file holds them, fp32 -- conv 2x2 / 2 w1 [4][1][2][2], b1 [4]; LayerNorm2d
// ln1 [4]; conv 2x2 / 2 w2 [16][4][2][2], b2 [16]; LayerNorm2d ln2 [16]; 1x1 conv proj_w [256][16], proj_b [256].
// MaskSource: where one prompt's mask input lies -- the four planes [4][256][256] a decode left and, when the plane is the
// best of 1..3 by the IoU predictions (the single-mask rule of a two-point prompt, chosen on the device), those four
// predictions; iou4 == nullptr: plane 0.
constexpr int kMaskHidden = 16;
struct MaskBranch {
    const float* w1 = nullptr; const float* b1 = nullptr; const float* ln1_w = nullptr; const float* ln1_b = nullptr;
    const float* w2 = nullptr; const float* b2 = nullptr; const float* ln2_w = nullptr; const float* ln2_b = nullptr;
    const float* proj_w = nullptr; const float* proj_b = nullptr;
};
struct MaskSource { const float* logits4; const float* iou4; };
// h[p][token][16] = GELU(LN2d(conv2(GELU(LN2d(conv1(plane of src[p])))))) for P prompts (src: host array): everything of the
// branch but its last convolution.  One launch, 16 workgroups per prompt.
void mask_embed(const MaskSource* src, const MaskBranch& branch, float* h /*[P][4096][16]*/, int P, hipStream_t);
// First launch of a decode.  tokens [P,T,256]: iou token, 4 mask tokens, T - 5 prompt tokens (the positional part later steps
// add); `first` (n_first <= 5 layers, K = 256, no LayerNorm / residual; their `in` is ignored) are applied to those same
// rows in this launch.  Image side, for all prompts: keys = emb[p] + no_mask (fp32 + f16), or -- prompts that all have a
// mask input: mask_h, a host array of P device pointers ([4096][16] each, mask_embed's h), and the branch -- keys = emb[p] +
// proj_b + h[p][token] . proj_w, SAM's dense embedding in no_mask's place.
// hq_token (optional, [256]): the prompts of a SAM-HQ model.  Their LAST point is a pseudo-point that carries SAM-HQ's output
// token: its label is kDecoderHqLabel, a value no caller's label can be, and its token row (row T - 1) is hq_token and nothing
// else -- no Fourier term, no point embedding.  The two-way transformer does not care where a row stands, so the HQ token
// travels as one more trailing row through every token-side kernel unchanged; output_heads reads it back from row T - 1.
constexpr float kDecoderHqLabel = -1024.0f;
struct PromptEncoderWeights {       // pe.gauss, pe.point, pe.not_a_point and the decoder's output tokens
    const float* gauss = nullptr; const float* point_embed = nullptr; const float* not_a_point = nullptr;
    const float* iou_token = nullptr; const float* mask_tokens = nullptr;
};
struct DecoderStartInputs {
    DecoderPrompts prompts{};
    PromptEncoderWeights pe;
    float* tokens = nullptr;
    const TokenLinear* first = nullptr;
    int n_first = 0;
    float* keys = nullptr;
    half_t* keys_h = nullptr;
    const float* no_mask = nullptr;                 // an unmasked launch; else both of:
    const float* const* mask_h = nullptr;
    const MaskBranch* mask = nullptr;
    const float* hq_token = nullptr;
};
void decoder_start(const DecoderStartInputs& in, int P, int T, hipStream_t s);
// up to 5 layers over the same rows (<= 112, whole prompts of T rows) in one launch
void token_linears(const TokenLinear* ops, int count, int rows, int T, hipStream_t);
// self-attention among the T tokens of each prompt + its output projection `out` (K = 256) in one launch
void token_self_attention_out(const float* q, const float* k, const float* v, const TokenLinear& out, int P, int T, hipStream_t);
// The same launch carrying a plain GEMM (no activation, no folded LayerNorm, fp32 bias / residual, f16 or fp32 result) that
// neither depends on it nor it on the GEMM: its 64 x 64 tiles are extra workgroups of the launch (decoder.hip).  Returns false
// without launching anything when `g` is not of that kind, or when the self-attention's workgroups are not a multiple of 8
// (the tiles behind them keep their XCDs only then); the caller then launches both on their own.
bool token_self_attention_out_with_gemm(const float* q, const float* k, const float* v, const TokenLinear& out, int P, int T,
                                        const GemmArgs& g, hipStream_t);
// token-to-image attention.  partials: per key group (max, sum, output) of every (prompt, head, token); the queries
// are q [P,T,128], or are computed in the launch as q_proj (256 -> 128, LayerNorm / positional part on the fly).  The
// fold of the partials + output projection `out` (128 -> 256, out_wt = its weight transposed [128][256]) + residual is
// done by the consumer's launch: token_merge_linear (writes out.Y and applies `next`, a K = 256 layer whose input is
// next.in's LayerNorm of out.Y) or output_heads.
void token_to_image_partials(const float* q, const TokenLinear* q_proj, const half_t* K, int ldk, const half_t* V, int ldv,
                             float* scratch, int P, int T, hipStream_t);
void token_merge_linear(const float* scratch, const TokenLinear& out, const float* out_wt, const TokenLinear& next, int P,
                        int T, hipStream_t);
// The image positions' half of a two-way block in one launch (kernels/decoder_image.hip):
// keys <- LayerNorm(keys + attention(q -> token k / v) Wo + bias), fp32 in place + f16 copy.  q: f16 [P*4096][ldq] (128 wide),
// tk / tv: fp32 [P][T][128], W: f16 [256][128].
void image_update(const half_t* q, int ldq, const float* tk, const float* tv, const half_t* W, const float* bias,
                  const float* ln_w, const float* ln_b, float eps, float* keys, half_t* keys_h, int P, int T, hipStream_t);
// Up-scaling path + mask product in one launch (kernels/decoder_image.hip): logits [P,4,256,256] from the f16 keys, the two
// transposed convolutions as GEMM weights (W1 [256][256], rows = sub-pixel * 64 + channel; W2 [128][64], rows = sub-pixel * 32
// + channel), the LayerNorm2d between them and the hyper vectors [P,4,32].
// u_out (optional, SAM-HQ models): the up-scaled embedding itself, [P][256][256][32] f16 in raster order, for hq_mask_path:
// each value is the f16 rounding of the fp32 value the mask product is taken with (the product itself never sees the
// rounding, and the logits are the same bits with and without u_out).
void upscale_logits(const half_t* keys_h, const half_t* W1, const float* b1, const float* ln_w, const float* ln_b, float eps,
                    const half_t* W2, const float* b2, const float* hyper, float* logits, int P, hipStream_t, half_t* u_out = nullptr);
// hyper-network MLPs (4 x 256->256->256->32) and IoU head (256->256->256->4) on the output tokens: the launch finishes the
// final token-to-image attention (scratch, out, out_wt as above) for the five tokens it needs (rows 0..4 of each prompt's
// T) and applies `norm` to them
struct HeadWeights { const float* w[5][3]; const float* b[5][3]; };
// hq (optional, SAM-HQ models): one more workgroup per prompt does the same for row T - 1, the HQ token, runs SAM-HQ's MLP
// (256->256->256->32) on it and writes hyper_hq [P,32].
struct HqHead { const float* w[3]; const float* b[3]; float* hyper_hq; };
void output_heads(const float* scratch, const TokenLinear& out, const float* out_wt, const TokenRows& norm /*ln_w, ln_b, eps*/,
                  const HeadWeights& hw, float* hyper /*[P,4,32]*/, float* iou /*[P,4]*/, int P, int T, hipStream_t,
                  const HqHead* hq = nullptr);

// ---- SAM-HQ (kernels/decoder_hq.hip) ---------------------------------------------------------
// Per image: hq_features [256][256][32] fp32 in raster order = the two branches' second transposed convolutions (GEMM results
// [4096 * 4][128], row = token * 4 + first sub-pixel, column = second sub-pixel * 32 + channel, without bias) + both biases.
void hq_features_finish(const float* vit, const float* emb, const float* b_vit, const float* b_emb, float* out, hipStream_t);
// Per prompt: logits[p][m] += hyper_hq[p] . (conv2_3x3(GELU(LN2d(conv1_3x3(U[p])))) + features[p]) for the four planes m.
// U: [P][256][256][32] f16 (upscale_logits' u_out); H: workspace [P][256][256][64] f16; features: host array of P device
// pointers; conv1_w [9][64][32] and conv2_w [9][32][64] f16, tap-major (tap = ky * 3 + kx), then output, then input channel.
struct HqMaskWeights {
    const half_t* conv1_w = nullptr; const float* conv1_b = nullptr; const float* ln_w = nullptr; const float* ln_b = nullptr;
    const half_t* conv2_w = nullptr; const float* conv2_b = nullptr;
};
void hq_mask_path(const half_t* U, const HqMaskWeights& w, float eps, half_t* H, const float* const* features,
                  const float* hyper_hq, float* logits, int P, hipStream_t);
// What hq_mask_path refuses for its prompts alone, which it does before anything else: more than kDecoderMaxPrompts prompts, a
// prompt whose entry of `features` is null or not 16-byte aligned.  False: P <= 0, the call does nothing.
bool hq_mask_path_prompts(const float* const* features, int P);

// ---- mask post-processing (K16) --------------------------------------------------------------
// For each of `count` jobs: logits plane job.src (256x256 f32, device) -> two-stage bilinear
// (256->1024, crop to prepadded ph x pw, -> out_h x out_w), threshold > 0 -> 255/0 into job.dst (device, packed rows).
// If job.select_iou != nullptr the plane is chosen on device as argmax over planes 1..3 of
// select_iou[0..3] (SamOnnxModel.select_masks with 2 prompt points) starting from job.src as plane 0.
// BiRefNet pre/post (kernels/objects.hip): channels 0..2 of an HWC u8 image -> normalised f32 planes; logits -> u8
void birefnet_prepare_image(const uint8_t* pixels, int w, int h, int stride, int bytes_pp, const float mean[3],
                            const float std[3], float* out, hipStream_t s);
void birefnet_process_mask(const float* logits, int w, int h, uint8_t* out, hipStream_t s);

struct PostJob { const float* src; const float* select_iou; uint8_t* dst; int out_w, out_h, pre_w, pre_h; };
void postprocess_masks(const PostJob* jobs_host, int count, hipStream_t);

// ---- mask clean-up (K17, kernels/mask_cleanup.hip) --------------------------------------------
// SAM's remove_small_regions on 0 / 255 masks, in place, 8-connectivity for both polarities.  Per job: (1) when max_hole > 0,
// every connected component of the BACKGROUND with area < max_hole becomes foreground; (2) when max_island > 0, on the result
// of (1), every connected component of the FOREGROUND with area < max_island becomes background -- except that when all
// components are below the threshold the largest one stays, among equal largest the one whose first pixel in raster order
// comes first.  Jobs of one call may differ in size.  Refused before anything is launched: a job with both thresholds 0 or
// a negative one, a null mask, an extent that is not positive or whose w * h does not fit an int.  Stream-ordered, no host
// synchronisation: at most four launches per polarity and 16 jobs.  workspace: mask_cleanup_workspace_bytes(jobs, count)
// bytes of device memory (8 per pixel and 8 per job), contents irrelevant before and after.
struct CleanJob { uint8_t* mask; int w, h; int max_hole, max_island; };   // mask: device memory, packed rows, in place
size_t mask_cleanup_workspace_bytes(const CleanJob* jobs, int count);
int mask_cleanup_launches(const CleanJob* jobs, int count);          // kernel launches mask_cleanup makes for these jobs
void mask_cleanup(const CleanJob* jobs_host, int count, void* workspace, hipStream_t);

// ---- label maps of a point grid (K18, kernels/mask_grid.hip) ----------------------------------
// "Segment everything": the candidates of a grid of one-click prompts are planes 1..3 of every prompt, candidate
// c = 3 * prompt + (plane - 1).  grid_harvest scores the candidates of one decode chunk and keeps their planes; the host
// selects (csrc/grid_plan.hpp); grid_paint writes the label map of the kept ones.
//
// A record is 8 int32 (32 bytes), csrc/grid_plan.hpp: GridRecord -- n_hi, n_mid, n_lo: logits > +1, > 0, > -1 (strict) over the
// SCORED region, low-res pixels x < ceil(pre_w / 4), y < ceil(pre_h / 4); x0, y0, x1, y1: the inclusive box of the logits > 0
// there ({0, 0, -1, -1} when there is none); cull: the inclusive box of the logits > 0 over the REACH region, one low-res
// column and row more (x <= min(ceil(pre_w / 4), 255), likewise y), as four bytes x0 | y0 << 8 | x1 << 16 | y1 << 24
// (kGridCullEmpty when there is none).  The reach region is what the taps of the post-processing can read: the pixels at the
// crop's edge sample row / column ceil(pre / 4) when pre mod 4 is 3 or 0, and never anything beyond it, so a pixel whose taps
// miss the cull box cannot be positive (its sample is a combination of non-positive logits with weights >= 0).
constexpr int kGridMaxKept = 255;
constexpr int kGridRecordInts = 8;
constexpr uint32_t kGridCullEmpty = 0x0000ffffu;
constexpr size_t kGridPlaneFloats = 256 * 256;
// logits [P][4][256][256] as a decode leaves them -> records[first_candidate + 3 p + plane - 1] and the same plane, bit for bit,
// at store + (first_candidate + 3 p + plane - 1) * 65536; store and records hold `candidates` entries (checked).  One
// workgroup per candidate, no atomics.
void grid_harvest(const float* logits, int P, int first_candidate, int pre_w, int pre_h, float* store, int candidates, int32_t* records,
                  hipStream_t);
// The kept candidates in label order (label k = entry k - 1) with their cull words; travels as kernel arguments.
struct GridKept { int count; int candidate[kGridMaxKept]; uint32_t cull[kGridMaxKept]; };
// dst [out_h][out_w] bytes: per pixel the largest label whose mask (what postprocess_masks delivers for the plane) is 255 there,
// 0 where none is.  candidates: planes the store holds (every kept candidate is checked against it before the launch).
// cull = false: every label is sampled at every pixel (measurements; same map).
void grid_paint(const float* store, int candidates, const GridKept& kept, uint8_t* dst, int out_w, int out_h, int pre_w, int pre_h,
                bool cull, hipStream_t);

// ---- prior marks (K19, kernels/mask_prior.hip) ------------------------------------------------
// A caller's mask as the mask input of a prompt: mask [H][W] u8, tightly packed, values 0 .. 255 read as coverage, of an image
// that was encoded at pre_w x pre_h -> plane [256][256] fp32 (16-byte aligned), which MaskSource{plane, nullptr} feeds to
// mask_embed.  With sw = ceil(pre_w / 4), sh = ceil(pre_h / 4), all products in 64 bits:
//   x < sw:  c0 = floor(4 x W / pre_w),  c1 = ceil(min(4 x + 4, pre_w) W / pre_w)          (c0 < c1 <= W)
//   y < sh:  r0 = floor(4 y H / pre_h),  r1 = ceil(min(4 y + 4, pre_h) H / pre_h)
//   sum = sum of mask[r0 .. r1)[c0 .. c1),  area = (r1 - r0) (c1 - c0),  s = float(strength_milli) / 1000.f
//   plane[y][x] = (float(2 sum - 255 area) / float(255 area)) * s      inside the scored region (x < sw and y < sh)
//   plane[y][x] = -1.f * s                                             elsewhere: padding is background
// one correctly rounded fp32 division and one fp32 multiply; both numerators stay below 2^24, so the conversions are exact --
// a mask so much larger than pre_w x pre_h that 255 area reaches 2^24 is refused, as is one whose 64 low-res columns span more
// than 8192 source columns.  strength_milli: 1 .. kPriorMaxStrength.  One launch, no atomics.
constexpr int kPriorMaxStrength = 100000;
void mask_prior(const uint8_t* mask, int W, int H, int pre_w, int pre_h, int strength_milli, float* plane, hipStream_t);

// ---- lasso marks (K20, kernels/mask_lasso.hip) ------------------------------------------------
// The box of a selection and its most interior cell, on the low-res grid: plane [256][256] fp32 as mask_prior wrote it for an
// image encoded at pre_w x pre_h.  With sw = ceil(pre_w / 4), sh = ceil(pre_h / 4): cell (x, y) is inside when x < sw, y < sh
// and plane[y][x] > 0 (2 sum > 255 area); every other cell of Z^2 is background.  d2(x, y): the exact squared Euclidean
// distance of an inside cell to the nearest background cell.
//   g_scratch [256][256] int32   the vertical distance of every cell to the nearest background cell of its column (0 outside)
//   rows [256][kLassoRowInts] int32, one record per low-res row y: {inside cells of the row, its first inside column, its last,
//        the column of its cell with the largest d2 (ties: the smallest), that d2, 0, 0, 0}; all zero for a row without one
// Integer arithmetic throughout.  Two launches, no atomics on global memory; lasso_plan.hpp (fold_lasso_rows) folds the rows into
// the prompt's record on the host, which reads them anyway.
constexpr int kLassoRowInts = 8;
void lasso_derive(const float* plane, int pre_w, int pre_h, int* g_scratch, int* rows, hipStream_t);

// ---- matte marks (K21, kernels/mask_matte.hip) ------------------------------------------------
// An image-guided soft edge for a delivered mask: the guided filter of He et al. with a grey guide, in integers, in place.
// mask p [H][W] u8 (any 0 .. 255 is taken as is), guide [H][W][c] u8 tightly packed, c = 1, 3 or 4:  G = the byte for c == 1,
// else (c0 + 2 c1 + c2 + 2) >> 2 (a fourth channel is ignored).  F = 16, E = eps; win(x, y) is the (2 r + 1)^2 square around
// the pixel clipped to the image, N its pixel count; fdiv is floor division.
//   pass 1, sums over win(x, y):  S_G, S_p, S_GG = sum G^2, S_Gp = sum G p
//     cov = N S_Gp - S_G S_p        den = N S_GG - S_G^2 + E N^2                          (int64, den > 0)
//     A   = fdiv(2 cov 2^F + den, 2 den)             B = fdiv(2 (S_p 2^F - A S_G) + N, 2 N)       (both int32)
//   pass 2, sums over the same window:  S_A, S_B (int64)
//     out = clamp(fdiv(2 (S_A G(x, y) + S_B) + N 2^F, 2 N 2^F), 0, 255)
// Where p is one value over the radius-2r square around a pixel, out == p there; with a constant guide the matte is the twice
// box-filtered mask.  radius 1 .. 32, eps 1 .. 65025 (squared grey levels).  Jobs of one call may differ in size.  Refused
// before anything is launched: a null pointer, an extent that is not positive, whose w * h does not fit an int or which is so
// thin that one mask needs 2^24 workgroups or more (1 x 2^31 - 1), parameters outside these ranges.  Stream-ordered, no host synchronisation, no global atomics: three launches per 16 jobs.  workspace:
// mask_matte_workspace_bytes(jobs, count) bytes of device memory (8 per pixel, 4 per 64 x 64 cell), contents irrelevant before
// and after.  shortcut = false: the blocks whose mask is one value over their halo are computed like any other (measurements
// and tests; same bytes).
struct MatteJob { uint8_t* mask; const uint8_t* guide; int w, h, channels, radius, eps; };   // mask: device, packed rows, in place
size_t mask_matte_workspace_bytes(const MatteJob* jobs, int count);
int mask_matte_launches(const MatteJob* jobs, int count);            // kernel launches mask_matte makes for these jobs
void mask_matte(const MatteJob* jobs_host, int count, void* workspace, hipStream_t, bool shortcut = true);

// ---- stroke marks (K22, kernels/mask_stroke.hip) ----------------------------------------------
// Clicks sampled from a caller's scribble: map [H][W] u8, tightly packed, of an image that was encoded at pre_w x pre_h; a pixel
// belongs to the stroke when its byte is >= 128.  With sw = ceil(pre_w / 4), sh = ceil(pre_h / 4) and the footprints c0, c1, r0,
// r1 of mask_prior above: cell (x, y), x < sw, y < sh, is ON when any pixel of map[r0 .. r1)[c0 .. c1) belongs to the stroke.
//   ballots [256][4] u64     bit b of word [y][w] is cell (64 w + b, y); 0 outside the scored region
//   record [kStrokeRecordInts] int32  {ON cells n, clicks, x0, y0 .. x7, y7, 0, 0}, cells; clicks not asked for are 0, and the
//        whole record is 0 when no cell is ON
//   click 0      the ON cell with the smallest (n x - Sx)^2 + (n y - Sy)^2 (int64; Sx, Sy the coordinate sums of the ON cells)
//   click c > 0  the ON cell with the largest minimum over the clicks before it of dx^2 + dy^2: farthest-point sampling; with
//                fewer ON cells than clicks a cell is chosen again
// Ties go to the smallest y, then the smallest x.  Integer arithmetic throughout.  clicks 1 .. kStrokeMaxClicks.  Two launches,
// no atomics on global memory, any W and H whose product fits 2^31; 16-byte loads when W is a multiple of 16 and the map aligned.
constexpr int kStrokeRecordInts = 20;
constexpr int kStrokeMaxClicks = 8;
constexpr int kStrokeBallotWords = 256 * 4;
void stroke_derive(const uint8_t* map, int W, int H, int pre_w, int pre_h, int clicks, unsigned long long* ballots, int32_t* record,
                   hipStream_t);

// ---- cut-out marks (K23, kernels/mask_cutout.hip) ---------------------------------------------
// A matte's foreground colours as RGBA: one pass of Forte's Blur-Fusion in integers (tests/cutout_ref.py restates it in numpy).
// coverage a [H][W] u8, guide [H][W][c] u8 tightly packed, c = 3 or 4 (a fourth channel is ignored), out [H][W][4] u8.  I_c is
// channel c of the guide (c = 0, 1, 2); win(x, y) the (2 r + 1)^2 square around the pixel clipped to the image, N its pixel
// count; fdiv is floor division.
//   sums over win(x, y):  S_a, S_I, S_Ia = sum I_c a;      S_b = 255 N - S_a      S_Ib = 255 S_I - S_Ia
//     Fh = fdiv(512 S_Ia + S_a, 2 S_a) if S_a > 0 else 256 I_c(x, y)        (the a-weighted mean of the window, in 1/256 levels)
//     Bh = fdiv(512 S_Ib + S_b, 2 S_b) if S_b > 0 else 256 I_c(x, y)        (the (255 - a)-weighted one)
//     num = 65025 Fh + a (65280 I_c - a Fh - (255 - a) Bh)                   D = 65025 * 256
//     out_c = clamp(fdiv(2 num + D, 2 D), 0, 255)                            out_3 = a
// Where a == 255 the pixel keeps its colour; where S_a == 0 too; a constant image stays constant.  radius 1 .. 32.  The kernels
// read coverage and guide and never write them; out is neither.  out, and a guide of 4 channels, are aligned to 4 bytes: one
// 4-byte store per pixel, one 4-byte load.  Jobs of one call may differ in size.  Refused before anything is launched: what
// mask_matte refuses, channels other than 3 or 4, a pointer not so aligned.  Stream-ordered, no host synchronisation, no global
// atomics: two launches per 16 jobs.  workspace: mask_cutout_workspace_bytes(jobs, count) bytes of device memory (4 per 64 x 64
// cell), contents irrelevant before and after.  shortcut = false: the blocks whose coverage is 0, or 255, over their halo --
// whose output is the guide's colours under that alpha -- are computed like any other (measurements and tests; same bytes).
struct CutoutJob { const uint8_t* coverage; const uint8_t* guide; uint8_t* out; int w, h, channels, radius; };
size_t mask_cutout_workspace_bytes(const CutoutJob* jobs, int count);
int mask_cutout_launches(const CutoutJob* jobs, int count);          // kernel launches mask_cutout makes for these jobs
void mask_cutout(const CutoutJob* jobs_host, int count, void* workspace, hipStream_t, bool shortcut = true);

// ---- edge marks (K24, kernels/mask_edge.hip) --------------------------------------------------
// Grow, shrink, feather and border a mask, in place: an exact Euclidean distance to the mask's edge, an offset, a map to bytes,
// in integers (tests/edge_ref.py restates it in numpy).  mask M [H][W] u8 tightly packed; a pixel is foreground when its byte is
// >= 128.  Pixels outside the image do not exist: they are neither foreground nor background, so a mask that touches the image's
// edge is not eroded from it.  d2 of a pixel: the exact squared distance to the nearest pixel of the other polarity, infinite
// where there is none.  isqrt rounds down, fdiv is floor division.
//     q = isqrt(65536 d2)                 S = q - 128 for a foreground pixel, -(q - 128) for a background one
//     T = S + 256 offset                  border > 0:  T <- 256 border - |T|
//     out = 255 if T > 0 else 0                                          (feather == 0)
//     out = clamp(fdiv(255 (T + 256 f) + 256 f, 512 f), 0, 255)           (feather == f > 0)
// offset -64 .. 64 (positive grows), feather 0 .. 32, border 0 .. 32, not all three 0.  With R = |offset| + feather + border + 1
// every d2 >= R^2, the infinite one too, gives the byte of d2 == R^2: distances are exact below R only.  Jobs of one call may
// differ in size.  Refused before anything is launched: a null mask, an extent that is not positive, whose w * h does not fit
// an int or which is so thin that one mask needs 2^24 workgroups or more, parameters outside these ranges, all three 0.
// Stream-ordered, no host synchronisation, no global atomics: three launches per 16 jobs (two with shortcut = false).
// workspace: mask_edge_workspace_bytes(jobs, count) bytes of device memory (2 per pixel, 4 per 64 x 64 cell), contents irrelevant
// before and after.  shortcut = false: the blocks whose mask is of one polarity over their halo of R pixels -- whose output is
// one byte -- are computed like any other (measurements and tests; same bytes).
struct EdgeJob { uint8_t* mask; int w, h, offset, feather, border; };   // mask: device, packed rows, in place
size_t mask_edge_workspace_bytes(const EdgeJob* jobs, int count);
int mask_edge_launches(const EdgeJob* jobs, int count);              // kernel launches mask_edge makes for these jobs
void mask_edge(const EdgeJob* jobs_host, int count, void* workspace, hipStream_t, bool shortcut = true);

}  // namespace k
}  // namespace dlimg
