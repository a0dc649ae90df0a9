/* dlimgedit_amd_test.h -- test and benchmark hooks of the MI355X build.  They are exported by lib/libdlimgedit_test.so
 * (the product's objects plus the hook sources, csrc/test_hooks.cpp and its neighbours) and by the tuning library, NOT by the product libdlimgedit.so, whose
 * dynamic symbols are dlimg_init and the entry points of dlimgedit_amd.h only (reference:
 * /root/reference/src/CMakeLists.txt:11).  Single kernels behind plain host buffers so that every HIP kernel can be
 * compared with the CPU oracle in isolation, host-logic checks that need no GPU, and kernels-alone timing loops.
 * All functions return 0 on success and non-zero on failure (message: dlimg_init()->last_error() of the SAME library)
 * unless stated otherwise.  f16 tensors cross the boundary as uint16_t bit patterns (IEEE binary16).
 */
#ifndef DLIMGEDIT_AMD_TEST_H_
#define DLIMGEDIT_AMD_TEST_H_

#include "dlimgedit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- host logic, callable without a GPU ------------------------------------------------------ */
/* Host logic of the mask transfer (csrc/mask_pieces.hpp), callable without a GPU (tests): for `count` masks of the given sizes
 * (+ extra_bytes behind them) the end offsets of the pieces the staging area travels in, and per piece the copies the host
 * makes once it has arrived, five numbers each: piece, mask, staging offset, offset inside the mask, bytes.  Returns the
 * number of copies (-1: error). */
DLIMG_API int dlimg_amd_test_mask_pieces(int count, long long const* mask_bytes, long long extra_bytes, long long* out_piece_end,
                                         int piece_capacity, long long* out_copies, int copy_capacity, int* out_pieces);
/* Host logic of the device-step queue behind dlimg_amd_encode_and_mask, callable without a GPU (tests): plans the passes
 * for `pending` waiting requests given the per-lane passes / images in flight and the lane cursor, updates those as if the
 * passes had been launched, writes (lane, images) per pass in launch order and returns the number of passes (-1: error). */
DLIMG_API int dlimg_amd_test_plan_steps(int lanes, int* passes_in_flight, int* images_in_flight, int* cursor, int pending, int width,
                                        int depth, int all, int* out_lane, int* out_images, int capacity);
/* Host logic of the lanes' enqueue threads (csrc/environment.hpp, LaneWorker), callable without a GPU (tests): `tasks` tasks
 * sleeping sleep_us each; drain must wait for all of them, they run in posting order, and a task posted after the drain has
 * run when the worker is destroyed.  out_order: tasks + 1 entries.  Returns the number of tasks that ran, -1 on error. */
DLIMG_API int dlimg_amd_test_lane_worker(int tasks, int sleep_us, int* out_order);

/* Host logic of the multi-GPU helper threads' CPU binding (csrc/environment.cpp, bind_thread_near_device): the sysfs cpulist
 * parser, "0-3,8,10-11" -> indices; returns their number, -1 on error. */
DLIMG_API int dlimg_amd_test_parse_cpu_list(char const* text, int* out_cpus, int capacity);

/* ---- single-kernel hooks (host buffers in and out; device memory handled inside) ------------- */
/* K1: pixels -> patch matrix [4096][768] f16. */
DLIMG_API int dlimg_amd_test_preprocess(uint8_t const* pixels, int width, int height, int stride, int channels,
                                        uint16_t* out_patches);
/* K16: planes [n_planes][256][256] fp32; iou (4 floats) non-null selects the plane as the single-mask
 * decoder does, otherwise plane 0 is used.  out_mask: out_w*out_h bytes. */
DLIMG_API int dlimg_amd_test_postprocess(float const* planes, int n_planes, float const* iou, int out_w, int out_h,
                                         uint8_t* out_mask);
/* K16, several masks in ONE launch (the form slot 14 uses for a chunk of prompts): plane i -> out_masks + i * out_w * out_h. */
DLIMG_API int dlimg_amd_test_postprocess_batch(float const* planes, int n_masks, int out_w, int out_h, uint8_t* out_masks);
/* Forces tile configuration `tile` (index into kernels/gemm.hip's table; < 0: off) in the GEMM test hooks below wherever it
 * fits the problem.  Affects only dlimg_amd_test_gemm / dlimg_amd_test_gemm_ln / the bench hooks, never the product path. */
DLIMG_API int dlimg_amd_test_force_gemm_tile(int tile);
/* A separate tile for the LayerNorm-folded consumer GEMM of dlimg_amd_test_gemm_ln (< 0: the one forced above); reset by
 * every dlimg_amd_test_force_gemm_tile call. */
DLIMG_API int dlimg_amd_test_force_gemm_consumer_tile(int tile);
/* Rows x columns of tile configuration `tile` (k::kGemmTiles, csrc/gemm_plan.hpp).  No GPU needed. */
DLIMG_API int dlimg_amd_test_gemm_tile_shape(int tile, int* out_bm, int* out_bn);
/* C = epilogue(A[M,K] . W[N,K]^T): bias[N], resid[resid_rows][N] (row m % resid_rows), act 0/1(GELU).  out_f32 or out_f16
 * may be NULL: the launch then gets the other result only (out_f16 alone: the f16-only epilogues). */
DLIMG_API int dlimg_amd_test_gemm(int M, int N, int K, uint16_t const* A, uint16_t const* W, float const* bias,
                                  float const* resid, int resid_rows, int act, float* out_f32, uint16_t* out_f16);
/* One stream-writing GEMM of the encoder, x = A[M,K] . W[D,K]^T + bias + (resid_hi + resid_lo), with its per-tile row
 * statistics (out_stats: M * 24 * 2 floats), in either representation of the residual stream: pair == 0 writes fp32 out_x and
 * its f16 copy out_hi, pair == 1 the f16 pair out_hi / out_lo (hi = f16(x), lo = f16(x - hi)); resid_hi / resid_lo may both be
 * NULL.  The two must agree exactly: hi, the statistics, and lo recomputed from out_x (tests/test_gpu_kernels.py). */
DLIMG_API int dlimg_amd_test_gemm_stream(int M, int D, int K, uint16_t const* A, uint16_t const* W, float const* bias,
                                         uint16_t const* resid_hi, uint16_t const* resid_lo, int pair, float* out_x,
                                         uint16_t* out_hi, uint16_t* out_lo, float* out_stats);
/* Two chained GEMMs with the LayerNorm between them folded in ("LayerNorm inside the GEMMs"):
 *   x = A1[M,K1] . W1[D,K1]^T + bias1 + resid[M,D]        -> out_x [M,D] fp32 and out_xh [M,D] f16
 *   y = act(rstd * (xh . Wg[N,D]^T - mean * colsum[N]) + bias2[N])   -> out_y [M,N]; mean / rstd of the rows of x,
 *       merged from the per-tile statistics the first GEMM leaves
 * Wg = W * diag(gamma) in f16, colsum = row sums of Wg, bias2 = b + W.beta: prepared by the caller.
 * The consumer writes out_y (fp32), out_yh (f16) or both, whichever is not NULL: out_yh alone is the launch qkv and fc1 are in
 * the product.  out_stats (may be NULL): the producer's row statistics, M * 24 * 2 floats laid out [D / block][M][2] =
 * (sum, sum of squared deviations from the block mean), with *out_block the producer's tile width. */
DLIMG_API int dlimg_amd_test_gemm_ln(int M, int D, int K1, int N, uint16_t const* A1, uint16_t const* W1,
                                     float const* bias1, float const* resid, uint16_t const* Wg, float const* colsum,
                                     float const* bias2, float eps, int act, float* out_x, uint16_t* out_xh,
                                     float* out_y, uint16_t* out_yh, float* out_stats, int* out_block);
/* ---- single-kernel hooks (host buffers in and out; device memory handled inside) ------------- */
DLIMG_API int dlimg_amd_test_layernorm(float const* x, float const* w, float const* b, float eps, int rows, int dim,
                                       int act, float* out_f32, uint16_t* out_f16);
/* Encoder attention on qkv [B*4096][3*heads*hd] f16 -> out [B*4096][heads*hd] f16.
 * global != 0: rel tables are [127][hd]; else windowed 14x14 with [27][hd] tables and qkv_bias [3*D]. */
DLIMG_API int dlimg_amd_test_attention(int global, uint16_t const* qkv, float const* qkv_bias, float const* rel_h,
                                       float const* rel_w, int batch, int heads, int hd, uint16_t* out);
/* The product's mask decoder (SamModel::decode, one call for all `count` prompts, on a lane of env's first replica) on
 * given embeddings: emb [n_emb][4096][256] fp32 (token-major, as dlimg_amd_get_embedding returns them), prompt i decodes
 * embedding emb_index[i] with the packed prompt coords [i][2][2] (resized-image pixels) and labels [i][2] (1 / -1: a
 * point, 2 / 3: a box).  out_logits [count][4][256][256], out_iou [count][4].  count < 1, an index out of range and null
 * pointers are errors. */
DLIMG_API int dlimg_amd_test_decode(dlimg_Environment env, int n_emb, float const* emb, int count, int const* emb_index,
                                    float const* coords, float const* labels, float* out_logits, float* out_iou);
/* The same decoder call with everything SamModel::decode takes: `points` points per prompt (2 .. 10, 5 + points token rows;
 * coords [count][points][2], labels [count][points]: clicks 1 / 0 in the caller's order, then the box corners 2 / 3 or the
 * padding point -1) and, optionally, a mask input per prompt: mask_planes [count][4][256][256] (host) and mask_iou [count][4],
 * the predictions the plane is chosen by on the device (NULL: plane 0).  A call of any size without mask input is cut into
 * launches by decode(); a masked call takes at most one launch's prompts (112 / (5 + points)).  out_state (optional, count == 1):
 * the token-side workspaces of that prompt, names and sizes in out_layout ("name:floats,..."), "mask_h" [4096][16] last after a
 * masked call.  Refused before anything is launched: points out of range, null pointers, an index out of range, a mask input
 * for a model without pe.mask.*, a masked call above the limit, a state for more than one prompt or a buffer too small. */
DLIMG_API int dlimg_amd_test_decode_prompts(dlimg_Environment env, int n_emb, float const* emb, int count, int const* emb_index,
                                            int points, float const* coords, float const* labels, float const* mask_planes,
                                            float const* mask_iou, float* out_logits, float* out_iou, float* out_state,
                                            int state_capacity, char* out_layout, int layout_capacity);
/* The product's image encoder on lane 0 of env's first replica, and a read-only view of what it left: upload + ONE
 * SamModel::encode for `count` (1 .. 4) RGBA images whose longest side is 1024, then the workspaces' contents for image
 * `image` of the pass as floats (f16 tensors widened) in out_state, names and sizes in out_layout ("name:floats,..."):
 * patches [4096][768], stream_hi / stream_lo [4096][D] (the residual stream behind the last block), stats [groups][4096][2]
 * (as the last stream writer left them), qkv [4096][3 D] and hidden [4096][mlp] of the last block, embedding [4096][256],
 * then one float each: groups, split (1: the f16-pair stream), nonfinite (the pass's overflow report).
 * layer > -2: additionally (count == 0: only) the device operands the loader left, in out_operands / out_operands_layout:
 * of block `layer` qkv.w / .b / .colsum, fc1.w / .b / .colsum, proj.w / .b, fc2.w / .b, rel_h16, rel_w16, qkv_pad (empty for a
 * global block), global; of layer -1 patch.w / .b, pos_embed, neck1.w, neck_ln1.w / .b, neck2.w, neck_ln2.w / .b.
 * Refused: counts and indices out of range, other image formats or sizes, null pointers, buffers too small. */
DLIMG_API int dlimg_amd_test_encoder_state(dlimg_Environment env, dlimg_ImageView const* images, int count, int image,
                                           float* out_state, long long state_capacity, char* out_layout, int layout_capacity,
                                           int layer, float* out_operands, long long operands_capacity,
                                           char* out_operands_layout, int operands_layout_capacity);
/* K17: the stb_image_resize-equivalent longest-side resampler (default filter, sRGB, clamp):
 * pixels [height][stride] -> out_pixels [out_h][out_w * bytes_per_pixel] packed. */
DLIMG_API int dlimg_amd_test_resize(uint8_t const* pixels, int width, int height, int stride, int channels, int out_w,
                                    int out_h, uint8_t* out_pixels);

/* ---- kernel-alone hooks of the encoder neck and the marks (one source file each beside csrc/test_hooks.cpp) ---- */
/* The two encoder-neck launches (k::neck_conv1x1_ln, k::neck_conv3x3_ln), one per entry point, on DEVICE buffers, as
 * SamModel::encode calls them.  in: [B*4096][K] f16 (1x1) or the f16 map [B][64][64][256] (3x3, zero pad 1); w: [256][K] /
 * [256][9*256] f16, 3x3 columns (ky*3+kx)*256 + c; gamma / beta [256] fp32.  Results, each optional: out_f16 [B*4096][256]; the
 * fp32 result of image i [4096][256] in out_f32[i] (a HOST array of B device pointers, or NULL) where that is given, else at
 * workspace + i*4096*256 (NULL: not written).  *out_flag: the launch's non-finite report, 1 when a row's statistics were an
 * infinity or a NaN. */
DLIMG_API int dlimg_amd_test_neck_conv1x1_ln(void const* in, int B, int K, void const* w, float const* gamma, float const* beta,
                                             float eps, void* out_f16, float* const* out_f32, float* workspace, int* out_flag);
DLIMG_API int dlimg_amd_test_neck_conv3x3_ln(void const* in, int B, void const* w, float const* gamma, float const* beta, float eps,
                                             void* out_f16, float* const* out_f32, float* workspace, int* out_flag);
/* The mask clean-up kernels (k::mask_cleanup) alone.  masks[i]: HOST memory, w[i] * h[i] bytes of 0 / 255 in packed rows,
 * cleaned in place with max_hole[i] / max_island[i].  All `count` masks are ONE k::mask_cleanup call on the current device's
 * null stream.  The launcher's refusals (shapes, thresholds, a null mask) arrive as the call's error; nothing is allocated or
 * copied for a list the launcher refuses for its shapes. */
DLIMG_API int dlimg_amd_test_mask_cleanup(uint8_t* const* masks, int const* w, int const* h, int const* max_hole,
                                          int const* max_island, int count);
/* The label-map kernels (k::grid_harvest, k::grid_paint) alone.  planes4 [prompts][4][256][256], iou4 [prompts][4]: HOST
 * memory, what a decode leaves for the prompts of a grid.  The planes are harvested in chunks of 16 prompts, as the runtime
 * harvests the chunks of its decodes; records_out [3 prompts][8] and store_out [3 prompts][256][256] (optional) receive what
 * the harvest left.  n_kept_in >= 0: kept_in are the candidates to paint, in label order; n_kept_in < 0: they are selected on
 * the host from the records and iou4 (csrc/grid_plan.hpp) with the two thresholds.  kept_out [255] / n_kept_out receive the
 * painted list, map_out [out_h][out_w] the label map.  Store, records and map are device buffers with 256 guard bytes on
 * either side; *guards_ok tells whether those are untouched.  iters > 0 (tools/grid_probe.py): the harvest of all chunks and
 * the paint launch are then repeated iters times each between two events, and ms_out[0] / ms_out[1] receive the milliseconds
 * of ONE harvest of all candidates / ONE paint launch. */
DLIMG_API int dlimg_amd_test_grid_kernels(float const* planes4, int prompts, float const* iou4, int out_w, int out_h, int pre_w, int pre_h,
                                          int iou_permille, int stability_permille, int const* kept_in, int n_kept_in, int cull,
                                          int32_t* records_out, float* store_out, uint8_t* map_out, int* kept_out, int* n_kept_out,
                                          int* guards_ok, int iters, float* ms_out);
/* The prior-plane kernel (k::mask_prior) alone.  mask [h][w] u8: HOST memory.  Its device copy and the plane [256][256] fp32
 * are device buffers with 256 guard bytes on either side; *guards_ok tells whether those are untouched after the launch.  The
 * copy is exactly w * h bytes long inside its guards: a sum that took in a byte behind the mask's last one would take in a
 * guard byte (0xA5) and miss the reference.  iters > 0 (tools/prior_probe.py): the launch is then repeated iters times between
 * two events, and *ms_out receives the milliseconds of ONE launch. */
DLIMG_API int dlimg_amd_test_prior_plane(uint8_t const* mask, int w, int h, int pre_w, int pre_h, int strength_milli, float* plane_out,
                                         int* guards_ok, int iters, float* ms_out);
/* The lasso derivation (k::lasso_derive) alone.  mask [h][w] u8: HOST memory, of an image that was encoded at pre_w x pre_h.
 * Upload, k::mask_prior (default strength), k::lasso_derive and the fold of csrc/lasso_plan.hpp, behind plain host buffers:
 * record_out [8] = {inside cells, box x0, y0, x1, y1, click x, click y, d2}.  The mask's device copy, the plane, g and the row
 * records are device buffers with 256 guard bytes on either side; *guards_ok tells whether those are untouched after the
 * launches.  iters > 0 (tools/lasso_probe.py): the two derive launches are then repeated iters times between two events, and
 * *ms_out receives the milliseconds of ONE derivation (both launches). */
DLIMG_API int dlimg_amd_test_lasso_derive(uint8_t const* mask, int w, int h, int pre_w, int pre_h, int32_t* record_out, int* guards_ok,
                                          int iters, float* ms_out);
/* The SAM-HQ kernels alone, and the kernel that feeds them: one launcher call each on the current device's null stream.  All
 * operands are HOST memory; every device buffer (operands, results, workspace) has 256 guard bytes of 0xA5 on either side, and
 * *guards_ok tells whether those are untouched after the launch.  A launcher's refusal arrives as the call's error, and what
 * it refuses for the prompts alone is refused before anything is allocated.
 *
 * k::hq_mask_path.  U [P][256][256][32] f16; conv1_w [9][64][32] and conv2_w [9][32][64] f16 (tap = ky * 3 + kx, then output,
 * then input channel), conv1_b / ln_w / ln_b [64] and conv2_b [32] fp32; features [n_feat][256][256][32] fp32, prompt i taking
 * image feat_index[i] (two prompts may share one; -1 passes a null pointer, which the launcher refuses); hyper_hq [P][32].
 * logits [P][4][256][256]: in and out, the launch adds the HQ plane to all four planes.  out_H (optional): the intermediate
 * [P][256][256][64] f16 as the launch left it.  P = 0 returns without touching anything. */
DLIMG_API int dlimg_amd_test_hq_mask_path(uint16_t const* U, int P, uint16_t const* conv1_w, float const* conv1_b, float const* ln_w,
                                          float const* ln_b, uint16_t const* conv2_w, float const* conv2_b, float eps,
                                          float const* features, int n_feat, int const* feat_index, float const* hyper_hq,
                                          float* logits, uint16_t* out_H, int* guards_ok);
/* k::upscale_logits.  keys_h [P*4096][256] f16; W1 [256][256] f16 (rows = sub-pixel * 64 + channel), b1 [256]; ln_w / ln_b [64];
 * W2 [128][64] f16 (rows = sub-pixel * 32 + channel), b2 [128]; hyper [P][4][32].  out_logits [P][4][256][256]; store_u != 0
 * selects the launch that also stores the up-scaled embedding, out_U [P][256][256][32] f16.  P: 1 .. 16. */
DLIMG_API int dlimg_amd_test_upscale_logits(uint16_t const* keys_h, int P, uint16_t const* W1, float const* b1, float const* ln_w,
                                            float const* ln_b, float eps, uint16_t const* W2, float const* b2, float const* hyper,
                                            int store_u, float* out_logits, uint16_t* out_U, int* guards_ok);
/* k::hq_features_finish.  vit / emb: the two GEMM results [16384][128] fp32 (row = token * 4 + first sub-pixel, column = second
 * sub-pixel * 32 + channel); b_vit / b_emb [32]; out [256][256][32]. */
DLIMG_API int dlimg_amd_test_hq_features_finish(float const* vit, float const* emb, float const* b_vit, float const* b_emb, float* out,
                                                int* guards_ok);
/* One branch of the SAM-HQ features alone, as the product's encoder runs it: lane 0 of env's first replica, under the lane's
 * mutex, through the entry SamModel::encode calls (which picks the branch's tensors).  branch 0: the early-ViT branch, K = the
 * model's embed_dim, C = 256; branch 1: the embedding branch, K = 256, C = 64.  a: f16 [B * 4096][K], B = batch in 1 .. 2.
 * Results: out_A fp32 [B * 4096][4 C] (transposed convolution as a GEMM, bias included), out_H f16 [B * 16384][C] (LayerNorm +
 * GELU of out_A read as [B * 16384][C]), out_Y fp32 [B * 16384][128] (second GEMM, without its bias).  The branch's loaded
 * operands: w1 f16 [4 C][K] and b1 [4 C], ln_w / ln_b [C], w2 f16 [128][C] and b2 [128]; any of the nine outputs may be NULL.
 * Refused by name before anything is launched: a model without dec.hq.* tensors, a branch other than 0 / 1, a batch outside
 * 1 .. 2, a null environment or input. */
DLIMG_API int dlimg_amd_test_hq_branch(dlimg_Environment env, int branch, uint16_t const* a, int batch, float* out_A, uint16_t* out_H,
                                       float* out_Y, uint16_t* w1, float* b1, float* ln_w, float* ln_b, uint16_t* w2, float* b2);
/* k::layernorm alone, one launcher call on the null stream; x [rows][dim], w / b [dim] HOST memory, every device buffer with 256
 * guard bytes of 0xA5 on either side (*guards_ok: untouched after the launch).  out_f32 / out_f16: either or both.  in_place != 0:
 * the launch gets out_f32 = x (needs out_f32).  misalign_x != 0: the device x starts 4 bytes behind a 16-byte boundary.
 * nonfinite (optional): in and out, the value of an int in host-visible memory the launch is given as its non-finite report.
 * A launcher's refusal arrives as the call's error; *nonfinite is then returned as it was found. */
DLIMG_API int dlimg_amd_test_layernorm_rows(float const* x, float const* w, float const* b, float eps, int rows, int dim, int act,
                                            int in_place, int misalign_x, float* out_f32, uint16_t* out_f16, int* nonfinite,
                                            int* guards_ok);
/* The other row kernels of kernels/elementwise.hip alone, guarded as above.  op 0: k::cast_f16, a fp32 [n] -> out_f16 [n].
 * op 1: k::add_cast, a fp32 [n] + b fp32 [b_mod] (NULL: nothing added; element i takes b[i % b_mod]) -> out_f32 / out_f16 [n],
 * either or both.  op 2: k::im2col3x3, in_h f16 [n = B][64][64][C = b_mod] -> out_f16 [B * 4096][9][C]. */
DLIMG_API int dlimg_amd_test_elementwise(int op, float const* a, uint16_t const* in_h, float const* b, long long b_mod, long long n,
                                         float* out_f32, uint16_t* out_f16, int* guards_ok);

/* ---- kernels alone, timed on device-resident data --------------------------------------------- */
/* Times the two pixel kernels of the path alone on `batch` (1..16) device-resident 1024x1024 RGBA images / mask requests in
 * ONE launch each: K1 pre-processing (4 MiB u8 in, 6 MiB f16 patch matrix out per image) and K16 post-processing (256 KiB
 * of fp32 logits in, 1 MiB u8 mask out per mask); average ms per launch.  Successive launches rotate over distinct input and
 * output sets with a footprint of `working_set_mb` MB (0: 768, three times the 256 MB Infinity Cache), so that the bytes a
 * launch moves come from and go to HBM.  At one image the kernels sit on the launch floor; at 16 they move 168 MB / 21 MB
 * per launch and can be read against the HBM rate. */
DLIMG_API int dlimg_amd_bench_prepost(int batch, int iters, int working_set_mb, double* out_pre_ms, double* out_post_ms);
/* Times `iters` back-to-back launches of an encoder attention kernel (global != 0: the 4096-token kernel, else the 14x14
 * windowed one) on device-resident random data of `batch` images; returns the average ms per launch. */
DLIMG_API int dlimg_amd_bench_attention(int global, int batch, int heads, int hd, int iters, double* out_ms);
/* Times `iters` launches of the GEMM on device-resident random operands; returns average ms per launch.
 * flavour 0: f16 output; 1: LayerNorm folded in; 2: bias + fp32 residual in place; 3: 2 + f16 copy of the result + row statistics;
 * 4: f16 output with bias. */
DLIMG_API int dlimg_amd_bench_gemm(int M, int N, int K, int act, int flavour, int iters, double* out_ms);
/* The same with the tile configuration forced (tile >= 0, index into kernels/gemm.hip's table; -1: chosen as in the
 * product, `shared` = the shared-GPU hint) and `streams` (1..8) concurrent copies of the problem launched round-robin;
 * out_ms = wall time per GEMM over all streams. */
DLIMG_API int dlimg_amd_bench_gemm_streams(int M, int N, int K, int act, int flavour, int tile, int shared, int streams,
                                           int iters, double* out_ms);
/* The same; additionally returns in-kernel time stamps of the LAST launch on stream 0 for kernels that record them
 * (the ping-pong GEMM): per workgroup 4 x u64 = {shader cycles, 100 MHz ticks} of the main loop and of the whole
 * kernel.  max_groups must be >= the grid size. */
DLIMG_API int dlimg_amd_bench_gemm_stamps(int M, int N, int K, int act, int flavour, int tile, int shared, int streams,
                                          int iters, double* out_ms, unsigned long long* out_stamps, int max_groups);

#ifdef __cplusplus
}
#endif

#endif /* DLIMGEDIT_AMD_TEST_H_ */
