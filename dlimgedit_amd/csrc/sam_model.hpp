// SamModel: device-resident weights + the HIP executor for the Segment-Anything path.
// Takes the place of the reference's SegmentAnythingModel, i.e. of its three onnxruntime Sessions
// (/root/reference/src/segmentation.hpp:17-32, /root/reference/src/session.cpp:57-136):
//   encode()  == image_embedder.run(...)            (segmentation.cpp:126-128)
//   decode()  == single/multi_mask_decoder()(...)   (segmentation.cpp:154-158)
// Tensors stay in HBM between the two; nothing round-trips through host memory as it does in the
// reference (environment.cpp:142 binds every Ort::Value to CPU memory).
#pragma once

#include "common.hpp"

#include <dlimgedit/dlimgedit.h>
#include "completion_events.hpp"
#include "kernels/kernels.hpp"
#include "lane_board.hpp"
#include "mask_transport_exec.hpp"
#include "resize_tables.hpp"
#include "stage_clock.hpp"
#include "weights.hpp"

#include <array>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace dlimg {

constexpr int kTokens = 4096;       // 64 x 64 embedding grid
constexpr int kEmbedDim = 256;      // channels of the image embedding
constexpr int kPatchK = 768;        // 3 * 16 * 16
constexpr int kImageSize = 1024;    // /root/reference/src/segmentation.cpp:17
constexpr int kDecTokens = 7;       // token rows of a two-point prompt (a point and its pad token, or a box): 5 + 2
constexpr int kDecMaxTokens = 15;   // ... of the largest prompt (8 clicks and a box, 10 points): the workspaces are sized by it
constexpr int kLowRes = 256;

struct LinearH {                    // f16 weight for MFMA GEMMs, fp32 bias
    DeviceBuffer<half_t> w;
    DeviceBuffer<float> b;
    int out = 0, in = 0;
    bool has_bias = false;
    // set when a preceding LayerNorm is folded in: w = W * diag(gamma), b = b + W.beta and
    // colsum[n] = sum_k w[n][k] (of the f16-rounded values) for the mean correction in the GEMM epilogue
    DeviceBuffer<float> colsum;
};
struct LinearF {                    // fp32 weight for the token-side kernels
    DeviceBuffer<float> w, b;
    int out = 0, in = 0;
};
struct NormW { DeviceBuffer<float> w, b; };

struct EncoderLayer {
    bool global = false;
    NormW ln1, ln2;
    LinearH qkv, proj, fc1, fc2;
    DeviceBuffer<half_t> qkv_pad;    // q|k|v of a window's zero-padding token = the plain qkv bias (windowed layers)
    DeviceBuffer<half_t> rel_h16, rel_w16;    // the attention kernels take the tables as f16 (global layers: pre-scaled)
};

struct TokenAttention { LinearF q, k, v, o; };

struct DecoderLayer {
    TokenAttention self_attn;
    NormW ln1, ln2, ln3, ln4;
    LinearF t2i_q, t2i_o;            // token side of token->image attention
    DeviceBuffer<float> t2i_o_t;     // t2i_o.w transposed: [128][256] (kernels/decoder.hip, out_projection_columns)
    LinearH img_kqv;                 // [t2i.k ; i2t.q ; t2i.v] fused: one GEMM over the keys
    DeviceBuffer<float> pos_kqv;     // [4096, 384] pos . [Wk ; Wq]^T, zeros for the v columns (which take no pos)
    LinearF mlp1, mlp2;
    LinearF i2t_k, i2t_v;            // token side of image->token attention
    LinearH i2t_o;                   // image side output projection (128 -> 256)
};

// Device-resident weights of one SAM variant; immutable after loading and shared by every execution lane.
struct SamWeights {
    explicit SamWeights(std::string const& weight_path, int device);
    SamWeights(SamWeights const&) = delete;
    SamWeights& operator=(SamWeights const&) = delete;

    int device = 0;
    SamGeometry geom_;
    bool fused_ln_ = true;            // encoder LayerNorms folded into the qkv / fc1 GEMMs
    LinearH patch_;                       // [D, 768] + bias
    DeviceBuffer<float> pos_embed_;       // [4096, D]
    std::vector<EncoderLayer> layers_;
    LinearH neck1_, neck2_;               // 1x1 conv [256, D]; 3x3 conv as [256, 9*256] (tap-major columns)
    NormW neck_ln1_, neck_ln2_;
    DeviceBuffer<half_t> zero_line_;      // 128 bytes of zeros: the padding the implicit 3x3 operand reads
    DeviceBuffer<float> pe_gauss_, pe_point_, pe_not_a_point_, pe_no_mask_;
    k::PromptEncoderWeights prompt_encoder() const {
        return k::PromptEncoderWeights{pe_gauss_.get(), pe_point_.get(), pe_not_a_point_.get(), iou_token_.get(), mask_tokens_.get()};
    }
    // the prompt encoder's mask branch (pe.mask.*), optional in the file: without it no prompt can take a mask input
    bool has_mask_branch_ = false;
    DeviceBuffer<float> mask_w1_, mask_b1_, mask_w2_, mask_b2_, mask_proj_w_, mask_proj_b_;
    NormW mask_ln1_, mask_ln2_;
    k::MaskBranch mask_branch() const {
        k::MaskBranch b;
        b.w1 = mask_w1_.get(); b.b1 = mask_b1_.get(); b.ln1_w = mask_ln1_.w.get(); b.ln1_b = mask_ln1_.b.get();
        b.w2 = mask_w2_.get(); b.b2 = mask_b2_.get(); b.ln2_w = mask_ln2_.w.get(); b.ln2_b = mask_ln2_.b.get();
        b.proj_w = mask_proj_w_.get(); b.proj_b = mask_proj_b_.get();
        return b;
    }
    DeviceBuffer<float> iou_token_, mask_tokens_;
    std::array<DecoderLayer, 2> dec_;
    LinearF final_q_, final_o_;
    DeviceBuffer<float> final_o_t_;       // final_o_.w transposed: [128][256]
    LinearH final_kv_;                    // [final.k ; final.v]
    DeviceBuffer<float> final_pos_kv_;    // [4096, 256] pos . Wk^T | 0
    NormW ln_final_;
    LinearH up1_, up2_;                   // transposed-conv weights as GEMM operands (sub-pixel-major rows)
    NormW up_ln_;
    std::array<std::array<LinearF, 3>, 5> heads_;   // 4 hyper MLPs + IoU head
    // SAM-HQ's decoder add-on (dec.hq.*), optional in the file, all or nothing: without it the model is plain SAM
    bool has_hq_ = false;
    bool has_hq() const { return has_hq_; }
    DeviceBuffer<float> hq_token_;                  // [256]
    std::array<LinearF, 3> hq_mlp_;                 // 256 -> 256 -> 256 -> 32
    LinearH hq_vit1_, hq_vit2_, hq_emb1_, hq_emb2_; // transposed convolutions as GEMM operands, like up1_ / up2_
    NormW hq_vit_ln_, hq_emb_ln_, hq_mask_ln_;
    DeviceBuffer<half_t> hq_conv1_w_, hq_conv2_w_;  // 3x3 convolutions, [9][64][32] and [9][32][64]: tap, output, input channel
    DeviceBuffer<float> hq_conv1_b_, hq_conv2_b_;
    k::HqMaskWeights hq_mask_weights() const {
        k::HqMaskWeights w;
        w.conv1_w = hq_conv1_w_.get(); w.conv1_b = hq_conv1_b_.get(); w.ln_w = hq_mask_ln_.w.get(); w.ln_b = hq_mask_ln_.b.get();
        w.conv2_w = hq_conv2_w_.get(); w.conv2_b = hq_conv2_b_.get();
        return w;
    }
};

// What a Segmentation handle keeps per image: the embedding [4096][256] fp32 and, behind it in the same buffer when the
// model is a SAM-HQ one, the image's HQ features [256][256][32] fp32.
constexpr size_t kEmbeddingFloats = (size_t)kTokens * kEmbedDim;
constexpr size_t kHqFeatureFloats = (size_t)kLowRes * kLowRes * 32;
constexpr size_t handle_floats(bool hq) { return kEmbeddingFloats + (hq ? kHqFeatureFloats : 0); }
constexpr int kHqMaxPoints = 9;      // a SAM-HQ prompt: the HQ token takes the 15th token row

enum class HqBranch { vit, emb };    // the two branches of the SAM-HQ features: early ViT block, final embedding

// One execution lane.  What is the lane's own here: the encoder, the decoder, image intake (staging ring, resize tables,
// staged resizes) and the pass flags with DeferredPass.  The rest are components with contracts of their own, which the
// methods below only forward to: StageClock (stage_clock.hpp; under mutex()), CompletionEvents (completion_events.hpp;
// thread-safe) and MaskTransport (mask_transport_exec.hpp; slots thread-safe, enqueuing under mutex()).
class SamModel {
  public:
    // One execution lane: own stream, workspaces and staging buffers over shared weights.  Several lanes
    // let independent images overlap on the GPU (tails and small kernels of one image hide behind the
    // large kernels of another) -- the serving counterpart of the reference's "Environment is
    // thread-safe" contract (reference: src/include/dlimgedit/dlimgedit.hpp:98-101).
    explicit SamModel(std::shared_ptr<SamWeights const> weights, int lane_index = 0, int lane_count = 1,
                      std::shared_ptr<LaneBoard> board = nullptr);
    ~SamModel();
    SamModel(SamModel const&) = delete;
    SamModel& operator=(SamModel const&) = delete;

    SamGeometry const& geometry() const { return weights_->geom_; }
    hipStream_t stream() const { return stream_; }
    std::mutex& mutex() { return mutex_; }
    int device() const { return device_; }
    int lane_index() const { return lane_index_; }
    LaneBoard const* board() const { return board_.get(); }

    // All methods below require mutex() to be held by the caller, unless stated otherwise.  The mutex covers the
    // ENQUEUE of a request (host-side state, staging areas), not its execution: workspaces are re-used in stream
    // order, so a caller records completion(), releases the mutex and waits for its own event while the next
    // request is already being enqueued behind it.

    // Host image (already at its encoder resolution: longest side 1024) -> slot `slot` of the patch
    // matrix.  Copies through pinned staging and runs the pre-processing kernel.
    // Pixels in pinned image memory of the library with packed rows are sent from where they lie; the caller waits for
    // that copy (wait_caller_copies) before it hands the pixels back to their owner.
    void upload_image(int slot, int batch, uint8_t const* pixels, int w, int h, int stride, int channels);
    void wait_caller_copies();           // mutex() held or not: the event is this lane's own, re-recorded under mutex()
    // Host image whose longest side is not 1024: uploaded at its own size and resampled on the device to
    // rw x rh (reference: dlimg::resize through stb, /root/reference/src/image.cpp:37-51).  The upload is enqueued
    // here; the resize of all such images of the pass is one launch per stage in front of encode().
    void upload_and_resize_image(int slot, int batch, uint8_t const* pixels, int w, int h, int stride, int channels,
                                 int rw, int rh);
    // Device-resident image variant (used by the batch benchmark so PCIe is outside the timed region).
    void preprocess_device_image(int slot, int batch, uint8_t const* dev_pixels, int w, int h, int stride, int channels);
    // All `batch` slots from device-resident images of any size (views carry device pixel pointers).  resized[i] is the
    // extent image i is encoded at (ResizeLongestSide); an image already of that extent takes the pre-processing launch,
    // the others are resampled on the way by the fused resize: one launch per stage for all of them.
    void preprocess_device_images(dlimg_ImageView const* views, int const* resized_wh, int batch);
    // Runs the encoder on `batch` uploaded images; embedding i [4096][256] fp32 in emb_dst[i] where that is given, else at
    // embeddings() + i * 4096 * 256 (DLIMGEDIT_FUSED_LN=0: there in any case, and copied to emb_dst[i]).  A SAM-HQ model
    // also leaves every image's HQ features: behind the embedding in emb_dst[i] (a buffer of handle_floats(true) floats),
    // else in a workspace of the lane.
    void encode(int batch, float* const* emb_dst = nullptr);
    bool has_hq() const { return weights_->has_hq_; }                          // no mutex needed
    float const* embeddings() const { return emb_.get(); }

    // Decoder for `count` prompts of `points` points each (2 .. 10: every prompt of a call has the same number, 5 + points
    // token rows). emb[i]: device embedding of prompt i's image; coords [count][points][2], labels [count][points] host
    // arrays. Results stay on device: logits() [count][4][256][256], iou() [count][4].
    // mask_input (optional, [count]): every prompt's mask input, SAM's click-to-refine loop -- device logits some decode left
    // (this lane's own logits() / iou() are fine: they are read before this decode writes them, in stream order).  All
    // prompts of a call have one or none; needs a model with the mask branch (has_mask_branch()).
    // handles: emb[i] are the buffers of Segmentation handles (handle_floats()).  A SAM-HQ model decodes nothing else: the
    // HQ features of the image lie behind the embedding there, and a bare embedding has none.  It appends the HQ token's
    // pseudo-point to every prompt itself (5 + points + 1 token rows), so its prompts hold at most kHqMaxPoints points.
    void decode(float const* const* emb, float const* coords, float const* labels, int count, int points = 2,
                k::MaskSource const* mask_input = nullptr, bool handles = false);
    // "Segment everything" (grid_plan.hpp; kernels.hpp K18): the side * side one-click prompts of a grid over the image whose
    // embedding is `emb` (a Segmentation handle's buffer), coords [side * side][2][2] / labels [side * side][2] packed as
    // one-click prompts are (click, padding point).  Decoded in chunks of k::decoder_max_prompts(token rows) prompts, one
    // decode() per chunk -- never one decode() for the whole grid, which would size every per-prompt workspace for it (about
    // 10 MB per prompt) -- each chunk harvested into the lane's grid store before the next one overwrites logits().  Behind the
    // last chunk the records and IoU predictions (44 bytes per candidate) go to pinned host memory, the call WAITS for the
    // stream (the one host round trip of a label map), and the segments are selected on the host (select_grid_segments).
    // Returns what the launch step of the label map's mask request paints from (enqueue_masks / enqueue_masks_device, `paint`);
    // valid until the next segment_grid of this lane, so the request is enqueued under the same hold of mutex().
    // pre_w, pre_h: the extent the image was encoded at.
    GridPaint const& segment_grid(float const* emb, float const* coords, float const* labels, int side, int pre_w, int pre_h,
                                  int iou_permille, int stability_permille);
    // Prior marks (prior_plan.hpp; kernels.hpp K19): the caller's mask [h][w] u8 (HOST memory, tightly packed) of an image that
    // was encoded at pre_w x pre_h -> the lane's prior plane, as the mask input of the decode enqueued next.  The bytes travel
    // through the pinned staging ring, packed before this returns (they may be the memory the prompt's mask goes to); a prior
    // in pinned image memory of the library is copied from where it lies, and the caller waits for that copy
    // (wait_caller_copies) as for image pixels.  One buffer for the bytes and one plane per lane, grown to the largest prior
    // seen and kept: the plane is valid until the next prior_plane of this lane, in stream order.
    k::MaskSource prior_plane(uint8_t const* mask, int w, int h, int pre_w, int pre_h, int strength_milli);
    // Lasso marks (lasso_plan.hpp; kernels.hpp K20): prior_plane of the selection, then the derivation behind it on the lane's
    // stream, the row records copied to pinned memory, ONE wait for the stream, and the rows folded into `record` ({inside cells,
    // box x0, y0, x1, y1, click x, click y, d2} in image pixels; all zero: the selection is empty).  Returns the plane, which is
    // the first stage's mask input when the mark asks for it.  strength_milli 0: the plane is scratch.
    k::MaskSource lasso_derive(uint8_t const* mask, int w, int h, int pre_w, int pre_h, int strength_milli, int32_t record[8]);
    // Matte marks (matte_plan.hpp; kernels.hpp K21): the guide [h][w][channels] u8 (HOST memory, tightly packed) uploaded to the
    // lane's guide buffer on the lane's stream, for the mask request enqueued behind the decode (MatteRequest::guide).  The bytes
    // travel as a prior's do: through the pinned staging ring, or copied from where they lie when they are pinned image memory
    // of the library, and then the caller waits for that copy (wait_caller_copies).  One buffer per lane, grown (behind a wait for
    // the stream) to the largest guide seen and kept: valid until the next matte_guide of this lane, in stream order.
    uint8_t const* matte_guide(uint8_t const* guide, int w, int h, int channels);
    // Stroke marks (stroke_plan.hpp; kernels.hpp K22): the stroke map [h][w] u8 (HOST memory, tightly packed) of an image that was
    // encoded at pre_w x pre_h uploaded as a prior's bytes are (staging ring, or in place from pinned image memory, and then the
    // caller waits for that copy: wait_caller_copies), the two launches of the derivation behind it on the lane's stream and the
    // record {ON cells, clicks, x0, y0 .. x7, y7, 0, 0} (cells) copied to pinned memory.  Nothing is waited for: the marks of one
    // prompt (kMaxClicks at most) are enqueued back to back, *record is where this one's will lie, and stroke_wait is the ONE wait
    // of the prompt, after which the records are valid until the next stroke_derive of this lane.
    void stroke_derive(uint8_t const* map, int w, int h, int pre_w, int pre_h, int clicks, int32_t const** record);
    void stroke_wait();
    // why a SAM-HQ model refuses a prompt of `points` points (empty: it does not)
    std::string hq_refusal(int points) const;
    bool has_mask_branch() const { return weights_->has_mask_branch_; }       // no mutex needed
    float const* logits() const { return logits_.get(); }
    // Diagnostic: the token-side workspaces as the last decode of ONE prompt left them (after synchronize()), one after
    // the other; names/sizes in decoder_state_layout().  What a parity or race hunt compares stage by stage.
    static std::vector<std::pair<const char*, size_t>> decoder_state_layout();
    void decoder_state(float* out) const;
    // The same for a prompt of `tokens` token rows (7 .. 15: 5 + its points); with_mask_h adds "mask_h" [4096][16], the mask
    // branch in front of its last convolution as the last MASKED decode of one prompt left it.
    // with_hq (SAM-HQ models, whose one-point prompt has 8 token rows, the HQ token last): adds "hyper_hq" [32] at the end.
    static std::vector<std::pair<const char*, size_t>> decoder_state_layout(int tokens, bool with_mask_h = false, bool with_hq = false);
    void decoder_state(float* out, int tokens, bool with_mask_h = false, bool with_hq = false) const;
    float const* iou() const { return iou_.get(); }
    // Diagnostic, the encoder's counterpart: what the last encode() of `batch` images left in this lane's workspaces for
    // image `image` of that pass (after synchronize()), one after the other as floats (f16 tensors widened, which is exact);
    // names/sizes in encoder_state_layout().  "patches" [4096][768]; "stream_hi" / "stream_lo" [4096][D]: the residual stream
    // behind the last block as the pair xn_ + xlo_ (fp32 stream: hi its f16 copy, lo = x - hi in fp32); "stats"
    // [groups][4096][2]: the row statistics the last stream writer left for these rows; "qkv" [4096][3 D] and "hidden"
    // [4096][mlp] of the last block; "embedding" [4096][256]; then one float each: "groups" (tile column blocks of the last
    // stream writer, from the same planner call encode() makes), "split" (1: the f16-pair stream) and "nonfinite" (the pass's
    // overflow report).  Reads only: encode() and its launches know nothing of it.
    std::vector<std::pair<std::string, size_t>> encoder_state_layout(int batch) const;
    void encoder_state(float* out, int image, int batch) const;
    // The device operands of encoder layer `layer` as the loader left them (folded, scaled, rounded), widened to floats:
    // qkv.w / .b / .colsum, fc1.w / .b / .colsum, proj.w / .b, fc2.w / .b, rel_h16, rel_w16, qkv_pad (windowed layers; empty
    // for global ones), "global" (one float).  layer == -1: patch.w / .b, pos_embed, neck1.w, neck_ln1.w / .b, neck2.w,
    // neck_ln2.w / .b.  colsum entries are empty when the LayerNorms are not folded.
    std::vector<std::pair<std::string, size_t>> encoder_operands_layout(int layer) const;
    void encoder_operands(float* out, int layer) const;

    // Diagnostic: one branch of the SAM-HQ features alone, as encode() runs it (the same private entry, which picks the
    // branch's tensors): a is a DEVICE input f16 [batch * 4096][K], K = the encoder's width (vit) or 256 (emb), batch 1..2.
    // Enqueued on the lane's stream under mutex(); after synchronize() the view's pointers are readable: A fp32
    // [batch * 4096][4 C] (hq_a_), H f16 [batch * 16384][C] (hq_h_), Y fp32 [batch * 16384][128] (the branch's workspace), and
    // the loaded operands w1 f16 [4 C][K], b1 [4 C], ln_w / ln_b [C], w2 f16 [128][C], b2 [128].
    struct HqBranchView {
        int K, C;
        float const* A; half_t const* H; float const* Y;
        half_t const* w1; float const* b1; float const* ln_w; float const* ln_b; half_t const* w2; float const* b2;
    };
    HqBranchView run_hq_branch(HqBranch which, half_t const* a, int batch);

    // Masks to the caller, in steps so that the wait happens outside mutex() (MaskTransport, mask_transport_exec.hpp):
    // acquire_mask_slot (no mutex needed; callers hold the slot as a MaskSlotLease, below), enqueue_masks with the first
    // n_iou IoU predictions of the last decode() (under mutex()), finish_masks (no mutex), release_mask_slot.
    // enqueue_masks_device / wait_masks: jobs[i].dst are pointers valid on HIP device dst_device, which may be ANOTHER GPU
    // ("all masks on one device").
    using MaskSlot = dlimg::MaskSlot;
    MaskSlot& acquire_mask_slot() { return masks_.acquire(); }
    void release_mask_slot(MaskSlot& s) { masks_.release(s); }
    void enqueue_masks(MaskSlot& slot, k::PostJob const* jobs, int count, int iou_count, CleanSpec const* clean = nullptr,
                       GridPaint const* paint = nullptr, MatteRequest const* matte = nullptr, EdgeRequest const* edge = nullptr) {
        masks_.enqueue(slot, jobs, count, iou_.get(), iou_count, clean, paint, matte, edge);
    }
    void finish_masks(MaskSlot& slot, k::PostJob const* jobs, int count, float* iou_out, int iou_count) { masks_.finish(slot, jobs, count, iou_out, iou_count); }
    void enqueue_masks_device(MaskSlot& slot, k::PostJob const* jobs, int count, int dst_device, CleanSpec const* clean = nullptr,
                              GridPaint const* paint = nullptr, EdgeRequest const* edge = nullptr) {
        masks_.enqueue_device(slot, jobs, count, dst_device, clean, paint, edge);
    }
    void wait_masks(MaskSlot& slot) { masks_.wait(slot); }
    // Blocking convenience form of the three calls above (mutex() held throughout).
    void masks_to_host(k::PostJob const* jobs, int count);
    // Same kernel, but jobs[i].dst are DEVICE pointers and nothing is copied or waited for.
    void masks_on_device(k::PostJob const* jobs, int count);

    void synchronize();
    // Event recorded behind everything enqueued so far; wait for it WITHOUT mutex(), then give it back.
    hipEvent_t completion() { return done_events_.record(); }
    // Overflow report of the encoder pass enqueued last (valid under mutex(), right after encode()): an int in pinned host
    // memory that the pass sets to 1 when an activation left the f16 range somewhere in the image (an infinity or a NaN
    // reached the last LayerNorm of the neck).  Read it after the pass's completion event; slots are reused after
    // kPassFlags further passes of this lane.
    static constexpr int kPassFlags = 64;
    const volatile int* last_pass_flag() const { return pass_flag_; }
    // An encoder pass nobody has waited for yet: SegmentationImpl::process hands the caller's thread back once the pass is
    // enqueued, and the first request that needs the embedding is queued on the SAME lane behind it (stream order), so the
    // GPU goes from the encoder's last kernel to the decoder's first without a round trip through the host.  Whoever gets
    // there first settles it -- the handle (first mask query, re-use, destruction) or this lane, before it re-uses the
    // pass's flag; settle() is idempotent and callable from any thread without mutex().
    struct DeferredPass {
        SamModel* lane = nullptr;
        bool settle();                    // waits for the pass; true when it reported non-finite values
      private:
        friend class SamModel;
        std::mutex mutex_;
        hipEvent_t done_ = nullptr;
        const volatile int* flag_ = nullptr;
        bool settled_ = false, overflowed_ = false;
    };
    // Under mutex(), right after encode(): completion() + last_pass_flag() of that pass as one object.
    std::shared_ptr<DeferredPass> defer_last_pass();
    void wait_and_recycle(hipEvent_t e) { done_events_.wait_and_recycle(e); }             // no mutex needed
    bool poll_and_recycle(hipEvent_t e) { return done_events_.poll_and_recycle(e); }      // no mutex needed: true (and the event is taken back) once it has completed

    // What the GEMM planner (gemm_plan.cpp) is told about the caller, for every GEMM of the model: whether other lanes share
    // the device, whether the pass has it to itself, and the rows of one image.
    static void plan_inputs(k::GemmArgs& a, bool shared_gpu, bool alone) { a.shared_gpu = shared_gpu; a.alone = alone; a.unit_rows = kTokens; }

    void set_profiling(bool on) { clock_.set_profiling(on); }
    StageStats take_stats() { return clock_.take_stats(); }

  private:
    void reserve_encoder(int batch);
    void reserve_decoder(int count);
    void decode_chunk(float const* const* emb, float const* coords, float const* labels, int count, int first, int points,
                      k::MaskSource const* mask_input);
    struct HqBranchTensors { LinearH const& conv1; NormW const& ln; LinearH const& conv2; };
    HqBranchTensors hq_tensors(HqBranch which) const;                         // the ONE place a branch's tensors are chosen
    void hq_branch(HqBranch which, half_t const* a, int M, float* out);
    void gemm(k::GemmArgs const& a, Stage shape = ST_COUNT);     // shape: ST_GEMM_PATCH / _PROJ / _FC2 for the stage clocks
    template <typename F> void neck_launch(double flops, F&& launch);     // launch(start, stop): one of k::neck_conv*_ln
    struct DeviceTap { std::string name; half_t const* h; float const* f; size_t n; };      // one of h / f; n elements
    std::vector<DeviceTap> encoder_operand_taps(int layer) const;
    int encoder_stat_groups(int batch) const;

    int device_ = 0;
    bool shared_gpu_ = false;            // other lanes run on this device too (GEMM tile choice, gemm_plan.cpp)
    std::shared_ptr<LaneBoard> board_;   // activity of the sibling lanes (null: a lane on its own)
    int lane_index_ = 0;
    bool alone_ = false;                 // the encoder pass being enqueued found every other lane idle (set by encode())
    void mark_activity() { if (board_) board_->mark(lane_index_, stream_); }
    void begin_activity() { if (board_) board_->begin(lane_index_); }
    hipStream_t stream_ = nullptr;
    std::mutex mutex_;

    std::shared_ptr<SamWeights const> weights_;

    // ---- encoder workspace (sized for enc_batch_ images)
    int enc_batch_ = 0;
    DeviceBuffer<uint8_t> img_dev_;
    // pinned staging for host images: a ring, each entry guarded by the event of the copy that last read it
    static constexpr int kStageRing = 4;
    struct ImageStage { PinnedBuffer pin; hipEvent_t copied = nullptr; };
    ImageStage stage_[kStageRing];
    unsigned stage_seq_ = 0;
    hipEvent_t caller_copied_ = nullptr;     // behind the last copy that read a caller's pinned pixels directly
    bool caller_copy_pending_ = false;
    uint8_t* stage_rows(uint8_t const* pixels, size_t row_bytes, int rows, int stride, hipEvent_t* copied);
    DeviceBuffer<half_t> patches_, xn_, xlo_, qkv_, att_, hid_;
    DeviceBuffer<float> x_, xstat_, emb_;
    DeviceBuffer<float> neck_f32_;       // DLIMGEDIT_FUSED_LN=0 only: the neck convolutions' fp32 results
    // SAM-HQ models: first transposed convolution fp32 / after its LayerNorm f16, the two branches' second convolutions,
    // the f16 copy of the embedding, and the features of passes that have no handle to write them to
    DeviceBuffer<float> hq_a_, hq_vit_, hq_embf_, hq_feat_;
    DeviceBuffer<half_t> hq_h_, emb_h_;
    // The residual stream as an f16 pair (xn_ = hi, which is also the consumers' A operand; xlo_ = lo) instead of fp32 x_ +
    // its f16 copy xn_: 8 instead of 10 bytes per element through every stream writer (kernels.hpp, GemmArgs::out_l).
    // Needs the ping-pong epilogue for every stream writer: folded LayerNorms, several lanes (the shared-GPU tile choice) and
    // an embedding width that is a multiple of 256 (ViT-B / L / H; the reduced test variants keep the fp32 stream).
    bool split_stream_ = false;
    static bool split_stream_allowed();

    // ---- longest-side resize (images whose longest side is not 1024)
    // Contributor tables of one axis, cached per lane by (in, out).  The host copy lives in pinned memory for as long as
    // the entry does: the tables reach the device by one stream-ordered copy, so a miss blocks nobody and a hit costs
    // a lookup (no allocation, no copy, no synchronisation).
    struct AxisDev {
        int in_size = 0, out_size = 0, taps = 0;
        PinnedBuffer host;                   // first [out] | count [out] | coef [out][taps]
        DeviceBuffer<uint8_t> dev;           // the same bytes
        int const* first = nullptr;
        int const* count = nullptr;
        float const* coef = nullptr;
    };
    std::shared_ptr<AxisDev const> axis_table(int in_size, int out_size);
    static constexpr size_t kAxisCacheEntries = 64;
    std::vector<std::shared_ptr<AxisDev const>> axis_cache_;     // least recently used first
    DeviceBuffer<float> srgb_decode_;
    DeviceBuffer<uint32_t> srgb_encode_;
    // host images: the upload at its own size, one buffer per slot of the pass, and the resizes staged so far -- they
    // run as ONE launch per stage when the pass is encoded (encode()), not one after the other as the images arrive.
    // Every function that fills a slot drops what was staged for it (preprocess_device_image, upload_and_resize_image,
    // preprocess_device_images).
    // Memory: a slot's buffer and the fp32 rows grow to the largest need seen and stay for the life of the lane: per
    // lane at most  sum over the slots of the largest source image seen in that slot  +  the largest pass's fp32 rows
    // (3 x h x 1024 x 4 bytes per image).  One 4000 x 3000 RGBA image at a time: 48 + 37 MB; a four-image pass of such
    // images (the most slot 13 puts into one pass): 192 + 148 MB on the lane that ran it.
    std::vector<DeviceBuffer<uint8_t>> resize_src_;
    DeviceBuffer<float> resize_tmp_;         // fp32 rows between the two stages, one area per image of the pass
    // Device pixels at their own size -> slot `slot` of the patch matrix at rw x rh, all images in one launch per stage
    struct ResizeRequest { uint8_t const* pixels; int w, h, stride, channels, rw, rh, slot; };
    void resize_into_patches(ResizeRequest const* requests, int count);
    std::vector<ResizeRequest> staged_resizes_;
    void forget_staged_resize(int slot);     // the slot is being filled anew
    void run_staged_resizes(int batch);

    // ---- decoder workspace (sized for dec_count_ prompts)
    int dec_count_ = 0;
    DeviceBuffer<float> keys_, logits_, iou_, hyper_;
    DeviceBuffer<float> hyper_hq_;       // SAM-HQ models: [launch's prompts][32]
    DeviceBuffer<half_t> hq_u_, hq_mid_; // ... the up-scaled embedding [.][256][256][32] and the 3x3 path's intermediate [.][256][256][64]
    DeviceBuffer<float> mask_h_;         // [launch's prompts][4096][16]: the mask branch in front of its last convolution (first masked decode)
    DeviceBuffer<half_t> keys_h_, kqv_h_;
    // label maps: the grid store [3 * side * side][256][256] fp32 (768 KB per prompt: 12 MiB at side 4, 192 MiB at side 16,
    // 768 MiB at side 32), reserved on first use, sized by the largest side seen, kept for the life of the lane; the records
    // (32 bytes per candidate) and their pinned host copy with the IoU predictions behind them
    DeviceBuffer<float> grid_store_;
    DeviceBuffer<int32_t> grid_records_;
    PinnedBuffer grid_host_;
    GridPaint grid_paint_;
    DeviceBuffer<uint8_t> prior_bytes_;  // prior marks: the caller's mask at its own size (grow-only) and its plane [256][256]
    DeviceBuffer<float> prior_plane_;
    DeviceBuffer<uint8_t> matte_guide_;  // matte marks: the guide of the prompt being decoded (grow-only, as prior_bytes_)
    DeviceBuffer<int32_t> lasso_scratch_;    // lasso marks: g [256][256] and the row records [256][8] behind it
    PinnedBuffer lasso_host_;
    DeviceBuffer<uint8_t> stroke_bytes_;     // stroke marks: the map being derived from (grow-only, as prior_bytes_)
    DeviceBuffer<int32_t> stroke_scratch_;   // the ballots [256][4] u64, then one record per mark of the prompt
    PinnedBuffer stroke_host_;               // the records
    int stroke_queued_ = 0;                  // marks enqueued since the last stroke_wait
    DeviceBuffer<float> tokens_, queries_, tk_, tv_, sq_, sk_, sv_, tsa_, tt2i_, tmlp_, t2i_part_;

    // ---- pass flags
    int* pass_flags_ = nullptr;          // [kPassFlags] pinned, host-visible; pass_flag_ = the slot of the pass enqueued last
    int* pass_flag_ = nullptr;
    unsigned pass_counter_ = 0;
    std::shared_ptr<DeferredPass> flag_owner_[kPassFlags];   // deferred passes by the flag they report through

    // ---- components (declared last: they are made after the stream and go before everything above)
    StageClock clock_;
    CompletionEvents done_events_;
    MaskTransport masks_;
};

// A mask slot of one lane for as long as the lease lives: taken in the constructor, handed back in the destructor or by
// release() before that, on every path.  What may still be queued on the slot is not the lease's business: an error path
// waits for the lane's stream BEFORE the lease ends (segmentation.cpp, drain_lane).
class MaskSlotLease {
  public:
    explicit MaskSlotLease(SamModel& model) : model_(&model), slot_(&model.acquire_mask_slot()) {}
    MaskSlotLease(MaskSlotLease&& o) noexcept : model_(o.model_), slot_(o.slot_) { o.slot_ = nullptr; }
    MaskSlotLease& operator=(MaskSlotLease&& o) noexcept {
        if (this != &o) {
            release();
            model_ = o.model_;
            slot_ = o.slot_;
            o.slot_ = nullptr;
        }
        return *this;
    }
    ~MaskSlotLease() { release(); }
    void release() noexcept {
        if (slot_) model_->release_mask_slot(*slot_);
        slot_ = nullptr;
    }
    bool held() const { return slot_ != nullptr; }
    SamModel& model() const { return *model_; }
    SamModel::MaskSlot& slot() const { return *slot_; }

  private:
    SamModel* model_;
    SamModel::MaskSlot* slot_;
};

}  // namespace dlimg
