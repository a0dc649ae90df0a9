// SegmentationImpl: per-image state of the Segment-Anything path.
// Counterpart of /root/reference/src/segmentation.{hpp,cpp} (SegmentationImpl, ResizeLongestSide):
// same life cycle (process once, query many masks), but the embedding lives in HBM.
#pragma once

#include "common.hpp"
#include "environment.hpp"
#include "prompt_geometry.hpp"       // Extent, Point, Region, scale_coord, ResizeLongestSide

#include <dlimgedit/dlimgedit.h>

namespace dlimg {

static_assert(kPromptFrame == kImageSize, "prompts are packed in the encoder's frame");

int channel_bytes(int channels);          // 4 for bgra/argb (reference: dlimgedit.impl.hpp:15)

// Packs one prompt and returns its number of points.  A point OR a region: two points, the way
// SegmentationImpl::compute_mask does (reference: segmentation.cpp:135-152; coords[4], labels[2]).  A point AND a region
// (the batch calls only): three points as SAM's PromptEncoder.forward orders them, the point in front of the box corners
// and no pad token, labels 1, 2, 3 (coords[6], labels[3]).  A one-entry call of pack_points (prompt_plan.hpp).
int pack_prompt(ResizeLongestSide const& rs, Point const* point, Region const* region, float* coords, float* labels);
// Which logits plane a single-mask query of `points` prompt points takes (SamOnnxModel.select_masks adds
// (points - 2.5) * 1000 to prediction 0): with two points the best of planes 1..3, chosen on the device from the IoU
// predictions; with three always plane 0.
inline k::PostJob single_mask_job(float const* logits4, float const* iou4, int points, uint8_t* dst, Extent o, Extent r) {
    return k::PostJob{logits4, points > 2 ? nullptr : iou4, dst, o.width, o.height, r.width, r.height};
}

struct BatchPrompts;         // segmentation.cpp

class SegmentationImpl {
  public:
    explicit SegmentationImpl(EnvironmentImpl& env);

    void process(dlimg_ImageView const& image);
    // Batched variant: segs[i] receives the embedding of images[i].
    static void process_batch(EnvironmentImpl& env, SegmentationImpl* const* segs, dlimg_ImageView const* images,
                              int count);

    void compute_mask(Point const* point, Region const* region, uint8_t* const out_masks[3],
                      float out_accuracy[3]) const;
    // points XOR regions: entry i is a point or a box query.  Both: entry i is the box regions[i] refined by the foreground
    // point points[i], one three-point prompt (pack_prompt).  An entry whose segs[i] is null adds one more click to the prompt
    // in front of it (prompt_plan.hpp: up to 8 clicks, foreground or background, with or without the box); its out_masks
    // entry is not read.  Prompts of different sizes may share a call.  A continuation entry {4, 0, 0, 0} is a refinement mark:
    // the prompt is decoded in stages, each taking the logits of the one before it as mask input (prompt_plan.hpp).
    static void compute_mask_batch(SegmentationImpl const* const* segs, int count, int const* points,
                                   int const* regions, uint8_t* const* out_masks);

    // Device-output form of compute_mask_batch: mask i is produced on the GPU that holds segs[i]'s embedding
    // and lands at dev_out + offset_i in the memory of HIP device `root_device` (offset_i = sum of width*height of the
    // prompts before it; also returned in out_offsets when given, a continuation entry repeating its prompt's).  Returns when
    // every mask is in place.
    static void compute_mask_batch_device(SegmentationImpl const* const* segs, int count, int const* points,
                                          int const* regions, int root_device, uint8_t* dev_out, size_t* out_offsets);

    Extent extent() const { return image_size_.original; }
    ResizeLongestSide const& geometry() const { return image_size_; }
    float const* embedding() const { settle(); return embedding_; }       // complete when this returns
    ~SegmentationImpl();
    SegmentationImpl(SegmentationImpl const&) = delete;
    SegmentationImpl& operator=(SegmentationImpl const&) = delete;
    EnvironmentImpl& environment() const { return env_; }
    int replica() const { return replica_; }      // which entry of the environment's device list holds the embedding
    void set_geometry(Extent e) { image_size_.set(e); }
    float* embedding_storage(int replica);

  private:
    // the per-GPU body of the two batch mask calls; Sink: where the masks go (segmentation.cpp)
    template <typename Sink>
    static void decode_batch_on(int replica, SegmentationImpl const* const* segs, BatchPrompts const& batch, int const* points,
                                int const* regions, Sink const& sink);

    EnvironmentImpl& env_;
    int replica_ = 0;
    ResizeLongestSide image_size_;
    float* embedding_ = nullptr;        // [4096][256] fp32, resident on the replica's GPU
    std::shared_ptr<EmbeddingPool> pool_;   // where embedding_ came from and goes back to

    // process() of ONE image returns once its encoder pass is enqueued (the pixels have been copied by then; argument
    // errors have been reported).  The pass is waited for by the first call that needs its result: compute_mask queues its
    // decoder on the same lane behind the encoder and waits once, for both; everything else settles first.  A pass that
    // reported non-finite values makes every query of this handle fail with the message process() would have thrown.
    // DLIMGEDIT_SYNC_PROCESS=1: process() waits itself, as in the reference (Ort::Session::Run).
    mutable std::mutex pending_mutex_;
    mutable std::shared_ptr<SamModel::DeferredPass> pending_;
    mutable std::atomic<bool> invalid_{false};
    std::shared_ptr<SamModel::DeferredPass> pending() const;
    void settle() const;                    // waits for a deferred pass; throws when the embedding is not usable
    void forget_pending() noexcept;         // the same without the verdict: the embedding is about to be replaced or freed
};

// Validates an image view the way the entry points need it; throws on nonsense.
void check_image(dlimg_ImageView const& image);

}  // namespace dlimg
