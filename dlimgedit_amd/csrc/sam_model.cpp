#include "sam_model.hpp"
#include "gemm_plan.hpp"
#include "grid_plan.hpp"
#include "image_memory.hpp"
#include "lasso_plan.hpp"
#include "roctx.hpp"
#include "stroke_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace dlimg {

namespace {

constexpr float kLnEps = 1e-6f;       // encoder blocks and every LayerNorm2d
// norm1..4 of the two-way blocks and norm_final_attn: nn.LayerNorm's default in Meta's mask decoder, which the
// reference's decoder graphs are exports of (/root/reference/script/export_models.py:29-43)
constexpr float kDecLnEps = 1e-5f;

hipStream_t make_lane_stream(int device, int lane_index) {
    HIP_CHECK(hipSetDevice(device));
    hipStream_t stream = nullptr;
    // The runtime multiplexes streams of one priority onto its hardware queues, shared with the host's other streams.
    // With the default four queues a fourth lane of the same priority ends up behind another lane's kernels and costs
    // 15 %; each priority level has its own queues, so the lanes are then spread over the three levels (no lane is
    // favoured for long because requests are dealt round-robin).  With eight queues plain streams are better: the
    // priority levels make four host threads wait on each other's lanes (ABI, config 2 from four threads: 479 against
    // 569-596 images/s; one prompt per call from four threads: 4900 against 5500 masks/s).  The library asks for eight
    // queues when it is loaded (environment.cpp) and remembers whether the runtime can have seen that request: plain
    // streams are the default only when it can (hardware_queues_trusted(): the host set >= 8 itself, or the library set
    // it before the runtime initialised); a host that initialised HIP first keeps the three-priority layout.
    // DLIMGEDIT_PLAIN_STREAMS=0/1 overrides the detection.
    static const bool plain = [] {
        if (const char* e = std::getenv("DLIMGEDIT_PLAIN_STREAMS")) return std::atoi(e) != 0;
        return hardware_queues_trusted();
    }();
    if (plain) {
        HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    } else {
        int least = 0, greatest = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        const int prio = least + (greatest - least) * (lane_index % 3) / 2;
        HIP_CHECK(hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, prio));
    }
    return stream;
}

}  // namespace

SamModel::SamModel(std::shared_ptr<SamWeights const> weights, int lane_index, int lane_count, std::shared_ptr<LaneBoard> board)
    : device_(weights->device), shared_gpu_(lane_count > 1), board_(std::move(board)), lane_index_(lane_index),
      stream_(make_lane_stream(device_, lane_index)), weights_(std::move(weights)), clock_(stream_), done_events_(stream_),
      masks_(device_, stream_, clock_, board_.get(), lane_index_) {
    for (auto& st : stage_) HIP_CHECK(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&caller_copied_, hipEventDisableTiming));
}

// The components' events (stage clock, completion events, mask slots) go with the components, after this body: every
// deferred pass has given its event back by then, and nothing is in flight.
SamModel::~SamModel() {
    if (stream_) (void)hipStreamSynchronize(stream_);
    for (auto& d : flag_owner_) {                // handles that outlive their lane find their pass settled
        try {
            if (d) d->settle();
        } catch (...) {
        }
    }
    for (auto& st : stage_)
        if (st.copied) (void)hipEventDestroy(st.copied);
    if (caller_copied_) (void)hipEventDestroy(caller_copied_);
    if (stream_) (void)hipStreamDestroy(stream_);
    if (pass_flags_) (void)hipHostFree(pass_flags_);
}

void SamModel::gemm(k::GemmArgs const& args, Stage shape) {
    k::GemmArgs a = args;
    plan_inputs(a, shared_gpu_, alone_);
    if (!clock_.profiling()) {
        k::gemm(a, stream_);
        return;
    }
    // the clock of a GEMM launch is the kernel's own dispatch-to-completion time (events attached to the dispatch)
    const Stage flavour = a.stats_out ? ST_GEMM_STATS : a.ln_stats ? (a.act == k::ACT_GELU ? ST_GEMM_NORM_GELU : ST_GEMM_NORM) : ST_GEMM_OTHER;
    const StageClock::Pending p = clock_.event_pair(ST_GEMM, 2.0 * a.M * a.N * a.K, flavour, shape);
    k::gemm(a, stream_, p.a, p.b);
    clock_.add(p);
}

// A neck launch, clocked like a GEMM of the "other" flavour (events attached to its dispatch)
template <typename F> void SamModel::neck_launch(double flops, F&& launch) {
    if (!clock_.profiling()) {
        launch(nullptr, nullptr);
        return;
    }
    const StageClock::Pending p = clock_.event_pair(ST_GEMM, flops, ST_GEMM_OTHER);
    launch(p.a, p.b);
    clock_.add(p);
}

void SamModel::synchronize() { HIP_CHECK(hipStreamSynchronize(stream_)); }

std::shared_ptr<SamModel::DeferredPass> SamModel::defer_last_pass() {
    DLIMG_ASSERT(pass_flag_ != nullptr);
    auto d = std::make_shared<DeferredPass>();
    d->lane = this;
    d->done_ = completion();
    d->flag_ = pass_flag_;
    flag_owner_[pass_flag_ - pass_flags_] = d;
    return d;
}

bool SamModel::DeferredPass::settle() {
    std::lock_guard<std::mutex> lock(mutex_);
    if (!settled_) {
        settled_ = true;                         // the event goes back to the lane whatever the wait reports
        lane->wait_and_recycle(done_);
        overflowed_ = *flag_ != 0;
        *const_cast<volatile int*>(flag_) = 0;
    }
    return overflowed_;
}

// ---------------------------------------------------------------------------------------------
// encoder

void SamModel::reserve_encoder(int batch) {
    SamWeights const& W = *weights_;
    if (batch <= enc_batch_) return;
    HIP_CHECK(hipStreamSynchronize(stream_));
    const size_t M = (size_t)batch * kTokens;
    const size_t D = W.geom_.embed_dim;
    const size_t wide = std::max<size_t>(W.geom_.mlp_dim, 9 * kEmbedDim);
    img_dev_.reserve((size_t)batch * kImageSize * kImageSize * 4);
    patches_.reserve(M * kPatchK);
    split_stream_ = W.fused_ln_ && shared_gpu_ && D % 256 == 0 && split_stream_allowed();
    if (split_stream_) xlo_.reserve(M * D);
    else x_.reserve(M * D);
    xn_.reserve(M * D);
    xstat_.reserve(M * k::kGemmMaxStatGroups * 2);   // (sum, M2) per tile column block and row
    qkv_.reserve(M * 3 * D);
    att_.reserve(M * std::max<size_t>(D, kEmbedDim));
    hid_.reserve(M * wide);
    if (!W.fused_ln_) neck_f32_.reserve(M * kEmbedDim);
    emb_.reserve(M * kEmbedDim);
    if (W.has_hq()) {
        hq_a_.reserve(M * 4 * kEmbedDim);
        hq_h_.reserve(M * 4 * kEmbedDim);
        hq_vit_.reserve(M * 4 * 128);
        hq_embf_.reserve(M * 4 * 128);
        emb_h_.reserve(M * kEmbedDim);
        hq_feat_.reserve((size_t)batch * kHqFeatureFloats);
    }
    enc_batch_ = batch;
}

bool SamModel::split_stream_allowed() {
    // measurement aid like DLIMGEDIT_FUSED_LN: =0 keeps the fp32 stream (same-box A/B of the two representations)
    static const bool on = [] { const char* e = std::getenv("DLIMGEDIT_SPLIT_STREAM"); return !e || std::atoi(e) != 0; }();
    return on;
}

void SamModel::preprocess_device_image(int slot, int batch, uint8_t const* dev_pixels, int w, int h, int stride,
                                       int channels) {
    DLIMG_ASSERT(slot >= 0 && slot < batch);
    reserve_encoder(batch);
    forget_staged_resize(slot);
    const int bytes = channels > 4 ? 4 : channels;
    clock_.timed(ST_PRE, (double)w * h * bytes + (double)kTokens * kPatchK * 2, [&] {
        k::preprocess(dev_pixels, w, h, stride, channels, patches_.get() + (size_t)slot * kTokens * kPatchK, stream_);
    });
}

void SamModel::preprocess_device_images(dlimg_ImageView const* views, int const* resized_wh, int batch) {
    DLIMG_ASSERT(views != nullptr && resized_wh != nullptr && batch > 0);
    reserve_encoder(batch);
    staged_resizes_.clear();                     // every slot of the pass is filled here
    std::vector<k::PreImage> images;
    std::vector<ResizeRequest> resizes;
    double bytes = 0;
    for (int i = 0; i < batch; ++i) {
        dlimg_ImageView const& v = views[i];
        const int rw = resized_wh[i * 2], rh = resized_wh[i * 2 + 1];
        if (rw == v.width && rh == v.height) {
            const int px = v.channels > 4 ? 4 : v.channels;
            images.push_back(k::PreImage{v.pixels, v.width, v.height, v.stride, v.channels,
                                         patches_.get() + (size_t)i * kTokens * kPatchK});
            bytes += (double)v.width * v.height * px + (double)kTokens * kPatchK * 2;
        } else {
            resizes.push_back(ResizeRequest{v.pixels, v.width, v.height, v.stride, v.channels, rw, rh, i});
        }
    }
    if (!images.empty()) clock_.timed(ST_PRE, bytes, [&] { k::preprocess_batch(images.data(), (int)images.size(), stream_); });
    if (!resizes.empty()) resize_into_patches(resizes.data(), (int)resizes.size());
}

// Packs `rows` rows of `row_bytes` bytes into the next entry of the pinned staging ring and returns it; *copied is the
// event the caller records behind its copy out of the entry (the entry is not touched again before that event).
uint8_t* SamModel::stage_rows(uint8_t const* pixels, size_t row_bytes, int rows, int stride, hipEvent_t* copied) {
    ImageStage& st = stage_[stage_seq_++ % kStageRing];
    HIP_CHECK(hipEventSynchronize(st.copied));       // the copy that last read this entry has run
    st.pin.reserve(row_bytes * rows);                // (re-allocation is safe for the same reason)
    uint8_t* pin = static_cast<uint8_t*>(st.pin.get());
    if ((size_t)stride == row_bytes) {
        std::memcpy(pin, pixels, row_bytes * rows);
    } else {
        for (int y = 0; y < rows; ++y) std::memcpy(pin + y * row_bytes, pixels + (size_t)y * stride, row_bytes);
    }
    *copied = st.copied;
    return pin;
}

void SamModel::upload_image(int slot, int batch, uint8_t const* pixels, int w, int h, int stride, int channels) {
    DLIMG_ASSERT(slot >= 0 && slot < batch);
    DLIMG_ASSERT(w > 0 && h > 0 && w <= kImageSize && h <= kImageSize);
    reserve_encoder(batch);
    const int bytes = channels > 4 ? 4 : channels;
    const size_t row = (size_t)w * bytes;
    const size_t slot_bytes = (size_t)kImageSize * kImageSize * 4;
    // Rows are packed on the way (the reference's create_image_tensor assumes packed rows when no
    // resize happens, segmentation.cpp:81-106; honouring the stride is identical for packed views).
    // In pieces of ~1 MiB: piece i crosses PCIe while the host packs piece i + 1 into the pinned area (a 4 MiB image:
    // 0.30 -> ~0.2 ms of a synchronous caller's 2.6 ms per image; one piece for small images)
    uint8_t* dev = img_dev_.get() + slot * slot_bytes;
    if ((size_t)stride == row && image_memory_is_pinned(pixels, row * h)) {
        // pixels the library allocated itself (an Image of the consumer: load_image / create_image) are pinned: one copy
        // command from where they lie, no packing pass
        // (the pre-processing kernel reading the pinned pixels itself, no copy command: 489 -> 476-485 images/s; not kept)
        HIP_CHECK(hipMemcpyAsync(dev, pixels, row * h, hipMemcpyHostToDevice, stream_));
        HIP_CHECK(hipEventRecord(caller_copied_, stream_));
        caller_copy_pending_ = true;
        preprocess_device_image(slot, batch, dev, w, h, (int)row, channels);
        return;
    }
    ImageStage& st = stage_[stage_seq_++ % kStageRing];
    HIP_CHECK(hipEventSynchronize(st.copied));       // the copy that last read this entry has run
    st.pin.reserve(row * h);                         // (re-allocation is safe for the same reason)
    uint8_t* pin = static_cast<uint8_t*>(st.pin.get());
    // (r06, the wrapper's own loop with a 4 MiB image: pieces of 4 / 2 / 1 / 0.5 / 0.25 MiB = 468 / 478 / 478 / 464 / 448 images/s
    // -- a copy command costs ~9 us of its own; from pinned image memory, one command and no packing: 493)
    const int pieces = (int)std::min<size_t>(8, std::max<size_t>(1, row * h / (1u << 20)));
    for (int p = 0; p < pieces; ++p) {
        const int y0 = (int)((long)h * p / pieces), y1 = (int)((long)h * (p + 1) / pieces);
        if ((size_t)stride == row) {
            std::memcpy(pin + (size_t)y0 * row, pixels + (size_t)y0 * stride, row * (size_t)(y1 - y0));
        } else {
            for (int y = y0; y < y1; ++y) std::memcpy(pin + (size_t)y * row, pixels + (size_t)y * stride, row);
        }
        HIP_CHECK(hipMemcpyAsync(dev + (size_t)y0 * row, pin + (size_t)y0 * row, row * (size_t)(y1 - y0), hipMemcpyHostToDevice, stream_));
    }
    HIP_CHECK(hipEventRecord(st.copied, stream_));
    preprocess_device_image(slot, batch, dev, w, h, (int)row, channels);
}

void SamModel::wait_caller_copies() {
    if (!caller_copy_pending_) return;
    caller_copy_pending_ = false;
    HIP_CHECK(hipEventSynchronize(caller_copied_));
}

std::shared_ptr<SamModel::AxisDev const> SamModel::axis_table(int in_size, int out_size) {
    for (size_t i = 0; i < axis_cache_.size(); ++i)
        if (axis_cache_[i]->in_size == in_size && axis_cache_[i]->out_size == out_size) {
            // most recently used entry last; eviction takes from the front
            std::rotate(axis_cache_.begin() + i, axis_cache_.begin() + i + 1, axis_cache_.end());
            return axis_cache_.back();
        }
    // A size this lane has not seen (or no longer remembers): the tables are built on this thread and allocated once;
    // they travel behind whatever the stream holds, nobody waits for them.
    AxisTable t = make_axis_table(in_size, out_size);
    auto a = std::make_shared<AxisDev>();
    a->in_size = in_size;
    a->out_size = out_size;
    a->taps = t.taps;
    const size_t n_first = t.first.size() * sizeof(int), n_count = t.count.size() * sizeof(int);
    const size_t n_coef = t.coef.size() * sizeof(float);
    a->host.reserve(n_first + n_count + n_coef);
    a->dev.reserve(n_first + n_count + n_coef);
    uint8_t* host = static_cast<uint8_t*>(a->host.get());
    std::memcpy(host, t.first.data(), n_first);
    std::memcpy(host + n_first, t.count.data(), n_count);
    std::memcpy(host + n_first + n_count, t.coef.data(), n_coef);
    HIP_CHECK(hipMemcpyAsync(a->dev.get(), host, n_first + n_count + n_coef, hipMemcpyHostToDevice, stream_));
    a->first = reinterpret_cast<int const*>(a->dev.get());
    a->count = reinterpret_cast<int const*>(a->dev.get() + n_first);
    a->coef = reinterpret_cast<float const*>(a->dev.get() + n_first + n_count);
    if (axis_cache_.size() >= kAxisCacheEntries) {
        // The only wait of this path, and only once a lane has seen more than kAxisCacheEntries (in, out) pairs: the
        // evicted entry's device tables may still be read by a resize queued on this lane's stream, and its pinned copy by
        // the upload in front of that.  Callers hold their own reference for the duration of the call, but the kernel
        // outlives the call.
        HIP_CHECK(hipStreamSynchronize(stream_));
        axis_cache_.erase(axis_cache_.begin());
    }
    axis_cache_.push_back(a);
    return a;
}

void SamModel::resize_into_patches(ResizeRequest const* requests, int count) {
    // At most as many images at a time as the table cache has entries for (two axes each): no lookup then evicts -- and
    // frees -- a table that an earlier lookup of the same group returned while its launches are still to come.  A later
    // group may evict an earlier group's tables; eviction waits for the stream first (axis_table).
    constexpr int kGroup = (int)(kAxisCacheEntries / 2);
    if (count > kGroup) {
        for (int base = 0; base < count; base += kGroup) resize_into_patches(requests + base, std::min(kGroup, count - base));
        return;
    }
    if (!srgb_decode_.get()) {               // first resize of this lane
        float lut[256];
        srgb_decode_table(lut);
        srgb_decode_.reserve(256);
        srgb_encode_.reserve(104);
        HIP_CHECK(hipMemcpy(srgb_decode_.get(), lut, sizeof(lut), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(srgb_encode_.get(), kSrgbEncodeTab4, sizeof(kSrgbEncodeTab4), hipMemcpyHostToDevice));
    }
    // the tables are held by value until the launch: looking up one axis may evict the entry of another
    std::vector<std::shared_ptr<AxisDev const>> held((size_t)count * 2);
    std::vector<size_t> offset(count);
    size_t floats = 0;
    double bytes = 0;
    for (int i = 0; i < count; ++i) {
        ResizeRequest const& r = requests[i];
        DLIMG_ASSERT(r.slot >= 0 && r.slot < enc_batch_);
        DLIMG_ASSERT(r.w > 0 && r.h > 0 && r.rw > 0 && r.rh > 0 && r.rw <= kImageSize && r.rh <= kImageSize);
        held[i * 2] = axis_table(r.w, r.rw);
        held[i * 2 + 1] = axis_table(r.h, r.rh);
        offset[i] = floats;
        floats += k::resize_preprocess_tmp_floats(r.h, r.rw, r.channels);
        bytes += (double)r.w * r.h * (r.channels > 4 ? 4 : r.channels) + (double)kTokens * kPatchK * 2;
    }
    // Every image of the pass has its own fp32 rows; the area as a whole is re-used by the next pass in stream order.
    // Growing it frees memory that queued kernels may still read, so everything queued runs first (a pass larger than
    // any before it on this lane; never in steady state).
    if (floats > resize_tmp_.capacity()) {
        HIP_CHECK(hipStreamSynchronize(stream_));
        resize_tmp_.reserve(floats);
    }
    std::vector<k::ResizeJob> jobs(count);
    for (int i = 0; i < count; ++i) {
        ResizeRequest const& r = requests[i];
        AxisDev const& ax = *held[i * 2];
        AxisDev const& ay = *held[i * 2 + 1];
        jobs[i] = k::ResizeJob{r.pixels, r.w, r.h, r.stride, r.channels,
                               k::ResizeAxis{ax.first, ax.count, ax.coef, ax.taps, r.rw},
                               k::ResizeAxis{ay.first, ay.count, ay.coef, ay.taps, r.rh},
                               resize_tmp_.get() + offset[i], patches_.get() + (size_t)r.slot * kTokens * kPatchK};
    }
    clock_.timed(ST_PRE, bytes, [&] {
        k::resize_preprocess_batch(jobs.data(), count, srgb_decode_.get(), srgb_encode_.get(), stream_);
    });
}

void SamModel::upload_and_resize_image(int slot, int batch, uint8_t const* pixels, int w, int h, int stride, int channels,
                                       int rw, int rh) {
    DLIMG_ASSERT(slot >= 0 && slot < batch);
    DLIMG_ASSERT(w > 0 && h > 0 && rw > 0 && rh > 0 && rw <= kImageSize && rh <= kImageSize);
    reserve_encoder(batch);
    const int bytes = channels > 4 ? 4 : channels;
    const size_t row = (size_t)w * bytes;
    forget_staged_resize(slot);
    if ((int)resize_src_.size() <= slot) resize_src_.resize(slot + 1);
    DeviceBuffer<uint8_t>& src = resize_src_[slot];
    // the slot's source buffer is re-used by the next pass in stream order; growing it frees memory that queued kernels
    // may still read, so everything queued runs first (the uploads of this pass lie in other slots' buffers)
    if (row * h > src.capacity()) {
        HIP_CHECK(hipStreamSynchronize(stream_));
        src.reserve(row * h);
    }
    if ((size_t)stride == row && image_memory_is_pinned(pixels, row * h)) {
        HIP_CHECK(hipMemcpyAsync(src.get(), pixels, row * h, hipMemcpyHostToDevice, stream_));     // as upload_image
        HIP_CHECK(hipEventRecord(caller_copied_, stream_));
        caller_copy_pending_ = true;
    } else {
        hipEvent_t copied = nullptr;
        uint8_t* pin = stage_rows(pixels, row, h, stride, &copied);
        HIP_CHECK(hipMemcpyAsync(src.get(), pin, row * h, hipMemcpyHostToDevice, stream_));
        HIP_CHECK(hipEventRecord(copied, stream_));
    }
    // the same launch as the device-resident path, for all resized images of the pass together (run_staged_resizes)
    staged_resizes_.push_back(ResizeRequest{src.get(), w, h, (int)row, channels, rw, rh, slot});
}

void SamModel::forget_staged_resize(int slot) {
    // only a pass that was given up between staging and encode() leaves anything behind here
    staged_resizes_.erase(std::remove_if(staged_resizes_.begin(), staged_resizes_.end(),
                                         [slot](ResizeRequest const& r) { return r.slot == slot; }),
                          staged_resizes_.end());
}

void SamModel::run_staged_resizes(int batch) {
    if (staged_resizes_.empty()) return;
    std::vector<ResizeRequest> now;
    now.swap(staged_resizes_);               // whatever happens below, nothing stays staged
    now.erase(std::remove_if(now.begin(), now.end(), [batch](ResizeRequest const& r) { return r.slot >= batch; }), now.end());
    if (!now.empty()) resize_into_patches(now.data(), (int)now.size());
}

// (Diagnostics: encoder_stat_groups() below restates the arguments writes_stream / stream_residual give the LAST fc2 launch in
// order to ask the planner for its tile again.  Whoever changes those arguments here changes them there.)
void SamModel::encode(int batch, float* const* emb_dst) {
    SamWeights const& W = *weights_;
    DLIMG_ASSERT(batch > 0 && batch <= enc_batch_);
    run_staged_resizes(batch);                   // host images of other sizes: resampled into their slots, one launch per stage
    // one image, and no other lane of this GPU has anything in flight: the pass may trade CU time for latency
    alone_ = batch == 1 && shared_gpu_ && board_ && board_->others_idle(lane_index_);
    if (board_ && batch == 1) board_->count_pass(alone_);
    begin_activity();                            // from here on this lane counts as busy for its siblings
    struct EndOnExit {                           // (an enqueue that throws must not leave the lane "busy" for ever)
        LaneBoard* board; int lane;
        ~EndOnExit() { if (board) board->end(lane); }
    } end_on_exit{board_.get(), lane_index_};
    const int D = W.geom_.embed_dim, H = W.geom_.num_heads, hd = W.geom_.head_dim(), mlp = W.geom_.mlp_dim;
    const int M = batch * kTokens;

    // Block structure: x += proj(attn(qkv(LN1(x)))); x += fc2(gelu(fc1(LN2(x)))).  With folded LayerNorms every
    // GEMM that writes the residual stream x (fp32) also leaves its f16 copy and, per tile column block, the row
    // statistics of what it wrote; the next GEMM multiplies the f16 copy by the gamma-scaled weight, merges the
    // statistics of its rows and normalises in its epilogue: the stream is read once (as f16) per consumer instead
    // of LN read + LN write + GEMM read.
    const bool fused = W.fused_ln_;
    int stat_groups = 0;                         // tile column blocks of the GEMM that last wrote the stream
    const bool split = split_stream_;
    auto stream_residual = [&](k::GemmArgs& a) {                 // += the stream itself, in place
        if (split) { a.resid_h = xn_.get(); a.resid_l = xlo_.get(); a.ldrs = D; }
        else { a.resid = x_.get(); a.ldr = D; }
        a.resid_mod = M;
    };
    auto writes_stream = [&](k::GemmArgs& a) {
        a.M = M; a.N = D;
        if (split) { a.out_l = xlo_.get(); }
        else { a.out_f32 = x_.get(); a.ldc32 = D; }
        if (fused) {
            a.out_h = xn_.get(); a.ldc16 = D; a.stats_out = xstat_.get();
            plan_inputs(a, shared_gpu_, alone_);
            stat_groups = D / k::gemm_choose_tile(a);    // the launch below uses exactly this tile (a.tile)
        }
    };
    auto reads_stream = [&](k::GemmArgs& a, LinearH const& lin, NormW const& norm) {
        if (fused) {
            a.ln_stats = xstat_.get(); a.ln_groups = stat_groups; a.ln_colsum = lin.colsum.get(); a.ln_eps = kLnEps;
        } else {
            clock_.timed(ST_LAYERNORM, (double)M * D * 6, [&] {
                k::layernorm(x_.get(), norm.w.get(), norm.b.get(), kLnEps, M, D, k::ACT_NONE, nullptr, xn_.get(), stream_);
            });
        }
        a.A = xn_.get(); a.lda = D; a.W = lin.w.get(); a.ldw = D; a.bias = lin.b.get(); a.M = M; a.N = lin.out; a.K = D;
    };

    k::GemmArgs g;
    g.A = patches_.get(); g.lda = kPatchK; g.W = W.patch_.w.get(); g.ldw = kPatchK; g.bias = W.patch_.b.get();
    g.resid = W.pos_embed_.get(); g.ldr = D; g.resid_mod = kTokens; g.K = kPatchK;
    writes_stream(g);
    gemm(g, ST_GEMM_PATCH);

    int layer_index = 0, first_global = -1;
    for (int gi : W.geom_.global_attn_indexes)
        if (first_global < 0 || gi < first_global) first_global = gi;
    for (EncoderLayer const& L : W.layers_) {
        g = k::GemmArgs{};
        reads_stream(g, L.qkv, L.ln1);
        g.out_h = qkv_.get(); g.ldc16 = 3 * D;
        gemm(g);
        if (L.global) {
            const double fl = (double)batch * (4.0 * kTokens * (double)kTokens * D + 4.0 * kTokens * 64.0 * hd * H);
            clock_.timed(ST_ATTN_GLOBAL, fl, [&] {
                k::attention_global(qkv_.get(), L.rel_h16.get(), L.rel_w16.get(), att_.get(), batch, H, hd, stream_);
            });
        } else {
            const double fl = (double)batch * 25.0 * (4.0 * 196.0 * 196.0 * D + 4.0 * 196.0 * 14.0 * hd * H);
            clock_.timed(ST_ATTN_WINDOW, fl, [&] {
                k::attention_window(qkv_.get(), L.qkv_pad.get(), L.rel_h16.get(), L.rel_w16.get(), att_.get(), batch, H, hd,
                                    stream_);
            });
        }
        g = k::GemmArgs{};
        g.A = att_.get(); g.lda = D; g.W = L.proj.w.get(); g.ldw = D; g.bias = L.proj.b.get(); g.K = D;
        stream_residual(g);
        writes_stream(g);
        gemm(g, ST_GEMM_PROJ);
        g = k::GemmArgs{};
        reads_stream(g, L.fc1, L.ln2);
        g.act = k::ACT_GELU; g.out_h = hid_.get(); g.ldc16 = mlp;
        gemm(g);
        g = k::GemmArgs{};
        g.A = hid_.get(); g.lda = mlp; g.W = L.fc2.w.get(); g.ldw = mlp; g.bias = L.fc2.b.get(); g.K = mlp;
        stream_residual(g);
        writes_stream(g);
        gemm(g, ST_GEMM_FC2);
        // SAM-HQ: the early ViT feature is the output of the FIRST global-attention block; xn_ holds its f16 copy right here
        if (W.has_hq() && layer_index == first_global) {
            if (!fused) {
                clock_.timed(ST_ENC_OTHER, (double)M * D * 6, [&] {
                    k::add_cast(x_.get(), nullptr, 0, (size_t)M * D, nullptr, xn_.get(), stream_);
                });
            }
            hq_branch(HqBranch::vit, xn_.get(), M, hq_vit_.get());
        }
        ++layer_index;
    }

    // neck: 1x1 conv -> LayerNorm2d -> 3x3 conv (pad 1) -> LayerNorm2d, all channel-last.
    // f16 operands and the f16 residual pair overflow to infinity beyond 65504; an infinity anywhere in an image turns
    // into NaNs that reach the last LayerNorm's input, which reports it (last_pass_flag) so that the caller refuses the
    // embedding instead of decoding masks from it
    if (!pass_flags_) {
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&pass_flags_), kPassFlags * sizeof(int), hipHostMallocDefault));
        std::memset(pass_flags_, 0, kPassFlags * sizeof(int));
    }
    const unsigned flag_slot = pass_counter_++ % kPassFlags;
    if (flag_owner_[flag_slot]) {                // a deferred pass of kPassFlags passes ago still reports through this flag
        flag_owner_[flag_slot]->settle();
        flag_owner_[flag_slot].reset();
    }
    pass_flag_ = pass_flags_ + flag_slot;
    *pass_flag_ = 0;
    // the embedding goes straight into the handle's storage where there is one; the unfused path copies a batch out per image
    float* direct = (emb_dst && batch == 1 && emb_dst[0]) ? emb_dst[0] : nullptr;
    if (fused) {
        // Two launches (kernels.hpp, neck_conv*_ln): each convolution with its LayerNorm2d as the epilogue, the 3x3 one
        // reading its operand straight from the f16 map.  No fp32 intermediate, no im2col matrix, no copy per image.
        std::vector<float*> dst(batch);
        for (int i = 0; i < batch; ++i)
            dst[i] = (emb_dst && emb_dst[i]) ? emb_dst[i] : emb_.get() + (size_t)i * kEmbeddingFloats;
        k::NeckOutputs map, emb;
        map.out_h = att_.get();
        emb.out_f32 = dst.data(); emb.out_h = W.has_hq() ? emb_h_.get() : nullptr; emb.nonfinite = pass_flag_;
        neck_launch(2.0 * M * kEmbedDim * D, [&](hipEvent_t a, hipEvent_t b) {
            k::neck_conv1x1_ln(xn_.get(), batch, D, W.neck1_.w.get(), W.neck_ln1_.w.get(), W.neck_ln1_.b.get(), kLnEps, map,
                               stream_, a, b);
        });
        neck_launch(2.0 * M * kEmbedDim * 9 * kEmbedDim, [&](hipEvent_t a, hipEvent_t b) {
            k::neck_conv3x3_ln(att_.get(), batch, W.neck2_.w.get(), W.zero_line_.get(), W.neck_ln2_.w.get(), W.neck_ln2_.b.get(),
                               kLnEps, emb, stream_, a, b);
        });
    } else {
        clock_.timed(ST_ENC_OTHER, (double)M * D * 6, [&] {
            k::add_cast(x_.get(), nullptr, 0, (size_t)M * D, nullptr, xn_.get(), stream_);
        });
        g = k::GemmArgs{};
        g.A = xn_.get(); g.lda = D; g.W = W.neck1_.w.get(); g.ldw = D;
        g.out_f32 = neck_f32_.get(); g.ldc32 = kEmbedDim; g.M = M; g.N = kEmbedDim; g.K = D;
        gemm(g);
        clock_.timed(ST_LAYERNORM, (double)M * kEmbedDim * 6, [&] {
            k::layernorm(neck_f32_.get(), W.neck_ln1_.w.get(), W.neck_ln1_.b.get(), kLnEps, M, kEmbedDim, k::ACT_NONE, nullptr,
                         att_.get(), stream_);
        });
        clock_.timed(ST_ENC_OTHER, (double)M * kEmbedDim * 2 * 10, [&] {
            k::im2col3x3(att_.get(), batch, kEmbedDim, hid_.get(), stream_);
        });
        g = k::GemmArgs{};
        g.A = hid_.get(); g.lda = 9 * kEmbedDim; g.W = W.neck2_.w.get(); g.ldw = 9 * kEmbedDim;
        g.out_f32 = neck_f32_.get(); g.ldc32 = kEmbedDim; g.M = M; g.N = kEmbedDim; g.K = 9 * kEmbedDim;
        gemm(g);
        clock_.timed(ST_LAYERNORM, (double)M * kEmbedDim * 8, [&] {
            k::layernorm(neck_f32_.get(), W.neck_ln2_.w.get(), W.neck_ln2_.b.get(), kLnEps, M, kEmbedDim, k::ACT_NONE,
                         direct ? direct : emb_.get(), W.has_hq() ? emb_h_.get() : nullptr, stream_, pass_flag_);
        });
    }
    if (W.has_hq()) {
        // the embedding branch of the HQ features, then per image: both branches and their biases, in raster order, behind
        // the embedding in the handle's buffer (or in the lane's workspace when the pass has no handle)
        hq_branch(HqBranch::emb, emb_h_.get(), M, hq_embf_.get());
        clock_.timed(ST_ENC_OTHER, (double)batch * kHqFeatureFloats * 12, [&] {
            for (int i = 0; i < batch; ++i) {
                float* dst = (emb_dst && emb_dst[i]) ? emb_dst[i] + kEmbeddingFloats : hq_feat_.get() + (size_t)i * kHqFeatureFloats;
                const size_t off = (size_t)i * kTokens * 4 * 128;
                k::hq_features_finish(hq_vit_.get() + off, hq_embf_.get() + off, W.hq_vit2_.b.get(), W.hq_emb2_.b.get(), dst, stream_);
            }
        });
    }
    if (emb_dst && !direct && !fused) {
        const size_t n = (size_t)kTokens * kEmbedDim;
        for (int i = 0; i < batch; ++i)
            if (emb_dst[i])
                HIP_CHECK(hipMemcpyAsync(emb_dst[i], emb_.get() + i * n, n * sizeof(float), hipMemcpyDeviceToDevice, stream_));
    }
    HIP_CHECK(hipGetLastError());     // a refused launch (bad grid, LDS size) is reported here, not at a later sync
    mark_activity();                  // behind the last kernel of the pass
}

// One branch of SAM-HQ's per-image features: two transposed convolutions (kernel 2, stride 2) as GEMMs over the image
// positions with a LayerNorm2d + GELU between them, which is a ROW LayerNorm once the first result [M][4 * C] is read as
// [4 M][C].  a: f16 [M][K]; out: fp32 [4 M][128], row = token * 4 + first sub-pixel, column = second sub-pixel * 32 + channel,
// without the second convolution's bias (hq_features_finish adds it).
SamModel::HqBranchTensors SamModel::hq_tensors(HqBranch which) const {
    SamWeights const& W = *weights_;
    if (which == HqBranch::vit) return {W.hq_vit1_, W.hq_vit_ln_, W.hq_vit2_};
    return {W.hq_emb1_, W.hq_emb_ln_, W.hq_emb2_};
}

void SamModel::hq_branch(HqBranch which, half_t const* a, int M, float* out) {
    const HqBranchTensors t = hq_tensors(which);
    LinearH const& conv1 = t.conv1;
    NormW const& ln = t.ln;
    LinearH const& conv2 = t.conv2;
    const int K = conv1.in;                      // the encoder's width (ViT branch) or the embedding's 256 channels
    const int C = conv1.out / 4;                 // channels between the two convolutions: 256 (ViT branch) or 64 (embedding branch)
    k::GemmArgs g;
    g.A = a; g.lda = K; g.W = conv1.w.get(); g.ldw = K; g.bias = conv1.b.get();
    g.out_f32 = hq_a_.get(); g.ldc32 = conv1.out; g.M = M; g.N = conv1.out; g.K = K;
    gemm(g);
    clock_.timed(ST_LAYERNORM, (double)M * conv1.out * 6, [&] {
        k::layernorm(hq_a_.get(), ln.w.get(), ln.b.get(), kLnEps, 4 * M, C, k::ACT_GELU, nullptr, hq_h_.get(), stream_);
    });
    g = k::GemmArgs{};
    g.A = hq_h_.get(); g.lda = C; g.W = conv2.w.get(); g.ldw = C;
    g.out_f32 = out; g.ldc32 = conv2.out; g.M = 4 * M; g.N = conv2.out; g.K = C;
    gemm(g);
}

// Diagnostic: one branch alone on a caller's device input, through the entry encode() calls.
SamModel::HqBranchView SamModel::run_hq_branch(HqBranch which, half_t const* a, int batch) {
    SamWeights const& W = *weights_;
    DLIMG_ASSERT(W.has_hq() && a != nullptr && batch >= 1 && batch <= 2);
    reserve_encoder(batch);
    alone_ = batch == 1 && shared_gpu_ && board_ && board_->others_idle(lane_index_);     // what encode() tells the GEMM planner
    float* out = which == HqBranch::vit ? hq_vit_.get() : hq_embf_.get();       // the workspace encode() gives the branch
    hq_branch(which, a, batch * kTokens, out);
    HIP_CHECK(hipGetLastError());
    const HqBranchTensors t = hq_tensors(which);
    return HqBranchView{t.conv1.in, t.conv1.out / 4, hq_a_.get(), hq_h_.get(), out, t.conv1.w.get(), t.conv1.b.get(),
                        t.ln.w.get(), t.ln.b.get(), t.conv2.w.get(), t.conv2.b.get()};
}

// ---------------------------------------------------------------------------------------------
// prompt encoder + mask decoder

void SamModel::reserve_decoder(int count) {
    if (count <= dec_count_) return;
    HIP_CHECK(hipStreamSynchronize(stream_));
    const size_t P = count, M = P * kTokens;
    keys_.reserve(M * 256);
    keys_h_.reserve(M * 256);
    kqv_h_.reserve(M * 384);
    logits_.reserve(P * 4 * kLowRes * kLowRes);
    iou_.reserve(P * 4);
    hyper_.reserve(P * 4 * 32);
    const size_t T = P * kDecMaxTokens;
    tokens_.reserve(T * 256);
    queries_.reserve(T * 256);
    tk_.reserve(T * 256);
    tv_.reserve(T * 256);
    sq_.reserve(T * 256);
    sk_.reserve(T * 256);
    sv_.reserve(T * 256);
    tsa_.reserve(T * 256);
    tt2i_.reserve(T * 256);
    t2i_part_.reserve(k::token_to_image_scratch_floats((int)P, kDecMaxTokens));
    tmlp_.reserve(T * 2048);
    if (weights_->has_hq()) {
        // the 3x3 path's workspaces are needed for the prompts of ONE launch (at most 14: 8 token rows)
        const size_t L = std::min<size_t>(P, k::decoder_max_prompts(8));
        hyper_hq_.reserve(P * 32);
        hq_u_.reserve(L * kLowRes * kLowRes * 32);          // 4 MB per prompt
        hq_mid_.reserve(L * kLowRes * kLowRes * 64);        // 8 MB per prompt
    }
    dec_count_ = count;
}

std::string SamModel::hq_refusal(int points) const {
    if (!has_hq() || points <= kHqMaxPoints) return {};
    return "a prompt of " + std::to_string(points) + " packed points (8 clicks and a box) is more than a SAM-HQ model takes: at most " +
           std::to_string(kHqMaxPoints) + " points, because the HQ token of the model file's dec.hq.* group travels as the 15th and last "
           "token row of the decoder";
}

void SamModel::decode(float const* const* emb, float const* coords, float const* labels, int count, int points,
                      k::MaskSource const* mask_input, bool handles) {
    DLIMG_ASSERT(count > 0);
    if (mask_input && !has_mask_branch()) throw Exception("a mask input needs the prompt encoder's mask branch: the model file has no pe.mask.* tensors");
    DLIMG_ASSERT(points >= 2 && points <= k::kDecoderMaxPoints);
    std::vector<float> hq_coords, hq_labels;
    if (has_hq()) {
        if (!handles)
            throw Exception("a SAM-HQ model (dec.hq.* in the model file) does not decode bare embeddings: the HQ features of the "
                            "image are part of the decode, and only a Segmentation handle holds them");
        const std::string why = hq_refusal(points);
        if (!why.empty()) throw Exception(why);
        // the HQ token as one more trailing pseudo-point of every prompt (kernels.hpp, kDecoderHqLabel): from here on the
        // prompts are those of a plain model with one point more
        const int np = points + 1;
        hq_coords.assign((size_t)count * np * 2, 0.f);
        hq_labels.assign((size_t)count * np, k::kDecoderHqLabel);
        for (int i = 0; i < count; ++i) {
            std::copy_n(coords + (size_t)i * points * 2, points * 2, hq_coords.data() + (size_t)i * np * 2);
            std::copy_n(labels + (size_t)i * points, points, hq_labels.data() + (size_t)i * np);
        }
        coords = hq_coords.data();
        labels = hq_labels.data();
        points = np;
    }
    static_assert(5 + k::kDecoderMaxPoints == kDecMaxTokens && k::decoder_tokens_supported(kDecTokens) &&
                  k::decoder_tokens_supported(kDecMaxTokens), "the kernels are built for these token counts");
    reserve_decoder(count);
    // the token-side kernels take at most 112 token rows per launch (16 prompts of 7 rows, 14 of 8, ... 7 of 15): larger requests run
    // in chunks that share the workspaces (stream order) and write their own part of logits() / iou()
    const int chunk = k::decoder_max_prompts(5 + points);
    if (mask_input) {
        // a later chunk's mask input must not be this call's own output of an earlier chunk
        DLIMG_ASSERT(count <= chunk);
        const size_t need = (size_t)count * kTokens * k::kMaskHidden;    // 256 KB per prompt of the launch
        if (need > mask_h_.capacity()) {
            HIP_CHECK(hipStreamSynchronize(stream_));                    // an earlier masked decode may still read the old one
            mask_h_.reserve(need);
        }
    }
    for (int c0 = 0; c0 < count; c0 += chunk)
        decode_chunk(emb + c0, coords + (size_t)c0 * points * 2, labels + (size_t)c0 * points, std::min(chunk, count - c0), c0,
                     points, mask_input ? mask_input + c0 : nullptr);
    mark_activity();
}

void SamModel::decode_chunk(float const* const* emb, float const* coords, float const* labels, int count, int first,
                            int points, k::MaskSource const* mask_input) {
    SamWeights const& W = *weights_;
    const int TOK = 5 + points;                      // token rows per prompt
    const bool hq = W.has_hq();
    const int P = count, M = P * kTokens, T = P * TOK;
    hipStream_t s = stream_;
    float* logits_out = logits_.get() + (size_t)first * 4 * kLowRes * kLowRes;
    float* iou_out = iou_.get() + (size_t)first * 4;

    auto body = [&] {
        // prompts travel as kernel arguments of the first launch
        k::DecoderStartInputs start;
        std::memcpy(start.prompts.coords, coords, (size_t)P * points * 2 * sizeof(float));
        std::memcpy(start.prompts.labels, labels, (size_t)P * points * sizeof(float));
        for (int i = 0; i < P; ++i) start.prompts.emb[i] = emb[i];

        // Token side.  `cur` is the running token matrix as its consumers read it: un-normalised rows plus the
        // LayerNorm that belongs in front of them (applied on the fly by whoever reads, kernels/decoder.hip).
        float const* qpe = tokens_.get();
        k::TokenRows cur;
        auto rows_of = [&](k::TokenRows r, bool with_pe) { if (with_pe) r.add = qpe; return r; };
        auto lin = [&](k::TokenRows in, int K, LinearF const& l, k::TokenRows resid, float* Y, int relu) {
            k::TokenLinear op;
            op.in = in; op.K = K; op.W = l.w.get(); op.b = l.b.get(); op.resid = resid; op.Y = Y; op.N = l.out; op.relu = relu;
            return op;
        };
        auto plain = [&](float const* x) { k::TokenRows r; r.x = x; return r; };
        auto normed = [&](float const* x, NormW const& n) {
            k::TokenRows r; r.x = x; r.ln_w = n.w.get(); r.ln_b = n.b.get(); r.eps = kDecLnEps; return r;
        };
        // image side of the attentions: all projections of the keys in one MFMA GEMM, the positional part of
        // (keys + pos) W as the constant addend SamWeights prepared
        auto img_gemm_args = [&](LinearH const& l, DeviceBuffer<float> const& pos) {
            k::GemmArgs g;
            g.A = keys_h_.get(); g.lda = 256; g.W = l.w.get(); g.ldw = 256; g.bias = l.b.get();
            g.resid = pos.get(); g.ldr = l.out; g.resid_mod = kTokens;
            g.out_h = kqv_h_.get(); g.ldc16 = l.out; g.M = M; g.N = l.out; g.K = 256;
            plan_inputs(g, shared_gpu_, /*alone*/ false);        // decodes run beside whatever the other lanes do
            return g;
        };
        auto img_gemm = [&](LinearH const& l, DeviceBuffer<float> const& pos) { k::gemm(img_gemm_args(l, pos), s); };

        // First launch: prompt tokens (= the positional part `qpe` of every later query), keys = image_embedding +
        // no_mask_embed (has_mask_input == 0, segmentation.cpp:43-45), and the q / k / v projections of the first
        // self-attention, whose input ARE the prompt tokens (no PE, no LayerNorm in front of the first block).
        {
            DecoderLayer const& L = W.dec_[0];
            k::TokenLinear qkv[3] = {lin({}, 256, L.self_attn.q, {}, sq_.get(), 0), lin({}, 256, L.self_attn.k, {}, sk_.get(), 0),
                                     lin({}, 256, L.self_attn.v, {}, sv_.get(), 0)};
            start.pe = W.prompt_encoder();
            start.tokens = tokens_.get(); start.first = qkv; start.n_first = 3;
            start.keys = keys_.get(); start.keys_h = keys_h_.get();
            // a SAM-HQ model: the last point of every prompt is the HQ token's pseudo-point (decode() appended it)
            if (hq) start.hq_token = W.hq_token_.get();
            const k::MaskBranch branch = W.mask_branch();
            float const* h[k::kDecoderMaxPrompts];
            if (mask_input) {
                // SAM's mask input: the branch's two strided convolutions on the logits, its last (1x1) one inside the keys'
                // initialisation, where the dense embedding takes the place of no_mask_embed
                k::mask_embed(mask_input, branch, mask_h_.get(), P, s);
                for (int i = 0; i < P; ++i) h[i] = mask_h_.get() + (size_t)i * kTokens * k::kMaskHidden;
                start.mask_h = h; start.mask = &branch;
            } else {
                start.no_mask = W.pe_no_mask_.get();
            }
            k::decoder_start(start, P, TOK, s);
        }
        for (int i = 0; i < 2; ++i) {
            DecoderLayer const& L = W.dec_[i];
            // (1) self attention of the tokens; the first layer has no residual.  The q / k / v projections were computed
            // by the launch that produced their input rows (decoder_start, or the first layer's step (4)).
            // (2) tokens -> image: [K | Q of step 4 | V] = [(keys + pos) Wk | (keys + pos) Wq | keys Wv]; the query
            // projection runs inside the attention launch, the fold + output projection inside the MLP's first launch.
            // The projection of the keys depends on (1) as little as (1) on it: its tiles ride in (1)'s launch (r06)
            const k::TokenLinear self_out = lin({}, 256, L.self_attn.o, i == 0 ? k::TokenRows{} : cur, tsa_.get(), 0);
            // (DLIMGEDIT_DECODER_RIDE=0: measurement aid, the two launches on their own)
            static const bool ride = [] { const char* e = std::getenv("DLIMGEDIT_DECODER_RIDE"); return !e || std::atoi(e) != 0; }();
            if (!ride || !k::token_self_attention_out_with_gemm(sq_.get(), sk_.get(), sv_.get(), self_out, P, TOK, img_gemm_args(L.img_kqv, L.pos_kqv), s)) {
                k::token_self_attention_out(sq_.get(), sk_.get(), sv_.get(), self_out, P, TOK, s);
                img_gemm(L.img_kqv, L.pos_kqv);
            }
            const k::TokenRows q1 = normed(tsa_.get(), L.ln1);
            const k::TokenLinear tq = lin(rows_of(q1, true), 256, L.t2i_q, {}, nullptr, 0);
            k::token_to_image_partials(nullptr, &tq, kqv_h_.get(), 384, kqv_h_.get() + 256, 384, t2i_part_.get(), P, TOK, s);
            const k::TokenRows q2 = normed(tt2i_.get(), L.ln2);
            // (3) token MLP
            k::token_merge_linear(t2i_part_.get(), lin({}, 128, L.t2i_o, q1, tt2i_.get(), 0), L.t2i_o_t.get(),
                                  lin(q2, 256, L.mlp1, {}, tmlp_.get(), 1), P, TOK, s);
            k::TokenLinear m2 = lin(plain(tmlp_.get()), 2048, L.mlp2, q2, queries_.get(), 0);
            k::token_linears(&m2, 1, T, TOK, s);
            const k::TokenRows q3 = normed(queries_.get(), L.ln3);
            // (4) image -> tokens.  Everything else that reads the same rows q3 rides in this launch: the next layer's
            // self-attention projections, or (last layer) the query projection of the final token -> image attention.
            k::TokenLinear kv[5] = {lin(rows_of(q3, true), 256, L.i2t_k, {}, tk_.get(), 0),
                                    lin(q3, 256, L.i2t_v, {}, tv_.get(), 0)};
            int n_ops = 2;
            if (i == 0) {
                DecoderLayer const& N = W.dec_[1];
                kv[n_ops++] = lin(rows_of(q3, true), 256, N.self_attn.q, {}, sq_.get(), 0);
                kv[n_ops++] = lin(rows_of(q3, true), 256, N.self_attn.k, {}, sk_.get(), 0);
                kv[n_ops++] = lin(q3, 256, N.self_attn.v, {}, sv_.get(), 0);
            } else {
                kv[n_ops++] = lin(rows_of(q3, true), 256, W.final_q_, {}, sq_.get(), 0);
            }
            k::token_linears(kv, n_ops, T, TOK, s);
            k::image_update(kqv_h_.get() + 128, 384, tk_.get(), tv_.get(), L.i2t_o.w.get(), L.i2t_o.b.get(), L.ln4.w.get(),
                            L.ln4.b.get(), kDecLnEps, keys_.get(), keys_h_.get(), P, TOK, s);
            cur = q3;
        }
        // final token -> image attention; its fold + output projection + norm_final_attn happen in output_heads
        img_gemm(W.final_kv_, W.final_pos_kv_);
        k::token_to_image_partials(sq_.get(), nullptr, kqv_h_.get(), 256, kqv_h_.get() + 128, 256, t2i_part_.get(), P, TOK, s);

        k::HeadWeights hw;
        for (int m = 0; m < 5; ++m)
            for (int j = 0; j < 3; ++j) {
                hw.w[m][j] = W.heads_[m][j].w.get();
                hw.b[m][j] = W.heads_[m][j].b.get();
            }
        k::HqHead hq_head{};
        if (hq) {
            for (int j = 0; j < 3; ++j) {
                hq_head.w[j] = W.hq_mlp_[j].w.get();
                hq_head.b[j] = W.hq_mlp_[j].b.get();
            }
            hq_head.hyper_hq = hyper_hq_.get();
        }
        k::output_heads(t2i_part_.get(), lin({}, 128, W.final_o_, cur, nullptr, 0), W.final_o_t_.get(), normed(nullptr, W.ln_final_),
                        hw, hyper_.get(), iou_out, P, TOK, s, hq ? &hq_head : nullptr);
        // upscaling ConvT(256->64) -> LN2d -> GELU -> ConvT(64->32) -> GELU and the product with the hyper vectors
        k::upscale_logits(keys_h_.get(), W.up1_.w.get(), W.up1_.b.get(), W.up_ln_.w.get(), W.up_ln_.b.get(), kLnEps,
                          W.up2_.w.get(), W.up2_.b.get(), hyper_.get(), logits_out, P, s, hq ? hq_u_.get() : nullptr);
        if (hq) {
            // SAM-HQ: the 3x3 path on the up-scaled embedding + the image's HQ features (behind the embedding in the handle's
            // buffer), times hyper_hq, added to all four planes: everything downstream sees masks_sam + masks_hq
            float const* feat[k::kDecoderMaxPrompts];
            for (int i = 0; i < P; ++i) feat[i] = emb[i] + kEmbeddingFloats;
            k::hq_mask_path(hq_u_.get(), W.hq_mask_weights(), kLnEps, hq_mid_.get(), feat, hyper_hq_.get(), logits_out, P, s);
        }
    };
    clock_.timed(ST_DECODER, (hq ? 3.62e9 + 4.83e9 : 3.62e9) * P, body);
    HIP_CHECK(hipGetLastError());
}

GridPaint const& SamModel::segment_grid(float const* emb, float const* coords, float const* labels, int side, int pre_w, int pre_h,
                                        int iou_permille, int stability_permille) {
    DLIMG_ASSERT(side >= 1 && side <= kGridMaxSide && emb && coords && labels);
    static_assert(kGridMaxSegments == k::kGridMaxKept && sizeof(GridRecord) == k::kGridRecordInts * sizeof(int32_t), "one record, one cap");
    const int prompts = side * side, candidates = 3 * prompts;
    const int chunk = k::decoder_max_prompts(kDecTokens + (has_hq() ? 1 : 0));       // 16 prompts of 7 token rows, 14 of 8
    const size_t store_floats = (size_t)candidates * k::kGridPlaneFloats;
    if (store_floats > grid_store_.capacity() || (size_t)candidates * k::kGridRecordInts > grid_records_.capacity()) {
        HIP_CHECK(hipStreamSynchronize(stream_));              // a label map queued earlier may still read the old store
        grid_store_.reserve(store_floats);
        grid_records_.reserve((size_t)candidates * k::kGridRecordInts);
    }
    const size_t record_bytes = (size_t)candidates * sizeof(GridRecord);
    grid_host_.reserve(record_bytes + (size_t)prompts * 4 * sizeof(float));
    GridRecord* const records = static_cast<GridRecord*>(grid_host_.get());
    float* const iou4 = reinterpret_cast<float*>(static_cast<uint8_t*>(grid_host_.get()) + record_bytes);
    const std::vector<float const*> embs((size_t)chunk, emb);
    for (int p0 = 0; p0 < prompts; p0 += chunk) {
        const int n = std::min(chunk, prompts - p0);
        {
            roctx::Range rd("dlimg.decode");
            decode(embs.data(), coords + (size_t)p0 * 4, labels + (size_t)p0 * 2, n, 2, nullptr, /*handles*/ true);
        }
        roctx::Range rh("dlimg.grid_harvest");
        // every candidate plane read once and written once
        clock_.timed(ST_POST, 3.0 * n * 2 * k::kGridPlaneFloats * sizeof(float), [&] {
            k::grid_harvest(logits_.get(), n, 3 * p0, pre_w, pre_h, grid_store_.get(), candidates, grid_records_.get(), stream_);
        });
        HIP_CHECK(hipMemcpyAsync(iou4 + (size_t)p0 * 4, iou_.get(), (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost, stream_));
    }
    HIP_CHECK(hipMemcpyAsync(records, grid_records_.get(), record_bytes, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));                  // the one host round trip of a label map
    std::vector<float> iou((size_t)candidates);
    for (int c = 0; c < candidates; ++c) iou[c] = iou4[4 * (c / 3) + 1 + c % 3];
    const GridSelection chosen = select_grid_segments(records, iou.data(), candidates, iou_permille, stability_permille);
    grid_paint_.store = grid_store_.get();
    grid_paint_.candidates = candidates;
    grid_paint_.kept.count = (int)chosen.kept.size();
    for (int i = 0; i < grid_paint_.kept.count; ++i) {
        grid_paint_.kept.candidate[i] = chosen.kept[i];
        grid_paint_.kept.cull[i] = records[chosen.kept[i]].cull;
    }
    return grid_paint_;
}

k::MaskSource SamModel::prior_plane(uint8_t const* mask, int w, int h, int pre_w, int pre_h, int strength_milli) {
    DLIMG_ASSERT(mask != nullptr && w > 0 && h > 0);
    roctx::Range range("dlimg.mask_prior");
    const size_t bytes = (size_t)w * h;
    // the lane's buffer is re-used by the next prior in stream order; growing it frees memory a queued kernel may still read
    if (bytes > prior_bytes_.capacity()) {
        HIP_CHECK(hipStreamSynchronize(stream_));
        prior_bytes_.reserve(bytes);
    }
    prior_plane_.reserve((size_t)kLowRes * kLowRes);
    if (image_memory_is_pinned(mask, bytes)) {
        HIP_CHECK(hipMemcpyAsync(prior_bytes_.get(), mask, bytes, hipMemcpyHostToDevice, stream_));     // as upload_image
        HIP_CHECK(hipEventRecord(caller_copied_, stream_));
        caller_copy_pending_ = true;
    } else {
        // packed into pinned staging here and now: the caller's bytes are not read again, so they may be the memory the
        // prompt's mask is delivered to
        hipEvent_t copied = nullptr;
        uint8_t* pin = stage_rows(mask, (size_t)w, h, w, &copied);
        HIP_CHECK(hipMemcpyAsync(prior_bytes_.get(), pin, bytes, hipMemcpyHostToDevice, stream_));
        HIP_CHECK(hipEventRecord(copied, stream_));
    }
    clock_.timed(ST_POST, (double)bytes + (double)kLowRes * kLowRes * sizeof(float), [&] {
        k::mask_prior(prior_bytes_.get(), w, h, pre_w, pre_h, strength_milli, prior_plane_.get(), stream_);
    });
    HIP_CHECK(hipGetLastError());
    return k::MaskSource{prior_plane_.get(), nullptr};
}

uint8_t const* SamModel::matte_guide(uint8_t const* guide, int w, int h, int channels) {
    DLIMG_ASSERT(guide != nullptr && w > 0 && h > 0 && (channels == 1 || channels == 3 || channels == 4));
    roctx::Range range("dlimg.matte_guide");
    const size_t row = (size_t)w * channels, bytes = row * h;
    // the lane's buffer is re-used by the next guide in stream order; growing it frees memory a queued kernel may still read
    if (bytes > matte_guide_.capacity()) {
        HIP_CHECK(hipStreamSynchronize(stream_));
        matte_guide_.reserve(bytes);
    }
    if (image_memory_is_pinned(guide, bytes)) {
        HIP_CHECK(hipMemcpyAsync(matte_guide_.get(), guide, bytes, hipMemcpyHostToDevice, stream_));     // as upload_image
        HIP_CHECK(hipEventRecord(caller_copied_, stream_));
        caller_copy_pending_ = true;
    } else {
        // packed into pinned staging here and now: the caller's bytes are not read again
        hipEvent_t copied = nullptr;
        uint8_t* pin = stage_rows(guide, row, h, (int)row, &copied);
        HIP_CHECK(hipMemcpyAsync(matte_guide_.get(), pin, bytes, hipMemcpyHostToDevice, stream_));
        HIP_CHECK(hipEventRecord(copied, stream_));
    }
    return matte_guide_.get();
}

k::MaskSource SamModel::lasso_derive(uint8_t const* mask, int w, int h, int pre_w, int pre_h, int strength_milli,
                                     int32_t record[kLassoRecordInts]) {
    static_assert(kLassoRowRecordInts == k::kLassoRowInts && kLassoRows == kLowRes, "one row record, one grid");
    // upload and plane as for a prior; without the mask bit the plane is scratch, at any valid strength
    const k::MaskSource plane = prior_plane(mask, w, h, pre_w, pre_h, strength_milli > 0 ? strength_milli : kPriorDefaultStrength);
    roctx::Range range("dlimg.lasso_derive");
    constexpr size_t kCells = (size_t)kLowRes * kLowRes, kRowInts = (size_t)kLassoRows * kLassoRowRecordInts;
    lasso_scratch_.reserve(kCells + kRowInts);         // allocated once: g [256][256], then the row records
    lasso_host_.reserve(kRowInts * sizeof(int32_t));
    int32_t* const rows_dev = lasso_scratch_.get() + kCells;
    clock_.timed(ST_POST, (double)(2 * kCells + kRowInts) * sizeof(int32_t) + (double)kCells * sizeof(float), [&] {
        k::lasso_derive(plane.logits4, pre_w, pre_h, lasso_scratch_.get(), rows_dev, stream_);
    }, 2);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(lasso_host_.get(), rows_dev, kRowInts * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));          // the one host round trip of a lasso prompt
    fold_lasso_rows(static_cast<int32_t const*>(lasso_host_.get()), w, h, pre_w, pre_h, record);
    return plane;
}

void SamModel::stroke_derive(uint8_t const* map, int w, int h, int pre_w, int pre_h, int clicks, int32_t const** record) {
    static_assert(kStrokeRecordInts == k::kStrokeRecordInts && kMaxClicks == k::kStrokeMaxClicks, "one record, one limit");
    DLIMG_ASSERT(map != nullptr && record != nullptr && w > 0 && h > 0 && stroke_queued_ < kMaxClicks);
    roctx::Range range("dlimg.stroke_derive");
    const size_t bytes = (size_t)w * h;
    // the lane's buffer is re-used by the next map in stream order; growing it frees memory a queued kernel may still read
    if (bytes > stroke_bytes_.capacity()) {
        HIP_CHECK(hipStreamSynchronize(stream_));
        stroke_bytes_.reserve(bytes);
    }
    constexpr size_t kBallotInts = (size_t)k::kStrokeBallotWords * 2, kRecords = (size_t)kMaxClicks * kStrokeRecordInts;
    stroke_scratch_.reserve(kBallotInts + kRecords);           // allocated once
    stroke_host_.reserve(kRecords * sizeof(int32_t));
    if (image_memory_is_pinned(map, bytes)) {
        HIP_CHECK(hipMemcpyAsync(stroke_bytes_.get(), map, bytes, hipMemcpyHostToDevice, stream_));       // as upload_image
        HIP_CHECK(hipEventRecord(caller_copied_, stream_));
        caller_copy_pending_ = true;
    } else {
        // packed into pinned staging here and now: the caller's bytes are not read again
        hipEvent_t copied = nullptr;
        uint8_t* pin = stage_rows(map, (size_t)w, h, w, &copied);
        HIP_CHECK(hipMemcpyAsync(stroke_bytes_.get(), pin, bytes, hipMemcpyHostToDevice, stream_));
        HIP_CHECK(hipEventRecord(copied, stream_));
    }
    int32_t* const record_dev = stroke_scratch_.get() + kBallotInts + (size_t)stroke_queued_ * kStrokeRecordInts;
    int32_t* const record_host = static_cast<int32_t*>(stroke_host_.get()) + (size_t)stroke_queued_ * kStrokeRecordInts;
    clock_.timed(ST_POST, (double)bytes + 2.0 * kBallotInts * sizeof(int32_t), [&] {
        k::stroke_derive(stroke_bytes_.get(), w, h, pre_w, pre_h, clicks, reinterpret_cast<unsigned long long*>(stroke_scratch_.get()),
                         record_dev, stream_);
    }, 2);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(record_host, record_dev, kStrokeRecordInts * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    ++stroke_queued_;
    *record = record_host;
}

void SamModel::stroke_wait() {
    stroke_queued_ = 0;
    HIP_CHECK(hipStreamSynchronize(stream_));          // the one host round trip of a prompt with stroke marks
}

std::vector<std::pair<const char*, size_t>> SamModel::decoder_state_layout() { return decoder_state_layout(kDecTokens); }

std::vector<std::pair<const char*, size_t>> SamModel::decoder_state_layout(int tokens, bool with_mask_h, bool with_hq) {
    DLIMG_ASSERT(k::decoder_tokens_supported(tokens));
    const size_t T = (size_t)tokens;
    std::vector<std::pair<const char*, size_t>> parts = {
        {"tokens", T * 256}, {"final_q", T * 128}, {"self_k", T * 256}, {"self_v", T * 256}, {"self_out", T * 256},
        {"t2i_out", T * 256}, {"mlp_hidden", T * 2048}, {"queries", T * 256}, {"i2t_k", T * 128}, {"i2t_v", T * 128},
        {"final_partials", k::token_to_image_scratch_floats(1, tokens)}, {"hyper", 4 * 32}, {"iou", 4}, {"keys_head", 4096}};
    if (with_mask_h) parts.push_back({"mask_h", (size_t)kTokens * k::kMaskHidden});
    if (with_hq) parts.push_back({"hyper_hq", 32});
    return parts;
}

void SamModel::decoder_state(float* out) const { decoder_state(out, kDecTokens); }

void SamModel::decoder_state(float* out, int tokens, bool with_mask_h, bool with_hq) const {
    std::vector<float const*> src = {tokens_.get(), sq_.get(), sk_.get(), sv_.get(), tsa_.get(), tt2i_.get(), tmlp_.get(), queries_.get(),
                                     tk_.get(), tv_.get(), t2i_part_.get(), hyper_.get(), iou_.get(), keys_.get()};
    if (with_mask_h) {
        DLIMG_ASSERT(mask_h_.capacity() >= (size_t)kTokens * k::kMaskHidden);
        src.push_back(mask_h_.get());
    }
    if (with_hq) {
        DLIMG_ASSERT(hyper_hq_.capacity() >= 32);
        src.push_back(hyper_hq_.get());
    }
    size_t off = 0, i = 0;
    for (auto const& part : decoder_state_layout(tokens, with_mask_h, with_hq)) {
        HIP_CHECK(hipMemcpy(out + off, src[i++], part.second * sizeof(float), hipMemcpyDeviceToHost));
        off += part.second;
    }
}

// ---------------------------------------------------------------------------------------------
// encoder diagnostics: read-only views of the workspaces and of the loaded operands

namespace {

void download_widened(float* out, half_t const* h, float const* f, size_t n, std::vector<half_t>& tmp) {
    if (!n) return;
    if (f) {
        HIP_CHECK(hipMemcpy(out, f, n * sizeof(float), hipMemcpyDeviceToHost));
        return;
    }
    tmp.resize(n);
    HIP_CHECK(hipMemcpy(tmp.data(), h, n * sizeof(half_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) out[i] = (float)tmp[i];
}

}  // namespace

// The tile column blocks of the pass's last stream writer (fc2 of the last block): the arguments encode() gives that launch,
// through the same planner call.  A RECOMPUTATION, not a record of what the launch used (encode() keeps the number in a local):
// it follows encode() only as long as the arguments below restate writes_stream / stream_residual there.  What holds the
// statistics' layout to the launch itself is the comparison of their values (gemm_ref.check_statistics at bn = 256).
int SamModel::encoder_stat_groups(int batch) const {
    SamWeights const& W = *weights_;
    if (!W.fused_ln_) return 0;
    const int D = W.geom_.embed_dim, mlp = W.geom_.mlp_dim, M = batch * kTokens;
    LinearH const& fc2 = W.layers_.back().fc2;
    k::GemmArgs a;
    a.A = hid_.get(); a.lda = mlp; a.W = fc2.w.get(); a.ldw = mlp; a.bias = fc2.b.get(); a.K = mlp;
    if (split_stream_) { a.resid_h = xn_.get(); a.resid_l = xlo_.get(); a.ldrs = D; a.out_l = xlo_.get(); }
    else { a.resid = x_.get(); a.ldr = D; a.out_f32 = x_.get(); a.ldc32 = D; }
    a.resid_mod = M; a.M = M; a.N = D;
    a.out_h = xn_.get(); a.ldc16 = D; a.stats_out = xstat_.get();
    plan_inputs(a, shared_gpu_, alone_);
    return D / k::gemm_choose_tile(a);
}

std::vector<std::pair<std::string, size_t>> SamModel::encoder_state_layout(int batch) const {
    DLIMG_ASSERT(batch > 0 && batch <= enc_batch_);
    const size_t T = kTokens, D = weights_->geom_.embed_dim, mlp = weights_->geom_.mlp_dim;
    return {{"patches", T * kPatchK}, {"stream_hi", T * D}, {"stream_lo", T * D}, {"stats", (size_t)encoder_stat_groups(batch) * T * 2},
            {"qkv", T * 3 * D}, {"hidden", T * mlp}, {"embedding", T * kEmbedDim}, {"groups", 1}, {"split", 1}, {"nonfinite", 1}};
}

void SamModel::encoder_state(float* out, int image, int batch) const {
    DLIMG_ASSERT(out != nullptr && batch > 0 && batch <= enc_batch_ && image >= 0 && image < batch && pass_flag_ != nullptr);
    const size_t T = kTokens, D = weights_->geom_.embed_dim, mlp = weights_->geom_.mlp_dim, M = (size_t)batch * T, row0 = (size_t)image * T;
    const int groups = encoder_stat_groups(batch);
    std::vector<half_t> tmp;
    size_t off = 0;
    auto take = [&](half_t const* h, float const* f, size_t n) { download_widened(out + off, h, f, n, tmp); off += n; };
    take(patches_.get() + row0 * kPatchK, nullptr, T * kPatchK);
    float* const hi = out + off;
    take(xn_.get() + row0 * D, nullptr, T * D);
    float* const lo = out + off;
    if (split_stream_) {
        take(xlo_.get() + row0 * D, nullptr, T * D);
    } else {
        take(nullptr, x_.get() + row0 * D, T * D);
        for (size_t i = 0; i < T * D; ++i) lo[i] -= hi[i];
    }
    for (int g = 0; g < groups; ++g) take(nullptr, xstat_.get() + ((size_t)g * M + row0) * 2, T * 2);
    take(qkv_.get() + row0 * 3 * D, nullptr, T * 3 * D);
    take(hid_.get() + row0 * mlp, nullptr, T * mlp);
    take(nullptr, emb_.get() + row0 * kEmbedDim, T * kEmbedDim);
    out[off++] = (float)groups;
    out[off++] = split_stream_ ? 1.f : 0.f;
    out[off++] = (float)*pass_flag_;
}

std::vector<SamModel::DeviceTap> SamModel::encoder_operand_taps(int layer) const {
    SamWeights const& W = *weights_;
    DLIMG_ASSERT(layer >= -1 && layer < (int)W.layers_.size());
    const size_t D = W.geom_.embed_dim, mlp = W.geom_.mlp_dim, hd = W.geom_.head_dim();
    const size_t folded = W.fused_ln_ ? 1 : 0;
    if (layer < 0)
        return {{"patch.w", W.patch_.w.get(), nullptr, D * kPatchK}, {"patch.b", nullptr, W.patch_.b.get(), D},
                {"pos_embed", nullptr, W.pos_embed_.get(), (size_t)kTokens * D},
                {"neck1.w", W.neck1_.w.get(), nullptr, (size_t)kEmbedDim * D},
                {"neck_ln1.w", nullptr, W.neck_ln1_.w.get(), kEmbedDim}, {"neck_ln1.b", nullptr, W.neck_ln1_.b.get(), kEmbedDim},
                {"neck2.w", W.neck2_.w.get(), nullptr, (size_t)kEmbedDim * 9 * kEmbedDim},
                {"neck_ln2.w", nullptr, W.neck_ln2_.w.get(), kEmbedDim}, {"neck_ln2.b", nullptr, W.neck_ln2_.b.get(), kEmbedDim}};
    EncoderLayer const& L = W.layers_[layer];
    const size_t rel = (size_t)(2 * (L.global ? 64 : 14) - 1) * hd;
    return {{"qkv.w", L.qkv.w.get(), nullptr, 3 * D * D}, {"qkv.b", nullptr, L.qkv.b.get(), 3 * D},
            {"qkv.colsum", nullptr, L.qkv.colsum.get(), folded * 3 * D},
            {"fc1.w", L.fc1.w.get(), nullptr, mlp * D}, {"fc1.b", nullptr, L.fc1.b.get(), mlp},
            {"fc1.colsum", nullptr, L.fc1.colsum.get(), folded * mlp},
            {"proj.w", L.proj.w.get(), nullptr, D * D}, {"proj.b", nullptr, L.proj.b.get(), D},
            {"fc2.w", L.fc2.w.get(), nullptr, D * mlp}, {"fc2.b", nullptr, L.fc2.b.get(), D},
            {"rel_h16", L.rel_h16.get(), nullptr, rel}, {"rel_w16", L.rel_w16.get(), nullptr, rel},
            {"qkv_pad", L.qkv_pad.get(), nullptr, L.global ? 0 : 3 * D}, {"global", nullptr, nullptr, 1}};
}

std::vector<std::pair<std::string, size_t>> SamModel::encoder_operands_layout(int layer) const {
    std::vector<std::pair<std::string, size_t>> parts;
    for (DeviceTap const& t : encoder_operand_taps(layer)) parts.emplace_back(t.name, t.n);
    return parts;
}

void SamModel::encoder_operands(float* out, int layer) const {
    DLIMG_ASSERT(out != nullptr);
    std::vector<half_t> tmp;
    size_t off = 0;
    for (DeviceTap const& t : encoder_operand_taps(layer)) {
        if (t.name == "global") out[off] = weights_->layers_[layer].global ? 1.f : 0.f;
        else download_widened(out + off, t.h, t.f, t.n, tmp);
        off += t.n;
    }
}

void SamModel::masks_on_device(k::PostJob const* jobs, int count) {
    if (count <= 0) return;
    double bytes = 0;
    for (int i = 0; i < count; ++i) bytes += (double)kLowRes * kLowRes * 4 + (double)jobs[i].out_w * jobs[i].out_h;
    clock_.timed(ST_POST, bytes, [&] { k::postprocess_masks(jobs, count, stream_); });
    mark_activity();
}

void SamModel::masks_to_host(k::PostJob const* jobs, int count) {
    MaskSlotLease lease(*this);
    enqueue_masks(lease.slot(), jobs, count, 0);
    finish_masks(lease.slot(), jobs, count, nullptr, 0);
}

}  // namespace dlimg
