#include "segmentation.hpp"

#include "edge_plan.hpp"
#include "grid_plan.hpp"
#include "lasso_plan.hpp"
#include "matte_plan.hpp"
#include "prior_plan.hpp"
#include "prompt_plan.hpp"
#include "roctx.hpp"
#include "stroke_plan.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <exception>
#include <future>
#include <thread>
#include <vector>

namespace dlimg {

int channel_bytes(int channels) { return channels > 4 ? 4 : channels; }

int pack_prompt(ResizeLongestSide const& rs, Point const* point, Region const* region, float* coords, float* labels) {
    DLIMG_ASSERT(point != nullptr || region != nullptr);
    // a call of one entry: its click when there is a point, its box when there is a region
    PromptSpec spec;
    spec.clicks = point ? 1 : 0;
    spec.box = region != nullptr;
    const int points[2] = {point ? point->x : 0, point ? point->y : 0};
    int regions[4] = {0, 0, 0, 0};
    if (region) {
        regions[0] = region->top_left.x; regions[1] = region->top_left.y;
        regions[2] = region->bottom_right.x; regions[3] = region->bottom_right.y;
    }
    return pack_points(rs, spec, unmarked_stages(spec), spec.clicks, points, regions, coords, labels);
}

// The prompts of a batch call, packed: prompt j's points start at point at[j] of coords / labels.  A staged prompt (stages[j]
// has more than one stage) is packed as its last stage, all of its clicks.
struct BatchPrompts {
    std::vector<PromptSpec> prompts;
    std::vector<PromptStages> stages;
    std::vector<CleanSpec> clean;      // [prompt]: what its clean-up mark asks for (nothing without one)
    bool any_clean = false;
    std::vector<GridSpec> grid;        // [prompt]: side > 0: a grid prompt (grid_plan.hpp); its packed points are not used
    std::vector<PriorSpec> prior;      // [prompt]: what its prior mark says (prior_plan.hpp; nothing without one)
    std::vector<uint8_t const*> prior_mask;    // [prompt]: the prior itself, out_masks[] of the mark's entry (null without one)
    std::vector<LassoSpec> lasso;      // [prompt]: what its lasso mark says (lasso_plan.hpp; nothing without one); its packed points
                                       // are written once its click and box are derived (decode_batch_on)
    std::vector<uint8_t const*> lasso_mask;    // [prompt]: the selection, out_masks[] of the mark's entry (null without one)
    std::vector<MatteSpec> matte;      // [prompt]: what its matte mark says (matte_plan.hpp; nothing without one)
    std::vector<uint8_t const*> matte_guide;   // [prompt]: the guide, out_masks[] of the mark's entry (null without one)
    bool any_matte = false;
    std::vector<CutoutSpec> cutout;    // [prompt]: what its cut-out mark says (cutout_plan.hpp; nothing without one)
    std::vector<uint8_t*> cutout_dst;  // [prompt]: where its RGBA goes, out_masks[] of the mark's entry (null without one)
    std::vector<EdgeSpec> edge;        // [prompt]: what its edge mark says (edge_plan.hpp; nothing without one)
    bool any_edge = false;
    std::vector<std::vector<StrokeSpec>> strokes;      // [prompt]: its stroke marks (stroke_plan.hpp; none without one); its packed
                                                       // points are written once their clicks are derived (decode_batch_on)
    std::vector<std::vector<uint8_t const*>> stroke_map;       // [prompt][mark]: the map, out_masks[] of the mark's entry
    // A call with stroke marks is REWRITTEN (stroke_plan.hpp): every list above numbers the entries of these arrays, which the
    // batch call goes on with in place of the caller's; entry_of[e] is the caller's entry, for what is reported.  Empty otherwise.
    std::vector<int> entry_of;
    std::vector<SegmentationImpl const*> segs;
    std::vector<int> points, regions;
    std::vector<uint8_t*> out_masks;                   // a placeholder click's: its mark's map
    int* derived_points = nullptr;                     // `points`, where decode_batch_on writes what the marks of a prompt derive
    bool rewritten() const { return !entry_of.empty(); }
    int caller_entry(int e) const { return rewritten() ? entry_of[e] : e; }
    std::vector<size_t> at;
    std::vector<float> coords, labels;
};

namespace {
constexpr int kPromptChunk = 8;          // prompts of one decode of a batch call, at most (prompt_plan.hpp)

// out_masks: the call's per-entry pointers, which a prior mark's prior is read from; null: the device form, which has none
BatchPrompts read_batch_prompts(SegmentationImpl const* const* segs, int count, int const* points, int const* regions,
                                uint8_t* const* out_masks) {
    std::vector<char> has_handle(count), has_pointer(count), same_as_head(count);
    SegmentationImpl const* any = nullptr;
    for (int i = 0, head = -1; i < count; ++i) {
        has_handle[i] = segs[i] != nullptr;
        has_pointer[i] = out_masks && out_masks[i] != nullptr;
        if (has_handle[i]) head = i;
        same_as_head[i] = has_pointer[i] && head >= 0 && head != i && out_masks[i] == out_masks[head];
        if (!any) any = segs[i];
    }
    BatchPrompts b;
    {
        // a mark needs the mask branch of the model; the environment's replicas share one model file
        const bool mask_branch = any && any->environment().lane(any->replica(), 0).has_mask_branch();
        EdgePlannedPrompts with_edges = plan_edge_prompts(has_handle, points != nullptr, regions, mask_branch, has_pointer,
                                                          /*device_form*/ out_masks == nullptr, same_as_head);
        b.edge = std::move(with_edges.edge);
        b.any_edge = with_edges.any_edge;
        CutoutPlannedPrompts& with_cutouts = with_edges.inner;
        b.cutout = std::move(with_cutouts.cutout);
        for (CutoutSpec const& c : b.cutout) b.cutout_dst.push_back(c.any() ? out_masks[c.entry] : nullptr);
        StrokePlannedPrompts& with_strokes = with_cutouts.inner;
        b.strokes = std::move(with_strokes.strokes);
        for (std::vector<StrokeSpec> const& marks : b.strokes) {
            b.stroke_map.emplace_back();
            for (StrokeSpec const& s : marks) b.stroke_map.back().push_back(out_masks[s.entry]);
        }
        if (with_strokes.any_stroke) {
            // from here on the call is the rewritten one: a placeholder click has no point yet
            b.entry_of = std::move(with_strokes.entry_of);
            b.regions = std::move(with_strokes.regions);
            for (size_t e = 0; e < b.entry_of.size(); ++e) {
                const int from = b.entry_of[e];
                b.segs.push_back(with_strokes.handles[e] ? segs[from] : nullptr);
                b.out_masks.push_back(out_masks[from]);
                const bool own = points && !with_strokes.derived[e];
                b.points.push_back(own ? points[2 * from] : 0);
                b.points.push_back(own ? points[2 * from + 1] : 0);
            }
            b.derived_points = b.points.data();
            segs = b.segs.data();
            points = b.points.data();
            regions = b.regions.data();
            out_masks = b.out_masks.data();
        }
        MattePlannedPrompts& with_mattes = with_strokes.inner;
        b.matte = std::move(with_mattes.matte);
        b.any_matte = with_mattes.any_matte;
        for (MatteSpec const& m : b.matte) b.matte_guide.push_back(m.any() ? out_masks[m.entry] : nullptr);
        LassoPlannedPrompts& with_lassos = with_mattes.inner;
        PriorPlannedPrompts& with_priors = with_lassos.inner;
        b.lasso = std::move(with_lassos.lasso);
        for (LassoSpec const& l : b.lasso) b.lasso_mask.push_back(l.any() ? out_masks[l.entry] : nullptr);
        GridPlannedPrompts& planned = with_priors.planned;
        CleanedPrompts& plan = planned.cleaned;
        b.prior = std::move(with_priors.prior);
        for (PriorSpec const& p : b.prior) b.prior_mask.push_back(p.any() ? out_masks[p.entry] : nullptr);
        b.grid = std::move(planned.grid);
        b.prompts = std::move(plan.staged.prompts);
        b.stages = std::move(plan.staged.stages);
        b.clean = std::move(plan.clean);
        b.any_clean = plan.any_clean;
        // a SAM-HQ model takes one point less (its HQ token is a token row): refused here, before any prompt of the call is launched
        if (any)
            for (size_t j = 0; j < b.prompts.size(); ++j) {
                const std::string why = any->environment().lane(any->replica(), 0).hq_refusal(b.prompts[j].points());
                if (why.empty()) continue;
                if (b.strokes[j].empty()) throw Exception(why);
                throw Exception("mask batch: entry " + std::to_string(b.strokes[j].back().entry) + ": the clicks a stroke mark stands for "
                                "count: " + why);
            }
    }
    size_t total = 0;
    for (PromptSpec const& p : b.prompts) {
        b.at.push_back(total);
        total += p.points();
    }
    b.coords.resize(total * 2);
    b.labels.resize(total);
    for (size_t j = 0; j < b.prompts.size(); ++j)
        // (a grid prompt's points are its grid's: pack_grid; a lasso prompt's and a stroke prompt's are derived)
        if (!b.grid[j].any() && !b.lasso[j].any() && b.strokes[j].empty())
            pack_points(segs[b.prompts[j].head]->geometry(), b.prompts[j], b.stages[j], b.prompts[j].clicks, points, regions,
                        &b.coords[b.at[j] * 2], &b.labels[b.at[j]]);
    return b;
}
// What one GPU decodes: its unstaged prompts in chunks as plan_prompt_chunks cuts them, then every staged prompt as a chunk
// of its own (its stages run one after the other on one lane; equal stages of several prompts are not batched).  A prompt with
// a prior is decoded the way a staged prompt is, whether it has refinement marks or not: its first stage takes a mask input.
// So is a prompt with a lasso mark: its click and box are derived on the lane in front of its stages.  And so is a prompt with
// a matte mark: its guide is uploaded on the lane in front of its decode.  And so is a prompt with stroke marks: the clicks they
// stand for are derived on the lane in front of its stages.
// A grid prompt is a chunk of its own too, behind those: its side * side decodes and its label map run on one lane.
struct BatchWork { PromptChunk part; bool staged; bool grid = false; };
std::vector<BatchWork> plan_batch_work(BatchPrompts const& b, std::vector<int> const& mine, int chunk) {
    std::vector<int> plain;
    for (int j : mine)
        if (!b.stages[j].staged() && !b.prior[j].any() && !b.lasso[j].any() && !b.matte[j].any() && b.strokes[j].empty() && !b.grid[j].any())
            plain.push_back(j);
    std::vector<BatchWork> work;
    for (PromptChunk& part : plan_prompt_chunks(b.prompts, plain, chunk)) work.push_back(BatchWork{std::move(part), false});
    for (int j : mine)
        if (b.stages[j].staged() || b.prior[j].any() || b.lasso[j].any() || b.matte[j].any() || !b.strokes[j].empty())
            work.push_back(BatchWork{PromptChunk{b.prompts[j].points(), {j}}, true});
    for (int j : mine)
        if (b.grid[j].any()) work.push_back(BatchWork{PromptChunk{b.prompts[j].points(), {j}}, false, true});
    return work;
}
// The side * side prompts of a grid over an image, each packed exactly as a one-click prompt at its pixel is (click, padding
// point): coords [side * side][2][2], labels [side * side][2].
void pack_grid(ResizeLongestSide const& rs, int side, std::vector<float>& coords, std::vector<float>& labels) {
    PromptSpec spec;
    spec.clicks = 1;
    const PromptStages stages = unmarked_stages(spec);
    coords.resize((size_t)side * side * 4);
    labels.resize((size_t)side * side * 2);
    for (int j = 0; j < side; ++j)
        for (int i = 0; i < side; ++i) {
            const Point at = grid_pixel(rs.original.width, rs.original.height, side, i, j);
            const int click[2] = {at.x, at.y};
            const size_t p = (size_t)j * side + i;
            pack_points(rs, spec, stages, 1, click, nullptr, &coords[p * 4], &labels[p * 2]);
        }
}
// The stages of staged prompt j in front of its last one, decoded on `model` (mutex held) one after the other; returns the
// mask input of the last stage: the plane the stage before it would deliver, where that decode left it.  first: the mask input
// of the first stage -- the plane of the prompt's prior, or {nullptr, nullptr} when it has none -- which is what comes back
// when the prompt has one stage only.
// spec, st, points, regions: the prompt and the arrays its clicks and box are read from -- the call's, or those of a lasso prompt
// with its derived click and box written in (lasso_prompt_arrays).
k::MaskSource run_early_stages(SamModel& model, PromptSpec const& spec, PromptStages const& st, float const* emb,
                               ResizeLongestSide const& rs, int const* points, int const* regions, k::MaskSource first) {
    float coords[2 * k::kDecoderMaxPoints], labels[k::kDecoderMaxPoints];
    k::MaskSource src = first;
    for (size_t s = 0; s + 1 < st.stage_clicks.size(); ++s) {
        const int npts = pack_points(rs, spec, st, st.stage_clicks[s], points, regions, coords, labels);
        model.decode(&emb, coords, labels, 1, npts, src.logits4 ? &src : nullptr, /*handles*/ true);
        // single_mask_job's rule: the best of planes 1..3 for a two-point stage, plane 0 otherwise
        src = k::MaskSource{model.logits(), npts > 2 ? nullptr : model.iou()};
    }
    return src;
}
// the prompts of one chunk, tightly packed for SamModel::decode
void gather_chunk(BatchPrompts const& b, PromptChunk const& chunk, std::vector<float>& cc, std::vector<float>& ll) {
    const int npts = chunk.points;
    cc.resize(chunk.prompts.size() * npts * 2);
    ll.resize(chunk.prompts.size() * npts);
    for (size_t j = 0; j < chunk.prompts.size(); ++j) {
        const size_t at = b.at[chunk.prompts[j]];
        std::copy_n(&b.coords[at * 2], npts * 2, &cc[j * npts * 2]);
        std::copy_n(&b.labels[at], npts, &ll[j * npts]);
    }
}
}  // namespace

void check_image(dlimg_ImageView const& image) {
    if (!image.pixels) throw Exception("Image has no pixel data");
    if (image.width <= 0 || image.height <= 0) throw Exception("Image extent must be positive");
    const int c = image.channels;
    if (!(c == 1 || c == 3 || c == 4 || c == 5 || c == 6))
        throw Exception("Unsupported channel order [" + std::to_string(c) + "]");
    DLIMG_ASSERT(image.stride >= image.width * channel_bytes(c));
}

namespace {
constexpr const char* kOverflowMessage =
    "the image encoder produced non-finite values: an activation left the f16 range (65504) of this build's MFMA operands "
    "and residual stream -- the embedding is refused (no masks are computed from it)";

// process() of one image leaves the wait to the first call that needs the embedding (segmentation.hpp)
bool deferred_process() {
    const char* e = std::getenv("DLIMGEDIT_SYNC_PROCESS");       // read per call: a deployer's switch, and the tests'
    return !(e && std::atoi(e) != 0);
}
}  // namespace

SegmentationImpl::SegmentationImpl(EnvironmentImpl& env) : env_(env) {
    env.load_all();     // loads the model (and reports a missing weight file) at the same point as the reference
}

SegmentationImpl::~SegmentationImpl() {
    forget_pending();                            // the pass still writes the buffer that goes back to the pool
    if (pool_) pool_->give(embedding_);
}

std::shared_ptr<SamModel::DeferredPass> SegmentationImpl::pending() const {
    std::lock_guard<std::mutex> lock(pending_mutex_);
    return pending_;
}

void SegmentationImpl::settle() const {
    if (auto p = pending()) {
        std::exception_ptr failed;
        try {
            if (p->settle()) invalid_ = true;
        } catch (...) {
            invalid_ = true;                     // the wait itself failed: nothing is known about the embedding
            failed = std::current_exception();
        }
        {
            std::lock_guard<std::mutex> lock(pending_mutex_);
            if (pending_ == p) pending_.reset();
        }
        if (failed) std::rethrow_exception(failed);
    }
    if (invalid_) throw Exception(kOverflowMessage);
}

void SegmentationImpl::forget_pending() noexcept {
    try {
        if (auto p = pending()) p->settle();
    } catch (...) {
    }
    std::lock_guard<std::mutex> lock(pending_mutex_);
    pending_.reset();
    invalid_ = false;
}

float* SegmentationImpl::embedding_storage(int replica) {
    if (embedding_ && replica != replica_) {
        pool_->give(embedding_);
        embedding_ = nullptr;
    }
    replica_ = replica;
    if (!embedding_) {
        pool_ = env_.embedding_pool(replica);
        embedding_ = pool_->take(handle_floats(env_.lane(replica, 0).has_hq()));
    }
    return embedding_;
}

namespace {

// Brings one host image into slot `slot` of the model's patch matrix (resizing on the device when
// the longest side is not 1024; reference: ResizeLongestSide::resize, segmentation.cpp:60-70).
void stage_image(SamModel& model, int slot, int batch, dlimg_ImageView const& image, ResizeLongestSide const& rs) {
    if (rs.scale != 1) {
        model.upload_and_resize_image(slot, batch, image.pixels, image.width, image.height, image.stride,
                                      image.channels, rs.resized.width, rs.resized.height);
    } else {
        model.upload_image(slot, batch, image.pixels, image.width, image.height, image.stride, image.channels);
    }
}

// Runs body(replica) for every replica in `used`: inline when there is one; otherwise the calling thread takes the first
// replica itself and hands the others to helper threads of ITS OWN (staging copies and kernel launches of different GPUs
// then proceed side by side).  The helpers are kept per calling thread and reused from call to call (r06; until then every
// call created and joined G threads): a caller's helpers serve nobody else, so concurrent callers never wait for each
// other here, and a helper that serves GPU g is bound to the CPUs of that GPU's NUMA node the first time it does
// (environment.cpp, bind_thread_near_device; DLIMGEDIT_NUMA_AFFINITY=0 switches that off).  The first exception wins.
struct ReplicaHelpers {
    std::vector<std::unique_ptr<LaneWorker>> workers;       // [helper]: joined when the calling thread ends
    std::vector<int> bound_to;                              // device the helper's thread was last bound near (-1: none)
};
template <typename F> void for_each_replica(EnvironmentImpl& env, std::vector<int> const& used, F&& body) {
    if (used.size() == 1) {
        body(used[0]);
        return;
    }
    thread_local ReplicaHelpers helpers;
    const size_t n_help = used.size() - 1;
    while (helpers.workers.size() < n_help) {
        helpers.workers.push_back(std::make_unique<LaneWorker>());
        helpers.bound_to.push_back(-1);
    }
    std::vector<std::future<void>> answers;
    for (size_t t = 0; t < n_help; ++t) {
        const int replica = used[t + 1], device = env.device_of(replica);
        const bool bind = helpers.bound_to[t] != device;
        helpers.bound_to[t] = device;
        answers.push_back(post_with_result(*helpers.workers[t], [&body, replica, device, bind] {
            if (bind) bind_thread_near_device(device);
            body(replica);
        }));
    }
    std::exception_ptr first;
    try {
        body(used[0]);
    } catch (...) {
        first = std::current_exception();
    }
    wait_for_all(answers, first, [](size_t) {}, [](size_t) {});
}

// overflow: the pass's report (SamModel::last_pass_flag), read once its event has been waited for
struct Waiting { SamModel* model; hipEvent_t done; const volatile int* overflow; };


// Error paths: a request that threw half-way may have queued kernels or copies that still write into buffers the
// caller is about to hand back (pooled embedding buffers, mask staging slots).  Everything queued on that lane runs
// to completion first; errors of the drain itself are not interesting any more.
void drain_lane(SamModel* model) noexcept {
    if (!model) return;
    try {
        std::lock_guard<std::mutex> lock(model->mutex());
        (void)hipSetDevice(model->device());
        model->synchronize();
    } catch (...) {
    }
}

void wait_all(std::vector<Waiting>& waiting) {
    std::exception_ptr first;
    for (auto& w : waiting) {
        try {
            w.model->wait_and_recycle(w.done);
            if (w.overflow && *w.overflow) {
                *const_cast<volatile int*>(w.overflow) = 0;      // reported here, once
                throw Exception(kOverflowMessage);
            }
        } catch (...) {
            if (!first) first = std::current_exception();
        }
    }
    waiting.clear();
    if (first) std::rethrow_exception(first);
}

}  // namespace

void SegmentationImpl::process(dlimg_ImageView const& image) {
    SegmentationImpl* self = this;
    process_batch(env_, &self, &image, 1);
}

// Independent images: image i goes to replica (GPU) r0 + i mod G and there to the next execution lane, as its own
// batch-1 pass -- upload, pre-processing and encoder of one image overlap those of the others on the lanes' streams,
// and the host copies of image i+1 run while image i is on the GPU.  Nothing is exchanged between GPUs.
void SegmentationImpl::process_batch(EnvironmentImpl& env, SegmentationImpl* const* segs, dlimg_ImageView const* images,
                                     int count) {
    if (count <= 0) return;
    for (int i = 0; i < count; ++i) {
        check_image(images[i]);
        segs[i]->forget_pending();               // a handle processed again: its earlier pass writes the same buffer
        segs[i]->image_size_.set(Extent{images[i].width, images[i].height});
    }
    const bool defer = count == 1 && deferred_process();
    const int G = env.replica_count();
    std::vector<int> replica_of(count), used;
    for (int i = 0; i < count; ++i) {
        replica_of[i] = env.next_replica();
        if (std::find(used.begin(), used.end(), replica_of[i]) == used.end()) used.push_back(replica_of[i]);
    }
    (void)G;
    static const bool trace = std::getenv("DLIMGEDIT_TIMING") != nullptr;     // diagnostic: host time of the two phases
    // Images per batched encoder pass.  Results do not depend on it (gemm_plan.cpp: the tiles a pass may use compute
    // the same bits); throughput does: every lane should get a pass, and passes of two or more images run the N = 768
    // GEMMs on 256 x 256 tiles (8 images through one host thread, ViT-B: 601 images/s as 2 x 4, 649 as 8 x 1, 674 as
    // 4 x 2).  Default: the GPU's share spread over its lanes, at most 4 per pass -- unless other threads have batch calls
    // in flight, which keep the other lanes busy anyway: then fewer, larger passes win (4 threads x 8 images: 685 images/s
    // with passes of 2, 736 with passes of 4).  DLIMGEDIT_ENCODE_BATCH overrides (1..16).
    static const int forced_chunk = [] {
        const char* e = std::getenv("DLIMGEDIT_ENCODE_BATCH");
        const int v = e ? std::atoi(e) : 0;
        return v < 0 ? 0 : (v > 16 ? 16 : v);
    }();
    struct InFlight {
        std::atomic<int>& n;
        int before;
        explicit InFlight(std::atomic<int>& c) : n(c), before(c.fetch_add(1)) {}
        ~InFlight() { n.fetch_sub(1); }
    } in_flight(env.batch_calls_in_flight);
    const bool alone = in_flight.before == 0;    // no other batch call is being worked on right now
    for_each_replica(env, used, [&](int replica) {
        HIP_CHECK(hipSetDevice(env.device_of(replica)));
        std::vector<Waiting> waiting;
        SamModel* enqueueing = nullptr;          // the lane whose request is being put together (error path: drained)
        const auto t0 = std::chrono::steady_clock::now();
        try {
            std::vector<int> mine;
            for (int i = 0; i < count; ++i)
                if (replica_of[i] == replica) mine.push_back(i);
            // chunks of up to `chunk` images: one batched pass per chunk on the next lane
            const size_t lanes = (size_t)std::max(1, env.effective_lane_count(replica));
            const size_t spread = std::max<size_t>(1, (mine.size() + lanes - 1) / lanes);     // one pass per lane
            const size_t chunk = forced_chunk ? (size_t)forced_chunk
                                 : alone      ? std::min<size_t>(4, spread)
                                              : std::min<size_t>(4, std::max(spread, (mine.size() + 1) / 2));
            // One pass: the chunk's images staged (host copy + upload) and encoded on `model`; returns the event behind it.
            struct Queued { hipEvent_t done; const volatile int* overflow; std::shared_ptr<SamModel::DeferredPass> deferred; };
            auto run_chunk = [&](SamModel& model, size_t base, int n) {
                std::vector<float*> emb(n);
                for (int j = 0; j < n; ++j) emb[j] = segs[mine[base + j]]->embedding_storage(replica);
                roctx::Range range("dlimg.process");
                std::lock_guard<std::mutex> lock(model.mutex());
                HIP_CHECK(hipSetDevice(model.device()));
                {
                    roctx::Range r("dlimg.pre");
                    for (int j = 0; j < n; ++j) {
                        const int i = mine[base + j];
                        stage_image(model, j, n, images[i], segs[i]->image_size_);
                    }
                }
                {
                    roctx::Range r("dlimg.encode");
                    model.encode(n, emb.data());
                }
                model.wait_caller_copies();       // pixels read in place (pinned image memory): theirs again when this returns
                if (defer) return Queued{nullptr, nullptr, model.defer_last_pass()};
                const volatile int* overflow = model.last_pass_flag();
                return Queued{model.completion(), overflow, nullptr};
            };
            const size_t chunks = (mine.size() + chunk - 1) / chunk;
            if (chunks > 1 && alone && env.use_step_workers) {
                // several passes and no other caller at work: each pass is put together by its lane's own host thread
                // (LaneWorker) -- packing and uploading the images and ~75 launches per pass take 0.5-1 ms of host time,
                // which one thread would spend lane after lane while the later lanes' part of the chip waits (8 images
                // from one thread: 718 -> 734 images/s).  With several callers the lanes are fed in parallel anyway and
                // the hand-over only costs (two threads x 8 images: 846 without, 824 with)
                std::vector<SamModel*> lanes_used;
                std::vector<std::future<Queued>> answers;
                for (size_t base = 0; base < mine.size(); base += chunk) {
                    const int n = (int)std::min<size_t>(chunk, mine.size() - base);
                    SamModel* model = &env.next_lane(replica);
                    lanes_used.push_back(model);
                    answers.push_back(post_with_result(env.lane_worker(replica, model->lane_index()),
                                                       [&run_chunk, model, base, n] { return run_chunk(*model, base, n); }));
                }
                wait_for_all(
                    answers, nullptr, [&](size_t i, Queued q) { waiting.push_back(Waiting{lanes_used[i], q.done, q.overflow}); },
                    [&](size_t i) { drain_lane(lanes_used[i]); });     // whatever the failed pass queued runs to completion first
            } else {
                for (size_t base = 0; base < mine.size(); base += chunk) {
                    const int n = (int)std::min<size_t>(chunk, mine.size() - base);
                    SamModel& model = env.next_lane(replica);
                    enqueueing = &model;
                    const Queued q = run_chunk(model, base, n);
                    enqueueing = nullptr;
                    if (q.deferred) {
                        // the caller's thread goes back now; the first mask query is queued behind the pass and waits
                        std::lock_guard<std::mutex> lock(segs[mine[base]]->pending_mutex_);
                        segs[mine[base]]->pending_ = q.deferred;
                    } else {
                        waiting.push_back(Waiting{&model, q.done, q.overflow});
                    }
                }
            }
        } catch (...) {
            // the chunk that threw has no completion event: whatever it queued (it writes the handles' embedding
            // buffers, which their destructors return to the pool) is waited for on its stream
            drain_lane(enqueueing);
            try { wait_all(waiting); } catch (...) {}
            throw;
        }
        // process() is synchronous in the reference (Ort::Session::Run returns when the result is there).  A batch is
        // waited for here and its errors surface in this call; one image is left to its first query (segmentation.hpp).
        const auto t1 = std::chrono::steady_clock::now();
        wait_all(waiting);
        if (trace) {
            const auto t2 = std::chrono::steady_clock::now();
            std::fprintf(stderr, "process_batch replica %d: enqueue %.3f ms, wait %.3f ms\n", replica,
                         std::chrono::duration<double, std::milli>(t1 - t0).count(),
                         std::chrono::duration<double, std::milli>(t2 - t1).count());
        }
    });
}

void SegmentationImpl::compute_mask(Point const* point, Region const* region, uint8_t* const out_masks[3],
                                    float out_accuracy[3]) const {
    DLIMG_ASSERT(point || region);
    DLIMG_ASSERT(embedding_ != nullptr);
    if (invalid_) throw Exception(kOverflowMessage);
    // a two-point prompt always: a given point wins and the region is ignored (reference: segmentation.cpp:146-152);
    // the three-point form of pack_prompt belongs to the batch calls
    if (point) region = nullptr;
    float coords[4], labels[2];
    const int npts = pack_prompt(image_size_, point, region, coords, labels);
    DLIMG_ASSERT(npts == 2);
    const bool is_single_mask = out_masks[1] == nullptr;
    if (is_single_mask) {
        DLIMG_ASSERT(out_masks[0] != nullptr);
    } else {
        for (int i = 0; i < 3; ++i) DLIMG_ASSERT(out_masks[i] != nullptr);
    }

    HIP_CHECK(hipSetDevice(env_.device_of(replica_)));
    // an encoder pass nobody has waited for yet: the decoder goes onto ITS lane, behind it in stream order, and the wait
    // for the masks is the wait for both (any number of threads may do so at once: the lane's mutex orders their requests)
    const std::shared_ptr<SamModel::DeferredPass> behind = pending();
    SamModel& model_ = behind ? *behind->lane : env_.next_lane(replica_);
    const Extent o = image_size_.original, r = image_size_.resized;
    k::PostJob jobs[3];
    int n_jobs = 0;
    float iou[4] = {0.f, 0.f, 0.f, 0.f};
    MaskSlotLease lease(model_);
    try {
        {
            roctx::Range range("dlimg.compute_mask");
            std::lock_guard<std::mutex> lock(model_.mutex());
            float const* emb = embedding_;
            {
                roctx::Range rd("dlimg.decode");
                model_.decode(&emb, coords, labels, 1, 2, nullptr, /*handles*/ true);
            }
            if (is_single_mask) {
                // single-mask decoder: best of the four by SamOnnxModel.select_masks, chosen on the device
                jobs[n_jobs++] = k::PostJob{model_.logits(), model_.iou(), out_masks[0], o.width, o.height, r.width, r.height};
            } else {
                // multi-mask decoder: outputs 1..3 (reference: segmentation.cpp:167-172)
                for (int i = 0; i < 3; ++i)
                    jobs[n_jobs++] = k::PostJob{model_.logits() + (size_t)(i + 1) * kLowRes * kLowRes, nullptr, out_masks[i],
                                                o.width, o.height, r.width, r.height};
            }
            roctx::Range rp("dlimg.post");
            model_.enqueue_masks(lease.slot(), jobs, n_jobs, is_single_mask ? 0 : 4);
        }
        model_.finish_masks(lease.slot(), jobs, n_jobs, iou, is_single_mask ? 0 : 4);      // waits outside the lane's mutex
    } catch (...) {
        drain_lane(&model_);                     // a copy into the slot's staging memory may still be queued
        throw;
    }
    lease.release();
    if (behind) settle();                        // has completed; an embedding with non-finite values: no masks, the error
    if (!is_single_mask)
        for (int i = 0; i < 3; ++i) out_accuracy[i] = iou[i + 1];
}

namespace {
// Where the masks of a batch call go and how a chunk of them gets there: what the two forms of the call differ in.
//   kRange         ROCTX range around a chunk's enqueue
//   kFinishBehind  the chunk that many chunks back is finished before the next one takes its slot (0: all at the end)
//   dst(head)      where the mask of the prompt that entry `head` opened goes
//   enqueue        under the lane's mutex, behind the chunk's decode (clean: null, or per job what its prompt's clean-up mark
//                  asks for);  finish: no mutex, returns when the masks are in place
struct HostMasks {
    static constexpr const char* kRange = "dlimg.compute_masks";
    // masks of a chunk are copied to the caller while the two chunks behind it are on the GPU
    static constexpr size_t kFinishBehind = 3;
    uint8_t* const* out_masks;
    uint8_t* dst(int head) const { return out_masks[head]; }
    void enqueue(SamModel& model, SamModel::MaskSlot& slot, std::vector<k::PostJob> const& jobs, CleanSpec const* clean,
                 GridPaint const* paint = nullptr, MatteRequest const* matte = nullptr, EdgeRequest const* edge = nullptr) const {
        model.enqueue_masks(slot, jobs.data(), (int)jobs.size(), 0, clean, paint, matte, edge);
    }
    void finish(SamModel& model, SamModel::MaskSlot& slot, std::vector<k::PostJob> const& jobs) const {
        model.finish_masks(slot, jobs.data(), (int)jobs.size(), nullptr, 0);
    }
};
struct DeviceMasks {
    static constexpr const char* kRange = "dlimg.compute_masks_device";
    static constexpr size_t kFinishBehind = 0;
    uint8_t* dev_out;
    std::vector<size_t> const& offsets;          // [entry]
    int root_device;
    uint8_t* dst(int head) const { return dev_out + offsets[head]; }
    void enqueue(SamModel& model, SamModel::MaskSlot& slot, std::vector<k::PostJob> const& jobs, CleanSpec const* clean,
                 GridPaint const* paint = nullptr, MatteRequest const* matte = nullptr, EdgeRequest const* edge = nullptr) const {
        DLIMG_ASSERT(!matte);                    // (the planner refuses a matte mark in the device form)
        model.enqueue_masks_device(slot, jobs.data(), (int)jobs.size(), root_device, clean, paint, edge);
    }
    void finish(SamModel& model, SamModel::MaskSlot& slot, std::vector<k::PostJob> const&) const { model.wait_masks(slot); }
};
}  // namespace

// The prompts of a batch call whose embeddings `replica` holds: grouped by their number of points (a decoder launch holds one
// count) and cut into chunks of at most kPromptChunk prompts (prompt_plan.hpp), each chunk decoded as one batch on the next
// lane and its masks handed to `sink`.  A prompt with refinement marks is a chunk of its own behind them: its stages run in
// order on one lane's stream, each taking the logits of the one before it as its mask input, and only the last one is
// post-processed.  A prompt with a clean-up mark has its mask cleaned on the GPU behind the post-processing (the mask of the
// last stage only; the logits fed back between stages are untouched).  A prompt with a matte mark has its mask -- the cleaned
// one when it has both -- turned into a coverage on the GPU behind that, guided by the image the mark brought.  A cut-out mark
// behind the matte mark has that image's foreground colours estimated behind that, and delivered beside the coverage.  A prompt
// with an edge mark has its mask -- the cleaned one -- grown, shrunk, feathered or bordered behind the clean-up and in front of
// the matte, which then filters what the edge mark delivered.
template <typename Sink>
void SegmentationImpl::decode_batch_on(int replica, SegmentationImpl const* const* segs, BatchPrompts const& batch, int const* points,
                                       int const* regions, Sink const& sink) {
    std::vector<PromptSpec> const& prompts = batch.prompts;
    EnvironmentImpl& env = segs[prompts[0].head]->env_;
    HIP_CHECK(hipSetDevice(env.device_of(replica)));
    std::vector<int> mine;
    for (int j = 0; j < (int)prompts.size(); ++j)
        if (segs[prompts[j].head]->replica_ == replica) mine.push_back(j);
    struct Chunk { MaskSlotLease lease; std::vector<k::PostJob> jobs; };
    std::vector<Chunk> chunks;
    std::vector<CleanSpec> clean;              // of the chunk being enqueued, [job]
    MatteRequest matte;                        // of the chunk being enqueued: a prompt with a matte mark is a chunk of its own
    std::vector<EdgeRequest> edge;             // of the chunk being enqueued, [job]
    auto finish = [&](Chunk& c) {
        if (!c.lease.held()) return;
        const MaskSlotLease lease = std::move(c.lease);      // the slot goes back whether the wait throws or not
        sink.finish(lease.model(), lease.slot(), c.jobs);
    };
    try {
        std::vector<float> cc, ll;
        for (BatchWork const& work : plan_batch_work(batch, mine, kPromptChunk)) {
            PromptChunk const& part = work.part;
            const int n = (int)part.prompts.size(), npts = part.points;
            std::vector<float const*> emb(n);
            for (int j = 0; j < n; ++j) emb[j] = segs[prompts[part.prompts[j]].head]->embedding_;
            gather_chunk(batch, part, cc, ll);
            SamModel& model = env.next_lane(replica);
            if (Sink::kFinishBehind && chunks.size() >= Sink::kFinishBehind) finish(chunks[chunks.size() - Sink::kFinishBehind]);
            chunks.push_back(Chunk{MaskSlotLease(model), std::vector<k::PostJob>(n)});
            Chunk& cur = chunks.back();
            roctx::Range range(Sink::kRange);
            std::lock_guard<std::mutex> lock(model.mutex());
            if (work.grid) {
                // a label map: the grid's prompts decoded and harvested chunk by chunk, the segments selected on the host (the
                // call waits for the lane's stream once), and the map painted where a mask of this prompt would be written
                const int j = part.prompts[0], i = prompts[j].head;
                GridSpec const& g = batch.grid[j];
                ResizeLongestSide const& rs = segs[i]->image_size_;
                pack_grid(rs, g.side, cc, ll);
                GridPaint const& paint = model.segment_grid(emb[0], cc.data(), ll.data(), g.side, rs.resized.width, rs.resized.height,
                                                            g.iou_permille, g.stability_permille);
                cur.jobs[0] = k::PostJob{paint.store, nullptr, sink.dst(i), rs.original.width, rs.original.height, rs.resized.width,
                                         rs.resized.height};
                roctx::Range rp("dlimg.grid_paint");
                sink.enqueue(model, cur.lease.slot(), cur.jobs, nullptr, &paint);
                continue;
            }
            if (work.staged) {
                const int j = part.prompts[0];
                ResizeLongestSide const& rs = segs[prompts[j].head]->image_size_;
                // a prior: its bytes and its plane are enqueued here, in front of the decode on the lane's stream
                k::MaskSource first{nullptr, nullptr};
                if (batch.prior[j].any())
                    first = model.prior_plane(batch.prior_mask[j], rs.original.width, rs.original.height, rs.resized.width, rs.resized.height,
                                              batch.prior[j].strength_milli);
                // a guide: its bytes are enqueued here too, for the matte behind the post-processing of this prompt's mask
                matte = MatteRequest{};
                if (batch.matte[j].any()) {
                    MatteSpec const& m = batch.matte[j];
                    // (its cut-out, if any: the destination may be the guide itself, whose bytes are taken here)
                    matte = MatteRequest{model.matte_guide(batch.matte_guide[j], rs.original.width, rs.original.height, m.channels), m.channels,
                                         m.radius, m.eps, CutoutRequest{batch.cutout_dst[j], batch.cutout[j].radius}};
                }
                if (!batch.strokes[j].empty()) {
                    // stroke marks: every map of the prompt uploaded and derived back to back, the call waits for the lane's
                    // stream once, and the pixels go where the placeholder clicks of the rewritten call stand
                    std::vector<StrokeSpec> const& marks = batch.strokes[j];
                    std::vector<int32_t const*> records(marks.size());
                    for (size_t m = 0; m < marks.size(); ++m)
                        model.stroke_derive(batch.stroke_map[j][m], rs.original.width, rs.original.height,
                                            rs.resized.width, rs.resized.height, marks[m].clicks, &records[m]);
                    model.stroke_wait();
                    model.wait_caller_copies();
                    for (size_t m = 0; m < marks.size(); ++m) {
                        if (records[m][0] == 0) {
                            // nothing of this prompt is queued (stroke_wait waited for the stream): its slot goes back unused, so
                            // that nothing is delivered to its out_masks
                            cur.lease.release();
                            throw Exception("mask batch: entry " + std::to_string(marks[m].entry) + ": the stroke mark's map is empty: no "
                                            "pixel of it is 128 or more, so there are no clicks to derive");
                        }
                        for (int c = 0; c < marks[m].clicks; ++c)
                            stroke_cell_pixel(records[m][2 + 2 * c], records[m][3 + 2 * c], rs.original.width, rs.original.height,
                                              rs.resized.width, rs.resized.height, batch.derived_points + 2 * marks[m].click_entry[c]);
                    }
                    if (!batch.lasso[j].any()) {
                        cc.resize((size_t)npts * 2);
                        ll.resize((size_t)npts);
                        pack_points(rs, prompts[j], batch.stages[j], prompts[j].clicks, points, regions, cc.data(), ll.data());
                    }
                }
                k::MaskSource src;
                if (batch.lasso[j].any()) {
                    // a selection: uploaded and turned into the plane as a prior is, its box and click derived behind that; the
                    // call waits for the lane's stream once, and the prompt is packed with what came back
                    LassoSpec const& l = batch.lasso[j];
                    int32_t record[kLassoRecordInts];
                    const k::MaskSource plane = model.lasso_derive(batch.lasso_mask[j], rs.original.width, rs.original.height,
                                                                   rs.resized.width, rs.resized.height, l.strength_milli, record);
                    model.wait_caller_copies();
                    if (record[0] == 0) {
                        // nothing of this prompt is queued (lasso_derive waited for the stream): its slot goes back unused, so
                        // that nothing is delivered to its out_masks
                        cur.lease.release();
                        throw Exception("mask batch: entry " + std::to_string(batch.caller_entry(l.entry)) + ": the lasso mark's selection is empty: no low-res "
                                        "cell of it reaches half coverage, so there is no box and no click to derive");
                    }
                    const LassoPromptArrays own = lasso_prompt_arrays(prompts[j], batch.stages[j], l, points, regions, record);
                    cc.resize((size_t)npts * 2);
                    ll.resize((size_t)npts);
                    pack_points(rs, own.spec, own.stages, own.spec.clicks, own.points.data(), own.regions.data(), cc.data(), ll.data());
                    if (l.mask()) first = plane;
                    src = run_early_stages(model, own.spec, own.stages, emb[0], rs, own.points.data(), own.regions.data(), first);
                } else {
                    src = run_early_stages(model, prompts[j], batch.stages[j], emb[0], rs, points, regions, first);
                }
                model.decode(emb.data(), cc.data(), ll.data(), 1, npts, src.logits4 ? &src : nullptr, /*handles*/ true);
                model.wait_caller_copies();        // a prior or a guide read in place (pinned image memory): the caller's again
            } else {
                matte = MatteRequest{};
                model.decode(emb.data(), cc.data(), ll.data(), n, npts, nullptr, /*handles*/ true);
            }
            for (int j = 0; j < n; ++j) {
                const int i = prompts[part.prompts[j]].head;
                const Extent o = segs[i]->image_size_.original, r = segs[i]->image_size_.resized;
                cur.jobs[j] = single_mask_job(model.logits() + (size_t)j * 4 * kLowRes * kLowRes, model.iou() + (size_t)j * 4, npts,
                                              sink.dst(i), o, r);
            }
            if (batch.any_clean) {
                clean.resize(n);
                for (int j = 0; j < n; ++j) clean[j] = batch.clean[part.prompts[j]];
            }
            if (batch.any_edge) {
                edge.resize(n);
                for (int j = 0; j < n; ++j) {
                    EdgeSpec const& e = batch.edge[part.prompts[j]];
                    edge[j] = EdgeRequest{e.offset, e.feather, e.border};
                }
            }
            // (a prompt with a matte mark is a chunk of its own: n == 1)
            sink.enqueue(model, cur.lease.slot(), cur.jobs, batch.any_clean ? clean.data() : nullptr, nullptr, matte.any() ? &matte : nullptr,
                         batch.any_edge ? edge.data() : nullptr);
        }
        for (auto& c : chunks) finish(c);
    } catch (...) {
        // a chunk whose enqueue failed has no valid completion event: drain the lanes before the slots go back
        for (auto& c : chunks)
            if (c.lease.held()) drain_lane(&c.lease.model());
        for (auto& c : chunks) {
            try { finish(c); } catch (...) {}
        }
        throw;
    }
}

// Prompts are grouped by the replica that holds their image's embedding and decoded there (decode_batch_on), the masks of a
// chunk copied out while the next chunks run.
void SegmentationImpl::compute_mask_batch(SegmentationImpl const* const* segs, int count, int const* points,
                                          int const* regions, uint8_t* const* out_masks) {
    if (count <= 0) return;
    DLIMG_ASSERT(points != nullptr || regions != nullptr);
    const BatchPrompts batch = read_batch_prompts(segs, count, points, regions, out_masks);
    if (batch.rewritten()) {
        // stroke marks: the call goes on as the rewritten one, whose placeholder clicks the derivation fills in (stroke_plan.hpp)
        segs = batch.segs.data();
        points = batch.points.data();
        regions = batch.regions.data();
        out_masks = batch.out_masks.data();
    }
    std::vector<PromptSpec> const& prompts = batch.prompts;
    EnvironmentImpl& env = segs[prompts[0].head]->env_;
    std::vector<int> used;
    for (PromptSpec const& p : prompts) {
        SegmentationImpl const* seg = segs[p.head];
        DLIMG_ASSERT(&seg->env_ == &env);
        DLIMG_ASSERT(seg->embedding_ != nullptr && out_masks[p.head] != nullptr);
        seg->settle();                           // prompts of a batch go to any lane: the embeddings are complete first
        if (std::find(used.begin(), used.end(), seg->replica_) == used.end()) used.push_back(seg->replica_);
    }
    const HostMasks sink{out_masks};
    for_each_replica(env, used, [&](int replica) { decode_batch_on(replica, segs, batch, points, regions, sink); });
}

// Device-output variant: the "gather" of SURVEY.md 8e.  Every GPU of the environment decodes the prompts whose
// embeddings it holds; a mask whose GPU is the root is written in place by the post-processing kernel, the others cross
// xGMI as one peer copy each (hipMemcpyPeerAsync on the producing lane's stream, so the copy of one chunk runs beside the
// decoder of the next).  No host memory is touched; every chunk is waited for at the end.  The reference has nothing
// comparable (one device, host tensors: /root/reference/src/session.cpp:63-66, /root/reference/src/environment.cpp:142).
void SegmentationImpl::compute_mask_batch_device(SegmentationImpl const* const* segs, int count, int const* points,
                                                 int const* regions, int root_device, uint8_t* dev_out,
                                                 size_t* out_offsets) {
    if (count <= 0) return;
    DLIMG_ASSERT(points != nullptr || regions != nullptr);
    DLIMG_ASSERT(dev_out != nullptr);
    if (root_device < 0 || root_device >= EnvironmentImpl::device_count())
        throw Exception("root device " + std::to_string(root_device) + " is out of range: " +
                        std::to_string(EnvironmentImpl::device_count()) + " device(s) visible");
    const BatchPrompts batch = read_batch_prompts(segs, count, points, regions, /*out_masks*/ nullptr);
    std::vector<PromptSpec> const& prompts = batch.prompts;
    EnvironmentImpl& env = segs[prompts[0].head]->env_;
    // one mask and one offset per prompt, in head order; the continuation entries of a prompt repeat its offset
    std::vector<size_t> offsets(count);
    std::vector<int> used;
    size_t total = 0;
    for (size_t j = 0; j < prompts.size(); ++j) {
        SegmentationImpl const* seg = segs[prompts[j].head];
        DLIMG_ASSERT(&seg->env_ == &env);
        DLIMG_ASSERT(seg->embedding_ != nullptr);
        seg->settle();
        const int end = j + 1 < prompts.size() ? prompts[j + 1].head : count;
        for (int i = prompts[j].head; i < end; ++i) offsets[i] = total;
        total += (size_t)seg->image_size_.original.width * seg->image_size_.original.height;
        if (std::find(used.begin(), used.end(), seg->replica_) == used.end()) used.push_back(seg->replica_);
    }
    if (out_offsets) std::copy(offsets.begin(), offsets.end(), out_offsets);
    const DeviceMasks sink{dev_out, offsets, root_device};
    for_each_replica(env, used, [&](int replica) { decode_batch_on(replica, segs, batch, points, regions, sink); });
}

}  // namespace dlimg
