#include "mask_transport_exec.hpp"
#include "image_memory.hpp"
#include "roctx.hpp"

#include <chrono>
#include <cstdlib>
#include <cstring>

namespace dlimg {

namespace {

constexpr double kLogitBytes = 256.0 * 256.0 * 4.0;     // what the kernel reads per mask: the low-resolution logits
constexpr double kCleanBytesPerPixelAndPass = 2 * 1 + 2 * 4 + 4 + 4 * 4 + 1;     // k::mask_cleanup, see MaskTransport::run
// k::mask_matte, no block uniform: the mask read twice (cells, pass 1) and written, A and B written and read
constexpr double kMatteBytesPerPixel = 2 * 1 + 1 + 2 * 2 * 4;
// k::mask_cutout, no block uniform: the coverage read twice (cells, sums), the RGBA written; the guide's channels on top
constexpr double kCutoutBytesPerPixel = 2 * 1 + 4;
// k::mask_edge at the largest reach, no block uniform: the mask read by the cells and, with the halo rows above and below a band,
// six times by the column pass; two bytes of distance written, read twice over with the halo columns; the mask written
constexpr double kEdgeBytesPerPixel = 1 + 6 + 2 + 4 + 1;

// Direct xGMI copies between two GPUs need peer access switched on once per direction (without it the runtime stages
// the copy through host memory: still correct, slower).  Failures are not errors: the copy falls back by itself.
void enable_peer_access(int from_device, int to_device) {
    static std::mutex m;
    static std::vector<std::pair<int, int>> done;
    std::lock_guard<std::mutex> lock(m);
    for (auto& d : done)
        if (d.first == from_device && d.second == to_device) return;
    done.emplace_back(from_device, to_device);
    if (from_device == to_device) return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, from_device, to_device) == hipSuccess && can) {
        (void)hipSetDevice(from_device);
        if (hipDeviceEnablePeerAccess(to_device, 0) != hipSuccess) (void)hipGetLastError();
    }
    if (hipDeviceCanAccessPeer(&can, to_device, from_device) == hipSuccess && can) {
        (void)hipSetDevice(to_device);
        if (hipDeviceEnablePeerAccess(from_device, 0) != hipSuccess) (void)hipGetLastError();
    }
    (void)hipSetDevice(prev);
}

bool any_cleanup(CleanSpec const* clean, int count) {
    for (int i = 0; clean && i < count; ++i)
        if (clean[i].any()) return true;
    return false;
}

bool any_edge(EdgeRequest const* edge, int count) {
    for (int i = 0; edge && i < count; ++i)
        if (edge[i].any()) return true;
    return false;
}

bool any_matte(MatteRequest const* matte, int count) {
    for (int i = 0; matte && i < count; ++i)
        if (matte[i].any()) return true;
    return false;
}

void fill_sizes(std::vector<size_t>& sizes, k::PostJob const* jobs, int count) {
    sizes.resize(count > 0 ? count : 0);
    for (int i = 0; i < count; ++i) sizes[i] = (size_t)jobs[i].out_w * jobs[i].out_h;
}

}  // namespace

MaskTransport::~MaskTransport() {
    for (auto& m : slots_) {
        if (m->done) (void)hipEventDestroy(m->done);
        for (auto e : m->piece_done) (void)hipEventDestroy(e);
    }
}

MaskSlot& MaskTransport::acquire() {
    {
        std::lock_guard<std::mutex> lock(mutex_);
        if (!free_.empty()) {
            MaskSlot* s = free_.back();
            free_.pop_back();
            return *s;
        }
    }
    // as many slots come into being as there are mask requests in flight on this lane at once
    auto fresh = std::make_unique<MaskSlot>();
    HIP_CHECK(hipSetDevice(device_));
    HIP_CHECK(hipEventCreateWithFlags(&fresh->done, hipEventDisableTiming));
    std::lock_guard<std::mutex> lock(mutex_);
    slots_.push_back(std::move(fresh));
    return *slots_.back();
}

void MaskTransport::release(MaskSlot& s) {
    std::lock_guard<std::mutex> lock(mutex_);
    free_.push_back(&s);
}

hipEvent_t MaskTransport::piece_event(MaskSlot& slot, int i) {
    while ((int)slot.piece_done.size() <= i) {
        hipEvent_t e = nullptr;
        HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        slot.piece_done.push_back(e);
    }
    return slot.piece_done[i];
}

// The plan of the slot, step by step, on the lane's stream; slot.done behind the last of them.
void MaskTransport::run(MaskSlot& slot, k::PostJob const* jobs, int count, float const* iou, int dst_device, CleanSpec const* clean,
                        GridPaint const* paint, MatteRequest const* matte, EdgeRequest const* edge) {
    MaskTransportPlan const& p = slot.plan;
    DLIMG_ASSERT(!paint || (count == 1 && !clean && !matte && !edge));
    // the slot is ours, and its previous user waited for the slot's event before letting go of it
    slot.dev.reserve(p.reserve_device);
    slot.pin.reserve(p.reserve_pinned);
    uint8_t* const dev = slot.dev.get();
    uint8_t* const pin = static_cast<uint8_t*>(slot.pin.get());
    uint8_t* const staging = p.mode == MaskMode::direct ? pin : dev;
    slot.cutout_dst = slot.cutout_staged_for = nullptr;
    slot.kernel_jobs.assign(jobs, jobs + count);
    for (int i = 0; i < count; ++i)
        if (p.kernel_dst[i] != kCallersPointer) slot.kernel_jobs[i].dst = staging + p.kernel_dst[i];
    if (p.mode == MaskMode::device_staged) enable_peer_access(device_, dst_device);
    auto address = [&](MaskMem mem, size_t offset, int mask) -> uint8_t* {
        switch (mem) {
            case MaskMem::iou: return reinterpret_cast<uint8_t*>(const_cast<float*>(iou)) + offset;
            case MaskMem::device: return dev + offset;
            case MaskMem::pinned: return pin + offset;
            default: return jobs[mask].dst + offset;
        }
    };
    for (MaskStep const& s : p.steps) {
        if (s.kind == MaskStep::launch) {
            double bytes = 0;
            if (paint) {
                // a label map: the planes of the kept segments read (at most once each, where their boxes lie), the map written
                k::PostJob const& j = slot.kernel_jobs[s.first];
                clock_.timed(ST_POST, kLogitBytes * paint->kept.count + (double)slot.input.sizes[s.first], [&] {
                    k::grid_paint(paint->store, paint->candidates, paint->kept, j.dst, j.out_w, j.out_h, j.pre_w, j.pre_h, /*cull*/ true, stream_);
                });
                continue;
            }
            for (int i = s.first; i < s.first + s.count; ++i) bytes += kLogitBytes + (double)slot.input.sizes[i];
            clock_.timed(ST_POST, bytes, [&] { k::postprocess_masks(&slot.kernel_jobs[s.first], s.count, stream_); });
            if (clean) run_cleanup(slot, s, clean);
            if (edge) run_edge(slot, s, edge);
            if (matte) run_matte(slot, s, matte);
        } else if (s.kind == MaskStep::event) {
            HIP_CHECK(hipEventRecord(piece_event(slot, s.first), stream_));
        } else if (s.to == MaskMem::peer) {
            HIP_CHECK(hipMemcpyPeerAsync(address(s.to, s.to_offset, s.mask), dst_device, address(s.from, s.from_offset, s.mask), device_, s.bytes, stream_));
        } else {
            HIP_CHECK(hipMemcpyAsync(address(s.to, s.to_offset, s.mask), address(s.from, s.from_offset, s.mask), s.bytes,
                                     s.to == MaskMem::device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream_));
        }
    }
    HIP_CHECK(hipEventRecord(slot.done, stream_));
    slot.cutout_dst = slot.cutout_staged_for;
}

// The clean-up of the masks of launch step `s`, behind its post-processing launch: in place where the launch wrote them, device
// memory in every mode a request with clean-up marks is planned in (never the direct mode, whose kernel writes pinned host
// memory).
void MaskTransport::run_cleanup(MaskSlot& slot, MaskStep const& s, CleanSpec const* clean) {
    slot.clean_jobs.clear();
    double clean_bytes = 0;
    for (int i = s.first; i < s.first + s.count; ++i) {
        if (!clean[i].any()) continue;
        DLIMG_ASSERT(slot.plan.mode != MaskMode::direct);
        k::PostJob const& j = slot.kernel_jobs[i];
        slot.clean_jobs.push_back(k::CleanJob{j.dst, j.out_w, j.out_h, clean[i].max_hole, clean[i].max_island});
        // per polarity pass and pixel: the mask read (K1, K4), labels and areas written (K1) and read (K3: areas,
        // K4: both twice), at most one byte written
        clean_bytes += kCleanBytesPerPixelAndPass * (double)slot.input.sizes[i] * ((clean[i].max_hole > 0) + (clean[i].max_island > 0));
    }
    if (slot.clean_jobs.empty()) return;
    const int n_clean = (int)slot.clean_jobs.size();
    slot.clean_workspace.reserve(k::mask_cleanup_workspace_bytes(slot.clean_jobs.data(), n_clean));
    clock_.timed(ST_POST, clean_bytes, [&] { k::mask_cleanup(slot.clean_jobs.data(), n_clean, slot.clean_workspace.get(), stream_); },
                 clock_.profiling() ? k::mask_cleanup_launches(slot.clean_jobs.data(), n_clean) : 1);
}

// The edge marks of the masks of launch step `s`, behind its post-processing launch and its clean-up and in front of its mattes:
// in place where the launch wrote them, device memory in every mode a request with edge marks is planned in (never the direct
// mode), as for clean-up.
void MaskTransport::run_edge(MaskSlot& slot, MaskStep const& s, EdgeRequest const* edge) {
    slot.edge_jobs.clear();
    double bytes = 0;
    for (int i = s.first; i < s.first + s.count; ++i) {
        if (!edge[i].any()) continue;
        DLIMG_ASSERT(slot.plan.mode != MaskMode::direct);
        k::PostJob const& j = slot.kernel_jobs[i];
        slot.edge_jobs.push_back(k::EdgeJob{j.dst, j.out_w, j.out_h, edge[i].offset, edge[i].feather, edge[i].border});
        bytes += kEdgeBytesPerPixel * (double)slot.input.sizes[i];
    }
    if (slot.edge_jobs.empty()) return;
    const int n = (int)slot.edge_jobs.size();
    roctx::Range range("dlimg.mask_edge");
    slot.edge_workspace.reserve(k::mask_edge_workspace_bytes(slot.edge_jobs.data(), n));
    clock_.timed(ST_POST, bytes, [&] { k::mask_edge(slot.edge_jobs.data(), n, slot.edge_workspace.get(), stream_); },
                 clock_.profiling() ? k::mask_edge_launches(slot.edge_jobs.data(), n) : 1);
    HIP_CHECK(hipGetLastError());        // a launch that was not taken is reported here, not by the copy behind it
}

// The mattes of the masks of launch step `s`, behind its post-processing launch and its clean-up: in place where the launch
// wrote them, the slot's device buffer (a request with a matte never takes the direct mode).
void MaskTransport::run_matte(MaskSlot& slot, MaskStep const& s, MatteRequest const* matte) {
    slot.matte_jobs.clear();
    double bytes = 0;
    for (int i = s.first; i < s.first + s.count; ++i) {
        if (!matte[i].any()) continue;
        DLIMG_ASSERT(slot.plan.mode != MaskMode::direct);
        k::PostJob const& j = slot.kernel_jobs[i];
        slot.matte_jobs.push_back(k::MatteJob{j.dst, matte[i].guide, j.out_w, j.out_h, matte[i].channels, matte[i].radius, matte[i].eps});
        bytes += (kMatteBytesPerPixel + 2 * matte[i].channels) * (double)slot.input.sizes[i];
    }
    if (slot.matte_jobs.empty()) return;
    const int n = (int)slot.matte_jobs.size();
    roctx::Range range("dlimg.mask_matte");
    slot.matte_workspace.reserve(k::mask_matte_workspace_bytes(slot.matte_jobs.data(), n));
    clock_.timed(ST_POST, bytes, [&] { k::mask_matte(slot.matte_jobs.data(), n, slot.matte_workspace.get(), stream_); },
                 clock_.profiling() ? k::mask_matte_launches(slot.matte_jobs.data(), n) : 1);
    HIP_CHECK(hipGetLastError());        // a launch that was not taken is reported here, not by the copy behind it
    for (int i = s.first; i < s.first + s.count; ++i)
        if (matte[i].any() && matte[i].cutout.any()) run_cutout(slot, slot.kernel_jobs[i], matte[i]);
}

// The cut-out of one mask behind its matte: the coverage read where the matte left it, the RGBA written to the slot's own buffer
// and sent on its way by one copy command.  A request holds one at most (a prompt with a matte is a chunk of its own).
void MaskTransport::run_cutout(MaskSlot& slot, k::PostJob const& j, MatteRequest const& m) {
    DLIMG_ASSERT(slot.cutout_staged_for == nullptr && slot.plan.mode != MaskMode::direct);
    roctx::Range range("dlimg.mask_cutout");
    const size_t pixels = (size_t)j.out_w * j.out_h, bytes = pixels * 4;
    slot.cutout_dev.reserve(bytes);
    const k::CutoutJob job{j.dst, m.guide, slot.cutout_dev.get(), j.out_w, j.out_h, m.channels, m.cutout.radius};
    slot.cutout_workspace.reserve(k::mask_cutout_workspace_bytes(&job, 1));
    clock_.timed(ST_POST, (kCutoutBytesPerPixel + m.channels) * (double)pixels,
                 [&] { k::mask_cutout(&job, 1, slot.cutout_workspace.get(), stream_); }, clock_.profiling() ? k::mask_cutout_launches(&job, 1) : 1);
    HIP_CHECK(hipGetLastError());
    // pinned image memory of the library: the copy command writes it; anything else goes through staging, and finish() copies
    uint8_t* to = m.cutout.dst;
    if (!image_memory_is_pinned(to, bytes)) {
        slot.cutout_pin.reserve(bytes);
        to = static_cast<uint8_t*>(slot.cutout_pin.get());
        slot.cutout_staged_for = m.cutout.dst;
        slot.cutout_bytes = bytes;
    }
    HIP_CHECK(hipMemcpyAsync(to, slot.cutout_dev.get(), bytes, hipMemcpyDeviceToHost, stream_));
}

void MaskTransport::enqueue(MaskSlot& slot, k::PostJob const* jobs, int count, float const* iou, int iou_count, CleanSpec const* clean,
                            GridPaint const* paint, MatteRequest const* matte, EdgeRequest const* edge) {
    if (count <= 0) return;
    // DLIMGEDIT_DIRECT_MASKS=0: measurement aid (always the copy path)
    static const bool direct_allowed = [] { const char* e = std::getenv("DLIMGEDIT_DIRECT_MASKS"); return !e || std::atoi(e) != 0; }();
    MaskTransportInput& in = slot.input;
    fill_sizes(in.sizes, jobs, count);
    in.iou_count = iou_count;
    if (!any_cleanup(clean, count)) clean = nullptr;
    if (!any_matte(matte, count)) matte = nullptr;
    if (!any_edge(edge, count)) edge = nullptr;
    in.direct_allowed = direct_allowed && !clean && !matte && !edge;     // a mask to clean, to edge or to matte goes through the slot's device buffer
    in.others_idle = mask_mode_asks_idle(count, in.direct_allowed) && (!board_ || board_->others_idle(lane_index_));
    // a destination in pinned image memory of the library (the Image the reference's wrapper allocates for the result
    // through create_image).  Direct mode looks at every destination, staged mode only asks whether all of them are pinned:
    // no lookup behind the first that is not
    const bool every = mask_transport_is_direct(in);
    in.dst_pinned.assign(count, 0);
    for (int i = 0; i < count; ++i) {
        in.dst_pinned[i] = image_memory_is_pinned(jobs[i].dst, in.sizes[i]);
        if (!in.dst_pinned[i] && !every) break;
    }
    plan_mask_transport(in, slot.plan);
    run(slot, jobs, count, iou, device_, clean, paint, matte, edge);
    if (board_) board_->mark(lane_index_, stream_);
}

void MaskTransport::finish(MaskSlot& slot, k::PostJob const* jobs, int count, float* iou_out, int iou_count) {
    if (count <= 0) return;
    static const bool trace = std::getenv("DLIMGEDIT_TIMING") != nullptr;     // diagnostic: host time of the two phases
    const auto t0 = std::chrono::steady_clock::now();
    MaskTransportPlan const& p = slot.plan;
    uint8_t const* pin = static_cast<uint8_t const*>(slot.pin.get());
    // piece by piece: what has arrived is copied to the callers' buffers while the rest is still on its way
    double waited_us = 0;
    MaskCursor cursor;
    size_t begin = 0;
    for (size_t i = 0; i < p.piece_end.size(); ++i) {
        const auto w0 = std::chrono::steady_clock::now();
        HIP_CHECK(hipEventSynchronize(slot.piece_done[i]));
        waited_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w0).count();
        for (MaskCopy const& c : mask_copies_in_piece(slot.input.sizes, begin, p.piece_end[i], cursor))
            if (!p.in_place[c.mask]) std::memcpy(jobs[c.mask].dst + c.mask_offset, pin + c.staging_offset, c.bytes);
        begin = p.piece_end[i];
    }
    HIP_CHECK(hipEventSynchronize(slot.done));
    if (slot.cutout_dst) std::memcpy(slot.cutout_dst, slot.cutout_pin.get(), slot.cutout_bytes);
    slot.cutout_dst = nullptr;
    const auto t1 = std::chrono::steady_clock::now();
    if (iou_out && iou_count > 0) std::memcpy(iou_out, pin + p.iou_offset, (size_t)iou_count * sizeof(float));
    if (trace)
        std::fprintf(stderr, "finish_masks: %.1f us in all, %.1f us of them waiting for the %zu pieces (%zu bytes)\n",
                     std::chrono::duration<double, std::micro>(t1 - t0).count(), waited_us, p.piece_end.size(), p.iou_offset);
}

void MaskTransport::enqueue_device(MaskSlot& slot, k::PostJob const* jobs, int count, int dst_device, CleanSpec const* clean,
                                   GridPaint const* paint, EdgeRequest const* edge) {
    if (count <= 0) return;
    // test hook: take the staging + peer-copy path even when the destination is this lane's own GPU (a one-GPU box
    // has no second device to copy to; the path is the same code, the copy degenerates to device-to-device)
    const char* fp = std::getenv("DLIMGEDIT_FORCE_PEER_COPY");       // read per call: the tests switch it on and off
    const bool force_peer = fp && std::atoi(fp) != 0;
    fill_sizes(slot.input.sizes, jobs, count);
    plan_mask_transport_device(slot.input.sizes, dst_device == device_ && !force_peer, slot.plan);
    run(slot, jobs, count, nullptr, dst_device, any_cleanup(clean, count) ? clean : nullptr, paint, nullptr, any_edge(edge, count) ? edge : nullptr);
}

void MaskTransport::wait(MaskSlot& slot) { HIP_CHECK(hipEventSynchronize(slot.done)); }

}  // namespace dlimg
