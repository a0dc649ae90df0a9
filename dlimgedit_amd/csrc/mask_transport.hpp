// The road of the masks of one request from the post-processing kernel to the caller's buffers, as a plan: pure host logic
// (no HIP, no environment, no lookups), tested without a GPU (tests/test_mask_transport.py, tests/sanitize/planners_fuzz.cpp).
// The caller says what it knows -- the masks' sizes, which destinations are pinned image memory of the library
// (image_memory.hpp), whether the sibling lanes are idle -- and gets the steps the lane's stream is to take, in order;
// MaskTransport (mask_transport_exec.hpp) walks them and decides nothing.  Layout and pieces: mask_pieces.hpp.
//   direct: one mask, or up to kDirectMasks while no other lane of this GPU has work in flight: the kernel writes each mask
//           STRAIGHT into pinned host memory (the caller's own where that is pinned), one launch and one event per mask --
//           the stores leave over PCIe while the kernel runs, and the host copies mask i out while mask i + 1 is being written.
//           [r04: one mask this way instead of a device buffer plus a copy command, 0.330 -> 0.309 ms per compute_mask call.
//           r06: several masks too -- a five-prompt call spent 265 us, 42 % of the call, on five ~1 MiB copy commands and
//           their events: one caller 7299 -> 8106 prompts/s.  But a kernel that waits for PCIe holds its lane's stream and
//           its CUs meanwhile, where a copy command runs beside the next kernels: with FOUR callers the same change cost
//           21 900 -> 18 300 prompts/s, hence the idle-lanes condition.]
//   staged: one launch into the slot's device buffer; then one copy command per mask to where the consumer reads it when
//           EVERY destination is pinned (nothing left for the host to copy), else the staging area in pieces to the slot's
//           pinned buffer, each piece with its own event.
//   device form (destinations in device memory, maybe another GPU's): the kernel writes them itself, or writes the slot's
//           device buffer and one peer copy per mask moves it over.
#pragma once

#include "mask_pieces.hpp"

namespace dlimg {

constexpr int kDirectMasks = 6;
constexpr size_t kCallersPointer = ~size_t(0);      // MaskTransportPlan::kernel_dst: the mask's own destination

struct MaskTransportInput {
    std::vector<size_t> sizes;          // out_w * out_h of every mask, bytes
    std::vector<char> dst_pinned;       // its destination is pinned image memory of the library
    int iou_count = 0;                  // IoU predictions (floats) that travel behind the masks
    bool direct_allowed = true;
    bool others_idle = true;            // true when there are no other lanes
};

enum class MaskMode { none, direct, staged, device_direct, device_staged };
// iou: the lane's IoU predictions; device / pinned: the slot's two buffers; caller: the destination of mask `mask`, host
// memory; peer: the same, device memory of the destination GPU
enum class MaskMem : char { iou, device, pinned, caller, peer };

struct MaskStep {
    enum Kind : char { launch, copy, event } kind;
    int first, count;                   // launch: masks [first, first + count) in one launch; event: of piece `first`
    MaskMem from, to;                   // copy: `bytes` bytes from `from` + from_offset to `to` + to_offset (`mask`: whose destination)
    int mask;
    size_t from_offset, to_offset, bytes;
};

struct MaskTransportPlan {
    MaskMode mode = MaskMode::none;
    std::vector<size_t> kernel_dst;     // where the kernel writes mask i: offset into the slot's pinned (direct) or device buffer, or kCallersPointer
    std::vector<char> in_place;         // mask i reaches its destination without the host copying it (finish_masks skips it)
    std::vector<MaskStep> steps;        // what the stream is given, in order; an event of the slot's own closes every request
    std::vector<size_t> piece_end;      // end offsets of the pieces finish_masks walks, one event each
    int launches = 0;
    size_t iou_offset = 0;              // of the IoU floats in the slot's pinned buffer
    size_t reserve_device = 0, reserve_pinned = 0;
};

// Whether the mode depends on MaskTransportInput::others_idle at all: asking costs an event query per sibling lane.
inline bool mask_mode_asks_idle(int count, bool direct_allowed) { return direct_allowed && count > 1 && count <= kDirectMasks; }
inline bool mask_transport_is_direct(MaskTransportInput const& in) {
    const int count = (int)in.sizes.size();
    return in.direct_allowed && (count == 1 || (count <= kDirectMasks && in.others_idle));
}

namespace detail {
inline MaskStep launch_step(int first, int count) { return MaskStep{MaskStep::launch, first, count, MaskMem::iou, MaskMem::iou, 0, 0, 0, 0}; }
inline MaskStep event_step(int piece) { return MaskStep{MaskStep::event, piece, 1, MaskMem::iou, MaskMem::iou, 0, 0, 0, 0}; }
inline MaskStep copy_step(MaskMem from, size_t from_offset, MaskMem to, size_t to_offset, size_t bytes, int mask = -1) {
    return MaskStep{MaskStep::copy, 0, 0, from, to, mask, from_offset, to_offset, bytes};
}
// kernel_dst = the staging layout; returns its end
inline size_t lay_out(std::vector<size_t> const& sizes, MaskTransportPlan& p) {
    p.kernel_dst.clear();
    p.in_place.assign(sizes.size(), 0);
    p.steps.clear();
    p.piece_end.clear();
    p.launches = 0;
    p.iou_offset = p.reserve_device = p.reserve_pinned = 0;
    size_t off = 0;
    for (size_t s : sizes) {
        p.kernel_dst.push_back(off);
        off += padded_mask_bytes(s);
    }
    return off;
}
}  // namespace detail

// Masks to HOST memory.  `plan` is re-used from request to request (its vectors keep their capacity).
inline void plan_mask_transport(MaskTransportInput const& in, MaskTransportPlan& p) {
    using namespace detail;
    const int count = (int)in.sizes.size();
    const size_t total = lay_out(in.sizes, p);
    p.mode = MaskMode::none;
    if (count <= 0) return;
    const size_t iou_bytes = (size_t)in.iou_count * sizeof(float);
    const size_t with_iou = total + iou_bytes;
    p.iou_offset = total;
    p.reserve_device = p.reserve_pinned = with_iou;
    if (mask_transport_is_direct(in)) {
        p.mode = MaskMode::direct;
        p.launches = count;
        for (int i = 0; i < count; ++i) {
            const bool last = i + 1 == count;
            p.piece_end.push_back(last ? with_iou : p.kernel_dst[i + 1]);
            p.in_place[i] = in.dst_pinned[i] != 0;
            if (p.in_place[i]) p.kernel_dst[i] = kCallersPointer;
            p.steps.push_back(launch_step(i, 1));
            if (last && in.iou_count > 0) p.steps.push_back(copy_step(MaskMem::iou, 0, MaskMem::pinned, total, iou_bytes));
            p.steps.push_back(event_step(i));
        }
        return;
    }
    p.mode = MaskMode::staged;
    p.launches = 1;
    p.steps.push_back(launch_step(0, count));
    if (in.iou_count > 0) p.steps.push_back(copy_step(MaskMem::iou, 0, MaskMem::device, total, iou_bytes));
    bool all_pinned = true;
    for (int i = 0; i < count && all_pinned; ++i) all_pinned = in.dst_pinned[i] != 0;
    if (all_pinned) {
        p.in_place.assign(count, 1);
        for (int i = 0; i < count; ++i) p.steps.push_back(copy_step(MaskMem::device, p.kernel_dst[i], MaskMem::caller, 0, in.sizes[i], i));
        if (in.iou_count > 0) p.steps.push_back(copy_step(MaskMem::device, total, MaskMem::pinned, total, iou_bytes));
        p.piece_end.push_back(with_iou);
        p.steps.push_back(event_step(0));
        return;
    }
    p.piece_end = mask_piece_ends(with_iou);
    size_t a = 0;
    for (size_t i = 0; i < p.piece_end.size(); ++i) {
        p.steps.push_back(copy_step(MaskMem::device, a, MaskMem::pinned, a, p.piece_end[i] - a));
        p.steps.push_back(event_step((int)i));
        a = p.piece_end[i];
    }
}

// Masks to DEVICE memory.  kernel_writes_dst: the destinations are on the lane's own GPU (and the peer copy is not forced).
inline void plan_mask_transport_device(std::vector<size_t> const& sizes, bool kernel_writes_dst, MaskTransportPlan& p) {
    using namespace detail;
    const int count = (int)sizes.size();
    const size_t total = lay_out(sizes, p);
    p.mode = MaskMode::none;
    if (count <= 0) return;
    p.mode = kernel_writes_dst ? MaskMode::device_direct : MaskMode::device_staged;
    p.launches = 1;
    p.steps.push_back(launch_step(0, count));
    if (kernel_writes_dst) {
        p.kernel_dst.assign(count, kCallersPointer);
        p.in_place.assign(count, 1);
        return;
    }
    p.reserve_device = total;
    for (int i = 0; i < count; ++i) p.steps.push_back(copy_step(MaskMem::device, p.kernel_dst[i], MaskMem::peer, 0, sizes[i], i));
}

}  // namespace dlimg
