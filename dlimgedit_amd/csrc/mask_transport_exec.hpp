// MaskTransport: the mask slots of one execution lane and the executor of their plans (mask_transport.hpp).
//   slot = acquire()                         any thread, no lock needed: a free slot (or a new one: never blocks), the
//                                            caller's until release()
//   enqueue(slot, jobs, n, iou, n_iou)       under the lane's mutex: plans the request and gives the plan's steps to the
//                                            lane's stream -- kernel, copy commands, one event per piece, slot.done last
//   finish(slot, jobs, n, iou_out, n_iou)    no lock: waits piece by piece and copies what the plan left in the slot's
//                                            pinned buffer into jobs[i].dst (HOST pointers of out_w*out_h bytes) and iou_out
//   enqueue_device / wait                    the same for destinations in DEVICE memory of any GPU; slot.done only
//   clean (enqueue, enqueue_device)          optional, [count]: the clean-up of mask i (prompt_plan.hpp: CleanSpec; both
//                                            thresholds 0: none).  A request with a mask to clean never takes the direct
//                                            mode: k::mask_cleanup runs right behind the post-processing launch, in place
//                                            where that launch wrote -- the slot's device buffer, or the destination itself
//                                            when that is memory of the lane's own GPU -- before any copy or event
//   edge (enqueue, enqueue_device)           optional, [count]: the edge mark of mask i (edge_plan.hpp; kernels.hpp K24; all three
//                                            values 0: none).  Treated as clean-up is: never the direct mode; k::mask_edge runs
//                                            behind the post-processing launch and behind k::mask_cleanup when both are asked
//                                            for, in place where the launch wrote -- the slot's device buffer, or the
//                                            destination itself when that is memory of the lane's own GPU -- before the matte
//                                            and before any copy or event; its workspace is pooled with the slot
//   matte (enqueue)                          optional, [count]: the matte of mask i (matte_plan.hpp; kernels.hpp K21; a null
//                                            guide: none).  Treated as clean-up is: never the direct mode; k::mask_matte runs
//                                            behind the post-processing launch and behind k::mask_cleanup when both are asked
//                                            for, in place in the slot's device buffer, before any copy or event.  The guide
//                                            is device memory of the lane (SamModel::matte_guide), valid in stream order
//   cut-out (MatteRequest::cutout)           optional, of a mask with a matte (cutout_plan.hpp; kernels.hpp K23; a null
//                                            destination: none): k::mask_cutout runs behind the matte, reads the coverage where
//                                            it lies and the guide, and writes the RGBA to a buffer of the slot's; one copy
//                                            command takes that to the destination when it is pinned image memory of the
//                                            library, else to pinned staging of the slot's from which finish() copies it -- all
//                                            in front of slot.done, so a cut-out costs no wait of its own
//   paint (enqueue, enqueue_device)          optional: the request is ONE job whose bytes are a label map (grid_plan.hpp,
//                                            kernels.hpp K18) -- the launch step runs k::grid_paint over the lane's grid store
//                                            in place of the post-processing kernel; planning, staging, copies and events are
//                                            those of a mask of the same size
// Contract: acquire / release are thread-safe (a mutex of the component's own around the free list, nothing else); a slot
// has one user at a time, who waits for slot.done before letting go of it, so its buffers and its plan need no lock.  The
// lane hands in what is the lane's: its stream and stage clock (used under the lane's mutex, as by the lane itself), its
// board, and per request the IoU predictions of the last decode.  The component outlives every request it was given.
#pragma once

#include "kernels/kernels.hpp"
#include "lane_board.hpp"
#include "mask_transport.hpp"
#include "prompt_plan.hpp"
#include "stage_clock.hpp"

namespace dlimg {

// What the launch step of a label-map request paints from: the lane's grid store and the kept list (SamModel::segment_grid).
struct GridPaint {
    float const* store = nullptr;
    int candidates = 0;
    k::GridKept kept{};
};

// What an edge mark asks of one mask of a request: the mark's ints (all 0: the mask is delivered as it is).
struct EdgeRequest {
    int offset = 0, feather = 0, border = 0;
    bool any() const { return offset != 0 || feather != 0 || border != 0; }
};

// What a cut-out mark asks of a mask with a matte: where the RGBA goes, and the mark's radius.
struct CutoutRequest {
    uint8_t* dst = nullptr;                 // HOST memory, [out_h][out_w][4]; null: no cut-out
    int radius = 0;
    bool any() const { return dst != nullptr; }
};

// What a matte mark asks of one mask of a request: the guide where the lane uploaded it, and the mark's ints.
struct MatteRequest {
    uint8_t const* guide = nullptr;         // device memory, [out_h][out_w][channels]; null: the mask is delivered as it is
    int channels = 0, radius = 0, eps = 0;
    CutoutRequest cutout{};                 // the cut-out mark behind the matte mark, if any
    bool any() const { return guide != nullptr; }
};

struct MaskSlot {
    DeviceBuffer<uint8_t> dev;
    PinnedBuffer pin;
    hipEvent_t done = nullptr;
    std::vector<hipEvent_t> piece_done;     // one per piece of the largest plan so far
    MaskTransportInput input;               // of the request the slot holds, kept for finish(); the vectors below are
    MaskTransportPlan plan;                 // re-used from request to request like these
    std::vector<k::PostJob> kernel_jobs;    // the caller's jobs with the destinations the plan gives the kernel
    std::vector<k::CleanJob> clean_jobs;    // the masks of the request that are cleaned, where the kernel wrote them
    DeviceBuffer<uint8_t> clean_workspace;  // labels and areas of k::mask_cleanup, pooled with the slot like `dev`
    std::vector<k::EdgeJob> edge_jobs;      // the masks of the request whose edge is moved, where the kernel wrote them
    DeviceBuffer<uint8_t> edge_workspace;   // the distances and the cells of k::mask_edge, pooled with the slot like `dev`
    std::vector<k::MatteJob> matte_jobs;    // the masks of the request that get a soft edge, where the kernel wrote them
    DeviceBuffer<uint8_t> matte_workspace;  // the A and B planes and the cells of k::mask_matte, pooled with the slot like `dev`
    DeviceBuffer<uint8_t> cutout_dev;       // the RGBA of the request's cut-out, 4 bytes per pixel, and the cells of k::mask_cutout:
    DeviceBuffer<uint8_t> cutout_workspace; // pooled with the slot likewise
    PinnedBuffer cutout_pin;                // its staging when the destination is not pinned; finish() copies cutout_bytes from
    uint8_t* cutout_dst = nullptr;          // here to cutout_dst (null: nothing to copy); set once slot.done is recorded, from
    uint8_t* cutout_staged_for = nullptr;   // what run_cutout noted: a request that failed half-way delivers no RGBA
    size_t cutout_bytes = 0;
};

class MaskTransport {
  public:
    MaskTransport(int device, hipStream_t stream, StageClock& clock, LaneBoard* board, int lane_index)
        : device_(device), stream_(stream), clock_(clock), board_(board), lane_index_(lane_index) {}
    ~MaskTransport();
    MaskTransport(MaskTransport const&) = delete;
    MaskTransport& operator=(MaskTransport const&) = delete;

    MaskSlot& acquire();
    void release(MaskSlot& s);
    void enqueue(MaskSlot& slot, k::PostJob const* jobs, int count, float const* iou, int iou_count, CleanSpec const* clean = nullptr,
                 GridPaint const* paint = nullptr, MatteRequest const* matte = nullptr, EdgeRequest const* edge = nullptr);
    void finish(MaskSlot& slot, k::PostJob const* jobs, int count, float* iou_out, int iou_count);
    void enqueue_device(MaskSlot& slot, k::PostJob const* jobs, int count, int dst_device, CleanSpec const* clean = nullptr,
                        GridPaint const* paint = nullptr, EdgeRequest const* edge = nullptr);
    void wait(MaskSlot& slot);

  private:
    hipEvent_t piece_event(MaskSlot& slot, int i);
    void run(MaskSlot& slot, k::PostJob const* jobs, int count, float const* iou, int dst_device, CleanSpec const* clean,
             GridPaint const* paint, MatteRequest const* matte = nullptr, EdgeRequest const* edge = nullptr);
    void run_cleanup(MaskSlot& slot, MaskStep const& step, CleanSpec const* clean);
    void run_edge(MaskSlot& slot, MaskStep const& step, EdgeRequest const* edge);
    void run_matte(MaskSlot& slot, MaskStep const& step, MatteRequest const* matte);
    void run_cutout(MaskSlot& slot, k::PostJob const& job, MatteRequest const& matte);

    int device_;
    hipStream_t stream_;
    StageClock& clock_;
    LaneBoard* board_;                      // null: a lane on its own
    int lane_index_;
    std::mutex mutex_;                      // guards the two lists, nothing else
    std::vector<std::unique_ptr<MaskSlot>> slots_;      // all ever made (owned)
    std::vector<MaskSlot*> free_;                       // those not handed out
};

}  // namespace dlimg
