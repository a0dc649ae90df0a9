// Which execution lanes of a GPU have work in flight: one marker event per lane, re-recorded behind everything the lane
// enqueues (encode, decode, mask transfer).  A lane that starts an encoder pass asks whether every OTHER lane's marker has
// been reached: then the pass has the GPU to itself -- the situation of a synchronous caller of slots 3 / 4, which is what
// every existing user of the reference is (/root/reference/src/include/dlimgedit/detail/dlimgedit.impl.hpp:70-116) -- and
// its one-image GEMMs may trade CU time for latency (gemm_plan.cpp, tile 11).  hipEventQuery on an event another
// thread is re-recording is allowed; a stale answer only costs or gains a tile choice, never a result (same bits).
#pragma once

#include "common.hpp"

#include <atomic>
#include <memory>

namespace dlimg {

class LaneBoard {
  public:
    LaneBoard(int device, int lanes);
    ~LaneBoard();
    LaneBoard(LaneBoard const&) = delete;
    LaneBoard& operator=(LaneBoard const&) = delete;
    void begin(int lane);                         // the lane starts enqueuing a pass: busy until the next mark() / end()
    void end(int lane) noexcept;                  // (no event: for the error path of an enqueue)
    void mark(int lane, hipStream_t stream);      // behind what the lane has just enqueued
    bool others_idle(int lane) const;
    // diagnostics: encoder passes of one image enqueued so far, and how many of them found every other lane idle
    void count_pass(bool alone) { passes_.fetch_add(1, std::memory_order_relaxed); if (alone) alone_.fetch_add(1, std::memory_order_relaxed); }
    long passes() const { return passes_.load(std::memory_order_relaxed); }
    long alone_passes() const { return alone_.load(std::memory_order_relaxed); }

  private:
    std::atomic<long> passes_{0}, alone_{0};
    std::vector<hipEvent_t> marker_;
    std::unique_ptr<std::atomic<bool>[]> armed_;
    std::unique_ptr<std::atomic<bool>[]> enqueuing_;
};

}  // namespace dlimg
