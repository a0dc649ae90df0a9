#include "lane_board.hpp"

#include <algorithm>

namespace dlimg {

LaneBoard::LaneBoard(int device, int lanes)
    : armed_(new std::atomic<bool>[std::max(1, lanes)]), enqueuing_(new std::atomic<bool>[std::max(1, lanes)]) {
    HIP_CHECK(hipSetDevice(device));
    for (int i = 0; i < lanes; ++i) {
        hipEvent_t e = nullptr;
        HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        marker_.push_back(e);
        armed_[i].store(false);
        enqueuing_[i].store(false);
    }
}

LaneBoard::~LaneBoard() {
    for (hipEvent_t e : marker_) (void)hipEventDestroy(e);
}

void LaneBoard::begin(int lane) {
    if (lane >= 0 && lane < (int)marker_.size()) enqueuing_[lane].store(true, std::memory_order_release);
}

void LaneBoard::end(int lane) noexcept {
    if (lane >= 0 && lane < (int)marker_.size()) enqueuing_[lane].store(false, std::memory_order_release);
}

void LaneBoard::mark(int lane, hipStream_t stream) {
    if (lane < 0 || lane >= (int)marker_.size()) return;
    HIP_CHECK(hipEventRecord(marker_[lane], stream));
    armed_[lane].store(true, std::memory_order_release);
    enqueuing_[lane].store(false, std::memory_order_release);
}

bool LaneBoard::others_idle(int lane) const {
    for (int i = 0; i < (int)marker_.size(); ++i) {
        if (i == lane) continue;
        if (enqueuing_[i].load(std::memory_order_acquire)) return false;       // a pass is being enqueued there right now
        if (!armed_[i].load(std::memory_order_acquire)) continue;
        const hipError_t st = hipEventQuery(marker_[i]);
        if (st == hipErrorNotReady) return false;
        if (st != hipSuccess) (void)hipGetLastError();      // not this call's problem: treated as "busy" is the safe answer
        if (st != hipSuccess) return false;
    }
    return true;
}

}  // namespace dlimg
