// Completion events of one execution lane: record() puts an event behind everything the lane's stream holds; whoever waits
// for it gives it back, from any thread.  Contract: thread-safe by itself (a mutex of its own around the pool, never held
// across a HIP call that waits); record() is called by whoever enqueues, i.e. under the lane's mutex; every event handed out
// comes back through wait_and_recycle() or poll_and_recycle() before the pool is destroyed.
#pragma once

#include "common.hpp"

namespace dlimg {

class CompletionEvents {
  public:
    explicit CompletionEvents(hipStream_t stream) : stream_(stream) {}
    ~CompletionEvents() { for (auto e : pool_) (void)hipEventDestroy(e); }
    CompletionEvents(CompletionEvents const&) = delete;
    CompletionEvents& operator=(CompletionEvents const&) = delete;

    hipEvent_t record() {
        hipEvent_t e = nullptr;
        {
            std::lock_guard<std::mutex> lock(mutex_);
            if (!pool_.empty()) {
                e = pool_.back();
                pool_.pop_back();
            }
        }
        if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(e, stream_));
        return e;
    }
    void wait_and_recycle(hipEvent_t e) {
        const hipError_t err = hipEventSynchronize(e);
        recycle(e);
        HIP_CHECK(err);
    }
    bool poll_and_recycle(hipEvent_t e) {       // true (and the event is taken back) once it has completed
        const hipError_t err = hipEventQuery(e);
        if (err == hipErrorNotReady) return false;
        recycle(e);
        HIP_CHECK(err);
        return true;
    }

  private:
    void recycle(hipEvent_t e) {
        std::lock_guard<std::mutex> lock(mutex_);
        pool_.push_back(e);
    }
    hipStream_t stream_;
    std::mutex mutex_;
    std::vector<hipEvent_t> pool_;
};

}  // namespace dlimg
