#include "stage_clock.hpp"

namespace dlimg {

StageClock::~StageClock() {
    for (auto& p : pending_) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    for (auto e : event_pool_) (void)hipEventDestroy(e);
}

void StageClock::set_profiling(bool on) {
    flush_events();
    profiling_ = on;
}

void StageClock::flush_events() {
    if (pending_.empty()) return;
    HIP_CHECK(hipStreamSynchronize(stream_));
    for (auto& p : pending_) {
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, p.a, p.b));
        stats_.ms[p.st] += ms;
        stats_.work[p.st] += p.work;
        stats_.launches[p.st] += p.launches;
        for (Stage extra : {p.also, p.shape}) {
            if (extra == ST_COUNT) continue;
            stats_.ms[extra] += ms;
            stats_.work[extra] += p.work;
            stats_.launches[extra] += p.launches;
        }
        event_pool_.push_back(p.a);
        event_pool_.push_back(p.b);
    }
    pending_.clear();
}

StageStats StageClock::take_stats() {
    flush_events();
    StageStats s = stats_;
    stats_ = StageStats{};
    return s;
}

hipEvent_t StageClock::take_event() {
    hipEvent_t e;
    if (!event_pool_.empty()) {
        e = event_pool_.back();
        event_pool_.pop_back();
    } else {
        HIP_CHECK(hipEventCreate(&e));
    }
    return e;
}

}  // namespace dlimg
