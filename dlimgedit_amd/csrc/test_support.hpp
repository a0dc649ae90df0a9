// Helpers of the test hooks (*_test_hooks.cpp) only: no source of the product library includes this file.
#pragma once

#include "ext_common.hpp"

namespace dlimg {
namespace extapi {

constexpr size_t kGuard = 256;
constexpr uint8_t kGuardByte = 0xA5;

// A device buffer of n bytes with kGuard bytes of kGuardByte on either side; intact(): both guards are as they were written.
struct Guarded {
    DeviceBuffer<uint8_t> buf;
    size_t bytes;
    explicit Guarded(size_t n) : bytes(n) {
        buf.reserve(n + 2 * kGuard);
        HIP_CHECK(hipMemset(buf.get(), kGuardByte, n + 2 * kGuard));
    }
    uint8_t* get() const { return buf.get() + kGuard; }
    bool intact() const {
        uint8_t g[2 * kGuard];
        HIP_CHECK(hipMemcpy(g, buf.get(), kGuard, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(g + kGuard, buf.get() + kGuard + bytes, kGuard, hipMemcpyDeviceToHost));
        for (uint8_t v : g)
            if (v != kGuardByte) return false;
        return true;
    }
};

// Two events on the null stream, destroyed on every path out.  mean_ms: `iters` back-to-back calls of launch() between them,
// the milliseconds of one.
struct EventPair {
    struct Event {                                  // a member of its own each: the first is destroyed when the second's creation throws
        hipEvent_t e = nullptr;
        Event() { HIP_CHECK(hipEventCreate(&e)); }
        Event(Event const&) = delete;
        Event& operator=(Event const&) = delete;
        ~Event() { (void)hipEventDestroy(e); }
    };
    Event a, b;
    template <typename F> float mean_ms(int iters, F&& launch) {
        HIP_CHECK(hipEventRecord(a.e, nullptr));
        for (int i = 0; i < iters; ++i) launch();
        HIP_CHECK(hipEventRecord(b.e, nullptr));
        HIP_CHECK(hipEventSynchronize(b.e));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, a.e, b.e));
        return ms / iters;
    }
};

}  // namespace extapi
}  // namespace dlimg
