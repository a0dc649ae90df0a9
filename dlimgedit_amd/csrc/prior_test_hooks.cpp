// Test hook of the prior-plane kernel (kernels.hpp: k::mask_prior) alone.  It lives in a library of its own,
// lib/libdlimgedit_prior_test.so (the product's objects plus this file; csrc/exports_prior_test.map): the set of hooks
// lib/libdlimgedit_test.so exports is pinned by tests/test_abi.py.  No header declares it; dlimgedit_amd/api.py
// (ext.test_prior_plane) binds it by name.
//
//   mask [h][w] u8: HOST memory.  Its device copy and the plane [256][256] fp32 are device buffers with 256 guard bytes on either
//   side; *guards_ok tells whether those are untouched after the launch.  The copy is exactly w * h bytes long inside its
//   guards: a sum that took in a byte behind the mask's last one would take in a guard byte (0xA5) and miss the reference.
//   iters > 0 (tools/prior_probe.py): the launch is then repeated iters times between two events, and *ms_out receives the
//   milliseconds of ONE launch.
#include "ext_common.hpp"

using namespace dlimg;
using namespace dlimg::extapi;

namespace {
constexpr size_t kGuard = 256;
constexpr uint8_t kGuardByte = 0xA5;

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
}  // namespace

extern "C" {

DLIMG_API int dlimg_amd_test_prior_plane(uint8_t const* mask, int w, int h, int pre_w, int pre_h, int strength_milli, float* plane_out,
                                         int* guards_ok, int iters, float* ms_out) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(mask && plane_out && guards_ok);
        DLIMG_ASSERT(w > 0 && h > 0 && (size_t)w * h <= (size_t)1 << 28);
        Guarded src((size_t)w * h);
        Guarded plane((size_t)256 * 256 * sizeof(float));
        HIP_CHECK(hipMemcpy(src.get(), mask, (size_t)w * h, hipMemcpyHostToDevice));
        auto launch = [&] { k::mask_prior(src.get(), w, h, pre_w, pre_h, strength_milli, reinterpret_cast<float*>(plane.get()), nullptr); };
        launch();
        HIP_CHECK(hipDeviceSynchronize());
        if (iters > 0 && ms_out) {
            hipEvent_t a = nullptr, b = nullptr;
            HIP_CHECK(hipEventCreate(&a));
            HIP_CHECK(hipEventCreate(&b));
            HIP_CHECK(hipEventRecord(a, nullptr));
            for (int i = 0; i < iters; ++i) launch();
            HIP_CHECK(hipEventRecord(b, nullptr));
            HIP_CHECK(hipEventSynchronize(b));
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, a, b));
            *ms_out = ms / iters;
            (void)hipEventDestroy(a);
            (void)hipEventDestroy(b);
        }
        download(reinterpret_cast<uint8_t*>(plane_out), static_cast<uint8_t const*>(plane.get()), plane.bytes);
        *guards_ok = src.intact() && plane.intact();
    });
}

}  // extern "C"
