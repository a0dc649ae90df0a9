// Test hook of the lasso derivation (kernels.hpp: k::lasso_derive) alone.  It lives in a library of its own,
// lib/libdlimgedit_lasso_test.so (the product's objects plus this file; csrc/exports_lasso_test.map): the set of hooks
// lib/libdlimgedit_test.so exports is pinned by tests/test_abi.py.  No header declares it; dlimgedit_amd/api.py
// (ext.test_lasso_derive) binds it by name.
//
//   mask [h][w] u8: HOST memory, of an image that was encoded at pre_w x pre_h.  Upload, k::mask_prior (default strength),
//   k::lasso_derive and the fold of lasso_plan.hpp, behind plain host buffers: record_out [8] = {inside cells, box x0, y0, x1,
//   y1, click x, click y, d2}.  The mask's device copy, the plane, g and the row records are device buffers with 256 guard bytes
//   on either side; *guards_ok tells whether those are untouched after the launches.
//   iters > 0 (tools/lasso_probe.py): the two derive launches are then repeated iters times between two events, and *ms_out
//   receives the milliseconds of ONE derivation (both launches).
#include "ext_common.hpp"
#include "lasso_plan.hpp"

#include <vector>

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

DLIMG_API int dlimg_amd_test_lasso_derive(uint8_t const* mask, int w, int h, int pre_w, int pre_h, int32_t* record_out, int* guards_ok,
                                          int iters, float* ms_out) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(mask && record_out && guards_ok);
        DLIMG_ASSERT(w > 0 && h > 0 && (size_t)w * h <= (size_t)1 << 28);
        constexpr size_t kCells = (size_t)kLassoRows * kLassoRows, kRowInts = (size_t)kLassoRows * kLassoRowRecordInts;
        Guarded src((size_t)w * h);
        Guarded plane(kCells * sizeof(float));
        Guarded g(kCells * sizeof(int32_t));
        Guarded rows(kRowInts * sizeof(int32_t));
        HIP_CHECK(hipMemcpy(src.get(), mask, (size_t)w * h, hipMemcpyHostToDevice));
        k::mask_prior(src.get(), w, h, pre_w, pre_h, kPriorDefaultStrength, reinterpret_cast<float*>(plane.get()), nullptr);
        auto launch = [&] {
            k::lasso_derive(reinterpret_cast<float const*>(plane.get()), pre_w, pre_h, reinterpret_cast<int*>(g.get()),
                            reinterpret_cast<int*>(rows.get()), nullptr);
        };
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
        std::vector<int32_t> host(kRowInts);
        download(reinterpret_cast<uint8_t*>(host.data()), static_cast<uint8_t const*>(rows.get()), rows.bytes);
        fold_lasso_rows(host.data(), w, h, pre_w, pre_h, record_out);
        *guards_ok = src.intact() && plane.intact() && g.intact() && rows.intact();
    });
}

}  // extern "C"
