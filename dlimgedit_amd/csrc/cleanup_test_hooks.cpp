// Test hook of the mask clean-up kernels (kernels.hpp: k::mask_cleanup) alone.  It lives in a library of its own,
// lib/libdlimgedit_cleanup_test.so (the product's objects plus this file; csrc/exports_cleanup_test.map): the set of hooks
// lib/libdlimgedit_test.so exports is pinned by tests/test_abi.py.  No header declares it; dlimgedit_amd/api.py
// (ext.test_mask_cleanup) binds it by name.
//
//   masks[i]: HOST memory, w[i] * h[i] bytes of 0 / 255 in packed rows, cleaned in place with max_hole[i] / max_island[i].
//   All `count` masks are ONE k::mask_cleanup call on the current device's null stream.  The launcher's refusals (shapes,
//   thresholds, a null mask) arrive as the call's error; nothing is allocated or copied for a list the launcher refuses for
//   its shapes.
#include "ext_common.hpp"

#include <vector>

using namespace dlimg;
using namespace dlimg::extapi;

extern "C" {

DLIMG_API int dlimg_amd_test_mask_cleanup(uint8_t* const* masks, int const* w, int const* h, int const* max_hole,
                                          int const* max_island, int count) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(count > 0 && masks && w && h && max_hole && max_island);
        std::vector<k::CleanJob> jobs(count);
        for (int i = 0; i < count; ++i) jobs[i] = k::CleanJob{nullptr, w[i], h[i], max_hole[i], max_island[i]};
        const size_t bytes = k::mask_cleanup_workspace_bytes(jobs.data(), count);      // shapes and thresholds are checked here
        std::vector<Upload<uint8_t>> dev;
        dev.reserve(count);
        for (int i = 0; i < count; ++i) {
            dev.emplace_back(masks[i], (size_t)w[i] * h[i]);
            jobs[i].mask = dev.back().get();                                           // null stays null: the launcher's refusal
        }
        DeviceBuffer<uint8_t> workspace;
        workspace.reserve(bytes);
        k::mask_cleanup(jobs.data(), count, workspace.get(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        for (int i = 0; i < count; ++i) download(masks[i], static_cast<uint8_t const*>(jobs[i].mask), (size_t)w[i] * h[i]);
    });
}

}  // extern "C"
