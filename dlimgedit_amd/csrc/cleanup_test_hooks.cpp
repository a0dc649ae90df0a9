// Test hook of the mask clean-up kernels (kernels.hpp: k::mask_cleanup) alone.  Its contract:
// include/dlimgedit/dlimgedit_amd_test.h; the Python side is ext.test_mask_cleanup (dlimgedit_amd/api.py).
#include "ext_common.hpp"

#include <dlimgedit/dlimgedit_amd_test.h>

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
