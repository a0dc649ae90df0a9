// Test hook of the prior-plane kernel (kernels.hpp: k::mask_prior) alone.  Its contract:
// include/dlimgedit/dlimgedit_amd_test.h; the Python side is ext.test_prior_plane (dlimgedit_amd/api.py).
#include "test_support.hpp"

#include <dlimgedit/dlimgedit_amd_test.h>

using namespace dlimg;
using namespace dlimg::extapi;

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
        if (iters > 0 && ms_out) *ms_out = EventPair().mean_ms(iters, launch);
        download(reinterpret_cast<uint8_t*>(plane_out), static_cast<uint8_t const*>(plane.get()), plane.bytes);
        *guards_ok = src.intact() && plane.intact();
    });
}

}  // extern "C"
