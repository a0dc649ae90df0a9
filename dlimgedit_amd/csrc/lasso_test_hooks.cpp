// Test hook of the lasso derivation (kernels.hpp: k::lasso_derive) alone.  Its contract:
// include/dlimgedit/dlimgedit_amd_test.h; the Python side is ext.test_lasso_derive (dlimgedit_amd/api.py).
#include "test_support.hpp"
#include "lasso_plan.hpp"

#include <dlimgedit/dlimgedit_amd_test.h>

#include <vector>

using namespace dlimg;
using namespace dlimg::extapi;

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
        if (iters > 0 && ms_out) *ms_out = EventPair().mean_ms(iters, launch);
        std::vector<int32_t> host(kRowInts);
        download(reinterpret_cast<uint8_t*>(host.data()), static_cast<uint8_t const*>(rows.get()), rows.bytes);
        fold_lasso_rows(host.data(), w, h, pre_w, pre_h, record_out);
        *guards_ok = src.intact() && plane.intact() && g.intact() && rows.intact();
    });
}

}  // extern "C"
