// Test hooks of the two encoder-neck launches (kernels.hpp: k::neck_conv1x1_ln, k::neck_conv3x3_ln), one per entry point, on
// DEVICE buffers, as SamModel::encode calls them.  Their contract: include/dlimgedit/dlimgedit_amd_test.h; the Python side is
// ext.test_neck_conv_ln (dlimgedit_amd/api.py).
#include "ext_common.hpp"

#include <dlimgedit/dlimgedit_amd_test.h>

#include <vector>

namespace dlimg {
namespace {

using namespace extapi;

// The destinations of SamModel::encode's last launch: image i's fp32 result goes to out_f32[i] where that is given, else to its
// place in the workspace.  The non-finite report is read once the launch has completed.
template <typename F>
void run_neck_hook(int B, float* const* out_f32, float* workspace, int* out_flag, F&& launch) {
    require_gpu();
    DLIMG_ASSERT(B > 0 && out_flag != nullptr);
    std::vector<float*> dst(B, nullptr);
    bool any = false;
    for (int i = 0; i < B; ++i) {
        dst[i] = (out_f32 && out_f32[i]) ? out_f32[i] : (workspace ? workspace + (size_t)i * kTokens * kEmbedDim : nullptr);
        any = any || dst[i];
    }
    int* flag = nullptr;
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&flag), sizeof(int), hipHostMallocDefault));
    *flag = 0;
    struct FreeFlag { int* p; ~FreeFlag() { (void)hipHostFree(p); } } free_flag{flag};
    k::NeckOutputs out;
    out.out_f32 = any ? dst.data() : nullptr;
    out.nonfinite = flag;
    launch(out);
    HIP_CHECK(hipDeviceSynchronize());
    *out_flag = *const_cast<volatile int*>(flag);
}

}  // namespace
}  // namespace dlimg

using namespace dlimg;

extern "C" {

DLIMG_API int dlimg_amd_test_neck_conv1x1_ln(void const* in, int B, int K, void const* w, float const* gamma, float const* beta,
                                             float eps, void* out_f16, float* const* out_f32, float* workspace, int* out_flag) {
    return guarded([&] {
        run_neck_hook(B, out_f32, workspace, out_flag, [&](k::NeckOutputs& out) {
            out.out_h = static_cast<half_t*>(out_f16);
            k::neck_conv1x1_ln(static_cast<half_t const*>(in), B, K, static_cast<half_t const*>(w), gamma, beta, eps, out, nullptr);
        });
    });
}

DLIMG_API int dlimg_amd_test_neck_conv3x3_ln(void const* in, int B, void const* w, float const* gamma, float const* beta, float eps,
                                             void* out_f16, float* const* out_f32, float* workspace, int* out_flag) {
    return guarded([&] {
        DeviceBuffer<half_t> zeros(64);
        HIP_CHECK(hipMemset(zeros.get(), 0, 64 * sizeof(half_t)));
        run_neck_hook(B, out_f32, workspace, out_flag, [&](k::NeckOutputs& out) {
            out.out_h = static_cast<half_t*>(out_f16);
            k::neck_conv3x3_ln(static_cast<half_t const*>(in), B, static_cast<half_t const*>(w), zeros.get(), gamma, beta, eps, out,
                               nullptr);
        });
    });
}

}  // extern "C"
