// Test hooks of the SAM-HQ kernels alone (kernels.hpp: k::hq_mask_path, k::hq_features_finish) and of the kernel that feeds
// them (k::upscale_logits), one launcher call each, on HOST operands.  Their contract:
// include/dlimgedit/dlimgedit_amd_test.h; the Python side is ext.test_hq_mask_path, ext.test_upscale_logits and
// ext.test_hq_features_finish (dlimgedit_amd/api.py).
#include "test_support.hpp"

#include <dlimgedit/dlimgedit_amd_test.h>

#include <vector>

using namespace dlimg;
using namespace dlimg::extapi;

namespace {

constexpr size_t kPixels = 256 * 256;

// A guarded device buffer that starts as a copy of n bytes of host memory.
struct GuardedCopy : Guarded {
    GuardedCopy(void const* host, size_t n) : Guarded(n) {
        DLIMG_ASSERT(host != nullptr);
        HIP_CHECK(hipMemcpy(get(), host, n, hipMemcpyHostToDevice));
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(get()); }
};

bool all_intact(std::initializer_list<Guarded const*> buffers) {
    bool ok = true;
    for (Guarded const* b : buffers) ok = b->intact() && ok;
    return ok;
}

}  // namespace

extern "C" {

DLIMG_API int dlimg_amd_test_hq_mask_path(uint16_t const* U, int P, uint16_t const* conv1_w, float const* conv1_b, float const* ln_w,
                                          float const* ln_b, uint16_t const* conv2_w, float const* conv2_b, float eps,
                                          float const* features, int n_feat, int const* feat_index, float const* hyper_hq,
                                          float* logits, uint16_t* out_H, int* guards_ok) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(U && conv1_w && conv1_b && ln_w && ln_b && conv2_w && conv2_b && features && feat_index && hyper_hq && logits &&
                     guards_ok);
        DLIMG_ASSERT(n_feat > 0 && n_feat <= k::kDecoderMaxPrompts);
        // the launcher's refusals for the prompts, on the pointers' validity alone: nothing is allocated for a refused call
        alignas(16) static const float some_features[4] = {};
        std::vector<const float*> feat(P > 0 ? P : 0, nullptr);
        for (int i = 0; i < P; ++i) {
            DLIMG_ASSERT(feat_index[i] < n_feat);
            feat[i] = feat_index[i] < 0 ? nullptr : some_features;
        }
        *guards_ok = 1;
        if (!k::hq_mask_path_prompts(feat.data(), P)) return;

        const size_t p = (size_t)P;
        GuardedCopy dU(U, p * kPixels * 32 * 2), dW1(conv1_w, 9 * 64 * 32 * 2), dB1(conv1_b, 64 * 4), dLw(ln_w, 64 * 4), dLb(ln_b, 64 * 4);
        GuardedCopy dW2(conv2_w, 9 * 32 * 64 * 2), dB2(conv2_b, 32 * 4), dF(features, (size_t)n_feat * kPixels * 32 * 4);
        GuardedCopy dHy(hyper_hq, p * 32 * 4), dL(logits, p * 4 * kPixels * 4);
        Guarded dH(p * kPixels * 64 * 2);
        for (int i = 0; i < P; ++i) feat[i] = dF.as<float>() + (size_t)feat_index[i] * kPixels * 32;
        k::HqMaskWeights w;
        w.conv1_w = dW1.as<half_t>(); w.conv1_b = dB1.as<float>(); w.ln_w = dLw.as<float>(); w.ln_b = dLb.as<float>();
        w.conv2_w = dW2.as<half_t>(); w.conv2_b = dB2.as<float>();
        k::hq_mask_path(dU.as<half_t>(), w, eps, reinterpret_cast<half_t*>(dH.get()), feat.data(), dHy.as<float>(), dL.as<float>(), P,
                        nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        download(reinterpret_cast<uint8_t*>(logits), static_cast<uint8_t const*>(dL.get()), dL.bytes);
        download(reinterpret_cast<uint8_t*>(out_H), static_cast<uint8_t const*>(dH.get()), dH.bytes);
        *guards_ok = all_intact({&dU, &dW1, &dB1, &dLw, &dLb, &dW2, &dB2, &dF, &dHy, &dL, &dH});
    });
}

DLIMG_API int dlimg_amd_test_upscale_logits(uint16_t const* keys_h, int P, uint16_t const* W1, float const* b1, float const* ln_w,
                                            float const* ln_b, float eps, uint16_t const* W2, float const* b2, float const* hyper,
                                            int store_u, float* out_logits, uint16_t* out_U, int* guards_ok) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(keys_h && W1 && b1 && ln_w && ln_b && W2 && b2 && hyper && out_logits && guards_ok);
        DLIMG_ASSERT(P > 0 && P <= k::kDecoderMaxPrompts && (!store_u || out_U));
        const size_t p = (size_t)P;
        GuardedCopy dK(keys_h, p * 4096 * 256 * 2), dW1(W1, 256 * 256 * 2), dB1(b1, 256 * 4), dLw(ln_w, 64 * 4), dLb(ln_b, 64 * 4);
        GuardedCopy dW2(W2, 128 * 64 * 2), dB2(b2, 128 * 4), dHy(hyper, p * 4 * 32 * 4);
        Guarded dL(p * 4 * kPixels * 4);
        Guarded dU(store_u ? p * kPixels * 32 * 2 : 16);
        k::upscale_logits(dK.as<half_t>(), dW1.as<half_t>(), dB1.as<float>(), dLw.as<float>(), dLb.as<float>(), eps, dW2.as<half_t>(),
                          dB2.as<float>(), dHy.as<float>(), reinterpret_cast<float*>(dL.get()), P, nullptr,
                          store_u ? reinterpret_cast<half_t*>(dU.get()) : nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        download(reinterpret_cast<uint8_t*>(out_logits), static_cast<uint8_t const*>(dL.get()), dL.bytes);
        if (store_u) download(reinterpret_cast<uint8_t*>(out_U), static_cast<uint8_t const*>(dU.get()), dU.bytes);
        *guards_ok = all_intact({&dK, &dW1, &dB1, &dLw, &dLb, &dW2, &dB2, &dHy, &dL, &dU});
    });
}

DLIMG_API int dlimg_amd_test_hq_features_finish(float const* vit, float const* emb, float const* b_vit, float const* b_emb, float* out,
                                                int* guards_ok) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(vit && emb && b_vit && b_emb && out && guards_ok);
        GuardedCopy dV(vit, (size_t)16384 * 128 * 4), dE(emb, (size_t)16384 * 128 * 4), dBv(b_vit, 32 * 4), dBe(b_emb, 32 * 4);
        Guarded dO(kPixels * 32 * 4);
        k::hq_features_finish(dV.as<float>(), dE.as<float>(), dBv.as<float>(), dBe.as<float>(), reinterpret_cast<float*>(dO.get()),
                              nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        download(reinterpret_cast<uint8_t*>(out), static_cast<uint8_t const*>(dO.get()), dO.bytes);
        *guards_ok = all_intact({&dV, &dE, &dBv, &dBe, &dO});
    });
}

}  // extern "C"
