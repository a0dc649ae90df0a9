// Test hooks of the SAM-HQ kernels alone (kernels.hpp: k::hq_mask_path, k::hq_features_finish) and of the kernel that feeds
// them (k::upscale_logits), one launcher call each, on HOST operands.  Their contract:
// include/dlimgedit/dlimgedit_amd_test.h; the Python side is ext.test_hq_mask_path, ext.test_upscale_logits and
// ext.test_hq_features_finish (dlimgedit_amd/api.py).  Behind them: the SAM-HQ feature branch as the product's encoder runs it
// (SamModel::run_hq_branch; ext.test_hq_branch) and the row kernels of kernels/elementwise.hip alone (k::layernorm in every
// form the launcher has, k::cast_f16, k::add_cast, k::im2col3x3; ext.test_layernorm_rows, ext.test_elementwise).
#include "test_support.hpp"

#include <dlimgedit/dlimgedit_amd_test.h>

#include <mutex>
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

// One int in host-visible memory, as SamModel::encode hands the last LayerNorm of the neck for its overflow report.
struct HostFlag {
    int* p = nullptr;
    explicit HostFlag(int value) {
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(int), hipHostMallocDefault));
        *p = value;
    }
    HostFlag(HostFlag const&) = delete;
    HostFlag& operator=(HostFlag const&) = delete;
    ~HostFlag() { (void)hipHostFree(p); }
};

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

DLIMG_API int dlimg_amd_test_hq_branch(dlimg_Environment env, int branch, uint16_t const* a, int batch, float* out_A, uint16_t* out_H,
                                       float* out_Y, uint16_t* w1, float* b1, float* ln_w, float* ln_b, uint16_t* w2, float* b2) {
    return guarded([&] {
        // every refusal is a host check in front of the first launch
        if (!env || !a) throw Exception("test_hq_branch: null pointer");
        if (branch != 0 && branch != 1) throw Exception("test_hq_branch: branch is 0 (early ViT features) or 1 (embedding)");
        if (batch < 1 || batch > 2) throw Exception("test_hq_branch: a call takes 1 or 2 images");
        SamModel& m = impl(env).lane(0, 0);
        if (!m.has_hq()) throw Exception("test_hq_branch: not a SAM-HQ model: the model file has no dec.hq.* tensors");
        std::lock_guard<std::mutex> lock(m.mutex());
        HIP_CHECK(hipSetDevice(m.device()));
        const HqBranch which = branch == 0 ? HqBranch::vit : HqBranch::emb;
        const size_t K = which == HqBranch::vit ? (size_t)m.geometry().embed_dim : (size_t)kEmbedDim;
        const size_t M = (size_t)batch * kTokens;
        Upload<half_t> dev(reinterpret_cast<half_t const*>(a), M * K);
        const SamModel::HqBranchView v = m.run_hq_branch(which, dev.get(), batch);
        m.synchronize();
        DLIMG_ASSERT((size_t)v.K == K);
        const size_t C = (size_t)v.C;
        download(out_A, v.A, M * 4 * C);
        download(reinterpret_cast<half_t*>(out_H), v.H, M * 4 * C);
        download(out_Y, v.Y, M * 4 * 128);
        download(reinterpret_cast<half_t*>(w1), v.w1, 4 * C * K);
        download(b1, v.b1, 4 * C);
        download(ln_w, v.ln_w, C);
        download(ln_b, v.ln_b, C);
        download(reinterpret_cast<half_t*>(w2), v.w2, 128 * C);
        download(b2, v.b2, 128);
    });
}

DLIMG_API int dlimg_amd_test_layernorm_rows(float const* x, float const* w, float const* b, float eps, int rows, int dim, int act,
                                            int in_place, int misalign_x, float* out_f32, uint16_t* out_f16, int* nonfinite,
                                            int* guards_ok) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(x && w && b && guards_ok && rows >= 0 && dim >= 0 && (!in_place || out_f32));
        *guards_ok = 1;
        // a refusal of the launcher for the extents needs no operands: the buffers below hold at least one element
        const size_t n = (size_t)rows * dim, nb = n ? n : 1, db_n = dim ? dim : 1;
        const size_t shift = misalign_x ? 4 : 0;                   // the device x starts 4 bytes behind a 16-byte boundary
        Guarded dx(nb * 4 + (shift ? 16 : 0));
        float* const xd = reinterpret_cast<float*>(dx.get() + shift);
        HIP_CHECK(hipMemcpy(xd, x, n * 4, hipMemcpyHostToDevice));
        GuardedCopy dw(w, db_n * 4), db(b, db_n * 4);
        Guarded o32(out_f32 && !in_place ? nb * 4 : 16), o16(out_f16 ? nb * 2 : 16);
        float* const p32 = !out_f32 ? nullptr : in_place ? xd : reinterpret_cast<float*>(o32.get());
        HostFlag flag(nonfinite ? *nonfinite : 0);
        k::layernorm(xd, dw.as<float>(), db.as<float>(), eps, rows, dim, act, p32, out_f16 ? reinterpret_cast<half_t*>(o16.get()) : nullptr,
                     nullptr, nonfinite ? flag.p : nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        download(out_f32, static_cast<float const*>(p32), out_f32 ? n : 0);
        download(reinterpret_cast<uint8_t*>(out_f16), static_cast<uint8_t const*>(o16.get()), out_f16 ? n * 2 : 0);
        if (nonfinite) *nonfinite = *flag.p;
        *guards_ok = all_intact({&dx, &dw, &db, &o32, &o16});
    });
}

DLIMG_API int dlimg_amd_test_elementwise(int op, float const* a, uint16_t const* in_h, float const* b, long long b_mod, long long n,
                                         float* out_f32, uint16_t* out_f16, int* guards_ok) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(guards_ok && op >= 0 && op <= 2 && n >= 0 && b_mod >= 0);
        *guards_ok = 1;
        if (op == 0) {                                             // k::cast_f16
            DLIMG_ASSERT(a && out_f16 && n > 0);
            GuardedCopy da(a, (size_t)n * 4);
            Guarded o16((size_t)n * 2);
            k::cast_f16(da.as<float>(), reinterpret_cast<half_t*>(o16.get()), (size_t)n, nullptr);
            HIP_CHECK(hipDeviceSynchronize());
            download(reinterpret_cast<uint8_t*>(out_f16), static_cast<uint8_t const*>(o16.get()), o16.bytes);
            *guards_ok = all_intact({&da, &o16});
        } else if (op == 1) {                                      // k::add_cast
            DLIMG_ASSERT(a && n > 0 && (out_f32 || out_f16));
            // the buffers are rounded up to whole 16-byte chunks: a length the launcher refuses allocates nothing short
            const size_t n16 = ((size_t)n + 3) / 4 * 4, b16 = ((size_t)b_mod + 3) / 4 * 4;
            Guarded da(n16 * 4), db(b ? (b16 ? b16 : 4) * 4 : 16);
            HIP_CHECK(hipMemcpy(da.get(), a, (size_t)n * 4, hipMemcpyHostToDevice));
            if (b && b_mod) HIP_CHECK(hipMemcpy(db.get(), b, (size_t)b_mod * 4, hipMemcpyHostToDevice));
            Guarded o32(out_f32 ? n16 * 4 : 16), o16(out_f16 ? n16 * 2 : 16);
            k::add_cast(reinterpret_cast<float*>(da.get()), b ? reinterpret_cast<float*>(db.get()) : nullptr, (size_t)b_mod, (size_t)n,
                        out_f32 ? reinterpret_cast<float*>(o32.get()) : nullptr, out_f16 ? reinterpret_cast<half_t*>(o16.get()) : nullptr,
                        nullptr);
            HIP_CHECK(hipDeviceSynchronize());
            download(reinterpret_cast<uint8_t*>(out_f32), static_cast<uint8_t const*>(o32.get()), out_f32 ? (size_t)n * 4 : 0);
            download(reinterpret_cast<uint8_t*>(out_f16), static_cast<uint8_t const*>(o16.get()), out_f16 ? (size_t)n * 2 : 0);
            *guards_ok = all_intact({&da, &db, &o32, &o16});
        } else {                                                   // k::im2col3x3: n images of b_mod channels
            DLIMG_ASSERT(in_h && out_f16 && n > 0 && n <= 4 && b_mod > 0 && b_mod <= 1280);
            const size_t map = (size_t)n * 4096 * (size_t)b_mod;
            GuardedCopy din(in_h, map * 2);
            Guarded o16(map * 9 * 2);
            k::im2col3x3(din.as<half_t>(), (int)n, (int)b_mod, reinterpret_cast<half_t*>(o16.get()), nullptr);
            HIP_CHECK(hipDeviceSynchronize());
            download(reinterpret_cast<uint8_t*>(out_f16), static_cast<uint8_t const*>(o16.get()), o16.bytes);
            *guards_ok = all_intact({&din, &o16});
        }
    });
}

}  // extern "C"
