// Test hook of the label-map kernels (kernels.hpp: k::grid_harvest, k::grid_paint) alone.  It lives in a library of its own,
// lib/libdlimgedit_grid_test.so (the product's objects plus this file; csrc/exports_grid_test.map): the set of hooks
// lib/libdlimgedit_test.so exports is pinned by tests/test_abi.py.  No header declares it; dlimgedit_amd/api.py
// (ext.test_grid_kernels) binds it by name.
//
//   planes4 [prompts][4][256][256], iou4 [prompts][4]: HOST memory, what a decode leaves for the prompts of a grid.  The planes
//   are harvested in chunks of 16 prompts, as the runtime harvests the chunks of its decodes; records_out [3 prompts][8] and
//   store_out [3 prompts][256][256] (optional) receive what the harvest left.  n_kept_in >= 0: kept_in are the candidates to
//   paint, in label order; n_kept_in < 0: they are selected on the host from the records and iou4 (csrc/grid_plan.hpp) with the
//   two thresholds.  kept_out [255] / n_kept_out receive the painted list, map_out [out_h][out_w] the label map.  Store,
//   records and map are device buffers with 256 guard bytes on either side; *guards_ok tells whether those are untouched.
//   iters > 0 (tools/grid_probe.py): the harvest of all chunks and the paint launch are then repeated iters times each between
//   two events, and ms_out[0] / ms_out[1] receive the milliseconds of ONE harvest of all candidates / ONE paint launch.
#include "ext_common.hpp"
#include "grid_plan.hpp"

#include <cstring>
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

DLIMG_API int dlimg_amd_test_grid_kernels(float const* planes4, int prompts, float const* iou4, int out_w, int out_h, int pre_w, int pre_h,
                                          int iou_permille, int stability_permille, int const* kept_in, int n_kept_in, int cull,
                                          int32_t* records_out, float* store_out, uint8_t* map_out, int* kept_out, int* n_kept_out,
                                          int* guards_ok, int iters, float* ms_out) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(planes4 && prompts > 0 && prompts <= 1024 && records_out && map_out && guards_ok);
        DLIMG_ASSERT(out_w > 0 && out_h > 0 && (size_t)out_w * out_h <= (size_t)1 << 28);
        DLIMG_ASSERT(n_kept_in < 0 ? iou4 != nullptr : (n_kept_in <= k::kGridMaxKept && (n_kept_in == 0 || kept_in)));
        const int candidates = 3 * prompts;
        Upload<float> planes(planes4, (size_t)prompts * 4 * k::kGridPlaneFloats);
        Guarded store((size_t)candidates * k::kGridPlaneFloats * sizeof(float));
        Guarded records((size_t)candidates * sizeof(GridRecord));
        Guarded map((size_t)out_w * out_h);
        constexpr int kChunk = 16;
        auto harvest = [&] {
            for (int p0 = 0; p0 < prompts; p0 += kChunk)
                k::grid_harvest(planes.get() + (size_t)p0 * 4 * k::kGridPlaneFloats, std::min(kChunk, prompts - p0), 3 * p0, pre_w, pre_h,
                                reinterpret_cast<float*>(store.get()), candidates, reinterpret_cast<int32_t*>(records.get()), nullptr);
        };
        harvest();
        HIP_CHECK(hipDeviceSynchronize());
        std::vector<GridRecord> rec(candidates);
        download(reinterpret_cast<uint8_t*>(rec.data()), static_cast<uint8_t const*>(records.get()), records.bytes);
        std::memcpy(records_out, rec.data(), records.bytes);
        std::vector<int> kept(kept_in, kept_in + (n_kept_in > 0 ? n_kept_in : 0));
        if (n_kept_in < 0) {
            std::vector<float> iou(candidates);
            for (int c = 0; c < candidates; ++c) iou[c] = iou4[4 * (c / 3) + 1 + c % 3];
            kept = select_grid_segments(rec.data(), iou.data(), candidates, iou_permille, stability_permille).kept;
        }
        k::GridKept list{};
        list.count = (int)kept.size();
        for (int i = 0; i < list.count; ++i) {
            DLIMG_ASSERT(kept[i] >= 0 && kept[i] < candidates);
            list.candidate[i] = kept[i];
            list.cull[i] = rec[kept[i]].cull;
        }
        auto paint = [&] {
            k::grid_paint(reinterpret_cast<float const*>(store.get()), candidates, list, map.get(), out_w, out_h, pre_w, pre_h, cull != 0, nullptr);
        };
        paint();
        HIP_CHECK(hipDeviceSynchronize());
        if (iters > 0 && ms_out) {
            hipEvent_t a = nullptr, b = nullptr;
            HIP_CHECK(hipEventCreate(&a));
            HIP_CHECK(hipEventCreate(&b));
            auto timed = [&](auto&& launch) {
                HIP_CHECK(hipEventRecord(a, nullptr));
                for (int i = 0; i < iters; ++i) launch();
                HIP_CHECK(hipEventRecord(b, nullptr));
                HIP_CHECK(hipEventSynchronize(b));
                float ms = 0;
                HIP_CHECK(hipEventElapsedTime(&ms, a, b));
                return ms / iters;
            };
            ms_out[0] = timed(harvest);
            ms_out[1] = timed(paint);
            (void)hipEventDestroy(a);
            (void)hipEventDestroy(b);
        }
        download(map_out, static_cast<uint8_t const*>(map.get()), map.bytes);
        if (store_out) download(reinterpret_cast<uint8_t*>(store_out), static_cast<uint8_t const*>(store.get()), store.bytes);
        if (kept_out) std::copy(kept.begin(), kept.end(), kept_out);
        if (n_kept_out) *n_kept_out = list.count;
        *guards_ok = store.intact() && records.intact() && map.intact();
    });
}

}  // extern "C"
