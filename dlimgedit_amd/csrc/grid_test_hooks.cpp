// Test hook of the label-map kernels (kernels.hpp: k::grid_harvest, k::grid_paint) alone.  Its contract:
// include/dlimgedit/dlimgedit_amd_test.h; the Python side is ext.test_grid_kernels (dlimgedit_amd/api.py).
#include "test_support.hpp"
#include "grid_plan.hpp"

#include <dlimgedit/dlimgedit_amd_test.h>

#include <cstring>
#include <vector>

using namespace dlimg;
using namespace dlimg::extapi;

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
            EventPair events;
            ms_out[0] = events.mean_ms(iters, harvest);
            ms_out[1] = events.mean_ms(iters, paint);
        }
        download(map_out, static_cast<uint8_t const*>(map.get()), map.bytes);
        if (store_out) download(reinterpret_cast<uint8_t*>(store_out), static_cast<uint8_t const*>(store.get()), store.bytes);
        if (kept_out) std::copy(kept.begin(), kept.end(), kept_out);
        if (n_kept_out) *n_kept_out = list.count;
        *guards_ok = store.intact() && records.intact() && map.intact();
    });
}

}  // extern "C"
