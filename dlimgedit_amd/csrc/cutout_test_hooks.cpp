// Test hook of the cut-out kernels (kernels.hpp: k::mask_cutout) alone; the Python side is ext.test_cutout (dlimgedit_amd/api.py).
// It lives in lib/libdlimgedit_matte_hooks.so beside the matte's and the stroke's (build.py: SIDE_HOOK_SOURCES) and is declared
// here, in no header.
//
// dlimg_amd_test_cutout: `count` (1 .. 64) jobs in ONE call of the launcher.  coverages[i] [h][w] u8, guides[i] [h][w][channels]
// u8 and outs[i] [h][w][4] u8: HOST memory; outs[i] receives the RGBA, and coverages[i] and guides[i] are written back from the
// device as the kernels left them (the caller compares them with what it gave).  Every coverage, guide and output and the
// workspace are device buffers of exactly their size with 256 guard bytes on either side; *guards_ok tells whether those are
// untouched after the launches.  A NULL guides[i] reaches the launcher as a null guide (which it refuses).  shortcut 0: the
// blocks whose coverage is 0 or 255 over their halo are computed like any other.  *launches_out (optional):
// k::mask_cutout_launches for the jobs.  iters > 0 (tools/cutout_probe.py): the call is then repeated iters times between two
// events, and *ms_out receives the milliseconds of ONE call.
#include "test_support.hpp"

#include <dlimgedit/dlimgedit.h>

#include <memory>
#include <vector>

using namespace dlimg;
using namespace dlimg::extapi;

extern "C" {

DLIMG_API int dlimg_amd_test_cutout(uint8_t* const* coverages, uint8_t* const* guides, uint8_t* const* outs, int const* w, int const* h,
                                    int const* channels, int const* radius, int count, int shortcut, int* guards_ok, int* launches_out,
                                    int iters, float* ms_out) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(coverages && guides && outs && w && h && channels && radius && guards_ok && count > 0 && count <= 64);
        std::vector<std::unique_ptr<Guarded>> bufs;
        std::vector<k::CutoutJob> jobs(count);
        for (int i = 0; i < count; ++i) {
            DLIMG_ASSERT(coverages[i] != nullptr && outs[i] != nullptr);
            jobs[i] = k::CutoutJob{nullptr, nullptr, nullptr, w[i], h[i], channels[i], radius[i]};
        }
        // the launcher's own refusals come first: nothing is allocated for a job it does not take
        const size_t ws_bytes = k::mask_cutout_workspace_bytes(jobs.data(), count);
        for (int i = 0; i < count; ++i) {
            const size_t px = (size_t)w[i] * h[i];
            bufs.push_back(std::make_unique<Guarded>(px));
            HIP_CHECK(hipMemcpy(bufs.back()->get(), coverages[i], px, hipMemcpyHostToDevice));
            jobs[i].coverage = bufs.back()->get();
            bufs.push_back(std::make_unique<Guarded>(px * 4));
            jobs[i].out = bufs.back()->get();
            if (!guides[i]) continue;           // a null guide: the launcher refuses it
            bufs.push_back(std::make_unique<Guarded>(px * channels[i]));
            HIP_CHECK(hipMemcpy(bufs.back()->get(), guides[i], px * channels[i], hipMemcpyHostToDevice));
            jobs[i].guide = bufs.back()->get();
        }
        Guarded ws(ws_bytes);
        if (launches_out) *launches_out = k::mask_cutout_launches(jobs.data(), count);
        auto launch = [&] { k::mask_cutout(jobs.data(), count, ws.get(), nullptr, shortcut != 0); };
        launch();
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        if (iters > 0 && ms_out) *ms_out = EventPair().mean_ms(iters, launch);      // (the inputs are read only: nothing to restore)
        for (int i = 0; i < count; ++i) {
            const size_t px = (size_t)w[i] * h[i];
            download(outs[i], static_cast<uint8_t const*>(jobs[i].out), px * 4);
            download(coverages[i], jobs[i].coverage, px);
            download(guides[i], jobs[i].guide, px * channels[i]);
        }
        bool ok = ws.intact();
        for (auto const& b : bufs) ok = ok && b->intact();
        *guards_ok = ok;
    });
}

}  // extern "C"
