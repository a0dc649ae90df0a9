// Test hook of the matte kernels (kernels.hpp: k::mask_matte) alone; the Python side is ext.test_matte (dlimgedit_amd/api.py).
// The hooks of lib/libdlimgedit_test.so and their declarations in include/dlimgedit/dlimgedit_amd_test.h are a closed list
// (tests/test_abi.py holds both to it), so this one is built into a library of its own, lib/libdlimgedit_matte_hooks.so
// (build.py), and declared here.
//
// dlimg_amd_test_matte: `count` (1 .. 64) jobs in ONE call of the launcher.  masks[i] [h][w] u8 and guides[i] [h][w][channels]
// u8: HOST memory; masks[i] receives the matte.  Every mask, every guide and the workspace are device buffers of exactly their
// size with 256 guard bytes on either side; *guards_ok tells whether those are untouched after the launches.  A NULL
// guides[i] reaches the launcher as a null guide (which it refuses).  shortcut 0: the blocks whose mask is one value over
// their halo are computed like any other.  *launches_out (optional): k::mask_matte_launches for the jobs.  iters > 0
// (tools/matte_probe.py): the call is then repeated iters times between two events, each time on the masks as they were
// given (a device copy goes back first), and *ms_out receives the milliseconds of ONE call.
#include "test_support.hpp"

#include <dlimgedit/dlimgedit.h>

#include <memory>
#include <vector>

using namespace dlimg;
using namespace dlimg::extapi;

extern "C" {

DLIMG_API int dlimg_amd_test_matte(uint8_t* const* masks, uint8_t const* const* guides, int const* w, int const* h, int const* channels,
                                   int const* radius, int const* eps, int count, int shortcut, int* guards_ok, int* launches_out,
                                   int iters, float* ms_out) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(masks && guides && w && h && channels && radius && eps && guards_ok && count > 0 && count <= 64);
        std::vector<std::unique_ptr<Guarded>> bufs;
        std::vector<k::MatteJob> jobs(count);
        for (int i = 0; i < count; ++i) {
            DLIMG_ASSERT(masks[i] != nullptr);
            jobs[i] = k::MatteJob{nullptr, nullptr, w[i], h[i], channels[i], radius[i], eps[i]};
        }
        // the launcher's own refusals come first: nothing is allocated for a job it does not take
        const size_t ws_bytes = k::mask_matte_workspace_bytes(jobs.data(), count);
        for (int i = 0; i < count; ++i) {
            const size_t px = (size_t)w[i] * h[i];
            bufs.push_back(std::make_unique<Guarded>(px));
            HIP_CHECK(hipMemcpy(bufs.back()->get(), masks[i], px, hipMemcpyHostToDevice));
            jobs[i].mask = bufs.back()->get();
            if (!guides[i]) continue;           // a null guide: the launcher refuses it
            bufs.push_back(std::make_unique<Guarded>(px * channels[i]));
            HIP_CHECK(hipMemcpy(bufs.back()->get(), guides[i], px * channels[i], hipMemcpyHostToDevice));
            jobs[i].guide = bufs.back()->get();
        }
        Guarded ws(ws_bytes);
        if (launches_out) *launches_out = k::mask_matte_launches(jobs.data(), count);
        auto launch = [&] { k::mask_matte(jobs.data(), count, ws.get(), nullptr, shortcut != 0); };
        launch();
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        if (iters > 0 && ms_out) {
            // every repetition starts from the mask as it was given: a device copy of it goes back in front of the launches
            // (w * h bytes read and written per job on top of the matte's own traffic); the last one leaves the result
            std::vector<std::unique_ptr<Upload<uint8_t>>> given;
            for (int i = 0; i < count; ++i) given.push_back(std::make_unique<Upload<uint8_t>>(masks[i], (size_t)w[i] * h[i]));
            *ms_out = EventPair().mean_ms(iters, [&] {
                for (int i = 0; i < count; ++i)
                    HIP_CHECK(hipMemcpyAsync(jobs[i].mask, given[i]->get(), (size_t)w[i] * h[i], hipMemcpyDeviceToDevice, nullptr));
                launch();
            });
        }
        for (int i = 0; i < count; ++i) download(masks[i], static_cast<uint8_t const*>(jobs[i].mask), (size_t)w[i] * h[i]);
        bool ok = ws.intact();
        for (auto const& b : bufs) ok = ok && b->intact();
        *guards_ok = ok;
    });
}

}  // extern "C"
