// Test hook of the edge kernels (kernels.hpp: k::mask_edge) alone; the Python side is ext.test_edge (dlimgedit_amd/api.py).
// It lives in lib/libdlimgedit_matte_hooks.so beside the matte's, the stroke's and the cut-out's (build.py: SIDE_HOOK_SOURCES)
// and is declared here, in no header: include/dlimgedit/dlimgedit_amd_test.h is a closed list (tests/test_abi.py).
//
// dlimg_amd_test_edge: `count` (1 .. 64) jobs in ONE call of the launcher.  masks[i] [h][w] u8: HOST memory; masks[i] receives
// the result.  Every mask and the workspace are device buffers of exactly their size with 256 guard bytes on either side;
// *guards_ok tells whether those are untouched after the launches.  A NULL masks[i] reaches the launcher as a null mask (which
// it refuses).  shortcut 0: the blocks whose mask is of one polarity over their halo are computed like any other.
// *launches_out (optional): k::mask_edge_launches for the jobs.  iters > 0 (tools/edge_probe.py): the call is then repeated
// iters times between two events, each time on the masks as they were given (a device copy goes back first), and ms_out[0]
// receives the milliseconds of ONE call with its copies, ms_out[1] those of the copies alone, timed the same way: a
// device-to-device hipMemcpyAsync of w * h bytes per job, the probe's yardstick for the memory system.
#include "test_support.hpp"

#include <dlimgedit/dlimgedit.h>

#include <memory>
#include <vector>

using namespace dlimg;
using namespace dlimg::extapi;

extern "C" {

DLIMG_API int dlimg_amd_test_edge(uint8_t* const* masks, int const* w, int const* h, int const* offset, int const* feather,
                                  int const* border, int count, int shortcut, int* guards_ok, int* launches_out, int iters,
                                  float* ms_out) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(masks && w && h && offset && feather && border && guards_ok && count > 0 && count <= 64);
        std::vector<std::unique_ptr<Guarded>> bufs;
        std::vector<k::EdgeJob> jobs(count);
        for (int i = 0; i < count; ++i) jobs[i] = k::EdgeJob{nullptr, w[i], h[i], offset[i], feather[i], border[i]};
        // the launcher's own refusals come first: nothing is allocated for a job it does not take
        const size_t ws_bytes = k::mask_edge_workspace_bytes(jobs.data(), count);
        for (int i = 0; i < count; ++i) {
            if (!masks[i]) continue;            // a null mask: the launcher refuses it
            const size_t px = (size_t)w[i] * h[i];
            bufs.push_back(std::make_unique<Guarded>(px));
            HIP_CHECK(hipMemcpy(bufs.back()->get(), masks[i], px, hipMemcpyHostToDevice));
            jobs[i].mask = bufs.back()->get();
        }
        Guarded ws(ws_bytes);
        if (launches_out) *launches_out = k::mask_edge_launches(jobs.data(), count);
        auto launch = [&] { k::mask_edge(jobs.data(), count, ws.get(), nullptr, shortcut != 0); };
        launch();
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        if (iters > 0 && ms_out) {
            // every repetition starts from the mask as it was given: a device copy of it goes back in front of the launches
            // (w * h bytes read and written per job on top of the kernels' own traffic); the last one leaves the result
            std::vector<std::unique_ptr<Upload<uint8_t>>> given;
            for (int i = 0; i < count; ++i) given.push_back(std::make_unique<Upload<uint8_t>>(masks[i], (size_t)w[i] * h[i]));
            auto restore = [&] {
                for (int i = 0; i < count; ++i)
                    HIP_CHECK(hipMemcpyAsync(jobs[i].mask, given[i]->get(), (size_t)w[i] * h[i], hipMemcpyDeviceToDevice, nullptr));
            };
            ms_out[1] = EventPair().mean_ms(iters, restore);
            ms_out[0] = EventPair().mean_ms(iters, [&] {
                restore();
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
