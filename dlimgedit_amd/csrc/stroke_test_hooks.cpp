// Test hook of the stroke derivation (kernels.hpp: k::stroke_derive) alone; the Python side is ext.test_stroke_derive
// (dlimgedit_amd/api.py).  Like the matte hook (matte_test_hooks.cpp) it lives in lib/libdlimgedit_matte_hooks.so, outside the
// closed list of the test library's hooks, and is declared here.
//
// dlimg_amd_test_stroke_derive: map [h][w] u8, HOST memory, of an image that was encoded at pre_w x pre_h; clicks 1 .. 8.  The
// map, the ballots and the record are device buffers of exactly their size with 256 guard bytes on either side; *guards_ok tells
// whether those are untouched after the launches.  record_out: the 20 int32 of the record, in CELLS (stroke_plan.hpp maps them to
// pixels); bits_out: the [256][4] u64 ballots.  iters > 0 (tools/stroke_probe.py): the two launches are then repeated iters times
// between two events and *ms_out receives the milliseconds of ONE derivation.
#include "test_support.hpp"

#include <dlimgedit/dlimgedit.h>

using namespace dlimg;
using namespace dlimg::extapi;

extern "C" {

DLIMG_API int dlimg_amd_test_stroke_derive(uint8_t const* map, int w, int h, int pre_w, int pre_h, int clicks, int32_t* record_out,
                                           uint64_t* bits_out, int* guards_ok, int iters, float* ms_out) {
    return guarded([&] {
        require_gpu();
        DLIMG_ASSERT(map && record_out && bits_out && guards_ok);
        DLIMG_ASSERT(w > 0 && h > 0 && (size_t)w * h <= (size_t)1 << 28);
        Guarded src((size_t)w * h);
        Guarded bits((size_t)k::kStrokeBallotWords * sizeof(uint64_t));
        Guarded record((size_t)k::kStrokeRecordInts * sizeof(int32_t));
        HIP_CHECK(hipMemcpy(src.get(), map, (size_t)w * h, hipMemcpyHostToDevice));
        auto launch = [&] {
            k::stroke_derive(src.get(), w, h, pre_w, pre_h, clicks, reinterpret_cast<unsigned long long*>(bits.get()),
                             reinterpret_cast<int32_t*>(record.get()), nullptr);
        };
        launch();
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        if (iters > 0 && ms_out) *ms_out = EventPair().mean_ms(iters, launch);
        HIP_CHECK(hipMemcpy(record_out, record.get(), record.bytes, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(bits_out, bits.get(), bits.bytes, hipMemcpyDeviceToHost));
        *guards_ok = src.intact() && bits.intact() && record.intact();
    });
}

}  // extern "C"
