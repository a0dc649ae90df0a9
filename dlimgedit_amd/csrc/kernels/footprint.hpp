// The footprint of a low-res index: the source pixels one pixel of the 256 x 256 low-res grid stands for, along one axis of
// `size` source pixels that was encoded at `pre`.  Shared by the prior plane (mask_prior.hip), which sums over footprints, and
// the lasso derivation (mask_lasso.hip, lasso_plan.hpp), which maps low-res cells back to image pixels; usable from plain host
// code (no HIP header needed).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DLIMG_FOOTPRINT_HD __host__ __device__
#else
#define DLIMG_FOOTPRINT_HD
#endif

namespace dlimg {

// first source index and one past the last of low-res index i along an axis of `size` source pixels encoded at `pre`
DLIMG_FOOTPRINT_HD inline int footprint_lo(int i, int size, int pre) { return (int)((int64_t)4 * i * size / pre); }
DLIMG_FOOTPRINT_HD inline int footprint_hi(int i, int size, int pre) {
    const int64_t e = 4 * i + 4 < pre ? 4 * i + 4 : pre;
    return (int)((e * size + pre - 1) / pre);
}

}  // namespace dlimg
