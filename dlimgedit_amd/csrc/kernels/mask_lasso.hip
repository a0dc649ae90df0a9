// K20  lasso marks: the box of a selection and its most interior cell, from the 256 x 256 fp32 plane k::mask_prior has just
// written (kernels.hpp, k::lasso_derive; lasso_plan.hpp folds the row records and maps cells to image pixels).
//
// A cell (x, y) of the scored region (x < sw, y < sh) is INSIDE when its plane value is positive; every other cell of Z^2 is
// background.  d2(x, y), for an inside cell, is the exact squared Euclidean distance to the nearest background cell -- an
// integer.  The transform is separable: g(x', y) is the vertical distance of (x', y) to the nearest background cell of its
// column (0 when the cell is background itself), and d2(x, y) = min over x' of (x - x')^2 + g(x', y)^2, the columns -1 and sw
// (background throughout) included.  Everything is integer arithmetic, so the records are the same bits wherever they are
// computed (tests/lasso_ref.py restates them in numpy).
//
// Two launches, no waiting between workgroups, no atomics on global memory, plain vector stores:
//   lasso_columns  one workgroup per low-res column, one thread per row.  The column's inside bits go to LDS as four 64-bit
//                  ballots; a thread finds the nearest zero bit above and below its own with clz / ctz.  Writes g [256][256]
//                  int32 (a strided store of 4 bytes per thread: 256 KB in all).
//   lasso_rows     one workgroup per low-res row, one thread per column, the row's g^2 in LDS (1 KB).  A thread runs over the
//                  256 columns (every lane reads the same LDS word: a broadcast, no bank conflict), 65536 inner steps per
//                  workgroup instead of the 16.7 M one workgroup would need for the plane.  The row's inside count, its first
//                  and last inside column and its best cell (largest d2, then smallest x) are reduced with LDS atomics and
//                  written as one record of 8 int32.
// What bounds them: neither bandwidth (512 KB read, 264 KB written) nor arithmetic (a workgroup's 256 steps of four integer
// operations per lane) -- the two launches and the dependent LDS round trips inside them are latency.  256 workgroups of 256
// threads and about 1 KB of LDS each: one workgroup per CU, occupancy is no limit.
#include "device_common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace dlimg {
namespace {

constexpr int LOW = 256;

__global__ __launch_bounds__(LOW) void lasso_columns_kernel(const float* plane, int sw, int sh, int* g) {
    __shared__ unsigned long long bits[LOW / 64];
    const int x = blockIdx.x, y = threadIdx.x;
    const bool inside = x < sw && y < sh && plane[y * LOW + x] > 0.f;
    const unsigned long long wave_bits = __ballot(inside);
    if ((y & 63) == 0) bits[y >> 6] = wave_bits;
    __syncthreads();
    int dist = 0;
    if (inside) {
        const int w = y >> 6, b = y & 63;
        // the nearest background row above: the highest zero bit below bit y, or row -1
        int up = y + 1;
        for (int ww = w; ww >= 0; --ww) {
            unsigned long long m = ~bits[ww];
            if (ww == w) m &= (1ull << b) - 1ull;
            if (m) {
                up = y - (ww * 64 + 63 - __builtin_clzll(m));
                break;
            }
        }
        // the nearest background row below: the lowest zero bit above bit y, or row 256 (rows sh .. 255 are zero bits)
        int down = LOW - y;
        for (int ww = w; ww < LOW / 64; ++ww) {
            unsigned long long m = ~bits[ww];
            if (ww == w) m = b == 63 ? 0ull : (m & (~0ull << (b + 1)));
            if (m) {
                down = ww * 64 + __builtin_ctzll(m) - y;
                break;
            }
        }
        dist = up < down ? up : down;
    }
    g[y * LOW + x] = dist;
}

__global__ __launch_bounds__(LOW) void lasso_rows_kernel(const int* g, int sw, int* rows) {
    __shared__ int g2[LOW];
    __shared__ int count, x_min, x_max;
    __shared__ unsigned best;                    // d2 << 8 | 255 - x: the largest d2, then the smallest x
    const int y = blockIdx.x, x = threadIdx.x;
    const int mine = g[y * LOW + x];
    g2[x] = mine * mine;
    if (x == 0) {
        count = 0;
        x_min = LOW;
        x_max = -1;
        best = 0u;
    }
    __syncthreads();
    if (mine > 0) {                              // inside: x < sw
        const int left = x + 1, right = sw - x;  // the columns -1 and sw are background throughout
        int d2 = left * left < right * right ? left * left : right * right;
        for (int xx = 0; xx < LOW; ++xx) {
            const int dx = x - xx, cand = dx * dx + g2[xx];
            d2 = cand < d2 ? cand : d2;
        }
        // d2 <= mine^2 <= 128^2: the key fits
        atomicAdd(&count, 1);
        atomicMin(&x_min, x);
        atomicMax(&x_max, x);
        atomicMax(&best, ((unsigned)d2 << 8) | (unsigned)(LOW - 1 - x));
    }
    __syncthreads();
    if (x < k::kLassoRowInts) {
        int v = 0;
        if (count > 0) {
            if (x == 0) v = count;
            if (x == 1) v = x_min;
            if (x == 2) v = x_max;
            if (x == 3) v = LOW - 1 - (int)(best & 255u);
            if (x == 4) v = (int)(best >> 8);
        }
        rows[y * k::kLassoRowInts + x] = v;
    }
}

}  // namespace

namespace k {

void lasso_derive(const float* plane, int pre_w, int pre_h, int* g_scratch, int* rows, hipStream_t s) {
    if (!plane || !g_scratch || !rows) throw_error("lasso_derive: null buffer");
    if (pre_w <= 0 || pre_h <= 0 || pre_w > 4 * LOW || pre_h > 4 * LOW) throw_error("lasso_derive: invalid extent");
    const int sw = (pre_w + 3) / 4, sh = (pre_h + 3) / 4;
    hipLaunchKernelGGL(lasso_columns_kernel, dim3(LOW), dim3(LOW), 0, s, plane, sw, sh, g_scratch);
    hipLaunchKernelGGL(lasso_rows_kernel, dim3(LOW), dim3(LOW), 0, s, (const int*)g_scratch, sw, rows);
}

}  // namespace k
}  // namespace dlimg
