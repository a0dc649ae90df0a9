// What the kernels that take box sums over a clipped (2r+1)^2 window share (mask_matte.hip, mask_cutout.hip; mask_edge.hip takes the cells alone): a workgroup of
// BLOCK threads takes a strip of BLOCK - 2r columns by a band of rows, thread t owning column x0 - r + t; column sums slide
// down the band in registers and block_scan turns a row of them into prefixes, so that a window sum is prefix[x + r] -
// prefix[x - r - 1].  The smallest and largest byte of every CELL x CELL cell of a plane (cell_extremes) let a block learn from
// a few ints whether the plane is one value over its pixels and their halo (uniform_over).
#pragma once

#include "device_common.hpp"

namespace dlimg {
namespace boxwin {

constexpr int BLOCK = 256;
constexpr int BAND = 128;        // the matte's; the cut-out, whose rows cost more, takes shorter bands of its own (mask_cutout.hip)
constexpr int CELL = 64;

// Inclusive scan of one value per thread over the block: prefix[t + 1] = v(0) + .. + v(t), prefix[0] = 0.  The caller places a
// __syncthreads() between this and its reads of prefix; totals and prefix alternate between two copies from row to row, so no
// third barrier is needed.
template <typename T, int K>
DLIMG_DEVICE void block_scan(T (&v)[K], T (*prefix)[BLOCK + 1], T (*totals)[K]) {
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T up = __shfl_up(v[k], d, 64);
            if (lane >= d) v[k] += up;
        }
    }
    if (lane == 63)
#pragma unroll
        for (int k = 0; k < K; ++k) totals[wave][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        T base = 0;
        for (int i = 0; i < wave; ++i) base += totals[i][k];
        prefix[k][t + 1] = v[k] + base;
        if (t == 0) prefix[k][0] = 0;
    }
}

// One workgroup: lo | hi << 8 of cell `cell` (row-major over cells_x cells a row) of plane [h][w] into cells[cell].
DLIMG_DEVICE void cell_extremes(const uint8_t* plane, int w, int h, int cells_x, int cell, int* cells) {
    __shared__ int s_lo, s_hi;
    const int x0 = (cell % cells_x) * CELL, y0 = (cell / cells_x) * CELL;
    const int t = (int)threadIdx.x;
    if (t == 0) {
        s_lo = 255;
        s_hi = 0;
    }
    __syncthreads();
    int lo = 255, hi = 0;
    const int x = x0 + (t & 63);
    if (x < w)
        for (int y = y0 + (t >> 6); y < y0 + CELL && y < h; y += BLOCK / 64) {
            const int v = plane[(size_t)y * w + x];
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    atomicMin(&s_lo, lo);
    atomicMax(&s_hi, hi);
    __syncthreads();
    if (t == 0) cells[cell] = s_lo | (s_hi << 8);
}

// The smallest and the largest byte of the plane over the pixels [xa, xb] x [ya, yb] (clipped to the image), by the cells that
// touch them.  Every thread of the block calls it and gets the same answer.  Job: w, h, cells, cells_x.
template <typename Job>
DLIMG_DEVICE void extremes_over(Job const& job, int xa, int xb, int ya, int yb, int* smallest, int* largest) {
    __shared__ int u_lo, u_hi;
    const int t = (int)threadIdx.x;
    if (t == 0) {
        u_lo = 255;
        u_hi = 0;
    }
    __syncthreads();
    xa = xa < 0 ? 0 : xa;
    ya = ya < 0 ? 0 : ya;
    xb = xb > job.w - 1 ? job.w - 1 : xb;
    yb = yb > job.h - 1 ? job.h - 1 : yb;
    const int cx0 = xa / CELL, cx1 = xb / CELL, cy0 = ya / CELL, cy1 = yb / CELL;
    const int nx = cx1 - cx0 + 1, n = nx * (cy1 - cy0 + 1);
    int lo = 255, hi = 0;
    for (int i = t; i < n; i += BLOCK) {
        const int c = job.cells[(cy0 + i / nx) * job.cells_x + cx0 + i % nx];
        lo = (c & 255) < lo ? (c & 255) : lo;
        hi = (c >> 8) > hi ? (c >> 8) : hi;
    }
    if (t < n) {
        atomicMin(&u_lo, lo);
        atomicMax(&u_hi, hi);
    }
    __syncthreads();
    *smallest = u_lo;
    *largest = u_hi;
}

// Whether the plane is one value there, by the same cells; the value in *value.
template <typename Job>
DLIMG_DEVICE bool uniform_over(Job const& job, int xa, int xb, int ya, int yb, int* value) {
    int hi;
    extremes_over(job, xa, xb, ya, yb, value, &hi);
    return *value == hi;
}

}  // namespace boxwin
}  // namespace dlimg
