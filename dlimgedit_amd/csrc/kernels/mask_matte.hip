// K21  matte marks: an image-guided soft edge for a delivered mask (He et al.'s guided filter with a grey guide), in place on
// masks in device memory, in integers throughout (kernels.hpp has the definition; tests/matte_ref.py restates it in numpy).
//
// Both passes are box sums over the clipped (2r+1)^2 window.  Integer sums are exact whichever way they are taken, so a pass
// keeps COLUMN sums over 2r+1 rows in registers and slides them down the image (one row added, one taken off per step), and a
// block-wide inclusive scan in LDS turns a row of column sums into window sums, prefix[x + r] - prefix[x - r - 1].  Columns and
// rows outside the image contribute nothing, which is the clipping.
//
// Three launches for up to 16 jobs of any sizes, the job taken from the grid; no atomics on global memory, no waiting:
//   K0 matte_cells   one workgroup per 64 x 64 cell of a mask: its smallest and largest byte, one int per cell.
//   K1 matte_ab      one workgroup per (strip of 256 - 2r columns) x (band of 128 rows); thread t owns column x0 - r + t, so the
//                    outer r threads on either side only feed the scan.  Four column sums (G, p, G^2, G p; 32 bits), then
//                    A and B per pixel: two 64-bit divisions, emulated; 8 bytes written per pixel (LABNOTES has what was measured).
//                    Grey is computed from the guide where it is read.
//   K2 matte_out     the same over the A and B planes (column sums in 64 bits), one grey read per pixel, the mask written in
//                    place: K2 reads A, B and the guide only, never the mask.
// The shortcut: where the mask is one value v over a block's pixels and their r halo, K1 writes A = 0, B = v 2^16 (what the
// formulas give there) without reading the guide or dividing; where it is one value over the 2r halo, K2 writes nothing --
// the bytes are v already.  Both are read off the cells of K0 (whole cells: a conservative test).  It pays on a mask with large
// uniform areas; on a noisy mask no block qualifies and the cells launch is pure cost.
//
// Widths: a column sum of G p over 65 rows is at most 65 * 255^2 < 2^23, the prefix over 256 columns of G^2 < 2^31; sums are
// unsigned, so even a wrapped prefix would leave the difference exact.  A fits 23 bits, B 31; the column sums of K2 are 64 bits.
#include "box_window.hpp"
#include "kernels.hpp"

namespace dlimg {
namespace {

using boxwin::BAND;        // the strips, bands, cells and scan mask_cutout.hip has too
using boxwin::BLOCK;
using boxwin::CELL;
using boxwin::block_scan;
using boxwin::cell_extremes;
using boxwin::uniform_over;
constexpr int MAX_JOBS = 16;
constexpr int F = 16;
constexpr int MAX_RADIUS = 32, MAX_EPS = 65025;
constexpr long long MAX_GRID = (1ll << 24) - 1;       // workgroups of one launch: gridDim.x * 256 threads stays below 2^32

typedef unsigned long long u64;
typedef long long i64;

struct PassJob {
    uint8_t* mask;
    const uint8_t* guide;
    int* A;
    int* B;
    int* cells;
    int w, h, channels, radius, eps;
    int strips, block_begin, cells_x, cells_y, cell_begin;
};
struct PassPack {
    PassJob j[MAX_JOBS];
    int n;
    int shortcut;
};

DLIMG_DEVICE int job_of_block(PassPack const& pack, int block) {
    int j = 0;
    for (int i = 1; i < pack.n; ++i)
        if (block >= pack.j[i].block_begin) j = i;
    return j;
}
DLIMG_DEVICE int job_of_cell(PassPack const& pack, int cell) {
    int j = 0;
    for (int i = 1; i < pack.n; ++i)
        if (cell >= pack.j[i].cell_begin) j = i;
    return j;
}

DLIMG_DEVICE int grey_at(const uint8_t* guide, int channels, size_t p) {
    if (channels == 1) return guide[p];
    const uint8_t* g = guide + p * (size_t)channels;
    return ((int)g[0] + 2 * (int)g[1] + (int)g[2] + 2) >> 2;
}

// floor(n / d), d > 0: one unsigned division
DLIMG_DEVICE i64 floor_div(i64 n, i64 d) {
    if (n >= 0) return (i64)((u64)n / (u64)d);
    return -(i64)(((u64)(-n) + (u64)d - 1ull) / (u64)d);
}

__global__ __launch_bounds__(BLOCK) void matte_cells_kernel(PassPack pack) {
    const PassJob job = pack.j[job_of_cell(pack, (int)blockIdx.x)];
    cell_extremes(job.mask, job.w, job.h, job.cells_x, (int)blockIdx.x - job.cell_begin, job.cells);
}

__global__ __launch_bounds__(BLOCK) void matte_ab_kernel(PassPack pack) {
    __shared__ unsigned prefix[2][4][BLOCK + 1];
    __shared__ unsigned totals[2][BLOCK / 64][4];
    const PassJob job = pack.j[job_of_block(pack, (int)blockIdx.x)];
    const int b = (int)blockIdx.x - job.block_begin;
    const int r = job.radius, w = job.w, h = job.h, so = BLOCK - 2 * r;
    const int x0 = (b % job.strips) * so, y0 = (b / job.strips) * BAND;
    const int y1 = y0 + BAND < h ? y0 + BAND : h;
    const int t = (int)threadIdx.x, x = x0 - r + t;
    const bool in_col = x >= 0 && x < w;
    const bool is_out = t >= r && t < BLOCK - r && x < w;
    int value = 0;
    if (pack.shortcut && uniform_over(job, x0 - r, x0 + so - 1 + r, y0 - r, y1 - 1 + r, &value)) {
        if (is_out)
            for (int y = y0; y < y1; ++y) {
                const size_t p = (size_t)y * w + x;
                job.A[p] = 0;
                job.B[p] = value << F;
            }
        return;
    }
    unsigned cG = 0, cP = 0, cGG = 0, cGP = 0;
    auto take = [&](int y, bool add) {
        if (!in_col) return;
        const size_t p = (size_t)y * w + x;
        const unsigned g = (unsigned)grey_at(job.guide, job.channels, p), m = job.mask[p];
        if (add) {
            cG += g; cP += m; cGG += g * g; cGP += g * m;
        } else {
            cG -= g; cP -= m; cGG -= g * g; cGP -= g * m;
        }
    };
    {
        // rows y0 - r - 1 .. y0 + r - 1: the first step adds row y0 + r and takes row y0 - r - 1 off
        const int ya = y0 - r - 1 < 0 ? 0 : y0 - r - 1, yb = y0 + r - 1 > h - 1 ? h - 1 : y0 + r - 1;
        for (int y = ya; y <= yb; ++y) take(y, true);
    }
    const int xl = x - r < 0 ? 0 : x - r, xr = x + r > w - 1 ? w - 1 : x + r;
    for (int y = y0; y < y1; ++y) {
        if (y + r < h) take(y + r, true);
        if (y - r - 1 >= 0) take(y - r - 1, false);
        const int buf = (y - y0) & 1;
        unsigned v[4] = {cG, cP, cGG, cGP};
        block_scan<unsigned, 4>(v, prefix[buf], totals[buf]);
        __syncthreads();
        if (!is_out) continue;
        const unsigned sG = prefix[buf][0][t + r + 1] - prefix[buf][0][t - r], sP = prefix[buf][1][t + r + 1] - prefix[buf][1][t - r];
        const unsigned sGG = prefix[buf][2][t + r + 1] - prefix[buf][2][t - r], sGP = prefix[buf][3][t + r + 1] - prefix[buf][3][t - r];
        const int yt = y - r < 0 ? 0 : y - r, yd = y + r > h - 1 ? h - 1 : y + r;
        const i64 N = (i64)(xr - xl + 1) * (yd - yt + 1);
        const i64 cov = N * (i64)sGP - (i64)sG * (i64)sP;
        const i64 den = N * (i64)sGG - (i64)sG * (i64)sG + (i64)job.eps * N * N;
        const i64 a = floor_div(2 * cov * ((i64)1 << F) + den, 2 * den);
        const i64 bb = floor_div(2 * ((i64)sP * ((i64)1 << F) - a * (i64)sG) + N, 2 * N);
        const size_t p = (size_t)y * w + x;
        job.A[p] = (int)a;
        job.B[p] = (int)bb;
    }
}

__global__ __launch_bounds__(BLOCK) void matte_out_kernel(PassPack pack) {
    __shared__ u64 prefix[2][2][BLOCK + 1];
    __shared__ u64 totals[2][BLOCK / 64][2];
    const PassJob job = pack.j[job_of_block(pack, (int)blockIdx.x)];
    const int b = (int)blockIdx.x - job.block_begin;
    const int r = job.radius, w = job.w, h = job.h, so = BLOCK - 2 * r;
    const int x0 = (b % job.strips) * so, y0 = (b / job.strips) * BAND;
    const int y1 = y0 + BAND < h ? y0 + BAND : h;
    const int t = (int)threadIdx.x, x = x0 - r + t;
    const bool in_col = x >= 0 && x < w;
    const bool is_out = t >= r && t < BLOCK - r && x < w;
    int value = 0;
    if (pack.shortcut && uniform_over(job, x0 - 2 * r, x0 + so - 1 + 2 * r, y0 - 2 * r, y1 - 1 + 2 * r, &value)) return;
    u64 cA = 0, cB = 0;
    auto take = [&](int y, bool add) {
        if (!in_col) return;
        const size_t p = (size_t)y * w + x;
        const u64 a = (u64)(i64)job.A[p], bb = (u64)(i64)job.B[p];
        if (add) {
            cA += a; cB += bb;
        } else {
            cA -= a; cB -= bb;
        }
    };
    {
        // rows y0 - r - 1 .. y0 + r - 1: the first step adds row y0 + r and takes row y0 - r - 1 off
        const int ya = y0 - r - 1 < 0 ? 0 : y0 - r - 1, yb = y0 + r - 1 > h - 1 ? h - 1 : y0 + r - 1;
        for (int y = ya; y <= yb; ++y) take(y, true);
    }
    const int xl = x - r < 0 ? 0 : x - r, xr = x + r > w - 1 ? w - 1 : x + r;
    for (int y = y0; y < y1; ++y) {
        if (y + r < h) take(y + r, true);
        if (y - r - 1 >= 0) take(y - r - 1, false);
        const int buf = (y - y0) & 1;
        u64 v[2] = {cA, cB};
        block_scan<u64, 2>(v, prefix[buf], totals[buf]);
        __syncthreads();
        if (!is_out) continue;
        const i64 sA = (i64)(prefix[buf][0][t + r + 1] - prefix[buf][0][t - r]), sB = (i64)(prefix[buf][1][t + r + 1] - prefix[buf][1][t - r]);
        const int yt = y - r < 0 ? 0 : y - r, yd = y + r > h - 1 ? h - 1 : y + r;
        const int N = (xr - xl + 1) * (yd - yt + 1);
        const size_t p = (size_t)y * w + x;
        const i64 q = sA * (i64)grey_at(job.guide, job.channels, p) + sB;
        // fdiv(2 q + N 2^F, 2 N 2^F) = fdiv(fdiv(2 q + N 2^F, 2^(F+1)), N): the shift floors, and what is left fits 32 bits
        const int n = (int)((2 * q + (i64)N * ((i64)1 << F)) >> (F + 1));
        int o = n >= 0 ? n / N : -((-n + N - 1) / N);
        o = o < 0 ? 0 : (o > 255 ? 255 : o);
        job.mask[p] = (uint8_t)o;
    }
}

size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }
int cells_of(int extent) { return (extent + CELL - 1) / CELL; }
int blocks_x(const k::MatteJob& j) { return (j.w + (BLOCK - 2 * j.radius) - 1) / (BLOCK - 2 * j.radius); }      // strips
int blocks_y(const k::MatteJob& j) { return (j.h + BAND - 1) / BAND; }                                          // bands

// Throws on the first bad job; returns nothing the kernels rely on.
void check_jobs(const k::MatteJob* jobs, int count, bool pointers) {
    if (count < 0 || (count > 0 && !jobs)) throw_error("mask_matte: invalid job list");
    for (int i = 0; i < count; ++i) {
        const k::MatteJob& j = jobs[i];
        if (j.w <= 0 || j.h <= 0) throw_error("mask_matte: invalid extent");
        if ((long long)j.w * (long long)j.h > 0x7fffffffLL) throw_error("mask_matte: w * h does not fit an int");
        if (j.channels != 1 && j.channels != 3 && j.channels != 4) throw_error("mask_matte: channels is 1, 3 or 4");
        if (j.radius < 1 || j.radius > MAX_RADIUS) throw_error("mask_matte: radius is 1 .. 32");
        if (j.eps < 1 || j.eps > MAX_EPS) throw_error("mask_matte: eps is 1 .. 65025");
        // an extent so thin that one mask alone needs more workgroups than a launch takes (1 x 2^31 - 1, say): no image is such
        if ((long long)blocks_x(j) * blocks_y(j) > MAX_GRID || (long long)cells_of(j.w) * cells_of(j.h) > MAX_GRID)
            throw_error("mask_matte: invalid extent: too many rows for its width");
        if (pointers && !j.mask) throw_error("mask_matte: null mask");
        if (pointers && !j.guide) throw_error("mask_matte: null guide");
    }
}

// per job: the A and B planes, 4 bytes per pixel each, and one int per 64 x 64 cell
size_t plane_words(const k::MatteJob& j) { return round_up((size_t)j.w * j.h, 4); }
size_t cell_words(const k::MatteJob& j) { return round_up((size_t)cells_of(j.w) * cells_of(j.h), 4); }

// The launches of one call, in order; dry: counted only.  Returns their number.
int run_passes(const k::MatteJob* jobs, int count, void* workspace, hipStream_t s, bool shortcut, bool dry) {
    int launches = 0;
    int* const words = static_cast<int*>(workspace);
    PassPack pack{};
    pack.shortcut = shortcut ? 1 : 0;
    long long blocks = 0, cells = 0;
    auto launch = [&] {
        if (pack.n == 0) return;
        launches += 3;
        if (!dry) hipLaunchKernelGGL(matte_cells_kernel, dim3((unsigned)cells), dim3(BLOCK), 0, s, pack);
        if (!dry) hipLaunchKernelGGL(matte_ab_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, pack);
        if (!dry) hipLaunchKernelGGL(matte_out_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, pack);
        pack.n = 0;
        blocks = cells = 0;
    };
    size_t at = 0;
    for (int i = 0; i < count; ++i) {
        const k::MatteJob& j = jobs[i];
        const size_t mine = at;
        at += 2 * plane_words(j) + cell_words(j);
        const int strips = blocks_x(j), bands = blocks_y(j);
        const long long nb = (long long)strips * bands, nc = (long long)cells_of(j.w) * cells_of(j.h);
        if (pack.n == MAX_JOBS || blocks + nb > MAX_GRID || cells + nc > MAX_GRID) launch();
        if (!dry)
            pack.j[pack.n] = PassJob{j.mask, j.guide, words + mine, words + mine + plane_words(j), words + mine + 2 * plane_words(j),
                                     j.w, j.h, j.channels, j.radius, j.eps, strips, (int)blocks, cells_of(j.w), cells_of(j.h), (int)cells};
        ++pack.n;
        blocks += nb;
        cells += nc;
    }
    launch();
    return launches;
}

}  // namespace

namespace k {

size_t mask_matte_workspace_bytes(const MatteJob* jobs, int count) {
    check_jobs(jobs, count, false);
    size_t bytes = 0;
    for (int i = 0; i < count; ++i) bytes += (2 * plane_words(jobs[i]) + cell_words(jobs[i])) * sizeof(int);
    return bytes;
}

int mask_matte_launches(const MatteJob* jobs, int count) {
    check_jobs(jobs, count, false);
    return run_passes(jobs, count, nullptr, nullptr, true, true);
}

void mask_matte(const MatteJob* jobs, int count, void* workspace, hipStream_t s, bool shortcut) {
    check_jobs(jobs, count, true);
    if (count == 0) return;
    if (!workspace) throw_error("mask_matte: null workspace");
    run_passes(jobs, count, workspace, s, shortcut, false);
}

}  // namespace k
}  // namespace dlimg
