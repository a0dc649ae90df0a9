// K23  cut-out marks: a matte's foreground colours as RGBA, one pass of Forte's Blur-Fusion in integers throughout (kernels.hpp
// has the definition; tests/cutout_ref.py restates it in numpy).
//
// The box sums are the matte's (box_window.hpp): COLUMN sums over 2r+1 rows slide down a band in registers, a block-wide
// inclusive scan in LDS turns a row of them into window sums.  Seven sums per column: a, the three I_c, the three I_c a.
//
// Two launches for up to 16 jobs of any sizes, the job taken from the grid; no atomics on global memory, no waiting:
//   K0 cutout_cells  one workgroup per 64 x 64 cell of a coverage: its smallest and largest byte, one int per cell.
//   K1 cutout_out    one workgroup per (strip of 256 - 2r columns) x (band of 32 rows); thread t owns column x0 - r + t, so the
//                    outer r threads on either side only feed the scan.  Per pixel and channel two weighted means and the
//                    correction; 4 bytes written per pixel in one store.  Reads coverage and guide only.
// The shortcut: where the coverage is 0, or 255, over a block's pixels and their r halo, every window has S_a == 0, or S_b == 0
// and a == 255, and the formulas give the guide's own colour: K1 copies it under that alpha without summing or dividing.  It is
// read off the cells of K0 (whole cells: a conservative test), which is most of a photograph around one object.
//
// The divisions: S_Ia <= 255 S_a, so with S_Ia = q S_a + rem the mean fdiv(512 S_Ia + S_a, 2 S_a) is 256 q + fdiv(512 rem + S_a,
// 2 S_a), and 512 rem + S_a < 513 * 255 * 65^2 < 2^30: two 32-bit divisions stand for the one of 64 bits by 32.  Likewise
// 2 D = 2^9 * 65025 and 0 < 2 num + D < 2^34, so the last division is a shift and a 32-bit division by a constant.
//
// Widths: a column sum of I a over 65 rows is at most 65 * 255^2 < 2^23, its prefix over 256 columns < 2^31; sums are unsigned,
// so even a wrapped prefix would leave the difference exact.  Fh, Bh <= 65280; a Fh and the bracket of num fit 32 bits signed,
// num itself does not.
#include "box_window.hpp"
#include "kernels.hpp"

namespace dlimg {
namespace {

using boxwin::BLOCK;
using boxwin::CELL;
using boxwin::block_scan;
using boxwin::cell_extremes;
using boxwin::uniform_over;

// Rows of a band.  A block walks its rows one after the other (two barriers and a scan a row), so a launch lasts as long as one
// block does however few blocks there are: at 4000 x 3000 the matte's 128 rows make 432 blocks of 0.45 ms each, 32 rows make 1728
// that all fit the GPU at once.  The price is the 2r + 1 rows a block sums up before its first row, loads without scans
// (LABNOTES has both measured).
constexpr int BAND = 32;
constexpr int MAX_JOBS = 16;
constexpr int MAX_RADIUS = 32;
constexpr int SUMS = 7;                               // a, I_0 .. I_2, I_0 a .. I_2 a
constexpr long long MAX_GRID = (1ll << 24) - 1;       // workgroups of one launch: gridDim.x * 256 threads stays below 2^32
constexpr long long D = 65025ll * 256;

typedef long long i64;
typedef unsigned long long u64;

struct PassJob {
    const uint8_t* coverage;
    const uint8_t* guide;
    uint32_t* out;
    int* cells;
    int w, h, channels, radius;
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

// the first three channels of pixel p, c0 in the low byte (a fourth channel in the high one, to be masked off by the caller)
DLIMG_DEVICE unsigned colours_at(const uint8_t* guide, int channels, size_t p) {
    if (channels == 4) return reinterpret_cast<const uint32_t*>(guide)[p];
    const uint8_t* g = guide + p * 3;
    return (unsigned)g[0] | ((unsigned)g[1] << 8) | ((unsigned)g[2] << 16);
}

// fdiv(512 s + d, 2 d) for d > 0, s <= 255 d, d <= 255 * 65^2 (see above)
DLIMG_DEVICE unsigned mean_256(unsigned s, unsigned d) {
    const unsigned q = s / d, rem = s - q * d;
    return 256u * q + (512u * rem + d) / (2u * d);
}

__global__ __launch_bounds__(BLOCK) void cutout_cells_kernel(PassPack pack) {
    const PassJob job = pack.j[job_of_cell(pack, (int)blockIdx.x)];
    cell_extremes(job.coverage, job.w, job.h, job.cells_x, (int)blockIdx.x - job.cell_begin, job.cells);
}

__global__ __launch_bounds__(BLOCK) void cutout_out_kernel(PassPack pack) {
    __shared__ unsigned prefix[2][SUMS][BLOCK + 1];
    __shared__ unsigned totals[2][BLOCK / 64][SUMS];
    const PassJob job = pack.j[job_of_block(pack, (int)blockIdx.x)];
    const int b = (int)blockIdx.x - job.block_begin;
    const int r = job.radius, w = job.w, h = job.h, so = BLOCK - 2 * r;
    const int x0 = (b % job.strips) * so, y0 = (b / job.strips) * BAND;
    const int y1 = y0 + BAND < h ? y0 + BAND : h;
    const int t = (int)threadIdx.x, x = x0 - r + t;
    const bool in_col = x >= 0 && x < w;
    const bool is_out = t >= r && t < BLOCK - r && x < w;
    int value = 0;
    if (pack.shortcut && uniform_over(job, x0 - r, x0 + so - 1 + r, y0 - r, y1 - 1 + r, &value) && (value == 0 || value == 255)) {
        if (is_out)
            for (int y = y0; y < y1; ++y) {
                const size_t p = (size_t)y * w + x;
                job.out[p] = (colours_at(job.guide, job.channels, p) & 0xffffffu) | ((unsigned)value << 24);
            }
        return;
    }
    unsigned col[SUMS] = {0, 0, 0, 0, 0, 0, 0};
    auto take = [&](int y, bool add) {
        if (!in_col) return;
        const size_t p = (size_t)y * w + x;
        const unsigned a = job.coverage[p], rgb = colours_at(job.guide, job.channels, p);
        unsigned v[SUMS];
        v[0] = a;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[1 + c] = (rgb >> (8 * c)) & 255u;
            v[4 + c] = v[1 + c] * a;
        }
#pragma unroll
        for (int k = 0; k < SUMS; ++k) col[k] = add ? col[k] + v[k] : col[k] - v[k];
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
        unsigned v[SUMS];
#pragma unroll
        for (int k = 0; k < SUMS; ++k) v[k] = col[k];
        block_scan<unsigned, SUMS>(v, prefix[buf], totals[buf]);
        __syncthreads();
        if (!is_out) continue;
        unsigned s[SUMS];
#pragma unroll
        for (int k = 0; k < SUMS; ++k) s[k] = prefix[buf][k][t + r + 1] - prefix[buf][k][t - r];
        const int yt = y - r < 0 ? 0 : y - r, yd = y + r > h - 1 ? h - 1 : y + r;
        const unsigned N = (unsigned)((xr - xl + 1) * (yd - yt + 1));
        const size_t p = (size_t)y * w + x;
        const unsigned a = job.coverage[p], rgb = colours_at(job.guide, job.channels, p);
        const unsigned sA = s[0], sB = 255u * N - sA;
        unsigned o = a << 24;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned I = (rgb >> (8 * c)) & 255u;
            const unsigned sIa = s[4 + c], sIb = 255u * s[1 + c] - sIa;
            const unsigned Fh = sA > 0 ? mean_256(sIa, sA) : 256u * I;
            const unsigned Bh = sB > 0 ? mean_256(sIb, sB) : 256u * I;
            const int bracket = 65280 * (int)I - (int)(a * Fh) - (int)((255u - a) * Bh);
            const i64 n2 = 2 * (65025ll * (i64)Fh + (i64)a * (i64)bracket) + D;
            // fdiv(n2, 2 D) = fdiv(n2 >> 9, 65025) for n2 > 0; at n2 <= 0 the clamp gives 0
            unsigned q = n2 <= 0 ? 0u : (unsigned)((u64)n2 >> 9) / 65025u;
            q = q > 255u ? 255u : q;
            o |= q << (8 * c);
        }
        job.out[p] = o;
    }
}

size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }
int cells_of(int extent) { return (extent + CELL - 1) / CELL; }
int blocks_x(const k::CutoutJob& j) { return (j.w + (BLOCK - 2 * j.radius) - 1) / (BLOCK - 2 * j.radius); }     // strips
int blocks_y(const k::CutoutJob& j) { return (j.h + BAND - 1) / BAND; }                                         // bands

// Throws on the first bad job; returns nothing the kernels rely on.
void check_jobs(const k::CutoutJob* jobs, int count, bool pointers) {
    if (count < 0 || (count > 0 && !jobs)) throw_error("mask_cutout: invalid job list");
    for (int i = 0; i < count; ++i) {
        const k::CutoutJob& j = jobs[i];
        if (j.w <= 0 || j.h <= 0) throw_error("mask_cutout: invalid extent");
        if ((long long)j.w * (long long)j.h > 0x7fffffffLL) throw_error("mask_cutout: w * h does not fit an int");
        if (j.channels != 3 && j.channels != 4) throw_error("mask_cutout: channels is 3 or 4");
        if (j.radius < 1 || j.radius > MAX_RADIUS) throw_error("mask_cutout: radius is 1 .. 32");
        // an extent so thin that one job alone needs more workgroups than a launch takes (1 x 2^31 - 1, say): no image is such
        if ((long long)blocks_x(j) * blocks_y(j) > MAX_GRID || (long long)cells_of(j.w) * cells_of(j.h) > MAX_GRID)
            throw_error("mask_cutout: invalid extent: too many rows for its width");
        if (!pointers) continue;
        if (!j.coverage) throw_error("mask_cutout: null coverage");
        if (!j.guide) throw_error("mask_cutout: null guide");
        if (!j.out) throw_error("mask_cutout: null out");
        if (reinterpret_cast<uintptr_t>(j.out) % 4 != 0) throw_error("mask_cutout: out is not aligned to 4 bytes");
        if (j.channels == 4 && reinterpret_cast<uintptr_t>(j.guide) % 4 != 0) throw_error("mask_cutout: a guide of 4 channels is not aligned to 4 bytes");
    }
}

// per job: one int per 64 x 64 cell
size_t cell_words(const k::CutoutJob& j) { return round_up((size_t)cells_of(j.w) * cells_of(j.h), 4); }

// The launches of one call, in order; dry: counted only.  Returns their number.
int run_passes(const k::CutoutJob* jobs, int count, void* workspace, hipStream_t s, bool shortcut, bool dry) {
    int launches = 0;
    int* const words = static_cast<int*>(workspace);
    PassPack pack{};
    pack.shortcut = shortcut ? 1 : 0;
    long long blocks = 0, cells = 0;
    auto launch = [&] {
        if (pack.n == 0) return;
        launches += shortcut ? 2 : 1;
        if (!dry && shortcut) hipLaunchKernelGGL(cutout_cells_kernel, dim3((unsigned)cells), dim3(BLOCK), 0, s, pack);
        if (!dry) hipLaunchKernelGGL(cutout_out_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, pack);
        pack.n = 0;
        blocks = cells = 0;
    };
    size_t at = 0;
    for (int i = 0; i < count; ++i) {
        const k::CutoutJob& j = jobs[i];
        const size_t mine = at;
        at += cell_words(j);
        const int strips = blocks_x(j), bands = blocks_y(j);
        const long long nb = (long long)strips * bands, nc = (long long)cells_of(j.w) * cells_of(j.h);
        if (pack.n == MAX_JOBS || blocks + nb > MAX_GRID || cells + nc > MAX_GRID) launch();
        if (!dry)
            pack.j[pack.n] = PassJob{j.coverage, j.guide, reinterpret_cast<uint32_t*>(j.out), words + mine, j.w, j.h, j.channels, j.radius,
                                     strips, (int)blocks, cells_of(j.w), cells_of(j.h), (int)cells};
        ++pack.n;
        blocks += nb;
        cells += nc;
    }
    launch();
    return launches;
}

}  // namespace

namespace k {

size_t mask_cutout_workspace_bytes(const CutoutJob* jobs, int count) {
    check_jobs(jobs, count, false);
    size_t bytes = 0;
    for (int i = 0; i < count; ++i) bytes += cell_words(jobs[i]) * sizeof(int);
    return bytes;
}

int mask_cutout_launches(const CutoutJob* jobs, int count) {
    check_jobs(jobs, count, false);
    return run_passes(jobs, count, nullptr, nullptr, true, true);
}

void mask_cutout(const CutoutJob* jobs, int count, void* workspace, hipStream_t s, bool shortcut) {
    check_jobs(jobs, count, true);
    if (count == 0) return;
    if (!workspace) throw_error("mask_cutout: null workspace");
    run_passes(jobs, count, workspace, s, shortcut, false);
}

}  // namespace k
}  // namespace dlimg
