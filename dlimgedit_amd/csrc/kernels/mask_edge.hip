// K24  edge marks: grow, shrink, feather and border a mask in place, by an exact Euclidean distance to its edge truncated at
// R = |offset| + feather + border + 1 <= 129 pixels (kernels.hpp has the definition; tests/edge_ref.py restates it in numpy).
// Integer arithmetic throughout; the one float is the first guess of the integer square root, corrected by comparison.
//
// The separable transform.  Up to three launches for up to 16 jobs of any sizes, the job taken from the grid; no atomics on
// global memory, no waiting:
//   K0 edge_cells    (shortcut only) one workgroup per 64 x 64 cell of a mask: its smallest and largest byte, one int per cell.
//   K1 edge_columns  one workgroup per (strip of 256 columns) x (band of 128 rows), thread t owning column x0 + t: loads coalesce.
//                    It walks down from R rows above its band, eight rows loaded at a time before the first is looked at,
//                    keeping the last row of either polarity, and leaves the distance up to the other polarity in LDS (a byte
//                    per pixel, 32 KiB, each thread its own column: no barrier); it walks back up from R rows below and stores
//                    min(up, down, R) | polarity << 15  per pixel, 2 bytes, in the workspace.  129 values and two polarities
//                    are 258: one more than a byte.
//   K2 edge_rows     one workgroup per (strip of 256 columns) x (band of 16 rows): the band's workspace rows with R columns of
//                    halo on either side in LDS (16 x 514 x 2 = 16 KiB), then thread t, for each row, the minimum over
//                    |x - x'| <= R of (x - x')^2 + g_c(x')^2 outwards from x' = x, ending once (x - x')^2 alone is no less than
//                    the minimum so far (which starts at R^2: the truncation); then q, T and the byte, stored in place.
// In place: K2 is the only kernel that writes the mask, and it reads nothing of it -- polarity and distance come from the
// workspace, the shortcut's verdict from the cells -- while K0 and K1, the only readers of the mask, are earlier launches on
// the same stream.  So no workgroup of K2 can see a neighbour's output where it wants that neighbour's input.
// The shortcut: a block of K1 whose mask is of one polarity over its columns and its rows +- R stores R for every pixel without
// reading the mask (it still stores: a neighbour's K2 block may read that halo); a block of K2 whose mask is of one polarity
// over its pixels and their R halo has d2 >= R^2 everywhere, so one byte, level(R^2), which is 0 or 255 and 0 for a border.
// Both read it off the cells of K0 (whole cells: a conservative test).  Polarity, not value: 200 and 255 are one polarity.
//
// Bounds and occupancy.  K1: 256 threads, 32 KiB of LDS: 5 workgroups, 20 waves a CU; each thread makes 2 (128 + 2R) byte
// loads, 772 at R = 129, and a 12-megapixel image is only 384 workgroups, one round: a launch lasts as long as ONE column walk,
// so the walk is bound by load latency and eight loads are kept in flight (LABNOTES has one at a time measured).  K2: 256
// threads, 16 KiB: 8 workgroups (the 32-wave cap) a CU; bound by its inner loop where the mask is far from an edge and the block
// not uniform, by memory elsewhere.  Bytes per pixel at R = 129, no block uniform: K0 reads 1; K1 reads 2 (128 + 258) / 128 = 6
// (the halo rows twice, mostly from L2) and writes 2; K2 reads 2 * 514 / 256 = 4 and writes 1: 14, of which 6 are compulsory
// (1 + 2 + 2 + 1).  Inner steps per pixel at R = 129: K1 6 loads; K2 at most 258 LDS reads of 2 bytes with about 8 integer
// operations each, and 2 d for a pixel at distance d < R of the edge.
//
// Widths: g <= 129, d2 <= R^2 = 16641, 65536 d2 < 2^31; |T| <= 33024 + 128 + 16384 + 8192 and 255 (|T| + 8192) + 8192 < 2^24.
#include "box_window.hpp"
#include "kernels.hpp"

namespace dlimg {
namespace {

using boxwin::BLOCK;
using boxwin::CELL;
using boxwin::cell_extremes;
using boxwin::extremes_over;

constexpr int MAX_JOBS = 16;
constexpr int MAX_OFFSET = 64;
constexpr int MAX_FEATHER = 32;
constexpr int MAX_BORDER = 32;
constexpr int MAX_REACH = MAX_OFFSET + MAX_FEATHER + MAX_BORDER + 1;      // 129
constexpr int STRIP = BLOCK;                          // columns of a block, both passes
constexpr int COLUMN_BAND = 128;                      // rows of a block of K1
constexpr int ROW_BAND = 16;                          // rows of a block of K2
constexpr int BATCH = 8;                              // rows of a column K1 loads before it looks at any: loads in flight per thread
constexpr long long MAX_GRID = (1ll << 24) - 1;       // workgroups of one launch: gridDim.x * 256 threads stays below 2^32
constexpr unsigned POLARITY = 0x8000u;

struct PassJob {
    uint8_t* mask;
    uint16_t* dist;
    int* cells;
    int w, h, offset, feather, border;
    int strips, column_begin, row_begin, cells_x, cells_y, cell_begin;
};
struct PassPack {
    PassJob j[MAX_JOBS];
    int n;
    int shortcut;
};

DLIMG_DEVICE int job_of_column_block(PassPack const& pack, int block) {
    int j = 0;
    for (int i = 1; i < pack.n; ++i)
        if (block >= pack.j[i].column_begin) j = i;
    return j;
}
DLIMG_DEVICE int job_of_row_block(PassPack const& pack, int block) {
    int j = 0;
    for (int i = 1; i < pack.n; ++i)
        if (block >= pack.j[i].row_begin) j = i;
    return j;
}
DLIMG_DEVICE int job_of_cell(PassPack const& pack, int cell) {
    int j = 0;
    for (int i = 1; i < pack.n; ++i)
        if (cell >= pack.j[i].cell_begin) j = i;
    return j;
}

DLIMG_DEVICE int reach_of(int offset, int feather, int border) { return (offset < 0 ? -offset : offset) + feather + border + 1; }

// isqrt(n), n < 2^31: the float root is within one of it
DLIMG_DEVICE int isqrt_exact(int n) {
    int r = (int)sqrtf((float)n);
    while (r * r > n) --r;
    while ((r + 1) * (r + 1) <= n) ++r;
    return r;
}

// the byte of a pixel of polarity fg whose squared distance to the other polarity is d2 <= R^2
DLIMG_DEVICE int level(int d2, bool fg, int offset, int feather, int border) {
    const int s = isqrt_exact(65536 * d2) - 128;
    int T = (fg ? s : -s) + 256 * offset;
    if (border > 0) T = 256 * border - (T < 0 ? -T : T);
    if (feather == 0) return T > 0 ? 255 : 0;
    const int num = 255 * (T + 256 * feather) + 256 * feather;
    if (num <= 0) return 0;             // fdiv of a negative numerator is negative: clamped
    const int v = num / (512 * feather);
    return v > 255 ? 255 : v;
}

__global__ __launch_bounds__(BLOCK) void edge_cells_kernel(PassPack pack) {
    const PassJob job = pack.j[job_of_cell(pack, (int)blockIdx.x)];
    cell_extremes(job.mask, job.w, job.h, job.cells_x, (int)blockIdx.x - job.cell_begin, job.cells);
}

__global__ __launch_bounds__(BLOCK) void edge_columns_kernel(PassPack pack) {
    __shared__ uint8_t up[COLUMN_BAND][STRIP];
    const PassJob job = pack.j[job_of_column_block(pack, (int)blockIdx.x)];
    const int b = (int)blockIdx.x - job.column_begin;
    const int w = job.w, h = job.h, R = reach_of(job.offset, job.feather, job.border);
    const int x0 = (b % job.strips) * STRIP, y0 = (b / job.strips) * COLUMN_BAND;
    const int y1 = y0 + COLUMN_BAND < h ? y0 + COLUMN_BAND : h;
    const int t = (int)threadIdx.x, x = x0 + t;
    if (pack.shortcut) {
        int lo, hi;
        extremes_over(job, x0, x0 + STRIP - 1, y0 - R, y1 - 1 + R, &lo, &hi);
        if (lo >= 128 || hi < 128) {
            const uint16_t v = (uint16_t)((unsigned)R | (lo >= 128 ? POLARITY : 0u));
            if (x < w)
                for (int y = y0; y < y1; ++y) job.dist[(size_t)y * w + x] = v;
            return;
        }
    }
    if (x >= w) return;
    const int far = -(1 << 20);
    {
        int last_bg = far, last_fg = far;          // the last row of either polarity at or above y
        const int ya = y0 - R < 0 ? 0 : y0 - R;
        for (int first = ya; first < y1; first += BATCH) {
            uint8_t v[BATCH];
#pragma unroll
            for (int k = 0; k < BATCH; ++k) v[k] = first + k < y1 ? job.mask[(size_t)(first + k) * w + x] : (uint8_t)0;
#pragma unroll
            for (int k = 0; k < BATCH; ++k) {
                const int y = first + k;
                if (y >= y1) break;
                const bool fg = v[k] >= 128;
                last_fg = fg ? y : last_fg;
                last_bg = fg ? last_bg : y;
                if (y >= y0) {
                    const int d = y - (fg ? last_bg : last_fg);
                    up[y - y0][t] = (uint8_t)(d > R ? R : d);
                }
            }
        }
    }
    int next_bg = 1 << 20, next_fg = 1 << 20;      // the next row of either polarity at or below y
    const int yb = y1 - 1 + R > h - 1 ? h - 1 : y1 - 1 + R;
    for (int first = yb; first >= y0; first -= BATCH) {
        uint8_t v[BATCH];
#pragma unroll
        for (int k = 0; k < BATCH; ++k) v[k] = first - k >= y0 ? job.mask[(size_t)(first - k) * w + x] : (uint8_t)0;
#pragma unroll
        for (int k = 0; k < BATCH; ++k) {
            const int y = first - k;
            if (y < y0) break;
            const bool fg = v[k] >= 128;
            next_fg = fg ? y : next_fg;
            next_bg = fg ? next_bg : y;
            if (y < y1) {
                const int d = (fg ? next_bg : next_fg) - y, u = up[y - y0][t];
                const int g = d < u ? d : u;             // u <= R
                job.dist[(size_t)y * w + x] = (uint16_t)((unsigned)g | (fg ? POLARITY : 0u));
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void edge_rows_kernel(PassPack pack) {
    __shared__ uint16_t tile[ROW_BAND][STRIP + 2 * MAX_REACH];
    const PassJob job = pack.j[job_of_row_block(pack, (int)blockIdx.x)];
    const int b = (int)blockIdx.x - job.row_begin;
    const int w = job.w, h = job.h, R = reach_of(job.offset, job.feather, job.border);
    const int x0 = (b % job.strips) * STRIP, y0 = (b / job.strips) * ROW_BAND;
    const int y1 = y0 + ROW_BAND < h ? y0 + ROW_BAND : h;
    const int t = (int)threadIdx.x, x = x0 + t;
    if (pack.shortcut) {
        int lo, hi;
        extremes_over(job, x0 - R, x0 + STRIP - 1 + R, y0 - R, y1 - 1 + R, &lo, &hi);
        if (lo >= 128 || hi < 128) {
            const uint8_t v = (uint8_t)level(R * R, lo >= 128, job.offset, job.feather, job.border);
            if (x < w)
                for (int y = y0; y < y1; ++y) job.mask[(size_t)y * w + x] = v;
            return;
        }
    }
    // tile[.][i] is column x0 - R + i; columns outside the image are neither stored nor read
    for (int y = y0; y < y1; ++y)
        for (int i = t; i < STRIP + 2 * R; i += BLOCK) {
            const int xx = x0 - R + i;
            if (xx >= 0 && xx < w) tile[y - y0][i] = job.dist[(size_t)y * w + xx];
        }
    __syncthreads();
    if (x >= w) return;
    const int left = x < R ? x : R, right = w - 1 - x < R ? w - 1 - x : R;       // how far the row reaches on either side
    for (int y = y0; y < y1; ++y) {
        const uint16_t* row = tile[y - y0] + R + t;
        const unsigned own = row[0], c = own & POLARITY;
        const int g = (int)(own & (POLARITY - 1));
        int best = g * g < R * R ? g * g : R * R;
        for (int d = 1; d <= R; ++d) {
            const int dd = d * d;
            if (dd >= best) break;
            if (d <= left) {
                const unsigned e = row[-d];
                const int v = (e & POLARITY) == c ? (int)(e & (POLARITY - 1)) : 0;
                best = dd + v * v < best ? dd + v * v : best;
            }
            if (d <= right) {
                const unsigned e = row[d];
                const int v = (e & POLARITY) == c ? (int)(e & (POLARITY - 1)) : 0;
                best = dd + v * v < best ? dd + v * v : best;
            }
        }
        job.mask[(size_t)y * w + x] = (uint8_t)level(best, c != 0, job.offset, job.feather, job.border);
    }
}

size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }
int cells_of(int extent) { return (extent + CELL - 1) / CELL; }
int strips_of(const k::EdgeJob& j) { return (j.w + STRIP - 1) / STRIP; }
long long column_blocks(const k::EdgeJob& j) { return (long long)strips_of(j) * ((j.h + COLUMN_BAND - 1) / COLUMN_BAND); }
long long row_blocks(const k::EdgeJob& j) { return (long long)strips_of(j) * ((j.h + ROW_BAND - 1) / ROW_BAND); }

// Throws on the first bad job; returns nothing the kernels rely on.
void check_jobs(const k::EdgeJob* jobs, int count, bool pointers) {
    if (count < 0 || (count > 0 && !jobs)) throw_error("mask_edge: invalid job list");
    for (int i = 0; i < count; ++i) {
        const k::EdgeJob& j = jobs[i];
        if (j.w <= 0 || j.h <= 0) throw_error("mask_edge: invalid extent");
        if ((long long)j.w * (long long)j.h > 0x7fffffffLL) throw_error("mask_edge: w * h does not fit an int");
        if (j.offset < -MAX_OFFSET || j.offset > MAX_OFFSET) throw_error("mask_edge: offset is -64 .. 64");
        if (j.feather < 0 || j.feather > MAX_FEATHER) throw_error("mask_edge: feather is 0 .. 32");
        if (j.border < 0 || j.border > MAX_BORDER) throw_error("mask_edge: border is 0 .. 32");
        if (j.offset == 0 && j.feather == 0 && j.border == 0) throw_error("mask_edge: offset, feather and border are all 0: the identity");
        // an extent so thin that one job alone needs more workgroups than a launch takes (1 x 2^31 - 1, say): no image is such
        if (row_blocks(j) > MAX_GRID || (long long)cells_of(j.w) * cells_of(j.h) > MAX_GRID)
            throw_error("mask_edge: invalid extent: too many rows for its width");
        if (pointers && !j.mask) throw_error("mask_edge: null mask");
    }
}

// per job: 2 bytes per pixel, then one int per 64 x 64 cell; each part a multiple of 16 bytes
size_t dist_bytes(const k::EdgeJob& j) { return round_up((size_t)j.w * j.h * sizeof(uint16_t), 16); }
size_t cell_bytes(const k::EdgeJob& j) { return round_up((size_t)cells_of(j.w) * cells_of(j.h) * sizeof(int), 16); }

// The launches of one call, in order; dry: counted only.  Returns their number.
int run_passes(const k::EdgeJob* jobs, int count, void* workspace, hipStream_t s, bool shortcut, bool dry) {
    int launches = 0;
    uint8_t* const bytes = static_cast<uint8_t*>(workspace);
    PassPack pack{};
    pack.shortcut = shortcut ? 1 : 0;
    long long columns = 0, rows = 0, cells = 0;
    auto launch = [&] {
        if (pack.n == 0) return;
        launches += shortcut ? 3 : 2;
        if (!dry && shortcut) hipLaunchKernelGGL(edge_cells_kernel, dim3((unsigned)cells), dim3(BLOCK), 0, s, pack);
        if (!dry) hipLaunchKernelGGL(edge_columns_kernel, dim3((unsigned)columns), dim3(BLOCK), 0, s, pack);
        if (!dry) hipLaunchKernelGGL(edge_rows_kernel, dim3((unsigned)rows), dim3(BLOCK), 0, s, pack);
        pack.n = 0;
        columns = rows = cells = 0;
    };
    size_t at = 0;
    for (int i = 0; i < count; ++i) {
        const k::EdgeJob& j = jobs[i];
        const size_t mine = at;
        at += dist_bytes(j) + cell_bytes(j);
        const long long nc = column_blocks(j), nr = row_blocks(j), ncell = (long long)cells_of(j.w) * cells_of(j.h);
        if (pack.n == MAX_JOBS || rows + nr > MAX_GRID || cells + ncell > MAX_GRID) launch();
        if (!dry)
            pack.j[pack.n] = PassJob{j.mask, reinterpret_cast<uint16_t*>(bytes + mine), reinterpret_cast<int*>(bytes + mine + dist_bytes(j)),
                                     j.w, j.h, j.offset, j.feather, j.border,
                                     strips_of(j), (int)columns, (int)rows, cells_of(j.w), cells_of(j.h), (int)cells};
        ++pack.n;
        columns += nc;
        rows += nr;
        cells += ncell;
    }
    launch();
    return launches;
}

}  // namespace

namespace k {

size_t mask_edge_workspace_bytes(const EdgeJob* jobs, int count) {
    check_jobs(jobs, count, false);
    size_t bytes = 0;
    for (int i = 0; i < count; ++i) bytes += dist_bytes(jobs[i]) + cell_bytes(jobs[i]);
    return bytes;
}

int mask_edge_launches(const EdgeJob* jobs, int count) {
    check_jobs(jobs, count, false);
    return run_passes(jobs, count, nullptr, nullptr, true, true);
}

void mask_edge(const EdgeJob* jobs, int count, void* workspace, hipStream_t s, bool shortcut) {
    check_jobs(jobs, count, true);
    if (count == 0) return;
    if (!workspace) throw_error("mask_edge: null workspace");
    if (reinterpret_cast<uintptr_t>(workspace) % 4 != 0) throw_error("mask_edge: workspace is not aligned to 4 bytes");
    run_passes(jobs, count, workspace, s, shortcut, false);
}

}  // namespace k
}  // namespace dlimg
