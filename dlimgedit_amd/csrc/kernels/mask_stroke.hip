// K22  stroke marks: the low-res cells a caller's scribble touches, and up to 8 clicks spread over them (kernels.hpp,
// k::stroke_derive; stroke_plan.hpp maps cells to image pixels).
//
// A pixel belongs to the stroke when its byte is >= 128.  Cell (x, y) of the scored region (x < sw, y < sh) is ON when ANY pixel
// of its footprint (footprint.hpp, both axes) belongs to the stroke: a maximum over the footprint, where the prior plane
// (mask_prior.hip) takes the mean, so a one-pixel line switches on every cell it crosses.  The first click is the ON cell nearest
// the centroid of the ON cells, the further ones are farthest-point samples; ties go to the smallest y, then the smallest x.
// Integer arithmetic throughout, so ballots and record are the same bits wherever they are computed (tests/stroke_ref.py restates
// them in numpy).
//
// Two launches, no waiting between workgroups, no atomics on global memory, plain vector stores:
//   stroke_cells   one workgroup of 1024 threads per low-res row y: four groups of 256 threads, group g taking the pixel rows
//                  r0 + g, r0 + g + 4, ... of the row's footprint.  A group runs over the image's columns in tiles of 4096: with
//                  a 16-byte aligned map whose width is a multiple of 16 a thread loads 16 consecutive bytes of a pixel row as one
//                  access (a wave: 1 KB contiguous); otherwise thread t loads the bytes t, t + 256, ... of the tile (a wave: 64
//                  contiguous bytes per access).  Either way the thread ORs what it saw over its pixel rows in a register and
//                  the tile's 4096 column bits go to LDS once per group; then thread x < 256 tests the bits of its own
//                  footprint.  The row's ON bits are four 64-bit ballots, written by one lane each.
//                  What bounds it: HBM.  The map is read once (a pixel row two footprints share, twice), up to 16 MB for a
//                  4096^2 image, and that is the only cost of the derivation that grows with the image; 4 KB are written.
//   stroke_sample  ONE workgroup of 1024 threads; a thread owns one ballot word, 64 cells of one row.  Count and coordinate
//                  sums, the centroid argmin, then up to 7 farthest-point rounds; a round recomputes every ON cell's distance to
//                  the <= 7 chosen cells from registers (no per-cell state: 65536 x 4 B would not fit the LDS).  A reduction is
//                  a lexicographic minimum of (key, y, x): a __shfl_xor butterfly inside the wave, 16 wave results through LDS.
//                  What bounds it: neither bandwidth (8 KB read, 80 B written) nor arithmetic (at most 64 cells x 7 chosen per
//                  thread and round) -- the launch and the nine dependent reductions, each two barriers and six shuffles, are
//                  latency.  One workgroup on one CU: occupancy is no limit.
#include "device_common.hpp"
#include "footprint.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace dlimg {
namespace {

constexpr int LOW = 256;
constexpr int kGroups = 4;                   // groups of LOW threads in a stroke_cells workgroup, each taking every fourth pixel row
constexpr int kTile = 4096;                  // image columns of one pass: 16 per thread of a group
constexpr int kTileWords = kTile / 64;

struct CellsArgs { const uint8_t* map; unsigned long long* ballots; int W, H, pre_w, pre_h, sw, sh, vector_loads; };

// the 16 bits "byte >= 128" of 16 consecutive bytes
DLIMG_DEVICE unsigned high_bits(uint4_t v) {
    unsigned out = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned m = v[q] & 0x80808080u;
        out |= (((m >> 7) & 1u) | ((m >> 14) & 2u) | ((m >> 21) & 4u) | ((m >> 28) & 8u)) << (4 * q);
    }
    return out;
}

__global__ __launch_bounds__(LOW * kGroups) void stroke_cells_kernel(CellsArgs a) {
    // bit c of group g's words: column t0 + c of the tile holds a stroke pixel in one of the group's pixel rows
    __shared__ unsigned long long seen[kGroups][kTileWords];
    const int y = blockIdx.x, t = threadIdx.x & (LOW - 1), g = threadIdx.x / LOW, lane = threadIdx.x & 63, wave = t >> 6;
    bool on = false;
    if (y < a.sh) {                                              // (uniform over the workgroup)
        const int r0 = footprint_lo(y, a.H, a.pre_h), r1 = footprint_hi(y, a.H, a.pre_h);       // 0 <= r0 < r1 <= H
        const int c0 = t < a.sw ? footprint_lo(t, a.W, a.pre_w) : 0, c1 = t < a.sw ? footprint_hi(t, a.W, a.pre_w) : 0;
        for (int t0 = 0; t0 < a.W; t0 += kTile) {
            unsigned mine = 0;
            if (a.vector_loads) {
                // W is a multiple of 16 and the map 16-byte aligned: the 16 bytes are in one row, inside the map, aligned
                const int c = t0 + 16 * t;
                if (c < a.W) {
#pragma unroll 4
                    for (int r = r0 + g; r < r1; r += kGroups)
                        mine |= high_bits(*reinterpret_cast<const uint4_t*>(a.map + (size_t)r * a.W + c));
                }
                // bits 16 t .. 16 t + 15 of the tile: four neighbouring lanes make one word
                unsigned long long word = (unsigned long long)mine << (16 * (t & 3));
                word |= __shfl_xor(word, 1, 64);
                word |= __shfl_xor(word, 2, 64);
                if ((t & 3) == 0) seen[g][t >> 2] = word;
            } else {
                for (int r = r0 + g; r < r1; r += kGroups) {
                    const uint8_t* row = a.map + (size_t)r * a.W;
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int c = t0 + LOW * j + t;
                        if (c < a.W) mine |= (unsigned)(row[c] >> 7) << j;
                    }
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const unsigned long long word = __ballot((mine >> j) & 1u);                 // columns 256 j + 64 wave + lane
                    if (lane == 0) seen[g][4 * j + wave] = word;
                }
            }
            __syncthreads();
            if (g == 0) {
                const int lo = (c0 > t0 ? c0 : t0) - t0, hi = (c1 < t0 + kTile ? c1 : t0 + kTile) - t0;      // bits [lo, hi) of the tile
                for (int w = lo >> 6; !on && lo < hi && w <= (hi - 1) >> 6; ++w) {
                    unsigned long long m = seen[0][w] | seen[1][w] | seen[2][w] | seen[3][w];
                    if (w == lo >> 6) m &= ~0ull << (lo & 63);
                    if (w == (hi - 1) >> 6 && (hi & 63)) m &= ~0ull >> (64 - (hi & 63));
                    on = m != 0;
                }
            }
            __syncthreads();                                     // the next tile overwrites the bits
        }
    }
    if (g == 0) {
        const unsigned long long word = __ballot(on);            // cells 64 wave .. 64 wave + 63 of row y
        if (lane == 0) a.ballots[y * (LOW / 64) + wave] = word;
    }
}

// ---- sampling ----------------------------------------------------------------------------------

struct Pick { long long key; int y, x; };                      // the smaller one wins: key, then y, then x
DLIMG_DEVICE bool better(Pick const& a, Pick const& b) {
    return a.key != b.key ? a.key < b.key : (a.y != b.y ? a.y < b.y : a.x < b.x);
}
constexpr long long kNoKey = 0x7fffffffffffffffll;

// the best Pick of the workgroup in every thread; slot: 0 or 1, alternating from call to call, so that one barrier per call is enough
DLIMG_DEVICE Pick block_best(Pick p, Pick (*wave_best)[16], int slot) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Pick o;
        o.key = __shfl_xor(p.key, d, 64);
        o.y = __shfl_xor(p.y, d, 64);
        o.x = __shfl_xor(p.x, d, 64);
        if (better(o, p)) p = o;
    }
    if ((threadIdx.x & 63) == 0) wave_best[slot][threadIdx.x >> 6] = p;
    __syncthreads();
    Pick best = wave_best[slot][0];
    for (int w = 1; w < 16; ++w) {
        const Pick o = wave_best[slot][w];
        if (better(o, best)) best = o;
    }
    return best;
}

__global__ __launch_bounds__(1024) void stroke_sample_kernel(const unsigned long long* ballots, int clicks, int* record) {
    __shared__ Pick wave_best[2][16];
    __shared__ int sums[16][3];
    const int y = threadIdx.x >> 2, x_first = (threadIdx.x & 3) * 64;
    const unsigned long long word = ballots[threadIdx.x];
    // the ON cells, their coordinate sums: at most 65536, 65536 * 255 each
    int n = __popcll(word), sx = 0, sy = n * y;
    for (unsigned long long m = word; m; m &= m - 1) sx += x_first + __builtin_ctzll(m);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        n += __shfl_xor(n, d, 64);
        sx += __shfl_xor(sx, d, 64);
        sy += __shfl_xor(sy, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sums[threadIdx.x >> 6][0] = n;
        sums[threadIdx.x >> 6][1] = sx;
        sums[threadIdx.x >> 6][2] = sy;
    }
    __syncthreads();
    n = sx = sy = 0;
    for (int w = 0; w < 16; ++w) {
        n += sums[w][0];
        sx += sums[w][1];
        sy += sums[w][2];
    }
    if (n == 0) {                                                // (uniform) an empty stroke: an all-zero record
        if (threadIdx.x < k::kStrokeRecordInts) record[threadIdx.x] = 0;
        return;
    }
    // the ON cell nearest the centroid: |n x - Sx|, |n y - Sy| < 2^24 + 2^24, the sum of squares below 2^51
    Pick mine{kNoKey, LOW, LOW};
    {
        const long long dy = (long long)n * y - sy;
        for (unsigned long long m = word; m; m &= m - 1) {       // x ascending: a tie keeps the smaller x
            const int x = x_first + __builtin_ctzll(m);
            const long long dx = (long long)n * x - sx, key = dx * dx + dy * dy;
            if (key < mine.key) mine = Pick{key, y, x};
        }
    }
    int cx[k::kStrokeMaxClicks], cy[k::kStrokeMaxClicks];
    Pick best = block_best(mine, wave_best, 0);
    cx[0] = best.x;
    cy[0] = best.y;
#pragma unroll
    for (int c = 1; c < k::kStrokeMaxClicks; ++c) {
        cx[c] = cy[c] = 0;
        if (c < clicks) {                                        // (uniform)
            // the ON cell farthest from the chosen ones: the largest minimum of dx^2 + dy^2 (<= 2 * 255^2), as the smallest key
            mine = Pick{kNoKey, LOW, LOW};
            for (unsigned long long m = word; m; m &= m - 1) {
                const int x = x_first + __builtin_ctzll(m);
                int nearest = 0x7fffffff;
#pragma unroll
                for (int j = 0; j < c; ++j) {
                    const int dx = x - cx[j], dy = y - cy[j], d2 = dx * dx + dy * dy;
                    nearest = d2 < nearest ? d2 : nearest;
                }
                if (-(long long)nearest < mine.key) mine = Pick{-(long long)nearest, y, x};
            }
            best = block_best(mine, wave_best, c & 1);
            cx[c] = best.x;
            cy[c] = best.y;
        }
    }
    if (threadIdx.x == 0) {
        record[0] = n;
        record[1] = clicks;
#pragma unroll
        for (int c = 0; c < k::kStrokeMaxClicks; ++c) {
            record[2 + 2 * c] = cx[c];
            record[3 + 2 * c] = cy[c];
        }
        record[18] = record[19] = 0;
    }
}

}  // namespace

namespace k {

void stroke_derive(const uint8_t* map, int W, int H, int pre_w, int pre_h, int clicks, unsigned long long* ballots, int32_t* record,
                   hipStream_t s) {
    if (!map || !ballots || !record) throw_error("stroke_derive: null buffer");
    if (W <= 0 || H <= 0 || pre_w <= 0 || pre_h <= 0 || pre_w > 4 * LOW || pre_h > 4 * LOW) throw_error("stroke_derive: invalid extent");
    if ((int64_t)W * H > (int64_t)1 << 31) throw_error("stroke_derive: the map is too large");
    if (clicks < 1 || clicks > kStrokeMaxClicks) throw_error("stroke_derive: clicks is 1..8");
    const int sw = (pre_w + 3) / 4, sh = (pre_h + 3) / 4;
    // what the kernel assumes: every footprint lies in the map
    if (!(footprint_lo(0, W, pre_w) == 0 && footprint_hi(sw - 1, W, pre_w) <= W && footprint_lo(sw - 1, W, pre_w) < W &&
          footprint_lo(0, H, pre_h) == 0 && footprint_hi(sh - 1, H, pre_h) <= H && footprint_lo(sh - 1, H, pre_h) < H))
        throw_error("stroke_derive: a footprint leaves the map");
    const int vector_loads = W % 16 == 0 && (((uintptr_t)map) & 15) == 0;
    const CellsArgs a{map, ballots, W, H, pre_w, pre_h, sw, sh, vector_loads};
    hipLaunchKernelGGL(stroke_cells_kernel, dim3(LOW), dim3(LOW * kGroups), 0, s, a);
    hipLaunchKernelGGL(stroke_sample_kernel, dim3(1), dim3(1024), 0, s, (const unsigned long long*)ballots, clicks, record);
}

}  // namespace k
}  // namespace dlimg
