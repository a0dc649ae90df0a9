// K18  label maps of a point grid ("segment everything"): kernels.hpp, k::grid_harvest / k::grid_paint.
//
// grid_harvest -- one workgroup of sixteen waves per candidate plane (256 x 256 fp32, 256 KB).  A wave-instruction loads one
// whole 1 KB logit row (16 bytes per lane); a wave owns 16 consecutive rows and issues all 16 loads before it touches the
// first value, so the whole plane of a workgroup is in flight at once -- a decode chunk has only 42-48 candidates, far fewer
// workgroups than CUs, and the first form (four waves, eight rows in flight each) spent its time waiting: 0.49 TB/s.  The plane
// is read once, copied as fp32 (the bits are kept) into the lane's grid store with 16-byte stores, and reduced on the way to
// seven integers and the cull box.  Reduction: shuffles inside a wave, 11 ints per wave through LDS, one thread writes the
// 32-byte record as two 16-byte vector stores.  No atomics, no waiting on other workgroups.  Memory-bound: 256 KB in, 256 KB
// out per workgroup; the workgroups of a launch touch disjoint planes, so there is nothing for an XCD's L2 to share and the
// workgroup ids are taken as they come (no xcd_remap).
//
// grid_paint -- one launch per label map, a lane owns 16 consecutive pixels of one row and writes them as one 16-byte store
// where the extent allows (W a multiple of 16, aligned destination), byte by byte otherwise.  The kept list travels in the
// kernel arguments and is walked from the highest label down, uniformly over the wave; a label is sampled at a pixel only
// when the low-res taps of that pixel can touch its cull box (kernels.hpp: the box over the REACH region, which grid_harvest
// reduces beside the scored box -- the choice between the two the design allows).  The sample is the post-processing's:
// kernels/bilinear_taps.hpp, same functions, same order, contraction off; the per-pixel form of postprocess.hip, to which
// its identity form is bit-identical.
#include "bilinear_taps.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace dlimg {
namespace {

using taps::LOW;
using taps::Tap;
using taps::make_tap;
using taps::stage1;
using taps::stage2;

typedef int int4_t __attribute__((ext_vector_type(4)));

constexpr int kPlane = LOW * LOW;
constexpr int kReduced = 11;       // n_hi n_mid n_lo | x0 y0 cx0 cy0 (minima) | x1 y1 cx1 cy1 (maxima)

DLIMG_DEVICE int wave_reduce_add(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
DLIMG_DEVICE int wave_reduce_min(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}
DLIMG_DEVICE int wave_reduce_max(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

constexpr int kHarvestWaves = 16, kHarvestRows = LOW / kHarvestWaves;       // rows of a wave, all in flight

// sw, sh: extent of the scored region; rw, rh: of the reach region (one more, at most LOW)
__global__ __launch_bounds__(64 * kHarvestWaves) void grid_harvest_kernel(const float* __restrict__ logits, int first_candidate, int sw,
                                                                          int sh, int rw, int rh, float* __restrict__ store,
                                                                          int32_t* __restrict__ records) {
    __shared__ int red[kHarvestWaves][kReduced];
    const int lc = blockIdx.x;                                   // candidate of the chunk: prompt lc / 3, plane 1 + lc % 3
    const float* src = logits + ((size_t)(lc / 3) * 4 + 1 + lc % 3) * kPlane;
    float* dst = store + (size_t)(first_candidate + lc) * kPlane;
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const int xb = lane * 4, yb = wave * kHarvestRows;
    int n_hi = 0, n_mid = 0, n_lo = 0;
    int x0 = LOW, y0 = LOW, x1 = -1, y1 = -1, cx0 = LOW, cy0 = LOW, cx1 = -1, cy1 = -1;
    // kFlight rows at a time: their loads are all issued before the first value is used
    constexpr int kFlight = kHarvestRows;
#pragma unroll 1
    for (int half = 0; half < kHarvestRows / kFlight; ++half) {
        const int yh = yb + half * kFlight;
        float4_t v[kFlight];
#pragma unroll
        for (int u = 0; u < kFlight; ++u) v[u] = *reinterpret_cast<const float4_t*>(src + (yh + u) * LOW + xb);
#pragma unroll
        for (int u = 0; u < kFlight; ++u) *reinterpret_cast<float4_t*>(dst + (yh + u) * LOW + xb) = v[u];
#pragma unroll
        for (int u = 0; u < kFlight; ++u) {
            const int y = yh + u;
            const bool reach_row = y < rh, scored_row = y < sh;      // (wave-uniform; rows beyond what any tap reads are copied, not scored)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int x = xb + e;
                const float f = v[u][e];
                const bool pos = f > 0.0f;
                if (scored_row && x < sw) {
                    n_hi += f > 1.0f ? 1 : 0;
                    n_mid += pos ? 1 : 0;
                    n_lo += f > -1.0f ? 1 : 0;
                    if (pos) { x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y); }
                }
                if (reach_row && pos && x < rw) { cx0 = min(cx0, x); cx1 = max(cx1, x); cy0 = min(cy0, y); cy1 = max(cy1, y); }
            }
        }
    }
    int r[kReduced] = {wave_reduce_add(n_hi), wave_reduce_add(n_mid), wave_reduce_add(n_lo),
                       wave_reduce_min(x0), wave_reduce_min(y0), wave_reduce_min(cx0), wave_reduce_min(cy0),
                       wave_reduce_max(x1), wave_reduce_max(y1), wave_reduce_max(cx1), wave_reduce_max(cy1)};
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kReduced; ++i) red[wave][i] = r[i];
    }
    __syncthreads();
    // across the waves: thread i folds value i (the first three are sums, then four minima, then four maxima)
    __shared__ int fin[kReduced];
    if (threadIdx.x < kReduced) {
        const int i = threadIdx.x;
        int a = red[0][i];
        for (int w = 1; w < kHarvestWaves; ++w) {
            const int b = red[w][i];
            a = i < 3 ? a + b : (i < 7 ? min(a, b) : max(a, b));
        }
        fin[i] = a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int i = 0; i < kReduced; ++i) r[i] = fin[i];
    const bool none = r[1] == 0;
    const uint32_t cull = r[9] < 0 ? k::kGridCullEmpty : (uint32_t)r[5] | (uint32_t)r[6] << 8 | (uint32_t)r[9] << 16 | (uint32_t)r[10] << 24;
    int4_t* rec = reinterpret_cast<int4_t*>(records + (size_t)(first_candidate + lc) * k::kGridRecordInts);
    rec[0] = int4_t{r[0], r[1], r[2], none ? 0 : r[3]};
    rec[1] = int4_t{none ? 0 : r[4], none ? -1 : r[7], none ? -1 : r[8], (int)cull};
}

struct PaintArgs { const float* store; uint8_t* dst; int W, H, pre_w, pre_h, cull; };

constexpr int PX = 16;             // pixels of a lane: one 16-byte store

__global__ __launch_bounds__(256) void grid_paint_kernel(PaintArgs a, k::GridKept kept) {
    const int W = a.W, H = a.H;
    const int groups_per_row = (W + PX - 1) / PX;
    const bool identity2 = (a.pre_w == W && a.pre_h == H);
    const float sy = (float)a.pre_h / (float)H, sx = (float)a.pre_w / (float)W;
    const bool wide = (W & (PX - 1)) == 0 && (((uintptr_t)a.dst) & 15) == 0;
    const long total = (long)H * groups_per_row;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
        const int oy = (int)(g / groups_per_row);
        const int ox0 = (int)(g % groups_per_row) * PX;
        const int n_px = min(PX, W - ox0);
        Tap t2y = Tap{oy, oy, 1.0f, 0.0f};
        if (!identity2) t2y = make_tap(oy, sy, a.pre_h);
        // the low-res rows / columns the taps of this lane's pixels read (monotone in the pixel: first and last bound them)
        const int ya = make_tap(t2y.i0, 0.25f, LOW).i0, yb = make_tap(t2y.i1, 0.25f, LOW).i1;
        const int first_x = identity2 ? ox0 : make_tap(ox0, sx, a.pre_w).i0;
        const int last_x = identity2 ? ox0 + n_px - 1 : make_tap(ox0 + n_px - 1, sx, a.pre_w).i1;
        const int gxa = make_tap(first_x, 0.25f, LOW).i0, gxb = make_tap(last_x, 0.25f, LOW).i1;
        uint32_t packed[4] = {0u, 0u, 0u, 0u};
        uint32_t open = n_px == PX ? 0xffffu : (1u << n_px) - 1u;      // pixels without a label yet
        for (int kk = kept.count; kk >= 1 && open; --kk) {
            int cx0 = 0, cy0 = 0, cx1 = LOW - 1, cy1 = LOW - 1;
            if (a.cull) {
                const uint32_t c = kept.cull[kk - 1];
                cx0 = c & 255; cy0 = (c >> 8) & 255; cx1 = (c >> 16) & 255; cy1 = c >> 24;
                if (cx1 < gxa || cx0 > gxb || cy1 < ya || cy0 > yb) continue;
            }
            const float* low = a.store + (size_t)kept.candidate[kk - 1] * kPlane;
#pragma unroll 4
            for (int i = 0; i < PX; ++i) {
                if (!(open >> i & 1u)) continue;
                const int ox = ox0 + i;
                float v;
                if (identity2) {
                    const Tap tx = make_tap(ox, 0.25f, LOW);
                    if (cx1 < tx.i0 || cx0 > tx.i1) continue;
                    v = stage1(low, oy, ox);
                } else {
                    const Tap t2x = make_tap(ox, sx, a.pre_w);
                    if (cx1 < make_tap(t2x.i0, 0.25f, LOW).i0 || cx0 > make_tap(t2x.i1, 0.25f, LOW).i1) continue;
                    v = stage2(low, t2y, t2x);
                }
                if (v > 0.f) {
                    packed[i >> 2] |= (uint32_t)kk << (8 * (i & 3));
                    open &= ~(1u << i);
                }
            }
        }
        uint8_t* dst = a.dst + (size_t)oy * W + ox0;
        if (wide) {
            *reinterpret_cast<uint4_t*>(dst) = uint4_t{packed[0], packed[1], packed[2], packed[3]};
        } else {
            for (int i = 0; i < n_px; ++i) dst[i] = (uint8_t)(packed[i >> 2] >> (8 * (i & 3)));
        }
    }
}

}  // namespace

namespace k {

static_assert(sizeof(GridKept) + sizeof(PaintArgs) <= 4096, "the kept list travels as kernel arguments");

void grid_harvest(const float* logits, int P, int first_candidate, int pre_w, int pre_h, float* store, int candidates, int32_t* records,
                  hipStream_t s) {
    if (P <= 0 || first_candidate < 0 || first_candidate > candidates - 3 * P) throw_error("grid_harvest: the chunk's candidates are not in the store");
    if (pre_w <= 0 || pre_h <= 0 || pre_w > taps::FULL || pre_h > taps::FULL) throw_error("grid_harvest: invalid extent");
    if (!logits || !store || !records) throw_error("grid_harvest: null buffer");
    if ((((uintptr_t)logits) | ((uintptr_t)store) | ((uintptr_t)records)) & 15) throw_error("grid_harvest: buffers are 16-byte aligned");
    const int sw = (pre_w + 3) / 4, sh = (pre_h + 3) / 4;
    const int rw = sw + 1 < LOW ? sw + 1 : LOW, rh = sh + 1 < LOW ? sh + 1 : LOW;
    hipLaunchKernelGGL(grid_harvest_kernel, dim3((unsigned)(3 * P)), dim3(64 * kHarvestWaves), 0, s, logits, first_candidate, sw, sh, rw, rh, store, records);
}

void grid_paint(const float* store, int candidates, const GridKept& kept, uint8_t* dst, int out_w, int out_h, int pre_w, int pre_h,
                bool cull, hipStream_t s) {
    if (out_w <= 0 || out_h <= 0 || pre_w <= 0 || pre_h <= 0 || pre_w > taps::FULL || pre_h > taps::FULL)
        throw_error("grid_paint: invalid extent");
    if (!store || !dst) throw_error("grid_paint: null buffer");
    if (kept.count < 0 || kept.count > kGridMaxKept) throw_error("grid_paint: more kept segments than a byte labels");
    for (int i = 0; i < kept.count; ++i)
        if (kept.candidate[i] < 0 || kept.candidate[i] >= candidates) throw_error("grid_paint: a kept candidate is not in the store");
    const long total = (long)out_h * ((out_w + PX - 1) / PX);
    long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    const PaintArgs a{store, dst, out_w, out_h, pre_w, pre_h, cull ? 1 : 0};
    hipLaunchKernelGGL(grid_paint_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, kept);
}

}  // namespace k
}  // namespace dlimg
