// K17  mask clean-up: fill small holes, drop small islands (SAM's remove_small_regions), in place on 0 / 255 masks in
// device memory.  8-connectivity for both polarities; holes first, islands on the result (kernels.hpp has the rule).
//
// One polarity pass = connected-component labelling of the pixels of that polarity + component areas + the flip, over all
// jobs of the call at once (a flat list of 64 x 64 tiles, one workgroup each), in four launches:
//   K1 tile_label     union-find in LDS over the tile: labels[p] = GLOBAL linear index of the tile-local root (the smallest
//                     index of the set; raster order inside a tile is raster order in the mask), -1 for the other polarity;
//                     area[p] = pixels of the tile-local component at its root, 0 elsewhere.  Also zeroes the job's `best`.
//   K2 border_merge   the pixels of every tile's top row and left column against their neighbours in the tiles above / left
//                     (the diagonals across tile corners included): union of the two roots in global memory.
//   K3 root_areas     every tile-local root finds its global root, stores it (so K4 reads labels[labels[p]]), and adds its
//                     area to the root's: one integer atomic per tile-local component, not per pixel.  Islands pass: the
//                     maximum of (area << 32 | ~root) per job, one atomic per workgroup -- the largest component, the first
//                     in raster order among equals (the partial sums an add returns never exceed the root's final key).
//   K4 apply          flips the pixels whose component is below the threshold; the islands pass keeps the `best` component
//                     (when some component reaches the threshold, `best` does so too).
//
// Cross-XCD visibility: K2 and K3 are the kernels in which workgroups read label (and area) words other workgroups of the
// SAME launch write; every such access there is a relaxed agent-scope atomic (load / store / fetch_min / fetch_add /
// fetch_max), which is served by memory all eight XCDs share.  Everything else relies on kernel boundaries: K1 writes only
// its own tile, K4 only reads what K1..K3 left and writes its own pixels.  No grid barrier, no persistent kernel.
// Determinism: roots are minimum indices, areas integer sums, the tie rule is total -- no result depends on scheduling.
#include "device_common.hpp"
#include "kernels.hpp"

namespace dlimg {
namespace {

constexpr int TILE = 64;
constexpr int TILE_PX = TILE * TILE;
constexpr int PX_PER_THREAD = TILE_PX / 256;
constexpr int MAX_JOBS = 16;

struct PassJob {
    uint8_t* mask;
    int* labels;
    int* area;
    unsigned long long* best;
    int w, h, threshold, tiles_x, tile_begin;
};
struct PassPack {
    PassJob j[MAX_JOBS];
    int n;
    int polarity;        // the pixel value the pass labels: 0 (holes) or 255 (islands)
};

#define RLX __ATOMIC_RELAXED
#define AGENT __HIP_MEMORY_SCOPE_AGENT
#define WG __HIP_MEMORY_SCOPE_WORKGROUP

DLIMG_DEVICE int job_of_block(PassPack const& pack, int block) {
    int j = 0;
    for (int i = 1; i < pack.n; ++i)
        if (block >= pack.j[i].tile_begin) j = i;
    return j;
}

// ---- union-find in LDS (K1) ------------------------------------------------------------------
DLIMG_DEVICE int lds_find(int* L, int x) {
    int n;
    while ((n = __hip_atomic_load(&L[x], RLX, WG)) != x) x = n;
    return x;
}
DLIMG_DEVICE void lds_union(int* L, int a, int b) {
    for (;;) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&L[a], b, RLX, WG);
        if (old == a) return;
        a = old;            // somebody else moved a meanwhile: its earlier parent still has to meet b
    }
}

// ---- union-find in global memory (K2, K3): agent-scope atomics only ---------------------------
DLIMG_DEVICE int g_find(int* L, int x) {
    int n;
    while ((n = __hip_atomic_load(&L[x], RLX, AGENT)) != x) x = n;
    return x;
}
DLIMG_DEVICE void g_union(int* L, int a, int b) {
    for (;;) {
        a = g_find(L, a);
        b = g_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&L[a], b, RLX, AGENT);
        if (old == a) return;
        a = old;
    }
}

// thread t of a tile's workgroup owns the pixels k = t + 256 i: column t & 63 of rows (t >> 6) + 4 i, a wave = one row
__global__ __launch_bounds__(256) void tile_label_kernel(PassPack pack) {
    __shared__ int L[TILE_PX];
    __shared__ int cnt[TILE_PX];
    const PassJob job = pack.j[job_of_block(pack, (int)blockIdx.x)];
    const int tile = (int)blockIdx.x - job.tile_begin;
    const int x0 = (tile % job.tiles_x) * TILE, y0 = (tile / job.tiles_x) * TILE;
    const int t = (int)threadIdx.x, lx = t & 63, x = x0 + lx;
    if (tile == 0 && t == 0) *job.best = 0ull;

    // rows as runs: a pixel starts with the first pixel of its horizontal run as parent
#pragma unroll
    for (int i = 0; i < PX_PER_THREAD; ++i) {
        const int ly = (t >> 6) + 4 * i, y = y0 + ly, k = ly * TILE + lx;
        const bool in = x < job.w && y < job.h;
        const bool work = in && job.mask[(size_t)y * job.w + x] == (uint8_t)pack.polarity;
        const unsigned long long bits = __ballot(work);
        const unsigned long long gaps = ~bits & ((1ull << lx) - 1ull);       // the other polarity, left of this lane
        const int start = gaps ? 64 - __clzll(gaps) : 0;
        L[k] = work ? ly * TILE + start : -1;
        cnt[k] = 0;
    }
    __syncthreads();
    // a run against the row above it: north where that is set (its run holds north-west and north-east), else the diagonals
#pragma unroll
    for (int i = 0; i < PX_PER_THREAD; ++i) {
        const int ly = (t >> 6) + 4 * i, k = ly * TILE + lx;
        if (ly == 0 || __hip_atomic_load(&L[k], RLX, WG) < 0) continue;
        if (__hip_atomic_load(&L[k - TILE], RLX, WG) >= 0) {
            lds_union(L, k, k - TILE);
        } else {
            if (lx > 0 && __hip_atomic_load(&L[k - TILE - 1], RLX, WG) >= 0) lds_union(L, k, k - TILE - 1);
            if (lx < TILE - 1 && __hip_atomic_load(&L[k - TILE + 1], RLX, WG) >= 0) lds_union(L, k, k - TILE + 1);
        }
    }
    __syncthreads();
    // roots and areas: the lanes of a wave that share a root add once
    int root[PX_PER_THREAD];
#pragma unroll
    for (int i = 0; i < PX_PER_THREAD; ++i) {
        const int k = ((t >> 6) + 4 * i) * TILE + lx;
        const bool work = L[k] >= 0;
        root[i] = work ? lds_find(L, k) : -1;
        unsigned long long rest = __ballot(work);
        while (rest) {
            const int src = __ffsll((long long)rest) - 1;
            const int lead = __shfl(root[i], src, 64);
            const unsigned long long same = __ballot(work && root[i] == lead);
            if (lx == src) __hip_atomic_fetch_add(&cnt[lead], __popcll(same), RLX, WG);
            rest &= ~same;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PX_PER_THREAD; ++i) {
        const int ly = (t >> 6) + 4 * i, y = y0 + ly, k = ly * TILE + lx;
        if (x >= job.w || y >= job.h) continue;
        const int p = y * job.w + x, r = root[i];
        job.labels[p] = r < 0 ? -1 : (y0 + (r >> 6)) * job.w + x0 + (r & 63);
        job.area[p] = r == k ? cnt[k] : 0;
    }
}

// 128 threads per tile: 0..63 its top row against the row above, 64..127 its left column against the column to the left
__global__ __launch_bounds__(128) void border_merge_kernel(PassPack pack) {
    const PassJob job = pack.j[job_of_block(pack, (int)blockIdx.x)];
    const int tile = (int)blockIdx.x - job.tile_begin;
    const int x0 = (tile % job.tiles_x) * TILE, y0 = (tile / job.tiles_x) * TILE;
    const int t = (int)threadIdx.x;
    int* L = job.labels;
    if (t < TILE) {
        const int x = x0 + t, y = y0;
        if (y == 0 || x >= job.w) return;
        const int p = y * job.w + x;
        if (__hip_atomic_load(&L[p], RLX, AGENT) < 0) return;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= job.w) continue;
            const int q = (y - 1) * job.w + xx;
            if (__hip_atomic_load(&L[q], RLX, AGENT) >= 0) g_union(L, p, q);
        }
    } else {
        const int x = x0, y = y0 + t - TILE;
        if (x == 0 || y >= job.h) return;
        const int p = y * job.w + x;
        if (__hip_atomic_load(&L[p], RLX, AGENT) < 0) return;
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= job.h) continue;
            const int q = yy * job.w + x - 1;
            if (__hip_atomic_load(&L[q], RLX, AGENT) >= 0) g_union(L, p, q);
        }
    }
}

__global__ __launch_bounds__(256) void root_areas_kernel(PassPack pack) {
    __shared__ unsigned long long wave_best[4];
    const PassJob job = pack.j[job_of_block(pack, (int)blockIdx.x)];
    const int tile = (int)blockIdx.x - job.tile_begin;
    const int x0 = (tile % job.tiles_x) * TILE, y0 = (tile / job.tiles_x) * TILE;
    const int t = (int)threadIdx.x, x = x0 + (t & 63);
    unsigned long long key = 0ull;
#pragma unroll
    for (int i = 0; i < PX_PER_THREAD; ++i) {
        const int y = y0 + (t >> 6) + 4 * i;
        if (x >= job.w || y >= job.h) continue;
        const int p = y * job.w + x;
        const int a = __hip_atomic_load(&job.area[p], RLX, AGENT);
        if (a <= 0) continue;                    // not the root of a tile-local component
        const int r = g_find(job.labels, p);
        int total;
        if (r != p) {
            __hip_atomic_store(&job.labels[p], r, RLX, AGENT);
            total = __hip_atomic_fetch_add(&job.area[r], a, RLX, AGENT) + a;
        } else {
            total = a;                           // whoever adds to this root later reports the larger sum itself
        }
        const unsigned long long mine = ((unsigned long long)(unsigned)total << 32) | (unsigned)~r;
        key = mine > key ? mine : key;
    }
    if (pack.polarity == 0) return;              // holes: no component is kept for being the largest
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off, 64);
        key = other > key ? other : key;
    }
    if ((t & 63) == 0) wave_best[t >> 6] = key;
    __syncthreads();
    if (t == 0) {
        for (int i = 1; i < 4; ++i) key = wave_best[i] > key ? wave_best[i] : key;
        if (key) __hip_atomic_fetch_max(job.best, key, RLX, AGENT);
    }
}

__global__ __launch_bounds__(256) void apply_kernel(PassPack pack) {
    const PassJob job = pack.j[job_of_block(pack, (int)blockIdx.x)];
    const int tile = (int)blockIdx.x - job.tile_begin;
    const int x0 = (tile % job.tiles_x) * TILE, y0 = (tile / job.tiles_x) * TILE;
    const int t = (int)threadIdx.x, x = x0 + (t & 63);
    const bool islands = pack.polarity != 0;
    const int kept = islands ? (int)~(unsigned)(*job.best) : -1;
#pragma unroll
    for (int i = 0; i < PX_PER_THREAD; ++i) {
        const int y = y0 + (t >> 6) + 4 * i;
        if (x >= job.w || y >= job.h) continue;
        const int p = y * job.w + x;
        const int l = job.labels[p];
        if (l < 0) continue;
        const int r = job.labels[l];
        if (job.area[r] < job.threshold && r != kept) job.mask[p] = (uint8_t)(255 - pack.polarity);
    }
}

size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

// Throws on the first bad job; returns nothing the kernels rely on.
void check_jobs(const k::CleanJob* jobs, int count, bool pointers) {
    if (count < 0 || (count > 0 && !jobs)) throw_error("mask_cleanup: invalid job list");
    for (int i = 0; i < count; ++i) {
        const k::CleanJob& j = jobs[i];
        if (j.w <= 0 || j.h <= 0) throw_error("mask_cleanup: invalid extent");
        if ((long long)j.w * (long long)j.h > 0x7fffffffLL) throw_error("mask_cleanup: w * h does not fit an int");
        if (j.max_hole < 0 || j.max_island < 0) throw_error("mask_cleanup: negative threshold");
        if (j.max_hole == 0 && j.max_island == 0) throw_error("mask_cleanup: both thresholds are 0: nothing to clean");
        if (pointers && !j.mask) throw_error("mask_cleanup: null mask");
    }
}

// per job: labels and areas, 4 bytes per pixel each; in front of them one 8-byte `best` word per job
size_t job_words(const k::CleanJob& j) { return round_up((size_t)j.w * j.h, 4); }

}  // namespace

namespace k {

size_t mask_cleanup_workspace_bytes(const CleanJob* jobs, int count) {
    check_jobs(jobs, count, false);
    size_t bytes = round_up((size_t)count * sizeof(unsigned long long), 16);
    for (int i = 0; i < count; ++i) bytes += 2 * job_words(jobs[i]) * sizeof(int);
    return bytes;
}

}  // namespace k

namespace {
// The launches of one call, in order; dry: counted only.  Returns their number.
int run_passes(const k::CleanJob* jobs, int count, void* workspace, hipStream_t s, bool dry) {
    using k::CleanJob;
    int launches = 0;
    unsigned long long* const best = static_cast<unsigned long long*>(workspace);
    int* const words = dry ? nullptr : reinterpret_cast<int*>(static_cast<uint8_t*>(workspace) + round_up((size_t)count * sizeof(unsigned long long), 16));
    for (int polarity = 0; polarity <= 255; polarity += 255) {
        PassPack pack{};
        pack.polarity = polarity;
        long long tiles = 0;
        auto launch = [&] {
            if (pack.n == 0) return;
            launches += 4;
            const dim3 grid((unsigned)tiles);
            if (!dry) hipLaunchKernelGGL(tile_label_kernel, grid, dim3(256), 0, s, pack);
            if (!dry) hipLaunchKernelGGL(border_merge_kernel, grid, dim3(128), 0, s, pack);
            if (!dry) hipLaunchKernelGGL(root_areas_kernel, grid, dim3(256), 0, s, pack);
            if (!dry) hipLaunchKernelGGL(apply_kernel, grid, dim3(256), 0, s, pack);
            pack.n = 0;
            tiles = 0;
        };
        size_t at = 0;
        for (int i = 0; i < count; ++i) {
            const CleanJob& j = jobs[i];
            const size_t mine = at;
            at += 2 * job_words(j);
            const int threshold = polarity == 0 ? j.max_hole : j.max_island;
            if (threshold == 0) continue;
            const int tiles_x = (j.w + TILE - 1) / TILE, tiles_y = (j.h + TILE - 1) / TILE;
            const long long n = (long long)tiles_x * tiles_y;
            if (pack.n == MAX_JOBS || tiles + n > 0x7fffffffLL) launch();
            if (!dry) pack.j[pack.n] = PassJob{j.mask, words + mine, words + mine + job_words(j), best + i, j.w, j.h, threshold, tiles_x, (int)tiles};
            ++pack.n;
            tiles += n;
        }
        launch();
    }
    return launches;
}
}  // namespace

namespace k {

int mask_cleanup_launches(const CleanJob* jobs, int count) {
    check_jobs(jobs, count, false);
    return run_passes(jobs, count, nullptr, nullptr, true);
}

void mask_cleanup(const CleanJob* jobs, int count, void* workspace, hipStream_t s) {
    check_jobs(jobs, count, true);
    if (count == 0) return;
    if (!workspace) throw_error("mask_cleanup: null workspace");
    run_passes(jobs, count, workspace, s, false);
}

}  // namespace k
}  // namespace dlimg
