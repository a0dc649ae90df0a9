// GEMM tile table and tile selection (gemm_plan.cpp): pure host code, a function of GemmArgs alone -- no GPU, no process
// state.  kernels/gemm.hip holds the kernels and one launcher per row of the table; each launcher static_asserts its
// template arguments against its row, so a row and its kernel cannot drift apart.  The selection is checked on the CPU:
// tests/test_gemm_plan.py (recorded choices) and tests/sanitize/planners_fuzz.cpp (invariants on random problems).
#pragma once

#include "kernels/kernels.hpp"

namespace dlimg {

// LayerNorm-folded consumers merge the row statistics their producer left, one (sum, M2) per group of columns.
// Ring kernels (gemm_f16_tile.inc, RowStats): kStatRegs partials per lane, 2 to 8 lanes per row.
constexpr int kStatRegs = 12;                    // partials per lane: N/BN <= 12 * (threads per row)
// Ping-pong kernels (gemm.hip, PPAux): LDS room for the raw partials of kPPStatGroups groups (ping-pong producers leave
// 3 / 4 / 5 for ViT-B / L / H; the 128- and 96-column tiles of a pass without other lanes up to 10)
constexpr int kPPStatGroups = 12;

namespace k {

// Most groups any consumer takes (every ring tile has at least 2 lanes per row); also the most column blocks a producer
// leaves per row, which is what sizes the statistics buffers: [kGemmMaxStatGroups][M][2] floats.
constexpr int kGemmMaxStatGroups = kStatRegs * 2;
constexpr int kGemmKStep = 64;                   // K must be a multiple of this for every configuration

enum class TileFamily {
    ring32,      // gemm_f16_kernel: v_mfma_f32_32x32x16_f16, ring of LDS stages
    ring16,      // gemm16_f16_kernel: v_mfma_f32_16x16x32_f16, BK 32, fragments one K tile ahead
    pingpong,    // gemm_pp_kernel / gemm_pp128_kernel: 8 waves in two groups one barrier apart, BK 64
};

// Tile configurations.  At batch 1 (M = 4096) a GEMM is only a few hundred workgroups, so what matters
// is how evenly they cover the 256 CUs: every scored configuration is rated by (fill of the last round of
// workgroup slots) x (relative efficiency of the tile) and the best one is launched.
struct GemmTile {
    int bm, bn;              // rows x columns of the output tile
    int per_cu;              // workgroups of this tile that share a CU (LDS)
    float eff;               // relative efficiency of the tile (scored tiles)
    int threads;             // per workgroup
    int lds;                 // dynamic LDS, bytes
    TileFamily family;
    bool pair_stream;        // epilogue reads / writes the residual stream as an f16 pair (resid_h / out_l)
    int stat_groups;         // most ln_groups a LayerNorm-folded consumer on this tile merges
    bool scored;             // the scored search rates it; otherwise reached by the shortcuts of gemm_pick_tile or by
                             // forcing, and by the search only where no scored tile fits
};
constexpr GemmTile kGemmTiles[] = {
    // bm   bn  /CU   eff  thr     lds  family                pair   groups              scored
    {128, 384, 1, 1.00f, 256, 135168, TileFamily::ring32, false, kGemmMaxStatGroups, true},     // 0: 2x2 waves (64x192 each), BK 64, 2 stages
    {128, 288, 1, 1.00f, 256, 163072, TileFamily::ring32, false, kGemmMaxStatGroups, true},     // 1: 4x1 waves (32x288 each), BK 64, 3 stages
    {128, 128, 2, 0.80f, 256, 67584, TileFamily::ring32, false, kGemmMaxStatGroups, true},      // 2: 2x2 waves, BK 64, 2 stages
    {128, 96, 1, 0.70f, 256, 116480, TileFamily::ring32, false, kGemmMaxStatGroups, true},      // 3: 4x1 waves, BK 64, 4 stages
    {128, 64, 3, 0.55f, 256, 50688, TileFamily::ring32, false, kGemmMaxStatGroups, true},       // 4: 2x2 waves, BK 64, 2 stages
    {64, 64, 4, 0.40f, 256, 33792, TileFamily::ring32, false, kGemmMaxStatGroups, true},        // 5: 2x2 waves, BK 64, 2 stages
    {256, 256, 1, 0.00f, 512, 135168, TileFamily::ring32, false, kGemmMaxStatGroups, false},    // 6: 8 waves 2x4 (128x64 each), BK 32, 4 stages
    {256, 256, 1, 0.00f, 512, 135168, TileFamily::ring16, false, kGemmMaxStatGroups, false},    // 7: as 6 on 16x16x32 (4096^3: 1010 TFLOP/s)
    {128, 128, 2, 0.00f, 256, 67584, TileFamily::ring16, false, kGemmMaxStatGroups, false},     // 8: 2x2 waves, BK 32, 4 stages (forced only until measured)
    {256, 256, 1, 1.60f, 512, 159744, TileFamily::pingpong, true, kPPStatGroups, true},         // 9: gemm_pp_kernel (4096^3: 1300 TFLOP/s at the 1.4 GHz
                                                                                                 //    the chip holds under that load)
    {128, 256, 1, 0.00f, 512, 162816, TileFamily::pingpong, true, kPPStatGroups, false},        // 10: gemm_pp128_kernel, one read slot + one MFMA slot per K tile
    {64, 256, 1, 0.00f, 512, 131584, TileFamily::pingpong, true, kPPStatGroups, false},         // 11: the same kernel with 64-row tiles: twice the workgroups
                                                                                                 //     for a pass that has the GPU to itself
};
constexpr int kGemmNumTiles = sizeof(kGemmTiles) / sizeof(kGemmTiles[0]);

[[noreturn]] void gemm_no_tile(const GemmArgs&);   // the error of a problem for which gemm_pick_tile returns -1

}  // namespace k
}  // namespace dlimg
