// Which tile configuration of gemm_plan.hpp runs a GEMM: argument checks, the fits rule and the choice.  Host only.
#include "gemm_plan.hpp"

namespace dlimg {
namespace k {

namespace {
// out_h alone: the ping-pong tiles then run their f16-rows epilogue (qkv, fc1), which takes bias, the folded LayerNorm and
// GELU in registers and nothing else
bool f16_rows_only(const GemmArgs& a) { return !a.out_f32 && !a.out_l; }
bool pingpong_drops(const GemmArgs& a) { return f16_rows_only(a) && (a.resid || a.resid_h || a.stats_out); }
}  // namespace

const char* gemm_check(const GemmArgs& a) {
    if (a.M <= 0 || a.N <= 0 || a.K <= 0) return "gemm: empty problem";
    if (a.M % 64 || a.N % 64 || a.K % kGemmKStep) return "gemm: M, N must be multiples of 64 and K of 64";
    if (a.lda % 8 || a.ldw % 8) return "gemm: operand leading dimensions must be multiples of 8 (16-byte rows)";
    if (a.lda < a.K || a.ldw < a.K) return "gemm: leading dimension smaller than K";
    if (((uintptr_t)a.A | (uintptr_t)a.W) & 15) return "gemm: operands must be 16-byte aligned";
    if (a.resid && (a.resid_mod <= 0 || a.resid_mod % 64)) return "gemm: resid_mod must be a positive multiple of 64";
    if (!a.out_f32 && !a.out_h) return "gemm: no output";
    if (a.out_l && (a.out_f32 || !a.out_h || ((uintptr_t)a.out_l & 7))) return "gemm: an f16-pair result needs out_h and out_l (8-byte aligned) and no out_f32";
    if ((a.resid_h != nullptr) != (a.resid_l != nullptr) || (a.resid_h && a.resid))
        return "gemm: the residual is either fp32 or an f16 pair (resid_h and resid_l)";
    if (a.resid_h && ((((uintptr_t)a.resid_h | (uintptr_t)a.resid_l) & 7) || a.ldrs % 4 || a.resid_mod <= 0 || a.resid_mod % 64))
        return "gemm: f16-pair residual rows must be 8-byte aligned, resid_mod a positive multiple of 64";
    if ((a.bias && ((uintptr_t)a.bias & 15)) || (a.resid && (((uintptr_t)a.resid & 15) || a.ldr % 4)) ||
        (a.out_f32 && (((uintptr_t)a.out_f32 & 15) || a.ldc32 % 4)) ||
        (a.out_h && (((uintptr_t)a.out_h & 7) || a.ldc16 % 4)))
        return "gemm: bias/residual/output rows must be 16-byte (f16 output: 8-byte) aligned";
    static_assert(kGemmMaxStatGroups == 24, "the message below names the bound");
    if (a.ln_stats && (!a.ln_colsum || ((uintptr_t)a.ln_colsum & 15) || a.ln_groups <= 0 || a.K % a.ln_groups ||
                       a.ln_groups > kGemmMaxStatGroups))
        return "gemm: folded LayerNorm needs aligned column sums and 1..24 statistic groups that divide K";
    if (a.stats_out && (a.ln_stats || a.act != ACT_NONE))
        return "gemm: row statistics cannot be combined with an activation or a folded LayerNorm";
    // an f16-pair residual runs on the ping-pong tiles only, and their f16-rows epilogue adds no residual (gemm_tile_fits)
    if (a.resid_h && f16_rows_only(a))
        return "gemm: an f16-pair residual needs an fp32 or f16-pair result (the f16-only epilogue of the ping-pong tiles adds no residual)";
    return nullptr;
}

// GemmArgs::shared_gpu -- with several execution lanes the GPU is shared between kernels of different images: tiles
// that leave room for a second workgroup on the CU (<= 64 KB LDS) let those kernels overlap, which is worth more
// than the better isolated efficiency of the one-workgroup-per-CU tiles (measured: +8 % images/s).  It is a property
// of the caller (SamModel knows how many lanes share its device), not process state.
bool gemm_tile_fits(const GemmArgs& a, int tile) {
    if (tile < 0 || tile >= kGemmNumTiles) return false;
    const GemmTile& t = kGemmTiles[tile];
    if ((a.out_l || a.resid_h) && !t.pair_stream) return false;          // f16-pair stream: ping-pong epilogue only
    if (a.ln_stats && a.ln_groups > t.stat_groups) return false;         // registers / LDS room for the raw partials
    // the f16-rows epilogue of the ping-pong kernels reads no residual and computes no row statistics: such problems
    // (the decoder's final_kv: fp32 residual, f16 result) belong to the ring tiles, which handle both
    if (t.family == TileFamily::pingpong && pingpong_drops(a)) return false;
    return a.M % t.bm == 0 && a.N % t.bn == 0 && !((a.resid || a.resid_h) && a.resid_mod % t.bm != 0);
}

int gemm_pick_tile(const GemmArgs& a) {
    if (a.tile >= 0) return gemm_tile_fits(a, a.tile) ? a.tile : -1;     // chosen earlier (pick once, use twice) or forced
    const int unit = (a.unit_rows > 0 && a.M % a.unit_rows == 0) ? a.unit_rows : a.M;   // rows the choice is made for
    // a residual that wraps (row m % resid_mod) must wrap on tile boundaries: the epilogue adds row offsets to the
    // tile's first residual row without a modulo per element
    auto wraps_inside = [&](int bm) { return (a.resid || a.resid_h) && a.resid_mod % bm != 0; };
    const bool shared = a.shared_gpu;
    // The two shortcuts to the ping-pong tiles; -1: neither applies.  (DLIMGEDIT_GEMM_PP128 and _BATCH_PP, the A/B
    // switches they were introduced behind, are gone; what they measured: LABNOTES section 4 and round 6.)
    auto shortcut = [&]() -> int {
        // 256x256 workgroups use a CU about 2.5x better than 128x128 ones (LDS fill rate per FLOP); with other lanes on
        // the remaining CUs that is worth having even when they cover a quarter of the chip (ViT-H proj / fc2: 80
        // workgroups, +2 % images/s; at 48, ViT-B proj / fc2, the longer kernel costs more than it frees)
        if (shared && unit % 256 == 0 && a.N % 256 == 0 && (unit / 256) * (a.N / 256) >= 64 && !wraps_inside(256)) {
            // one image with the GPU to itself and fewer than half the CUs covered (ViT-H's proj / fc2: 80 tiles): the
            // 128-row tiles double the workgroups (160); same bits for a stream writer (not for a LayerNorm-folded consumer)
            if (a.alone && !a.ln_stats && a.M == unit && (unit / 256) * (a.N / 256) < 128 && (unit / 128) * (a.N / 256) <= 256 &&
                !wraps_inside(128))
                return 10;
            return 9;
        }
        // The same with the rows of a whole BATCHED pass (several images stacked in M): two images give ViT-B's proj / fc2
        // 96 tiles of 256 x 256.  Tiles 9 and 10 compute the same bits (BN = 256, the same MFMA, K order, epilogue
        // arithmetic and 64-column statistics groups), so the result does not depend on which one a pass uses -- the
        // batch-equals-single tests assert it.
        // (only where a single unit would run tile 10: the other tiles use a different MFMA shape, i.e. another summation order)
        // too few 256 x 256 tiles (ViT-B proj / fc2: 48): the 128 x 256 ping-pong kernel doubles them
        if (shared && unit % 128 == 0 && a.N % 256 == 0 && (unit / 128) * (a.N / 256) >= 64 && !wraps_inside(128)) {
            // (not for a LayerNorm-folded consumer: its row statistics are merged in an order that depends on the tile height
            // -- RowStats, threads per row -- so a consumer that lands in this branch keeps tile 10 whatever the pass looks like;
            // ViT-B / L / H consumers never do: their N gives >= 64 tiles of 256 x 256)
            if (a.ln_stats) return 10;
            // (proj -- the stream writer with K = N -- on the 128-row tile while fc2 keeps the 256-row one: -1.3 %, r06, not kept)
            if (a.M % 256 == 0 && (a.M / 256) * (a.N / 256) >= 96 && !wraps_inside(256)) return 9;
            // one image with the GPU to itself: 64-row tiles while they still fit the chip in one round (ViT-B's patch / proj /
            // fc2: 96 -> 192 workgroups; ViT-H's 160 would become 320, more than one round: stays)
            if (a.alone && a.M == unit && unit % 64 == 0 && (unit / 64) * (a.N / 256) <= 256 && !wraps_inside(64)) return 11;
            return 10;
        }
        return -1;
    };
    // a shortcut's tile that cannot run the problem (a consumer with more statistic groups than the ping-pong kernels
    // have LDS room for) leaves the choice to the search
    if (const int t = shortcut(); gemm_tile_fits(a, t)) return t;
    int best = -1;
    float best_score = -1.f;
    for (int i = 0; i < kGemmNumTiles; ++i) {
        const GemmTile& t = kGemmTiles[i];
        if (unit % t.bm || a.N % t.bn || wraps_inside(t.bm) || !gemm_tile_fits(a, i)) continue;
        // shared GPU: other lanes fill the CUs this launch leaves free, so the only question is operand
        // traffic per FLOP -- the 256x256 tile (128 FLOP/B) whenever it yields enough workgroups (the shortcuts
        // above), otherwise the tiles that can share a CU
        if (shared && t.per_cu < 2) continue;
        const int blocks = (unit / t.bm) * (a.N / t.bn);
        const int slots = 256 * t.per_cu;
        const int rounds = (blocks + slots - 1) / slots;
        // an unscored tile is taken only where no scored one fits (an f16-pair stream without other lanes whose rows
        // rule out tile 9: the first that fits)
        const float score = t.scored ? t.eff * (float)blocks / (float)(rounds * slots) : 0.f;
        if (score > best_score) { best_score = score; best = i; }
    }
    return best;
}

int gemm_choose_tile(GemmArgs& a) {
    if (const char* err = gemm_check(a)) throw_error(err);
    if (!gemm_tile_fits(a, a.tile)) a.tile = -1;      // a tile set beforehand (test hooks) stays if it can run the problem
    a.tile = gemm_pick_tile(a);
    if (a.tile < 0) gemm_no_tile(a);
    return kGemmTiles[a.tile].bn;
}

void gemm_no_tile(const GemmArgs& a) {
    if (a.tile >= 0 && a.tile < kGemmNumTiles && kGemmTiles[a.tile].family == TileFamily::pingpong && pingpong_drops(a))
        throw_error("gemm: a ping-pong tile with an f16-only result takes no residual and writes no row statistics");
    if (a.out_l || a.resid_h) throw_error("gemm: the f16-pair stream needs a ping-pong tile (N % 256 == 0, shared GPU)");
    throw_error("gemm: no tile configuration fits this shape");
}

}  // namespace k
}  // namespace dlimg
