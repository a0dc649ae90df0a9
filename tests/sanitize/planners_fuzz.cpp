// ASan + UBSan harness for the pure host planners (tests/test_sanitizers.py): csrc/step_queue.hpp (which lane takes which
// requests), csrc/mask_pieces.hpp (how a batch of masks is cut into transfer pieces), csrc/mask_transport.hpp (which road
// the masks of a request take to the caller), csrc/resize_tables.cpp (the contributor tables the resize kernels index
// with), csrc/gemm_plan.cpp (which tile configuration runs a GEMM) and csrc/prompt_plan.hpp (the entries of a batch mask
// call as prompts, stages and packed points) on a few hundred thousand random inputs, with the invariants the callers rely
// on checked on every one.
#include "gemm_plan.hpp"
#include "mask_pieces.hpp"
#include "mask_transport.hpp"
#include "prompt_plan.hpp"
#include "resize_tables.hpp"
#include "step_queue.hpp"

#include <cstdint>
#include <cmath>
#include <cstdio>
#include <numeric>

using namespace dlimg;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % (n ? n : 1));
}

struct PlanError { const char* msg; };
namespace dlimg { void throw_error(const char* msg) { throw PlanError{msg}; } }

// csrc/gemm_plan.cpp: valid and invalid GemmArgs (the planner reads addresses for their alignment only).  What gemm.hip's
// launchers rely on: a picked tile fits, and a tile that fits divides the problem, takes the f16-pair stream only on a
// ping-pong kernel and has room for the consumer's statistic groups.  What the batch-equals-single tests rely on: a batch
// of units runs the tile of one unit, or -- not for a LayerNorm-folded consumer -- another ping-pong tile (same bits).
static bool is_pingpong(int tile) { return tile >= 0 && k::kGemmTiles[tile].family == k::TileFamily::pingpong; }
static const char* check_pick(k::GemmArgs const& a, int* picked) {
    const int t = *picked = k::gemm_pick_tile(a);
    if (t != -1 && !k::gemm_tile_fits(a, t)) return "picked a tile that does not fit";
    if (a.tile >= 0 && t != (k::gemm_tile_fits(a, a.tile) ? a.tile : -1)) return "a preset tile is returned exactly when it fits";
    return nullptr;
}
static const char* fuzz_gemm_plan_once(int* valid) {
    alignas(16) static char mem[32];
    auto addr = [&](int odds_bad) { return mem + (rnd(odds_bad) ? 0 : 1 + rnd(15)); };
    auto dim = [&] { const int d = 64 * (1 + (int)rnd(80)); return rnd(12) ? d : rnd(2) ? d + 1 + (int)rnd(63) : (int)rnd(3) - 1; };
    k::GemmArgs a;
    a.unit_rows = rnd(3) ? 64 * (1 + (int)rnd(64)) : rnd(3) ? 0 : (int)rnd(5000);
    a.M = (a.unit_rows > 0 && rnd(2)) ? a.unit_rows : dim();
    a.N = rnd(3) ? 256 * (1 + (int)rnd(20)) : dim();
    a.ln_groups = (int)rnd(31);
    a.K = (a.ln_groups > 0 && rnd(4)) ? a.ln_groups * 64 * (1 + (int)rnd(4)) : dim();
    a.A = reinterpret_cast<half_t*>(addr(40)); a.W = reinterpret_cast<half_t*>(addr(40));
    a.lda = rnd(20) ? a.K + 8 * (int)rnd(3) : a.K - 8 + (int)rnd(12);
    a.ldw = rnd(20) ? a.K + 8 * (int)rnd(3) : a.K - 8 + (int)rnd(12);
    if (rnd(2)) a.bias = reinterpret_cast<float*>(addr(40));
    const int resid = (int)rnd(rnd(20) ? 3 : 5);         // none, fp32, pair; rarely half a pair, or both kinds
    if (resid == 1 || resid == 4) { a.resid = reinterpret_cast<float*>(addr(40)); a.ldr = a.N + (rnd(20) ? 0 : 1 + (int)rnd(3)); }
    if (resid >= 2) { a.resid_h = reinterpret_cast<half_t*>(addr(40)); a.ldrs = a.N + (rnd(20) ? 0 : 1 + (int)rnd(3)); }
    if (resid == 2 || resid == 4) a.resid_l = reinterpret_cast<half_t*>(addr(40));
    const uint32_t mod = rnd(8);
    a.resid_mod = mod < 3 ? a.M : mod < 5 ? a.unit_rows : mod < 7 ? 64 * (1 + (int)rnd(8)) : (int)rnd(200) - 10;
    const int out = (int)rnd(rnd(20) ? 4 : 6);           // fp32, f16, both, pair; rarely none, or a pair beside fp32
    if (out == 0 || out == 2 || out == 5) { a.out_f32 = reinterpret_cast<float*>(addr(40)); a.ldc32 = a.N + (rnd(20) ? 0 : 2); }
    if (out == 1 || out == 2 || out == 3 || out == 5) { a.out_h = reinterpret_cast<half_t*>(addr(40)); a.ldc16 = a.N + (rnd(20) ? 0 : 2); }
    if (out == 3 || out == 5) a.out_l = reinterpret_cast<half_t*>(addr(40));
    if (!rnd(4)) a.stats_out = reinterpret_cast<float*>(mem);
    if (!rnd(3)) { a.ln_stats = reinterpret_cast<float*>(mem); a.ln_colsum = rnd(30) ? reinterpret_cast<float*>(addr(40)) : nullptr; }
    a.act = rnd(3) ? k::ACT_NONE : k::ACT_GELU;
    a.shared_gpu = rnd(2) != 0; a.alone = rnd(2) != 0;
    a.tile = rnd(4) ? -1 : (int)rnd(15) - 2;             // preset: -2 .. 12
    if (k::gemm_check(a)) return nullptr;
    ++*valid;
    int picked;
    if (const char* bad = check_pick(a, &picked)) return bad;
    for (int t = -1; t <= k::kGemmNumTiles; ++t) {
        if (!k::gemm_tile_fits(a, t)) continue;
        if (t < 0 || t >= k::kGemmNumTiles) return "a tile outside the table fits";
        k::GemmTile const& row = k::kGemmTiles[t];
        if (a.M % row.bm || a.N % row.bn || ((a.resid || a.resid_h) && a.resid_mod % row.bm)) return "a tile that fits does not divide the problem";
        if ((a.out_l || a.resid_h) && !(row.pair_stream && is_pingpong(t))) return "f16-pair stream on a tile without the ping-pong epilogue";
        if (a.ln_stats && a.ln_groups > row.stat_groups) return "more statistic groups than the tile merges";
        if (is_pingpong(t) && !a.out_f32 && !a.out_l && (a.resid || a.resid_h || a.stats_out))
            return "a residual or row statistics on a ping-pong tile's f16-rows epilogue, which has neither";
    }
    k::GemmArgs once = a;
    try {
        const int bn = k::gemm_choose_tile(once);
        k::GemmArgs twice = once;
        if (once.tile < 0 || bn != k::kGemmTiles[once.tile].bn || k::gemm_choose_tile(twice) != bn || twice.tile != once.tile)
            return "gemm_choose_tile twice differs";
        if (k::gemm_pick_tile(once) != once.tile) return "the launch would not use the chosen tile";
    } catch (PlanError const&) {
        k::GemmArgs free_choice = a;
        if (!k::gemm_tile_fits(a, a.tile)) free_choice.tile = -1;
        if (k::gemm_pick_tile(free_choice) != -1) return "gemm_choose_tile refuses a problem that has a tile";
    }
    if (a.tile < 0 && a.unit_rows > 0 && a.M == a.unit_rows) {           // one unit against a batch of them
        k::GemmArgs batch = a;
        batch.M = a.M * (2 + (int)rnd(7));
        if ((a.resid || a.resid_h) && a.resid_mod == a.M && rnd(2)) batch.resid_mod = batch.M;      // the stream itself as residual
        if (k::gemm_check(batch)) return "a batch of valid units is refused";
        int batch_picked;
        if (const char* bad = check_pick(batch, &batch_picked)) return bad;
        if (batch_picked != picked && (a.ln_stats || !is_pingpong(picked) || !is_pingpong(batch_picked)))
            return "a batch runs another tile than its units";
    }
    return nullptr;
}
static void print_gemm(k::GemmArgs const& a) {
    std::printf("M %d N %d K %d resid %d/%d mod %d pair out %d stats %d ln %d groups %d shared %d alone %d unit %d tile %d\n", a.M, a.N, a.K,
                a.resid != nullptr, a.resid_h != nullptr, a.resid_mod, a.out_l != nullptr, a.stats_out != nullptr, a.ln_stats != nullptr,
                a.ln_groups, (int)a.shared_gpu, (int)a.alone, a.unit_rows, a.tile);
}
static bool fuzz_gemm_plan() {
    int valid = 0;
    for (int iter = 0; iter < 100000; ++iter)
        if (const char* bad = fuzz_gemm_plan_once(&valid)) { std::printf("gemm plan: %s (iteration %d)\n", bad, iter); return false; }
    if (valid < 30000) { std::printf("gemm plan: only %d of the random problems pass gemm_check\n", valid); return false; }
    // A LayerNorm-folded consumer beside other lanes whose shape asks for a ping-pong tile (N % 256 == 0, >= 64 tiles) but
    // whose producer left more groups than those kernels have LDS room for: any tile but a ping-pong one
    alignas(16) static char mem[16];
    for (int groups = kPPStatGroups + 1; groups <= k::kGemmMaxStatGroups; ++groups)
        for (int variant = 0; variant < 8; ++variant) {
            k::GemmArgs a;
            a.A = a.W = reinterpret_cast<half_t*>(mem); a.out_h = reinterpret_cast<half_t*>(mem);
            a.ln_stats = a.ln_colsum = reinterpret_cast<float*>(mem); a.ln_groups = groups;
            a.unit_rows = 4096; a.M = (variant & 1) ? 8192 : 4096; a.N = (variant & 2) ? 1024 : 2304 + 256; a.K = groups * 64;
            a.lda = a.ldw = a.K; a.ldc16 = a.N; a.shared_gpu = true; a.alone = (variant & 4) != 0;
            const int t = k::gemm_check(a) ? -1 : k::gemm_pick_tile(a);
            if (t < 0 || is_pingpong(t) || !k::gemm_tile_fits(a, t)) { std::printf("gemm plan: consumer with %d groups on tile %d\n", groups, t); print_gemm(a); return false; }
        }
    return true;
}

// csrc/mask_transport.hpp: 1-33 masks of 1 B to 12 MB with random pinned destinations, idle flags and IoU counts (and the
// device form of the same masks).  What the executor and finish_masks rely on: the layout is 256-aligned and strictly
// increasing, the pieces are strictly increasing and end where the reservation does, walking them with
// mask_copies_in_piece copies every byte of every mask that is not in place exactly once from where the kernel was told to
// write it (and nothing of a mask in place), a direct piece is not waited for before its mask is complete, and no launch,
// copy command or host copy leaves the reservation.
static const char* fuzz_mask_transport_once(MaskTransportInput& in, MaskTransportPlan& p) {
    const int count = 1 + (int)rnd(33);
    in.sizes.resize(count);
    in.dst_pinned.resize(count);
    const uint32_t pinned_odds = rnd(3);         // none, about half, all
    for (int i = 0; i < count; ++i) {
        in.sizes[i] = 1 + rnd(rnd(3) ? 12000000 : rnd(2) ? 70000 : 600);
        in.dst_pinned[i] = pinned_odds == 0 ? 0 : pinned_odds == 2 ? 1 : (char)rnd(2);
    }
    in.iou_count = rnd(3) ? 4 * (int)rnd(count + 1) : 0;
    in.direct_allowed = rnd(8) != 0;
    in.others_idle = rnd(2) != 0;
    plan_mask_transport(in, p);
    const bool direct = in.direct_allowed && (count == 1 || (count <= 6 && in.others_idle));
    if ((p.mode == MaskMode::direct) != direct || (!direct && p.mode != MaskMode::staged)) return "mode";
    if ((int)p.kernel_dst.size() != count || (int)p.in_place.size() != count) return "a vector per mask has another length";
    std::vector<size_t> off(count);
    size_t total = 0;
    for (int i = 0; i < count; ++i) {
        off[i] = total;
        if (off[i] % 256 || (i && off[i] <= off[i - 1])) return "offsets not aligned or not increasing";
        total += padded_mask_bytes(in.sizes[i]);
    }
    const size_t with_iou = total + 4 * (size_t)in.iou_count;
    if (p.iou_offset != total || p.reserve_device != with_iou || p.reserve_pinned != with_iou) return "reservation";
    for (int i = 0; i < count; ++i) {
        if (p.kernel_dst[i] == kCallersPointer ? !(direct && in.dst_pinned[i]) : p.kernel_dst[i] != off[i]) return "kernel destination";
        if (p.kernel_dst[i] != kCallersPointer && p.kernel_dst[i] + in.sizes[i] > with_iou) return "a mask leaves the reservation";
        if (direct && (p.kernel_dst[i] == kCallersPointer) != (p.in_place[i] != 0)) return "direct: in place without the kernel writing there";
    }
    if (p.piece_end.empty() || p.piece_end.back() != with_iou) return "the pieces do not end where the reservation does";
    for (size_t i = 1; i < p.piece_end.size(); ++i)
        if (p.piece_end[i] <= p.piece_end[i - 1]) return "pieces not increasing";
    if (direct)
        for (int i = 0; i < count; ++i)
            if ((int)p.piece_end.size() != count || p.piece_end[i] < off[i] + in.sizes[i]) return "direct: a piece ends before its mask";
    // the steps: every mask launched once and in order, an event per piece in order, copies inside the reservation; in
    // staged mode what reaches the pinned buffer piece by piece is the device buffer at the same offsets
    int launched = 0, events = 0;
    size_t arrived = 0;                           // staged pieces: the pinned buffer holds the staging area up to here
    std::vector<size_t> sent(count, 0);           // bytes of mask i a copy command took to its destination
    for (MaskStep const& s : p.steps) {
        if (s.kind == MaskStep::launch) {
            if (s.first != launched || s.count <= 0 || (direct ? s.count != 1 : s.count != count)) return "launch";
            launched += s.count;
        } else if (s.kind == MaskStep::event) {
            if (s.first != events++ || launched < (direct ? s.first + 1 : count)) return "event";
        } else {
            if (s.bytes == 0 || launched == 0) return "empty or early copy";
            if (s.from == MaskMem::iou) {
                if (s.from_offset != 0 || s.bytes != 4 * (size_t)in.iou_count || s.to_offset != total || s.to != (direct ? MaskMem::pinned : MaskMem::device)) return "IoU copy";
            } else if (s.from != MaskMem::device || s.from_offset + s.bytes > with_iou) {
                return "copy from outside the device buffer";
            } else if (s.to == MaskMem::caller) {
                if (s.mask < 0 || s.mask >= count || !p.in_place[s.mask] || s.from_offset != off[s.mask] || s.to_offset != 0 || s.bytes != in.sizes[s.mask]) return "copy to a caller";
                sent[s.mask] += s.bytes;
            } else if (s.to == MaskMem::pinned) {
                if (s.to_offset != s.from_offset || s.to_offset + s.bytes > with_iou) return "copy to the pinned buffer";
                if (s.from_offset == arrived) arrived += s.bytes;
            } else {
                return "copy to nowhere";
            }
        }
    }
    if (launched != count || p.launches != (direct ? count : 1) || events != (int)p.piece_end.size()) return "launches or events";
    // finish_masks' walk
    MaskCursor cursor;
    size_t begin = 0;
    std::vector<size_t> copied(count, 0);
    for (size_t end : p.piece_end) {
        for (MaskCopy const& c : mask_copies_in_piece(in.sizes, begin, end, cursor)) {
            if (p.in_place[c.mask]) continue;
            if (c.staging_offset != p.kernel_dst[c.mask] + c.mask_offset || c.mask_offset != copied[c.mask]) return "host copy not from where the kernel wrote";
            if (!direct && c.staging_offset + c.bytes > arrived) return "host copy of bytes no copy command brought";
            copied[c.mask] += c.bytes;
        }
        begin = end;
    }
    for (int i = 0; i < count; ++i) {
        if (copied[i] != (p.in_place[i] ? 0 : in.sizes[i])) return "host copies do not cover the masks";
        if (!direct && sent[i] != (p.in_place[i] ? in.sizes[i] : 0)) return "copy commands do not cover the masks in place";
    }
    // device form of the same masks
    const bool own = rnd(2) != 0;
    plan_mask_transport_device(in.sizes, own, p);
    if (p.mode != (own ? MaskMode::device_direct : MaskMode::device_staged) || p.launches != 1 || !p.piece_end.empty()) return "device form: mode";
    if (p.reserve_pinned != 0 || p.reserve_device != (own ? 0 : total)) return "device form: reservation";
    if (p.steps.size() != (own ? 1u : 1u + count) || p.steps[0].kind != MaskStep::launch || p.steps[0].first != 0 || p.steps[0].count != count) return "device form: steps";
    for (int i = 0; i < count; ++i) {
        if (p.kernel_dst[i] != (own ? kCallersPointer : off[i])) return "device form: kernel destination";
        if (own) continue;
        MaskStep const& s = p.steps[1 + i];
        if (s.kind != MaskStep::copy || s.from != MaskMem::device || s.to != MaskMem::peer || s.mask != i || s.from_offset != off[i] ||
            s.to_offset != 0 || s.bytes != in.sizes[i] || s.from_offset + s.bytes > p.reserve_device) return "device form: peer copy";
    }
    return nullptr;
}

// csrc/prompt_plan.hpp: calls of 1 to 24 entries -- handles, clicks, marks, now and then a bad label or a mark out of place --
// with any combination of the two arrays.  What the batch calls rely on: a call is refused or read into prompts whose clicks
// travel in entries of the call, whose stages grow and end at all clicks; and pack_points writes exactly the points of the
// stage -- the buffers here hold that many and not one more -- clicks first (labels 0 / 1, the head's 1), then the corners
// (2, 3) or the padding point (-1).
static const char* fuzz_prompt_plan_once(int* valid) {
    const int count = 1 + (int)rnd(24);
    std::vector<char> has_handle(count);
    std::vector<int> points(2 * count), regions(4 * count, 0);
    const bool points_given = rnd(6) != 0, regions_given = rnd(4) != 0, branch = rnd(8) != 0;
    for (int i = 0; i < count; ++i) {
        has_handle[i] = i == 0 ? rnd(30) != 0 : rnd(3) == 0;
        points[2 * i] = (int)rnd(5000) - 500;
        points[2 * i + 1] = (int)rnd(5000) - 500;
        int* r = &regions[4 * i];
        if (has_handle[i]) {
            r[0] = (int)rnd(2000); r[1] = (int)rnd(2000);
            r[2] = rnd(3) ? r[0] + (int)rnd(2000) : -1; r[3] = rnd(3) ? r[1] + (int)rnd(2000) : -1;
        } else {
            r[0] = rnd(5) == 0 ? kRefineMark : rnd(40) ? (int)rnd(2) : (int)rnd(8) - 2;
            if (!rnd(60)) r[1 + rnd(3)] = 1 + (int)rnd(3);
        }
    }
    int const* reg = regions_given ? regions.data() : nullptr;
    StagedPrompts plan;
    try {
        plan = plan_staged_prompts(has_handle, points_given, reg, branch);
    } catch (std::invalid_argument const&) {
        return nullptr;
    }
    ++*valid;
    if (plan.prompts.empty() || plan.prompts.size() != plan.stages.size()) return "prompts and stages";
    for (size_t j = 0; j < plan.prompts.size(); ++j) {
        PromptSpec const& p = plan.prompts[j];
        PromptStages const& st = plan.stages[j];
        if (p.head < 0 || p.head >= count || !has_handle[p.head] || p.clicks < 0 || p.clicks > kMaxClicks) return "prompt";
        if (p.clicks != (points_given ? (int)st.click_entry.size() : 0) || (p.box && !reg)) return "clicks or box without their array";
        for (int c = 0; c < p.clicks; ++c) {
            const int e = st.click_entry[c];
            if (e < p.head || e >= count || (c == 0 ? e != p.head : (has_handle[e] || e <= st.click_entry[c - 1]))) return "click entry";
            if (c && is_mark_entry(reg, e)) return "a mark read as a click";
        }
        if (st.stage_clicks.empty() || st.stage_clicks.back() != p.clicks) return "the last stage does not take all clicks";
        for (size_t k = 1; k < st.stage_clicks.size(); ++k)
            if (st.stage_clicks[k] <= st.stage_clicks[k - 1] || st.stage_clicks[0] < 1) return "stages do not grow";
        ResizeLongestSide rs;
        rs.set(Extent{1 + (int)rnd(rnd(2) ? 1024 : 8000), 1 + (int)rnd(rnd(2) ? 1024 : 8000)});
        for (int clicks : st.stage_clicks) {
            const int want = clicks + (p.box ? 2 : 1);
            if (clicks == p.clicks && want != p.points()) return "points()";
            std::vector<float> coords(2 * want), labels(want);          // exactly: ASan sees one write too many
            if (pack_points(rs, p, st, clicks, points_given ? points.data() : nullptr, reg, coords.data(), labels.data()) != want) return "pack_points: count";
            for (int c = 0; c < clicks; ++c) {
                if (labels[c] != (c == 0 ? 1.f : reg ? (float)reg[4 * st.click_entry[c]] : 1.f) || (labels[c] != 0.f && labels[c] != 1.f)) return "pack_points: click label";
                const Point t = rs.transform(Point{points[2 * st.click_entry[c]], points[2 * st.click_entry[c] + 1]});
                if (coords[2 * c] != (float)t.x || coords[2 * c + 1] != (float)t.y) return "pack_points: click";
            }
            if (p.box) {
                const Point a = rs.transform(Point{reg[4 * p.head], reg[4 * p.head + 1]}), b = rs.transform(Point{reg[4 * p.head + 2], reg[4 * p.head + 3]});
                if (labels[clicks] != 2.f || labels[clicks + 1] != 3.f || coords[2 * clicks] != (float)a.x || coords[2 * clicks + 1] != (float)a.y ||
                    coords[2 * clicks + 2] != (float)b.x || coords[2 * clicks + 3] != (float)b.y) return "pack_points: box";
            } else if (labels[clicks] != -1.f || coords[2 * clicks] != 0.f || coords[2 * clicks + 1] != 0.f) {
                return "pack_points: padding point";
            }
        }
    }
    return nullptr;
}

int main() {
    if (!fuzz_gemm_plan()) return 1;
    {
        int valid = 0;
        for (int iter = 0; iter < 100000; ++iter)
            if (const char* bad = fuzz_prompt_plan_once(&valid)) { std::printf("prompt plan: %s (iteration %d)\n", bad, iter); return 1; }
        if (valid < 20000) { std::printf("prompt plan: only %d of the random calls are served\n", valid); return 1; }
    }
    {
        MaskTransportInput in;                   // re-used like a slot's
        MaskTransportPlan plan;
        for (int iter = 0; iter < 30000; ++iter)
            if (const char* bad = fuzz_mask_transport_once(in, plan)) { std::printf("mask transport: %s (iteration %d)\n", bad, iter); return 1; }
    }
    for (int iter = 0; iter < 200000; ++iter) {
        StepQueueState st;
        const int lanes = 1 + (int)rnd(8);
        for (int l = 0; l < lanes; ++l) {
            const int passes = (int)rnd(4);
            st.passes_in_flight.push_back(passes);
            st.images_in_flight.push_back(passes * (1 + (int)rnd(4)));
        }
        st.cursor = (int)rnd(lanes);
        const int pending = (int)rnd(40), width = (int)rnd(9), depth = 1 + (int)rnd(4);
        const bool all = rnd(2) != 0;
        const std::vector<int> before = st.images_in_flight;
        const std::vector<StepPlanPass> plan = plan_device_steps(st, pending, width, depth, all);
        int planned = 0;
        for (StepPlanPass const& p : plan) {
            if (p.lane < 0 || p.lane >= lanes || p.images <= 0 || p.images > std::max(1, width)) { std::printf("bad pass\n"); return 1; }
            planned += p.images;
        }
        if (planned > pending || (all && planned != pending)) { std::printf("planned %d of %d (all %d)\n", planned, pending, (int)all); return 1; }
        int now = std::accumulate(st.images_in_flight.begin(), st.images_in_flight.end(), 0);
        if (now != std::accumulate(before.begin(), before.end(), 0) + planned) { std::printf("state out of step\n"); return 1; }
        if (st.cursor < 0 || st.cursor >= lanes) { std::printf("cursor out of range\n"); return 1; }
    }
    for (int iter = 0; iter < 20000; ++iter) {
        const int count = (int)rnd(40);
        std::vector<size_t> sizes(count);
        size_t total = 0;
        for (auto& s : sizes) { s = 1 + rnd(rnd(4) ? 3000000 : 70); total += padded_mask_bytes(s); }
        total += rnd(2) ? rnd(64) * 4 : 0;
        const std::vector<size_t> ends = mask_piece_ends(total);
        if (total && (ends.empty() || ends.back() != total)) { std::printf("pieces do not cover the staging area\n"); return 1; }
        MaskCursor cursor;
        size_t begin = 0;
        std::vector<size_t> copied(count, 0);
        for (size_t end : ends) {
            if (end <= begin) { std::printf("empty piece\n"); return 1; }
            for (MaskCopy const& c : mask_copies_in_piece(sizes, begin, end, cursor)) {
                if (c.mask < 0 || c.mask >= count || c.bytes == 0 || c.mask_offset + c.bytes > sizes[c.mask] ||
                    c.staging_offset < begin || c.staging_offset + c.bytes > end) { std::printf("copy outside its piece or mask\n"); return 1; }
                if (c.mask_offset != copied[c.mask]) { std::printf("mask bytes out of order\n"); return 1; }
                copied[c.mask] += c.bytes;
            }
            begin = end;
        }
        for (int i = 0; i < count; ++i)
            if (copied[i] != sizes[i]) { std::printf("mask %d: %zu of %zu bytes copied\n", i, copied[i], sizes[i]); return 1; }
    }
    // resize tables: any axis from 1 pixel to far beyond what an image has, both filters; the kernels read coef[o * taps + k]
    // for k < count[o] and clamp first[o] + k into the source
    for (int iter = 0; iter < 1500; ++iter) {
        const int shape = (int)rnd(12);
        const int in_size = shape == 0 ? 1 + (int)rnd(4) : shape == 1 ? 20000 + (int)rnd(20000) : 1 + (int)rnd(4000);
        const int out_size = shape == 2 ? 1 + (int)rnd(4) : shape == 3 ? 1024 : 1 + (int)rnd(2048);
        const ResizeFilter filter = rnd(2) ? ResizeFilter::default_ : ResizeFilter::box;
        const AxisTable t = make_axis_table(in_size, out_size, filter);
        if (t.in_size != in_size || t.out_size != out_size || t.taps <= 0 || (int)t.first.size() != out_size ||
            (int)t.count.size() != out_size || t.coef.size() != (size_t)out_size * t.taps) { std::printf("table shape %d -> %d\n", in_size, out_size); return 1; }
        for (int o = 0; o < out_size; ++o) {
            if (t.count[o] <= 0 || t.count[o] > t.taps) { std::printf("count %d -> %d at %d\n", in_size, out_size, o); return 1; }
            // a contributor may lie outside the source (edge clamp), but never further than the filter reaches
            if (t.first[o] < -t.taps || t.first[o] + t.count[o] > in_size + t.taps) { std::printf("first %d -> %d at %d\n", in_size, out_size, o); return 1; }
            double sum = 0;
            for (int k = 0; k < t.taps; ++k) {
                const float c = t.coef[(size_t)o * t.taps + k];
                if (!std::isfinite(c) || (k >= t.count[o] && c != 0.0f)) { std::printf("coef %d -> %d at %d\n", in_size, out_size, o); return 1; }
                sum += c;
            }
            if (std::fabs(sum - 1.0) > 1e-3) { std::printf("weights of %d -> %d at %d sum to %g\n", in_size, out_size, o, sum); return 1; }
        }
    }
    std::printf("ok\n");
    return 0;
}
