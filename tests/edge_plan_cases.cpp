// Prints what csrc/edge_plan.hpp makes of one batch mask call that may hold edge marks, for tests/test_edge_plan.py to compare
// with what the rules say (built there with the host compiler).
//   edge_plan_cases <edge|cutout> <points given 0|1> <regions given 0|1> <mask branch 0|1> <device form 0|1> [<entry>]...
//       edge: plan_edge_prompts; cutout: plan_cutout_prompts on the same call (what a call without edge marks must equal)
//       entry: <h|c>:<a>,<b>,<c>,<d>[!][=]   h: the entry has a handle, c: it has none; the four ints of its region; `!`: its
//                                            out_masks pointer is NULL; `=`: its pointer is its head's
//   Output: `error <message>` when the call is refused, else one line per prompt -- the line tests/cutout_plan_cases.cpp prints,
//   with ` edge <entry>,<offset>,<feather>,<border>` behind it for a prompt that has one -- then the `any_*` lines of that program
//   and `any_edge 1` in a call with edge marks.
//   edge_plan_cases fuzz <calls> <seed>        plans that many random entry lists and checks of every served call what the batch
//       calls rely on; prints `ok`
#include "edge_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace dlimg;

static int fuzz(int calls, unsigned seed) {
    unsigned long long state = seed * 2862933555777941757ull + 3037000493ull;
    auto next = [&](int n) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((state >> 33) % (unsigned)n);
    };
    long served = 0, refused = 0, with_edge = 0;
    for (int c = 0; c < calls; ++c) {
        const int count = 1 + next(9);
        std::vector<char> has_handle(count), has_pointer(count), same(count);
        std::vector<int> regions((size_t)count * 4);
        for (int i = 0; i < count; ++i) {
            has_handle[i] = next(3) == 0 || (i == 0 && next(8) != 0);
            has_pointer[i] = next(12) != 0;
            same[i] = next(15) == 0;
            int* r = &regions[(size_t)4 * i];
            if (has_handle[i]) {
                const bool empty = next(2) == 0;
                r[0] = empty ? 0 : next(50); r[1] = next(50); r[2] = empty ? -1 : r[0] + next(50); r[3] = r[1] + next(50);
                continue;
            }
            static const int kinds[] = {0, 1, 1, 4, 6, 8, 10, 11, 12, 13, 14, 14, 14, 5};
            // a cut-out mark mostly where it belongs: behind a matte mark
            r[0] = (i > 0 && !has_handle[i - 1] && regions[(size_t)4 * (i - 1)] == 11 && next(3)) ? 13 : kinds[next(14)];
            r[1] = r[2] = r[3] = 0;
            if (r[0] == 6) { r[1] = next(9); r[2] = next(9); }
            if (r[0] == 8) r[1] = next(20) ? next(100001) : -1;
            if (r[0] == 10) { r[1] = next(3) ? 0 : next(5000); r[2] = next(9); }
            if (r[0] == 11) { r[1] = 1 + next(32); r[2] = next(65026); r[3] = next(8) ? (next(2) ? 4 : 3) : 1; }
            if (r[0] == 12) { r[1] = next(4); r[2] = next(2); }
            if (r[0] == 13) { r[1] = next(33); }
            if (r[0] == 14) { r[1] = next(12) ? next(129) - 64 : next(200) - 100; r[2] = next(12) ? next(33) : next(40) - 3; r[3] = next(12) ? next(33) : 33; }
        }
        const bool points = next(6) != 0, regs = next(12) != 0, branch = next(8) != 0, device = next(10) == 0;
        try {
            const EdgePlannedPrompts plan = plan_edge_prompts(has_handle, points, regs ? regions.data() : nullptr, branch, has_pointer, device, same);
            ++served;
            StrokePlannedPrompts const& ws = plan.inner.inner;
            PriorPlannedPrompts const& in = ws.inner.inner.inner;
            StagedPrompts const& st = in.planned.cleaned.staged;
            const size_t n = st.prompts.size();
            if (plan.edge.size() != n || plan.inner.cutout.size() != n || ws.strokes.size() != n || ws.inner.matte.size() != n) return 3;
            int heads = 0;
            for (int i = 0; i < count; ++i) heads += has_handle[i] != 0;
            if ((int)n != heads) return 4;
            bool any = false;
            for (size_t j = 0; j < n; ++j) {
                const int head = ws.caller_entry(st.prompts[j].head);
                if (head < 0 || head >= count || !has_handle[head]) return 5;
                int end = head + 1;
                while (end < count && !has_handle[end]) ++end;
                for (StrokeSpec const& s : ws.strokes[j])
                    if (s.entry <= head || s.entry >= end || regions[(size_t)4 * s.entry] != kStrokeMark) return 6;
                for (int e : st.stages[j].click_entry)
                    if (ws.caller_entry(e) < head || ws.caller_entry(e) >= end) return 13;
                MatteSpec const& m = ws.inner.matte[j];
                if (m.any() && (ws.caller_entry(m.entry) <= head || ws.caller_entry(m.entry) >= end ||
                                regions[(size_t)4 * ws.caller_entry(m.entry)] != kMatteMark))
                    return 7;
                CutoutSpec const& cut = plan.inner.cutout[j];
                if (cut.any() && (cut.entry != end - 1 || regions[(size_t)4 * cut.entry] != kCutoutMark || !m.any() ||
                                  ws.caller_entry(m.entry) != cut.entry - 1))
                    return 8;
                EdgeSpec const& e = plan.edge[j];
                if (!e.any()) continue;
                any = true;
                if (!regs) return 9;
                if (e.entry <= head || e.entry >= end || has_handle[e.entry] || regions[(size_t)4 * e.entry] != kEdgeMark) return 10;
                if (e.offset != regions[(size_t)4 * e.entry + 1] || e.feather != regions[(size_t)4 * e.entry + 2] ||
                    e.border != regions[(size_t)4 * e.entry + 3] || e.offset < -64 || e.offset > 64 || e.feather < 0 || e.feather > 32 ||
                    e.border < 0 || e.border > 32 || (!e.offset && !e.feather && !e.border))
                    return 11;
                // behind it: the matte mark and its cut-out mark only; no grid
                const int behind = end - 1 - e.entry;
                if (behind != (m.any() ? 1 : 0) + (cut.any() ? 1 : 0) || in.planned.grid[j].any()) return 12;
                if (m.any() && ws.caller_entry(m.entry) != e.entry + 1) return 14;
            }
            if (any != plan.any_edge && any) return 15;
            with_edge += any;
        } catch (std::invalid_argument const& e) {
            ++refused;
            if (std::strncmp(e.what(), "mask batch", 10) != 0) return 16;
        }
    }
    std::printf("served %ld refused %ld with an edge mark %ld\nok\n", served, refused, with_edge);
    return served > 0 && refused > 0 && with_edge > 0 ? 0 : 17;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "fuzz")) return fuzz(std::atoi(argv[2]), (unsigned)std::atoi(argv[3]));
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <edge|cutout> <points given> <regions given> <mask branch> <device form> [<h|c>:<a>,<b>,<c>,<d>[!][=]]...\n",
                     argv[0]);
        return 2;
    }
    const bool edge = !std::strcmp(argv[1], "edge");
    const bool points = std::atoi(argv[2]) != 0, regions_given = std::atoi(argv[3]) != 0, branch = std::atoi(argv[4]) != 0,
               device = std::atoi(argv[5]) != 0;
    std::vector<char> has_handle, has_pointer, same;
    std::vector<int> regions;
    for (int i = 6; i < argc; ++i) {
        int r[4] = {0, 0, 0, 0};
        char kind = 0;
        if (std::sscanf(argv[i], "%c:%d,%d,%d,%d", &kind, &r[0], &r[1], &r[2], &r[3]) != 5 || (kind != 'h' && kind != 'c')) {
            std::fprintf(stderr, "bad entry %s\n", argv[i]);
            return 2;
        }
        has_handle.push_back(kind == 'h');
        has_pointer.push_back(std::strchr(argv[i], '!') == nullptr);
        same.push_back(std::strchr(argv[i], '=') != nullptr);
        regions.insert(regions.end(), r, r + 4);
    }
    EdgePlannedPrompts plan;
    try {
        if (edge) {
            plan = plan_edge_prompts(has_handle, points, regions_given ? regions.data() : nullptr, branch, has_pointer, device, same);
        } else {
            plan.inner = plan_cutout_prompts(has_handle, points, regions_given ? regions.data() : nullptr, branch, has_pointer, device, same);
            plan.edge.resize(plan.inner.cutout.size());
        }
    } catch (std::exception const& e) {
        std::printf("error %s\n", e.what());
        return 0;
    }
    StrokePlannedPrompts const& ws = plan.inner.inner;
    PriorPlannedPrompts const& in = ws.inner.inner.inner;
    StagedPrompts const& st = in.planned.cleaned.staged;
    const size_t n = st.prompts.size();
    if (in.planned.cleaned.clean.size() != n || in.planned.grid.size() != n || st.stages.size() != n || in.prior.size() != n ||
        ws.inner.inner.lasso.size() != n || ws.inner.matte.size() != n || ws.strokes.size() != n || plan.inner.cutout.size() != n ||
        plan.edge.size() != n)
        return 3;
    for (size_t j = 0; j < n; ++j) {
        PromptSpec const& p = st.prompts[j];
        std::printf("prompt %d clicks %d box %d points %d entries", p.head, p.clicks, (int)p.box, p.points());
        for (size_t c = 0; c < st.stages[j].click_entry.size(); ++c) std::printf("%c%d", c ? ',' : ' ', st.stages[j].click_entry[c]);
        std::printf(" stages");
        for (size_t k = 0; k < st.stages[j].stage_clicks.size(); ++k) std::printf("%c%d", k ? ',' : ' ', st.stages[j].stage_clicks[k]);
        std::printf(" clean %d,%d grid %d,%d,%d", in.planned.cleaned.clean[j].max_hole, in.planned.cleaned.clean[j].max_island,
                    in.planned.grid[j].side, in.planned.grid[j].iou_permille, in.planned.grid[j].stability_permille);
        if (in.prior[j].any()) std::printf(" prior %d,%d", in.prior[j].entry, in.prior[j].strength_milli);
        LassoSpec const& l = ws.inner.inner.lasso[j];
        if (l.any()) std::printf(" lasso %d,%d,%d", l.entry, l.what, l.strength_milli);
        MatteSpec const& m = ws.inner.matte[j];
        if (m.any()) std::printf(" matte %d,%d,%d,%d", m.entry, m.radius, m.eps, m.channels);
        for (StrokeSpec const& s : ws.strokes[j]) {
            std::printf(" stroke %d,%d,%d:", s.entry, s.label, s.clicks);
            for (size_t c = 0; c < s.click_entry.size(); ++c) std::printf("%s%d", c ? "," : "", s.click_entry[c]);
        }
        if (plan.inner.cutout[j].any()) std::printf(" cutout %d,%d", plan.inner.cutout[j].entry, plan.inner.cutout[j].radius);
        if (plan.edge[j].any()) std::printf(" edge %d,%d,%d,%d", plan.edge[j].entry, plan.edge[j].offset, plan.edge[j].feather, plan.edge[j].border);
        std::printf("\n");
    }
    std::printf("any_clean %d\nany_grid %d\n", (int)in.planned.cleaned.any_clean, (int)in.planned.any_grid);
    if (in.any_prior) std::printf("any_prior 1\n");
    if (ws.inner.inner.any_lasso) std::printf("any_lasso 1\n");
    if (ws.inner.any_matte) std::printf("any_matte 1\n");
    if (ws.any_stroke) {
        std::printf("any_stroke 1\nentry_of");
        for (int e : ws.entry_of) std::printf(" %d", e);
        std::printf("\n");
    }
    if (plan.inner.any_cutout) std::printf("any_cutout 1\n");
    if (plan.any_edge) std::printf("any_edge 1\n");
    return 0;
}
