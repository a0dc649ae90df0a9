// Prints what csrc/stroke_plan.hpp makes of one batch mask call that may hold stroke marks, for tests/test_stroke_plan.py to compare
// with what the rules say (built there with the host compiler).
//   stroke_plan_cases <stroke|matte> <points given 0|1> <regions given 0|1> <mask branch 0|1> <device form 0|1> [<entry>]...
//       stroke: plan_stroke_prompts; matte: plan_matte_prompts on the same call (what a call without stroke marks must equal)
//       entry: <h|c>:<a>,<b>,<c>,<d>[!]    h: the entry has a handle, c: it has none; the four ints of its region; `!`: its
//                                          out_masks pointer is NULL
//   Output: `error <message>` when the call is refused, else one line per prompt -- the line tests/matte_plan_cases.cpp prints, in
//   a call with stroke marks in the REWRITTEN call's numbering, with ` stroke <caller's entry>,<label>,<clicks>:<entry>/<entry>...`
//   behind it for every stroke mark of the prompt (the rewritten entries its derived clicks travel in) -- then the `any_` lines of
//   matte_plan_cases and, in a call with stroke marks, `any_stroke 1` and the rewritten call: `rewritten` and per entry
//   ` <h|c><caller's entry>[*]:<a>,<b>,<c>,<d>[!]`, `*` for an entry whose point is derived.
//   stroke_plan_cases fuzz <calls> <seed>     plans that many random entry lists (what the sanitizer build runs) and checks
//       of every served call what the batch calls rely on; prints `ok`
#include "stroke_plan.hpp"

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
    long served = 0, refused = 0, with_strokes = 0;
    for (int c = 0; c < calls; ++c) {
        const int count = 1 + next(9);
        std::vector<char> has_handle(count), has_pointer(count);
        std::vector<int> regions((size_t)count * 4);
        for (int i = 0; i < count; ++i) {
            has_handle[i] = next(3) == 0 || (i == 0 && next(8) != 0);
            has_pointer[i] = next(12) != 0;
            int* r = &regions[(size_t)4 * i];
            if (has_handle[i]) {
                const bool empty = next(2) == 0;
                r[0] = empty ? 0 : next(50); r[1] = next(50); r[2] = empty ? -1 : r[0] + next(50); r[3] = r[1] + next(50);
                continue;
            }
            static const int kinds[] = {0, 1, 4, 6, 7, 8, 10, 11, 12, 12, 12, 12, 5};
            r[0] = kinds[next(13)];
            r[1] = r[2] = r[3] = 0;
            if (r[0] == 6) { r[1] = next(9); r[2] = next(9); }
            if (r[0] == 7) { r[1] = next(3) ? 4 : next(40); r[2] = next(1100); }
            if (r[0] == 8) r[1] = next(20) ? next(100001) : -1;
            if (r[0] == 10) { r[1] = next(3) ? 0 : next(5000); r[2] = next(9); }
            if (r[0] == 11) { r[1] = 1 + next(32); r[2] = next(65026); r[3] = next(2) ? 4 : 1; }
            if (r[0] == 12) { r[1] = next(12) ? next(4) : next(11) - 1; r[2] = next(12) ? next(2) : next(4) - 1; r[3] = next(15) ? 0 : 1; }
        }
        const bool points = next(3) != 0, regs = next(12) != 0, branch = next(8) != 0, device = next(12) == 0;
        try {
            const StrokePlannedPrompts plan = plan_stroke_prompts(has_handle, points, regs ? regions.data() : nullptr, branch, has_pointer, device);
            ++served;
            StagedPrompts const& st = plan.inner.inner.inner.planned.cleaned.staged;
            const size_t n = st.prompts.size();
            if (plan.strokes.size() != n || plan.inner.matte.size() != n || st.stages.size() != n) return 3;
            int heads = 0;
            for (int i = 0; i < count; ++i) heads += has_handle[i] != 0;
            if ((int)n != heads) return 4;
            const int rewritten = plan.any_stroke ? (int)plan.handles.size() : count;
            if (plan.any_stroke) {
                ++with_strokes;
                if (device || !regs) return 5;
                if ((int)plan.entry_of.size() != rewritten || (int)plan.derived.size() != rewritten || (int)plan.pointers.size() != rewritten ||
                    (int)plan.regions.size() != 4 * rewritten)
                    return 6;
                for (int e = 0; e < rewritten; ++e) {
                    if (plan.entry_of[e] < 0 || plan.entry_of[e] >= count || (e && plan.entry_of[e] < plan.entry_of[e - 1])) return 7;
                    if (plan.handles[e] && !has_handle[plan.entry_of[e]]) return 8;
                    if (!plan.handles[e] && plan.regions[(size_t)4 * e] == kStrokeMark) return 9;
                }
            }
            bool any = false;
            for (size_t j = 0; j < n; ++j) {
                PromptSpec const& p = st.prompts[j];
                if (p.head < 0 || p.head >= rewritten || !has_handle[plan.caller_entry(p.head)]) return 10;
                if (p.clicks > kMaxClicks) return 11;
                const int end = j + 1 < n ? st.prompts[j + 1].head : rewritten;
                std::vector<char> is_click(rewritten, 0);
                for (int e : st.stages[j].click_entry) {
                    if (e < p.head || e >= end) return 12;
                    is_click[e] = 1;
                }
                if (!plan.any_stroke && !plan.strokes[j].empty()) return 13;
                int derived = 0;
                for (StrokeSpec const& s : plan.strokes[j]) {
                    any = true;
                    if (has_handle[s.entry] || regions[(size_t)4 * s.entry] != kStrokeMark || !has_pointer[s.entry]) return 14;
                    if (s.clicks < 1 || s.clicks > kMaxClicks || (int)s.click_entry.size() != s.clicks || (s.label != 0 && s.label != 1)) return 15;
                    for (int e : s.click_entry) {
                        // every derived click is a click of the prompt, of the mark's label, and its point is nobody else's
                        if (e < p.head || e >= end || !is_click[e] || !plan.derived[e]) return 16;
                        if (e == p.head ? (points || s.label != 1) : (plan.regions[(size_t)4 * e] != s.label || plan.entry_of[e] != s.entry)) return 17;
                        is_click[e] = 2;
                        ++derived;
                    }
                }
                // and no other click of the prompt is derived
                for (int e = p.head; e < end; ++e)
                    if (plan.any_stroke && plan.derived[e] && is_click[e] == 1 && !(e == p.head && !points)) return 18;
                if (plan.any_stroke && !points && is_click[p.head] != 2 &&
                    !(plan.inner.inner.lasso[j].any() && plan.inner.inner.lasso[j].click() && st.stages[j].click_entry[0] != p.head))
                    return 19;
                if (!plan.strokes[j].empty() && plan.inner.inner.inner.planned.grid[j].any()) return 20;
                (void)derived;
            }
            if (any != plan.any_stroke) return 21;
        } catch (std::invalid_argument const& e) {
            ++refused;
            if (std::strncmp(e.what(), "mask batch", 10) != 0) return 22;
        }
    }
    std::printf("served %ld refused %ld strokes %ld\nok\n", served, refused, with_strokes);
    return served > 0 && refused > 0 && with_strokes > 0 ? 0 : 23;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "fuzz")) return fuzz(std::atoi(argv[2]), (unsigned)std::atoi(argv[3]));
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <stroke|matte> <points given> <regions given> <mask branch> <device form> [<h|c>:<a>,<b>,<c>,<d>[!]]...\n",
                     argv[0]);
        return 2;
    }
    const bool stroke = !std::strcmp(argv[1], "stroke");
    const bool points = std::atoi(argv[2]) != 0, regions_given = std::atoi(argv[3]) != 0, branch = std::atoi(argv[4]) != 0,
               device = std::atoi(argv[5]) != 0;
    std::vector<char> has_handle, has_pointer;
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
        regions.insert(regions.end(), r, r + 4);
    }
    StrokePlannedPrompts plan;
    try {
        if (stroke) {
            plan = plan_stroke_prompts(has_handle, points, regions_given ? regions.data() : nullptr, branch, has_pointer, device);
        } else {
            plan.inner = plan_matte_prompts(has_handle, points, regions_given ? regions.data() : nullptr, branch, has_pointer, device);
            plan.strokes.resize(plan.inner.inner.inner.planned.cleaned.staged.prompts.size());
        }
    } catch (std::exception const& e) {
        std::printf("error %s\n", e.what());
        return 0;
    }
    PriorPlannedPrompts const& in = plan.inner.inner.inner;
    StagedPrompts const& st = in.planned.cleaned.staged;
    if (in.planned.cleaned.clean.size() != st.prompts.size() || in.planned.grid.size() != st.prompts.size() ||
        st.stages.size() != st.prompts.size() || in.prior.size() != st.prompts.size() || plan.inner.inner.lasso.size() != st.prompts.size() ||
        plan.inner.matte.size() != st.prompts.size() || plan.strokes.size() != st.prompts.size())
        return 3;
    for (size_t j = 0; j < st.prompts.size(); ++j) {
        PromptSpec const& p = st.prompts[j];
        std::printf("prompt %d clicks %d box %d points %d entries", p.head, p.clicks, (int)p.box, p.points());
        for (size_t c = 0; c < st.stages[j].click_entry.size(); ++c) std::printf("%c%d", c ? ',' : ' ', st.stages[j].click_entry[c]);
        std::printf(" stages");
        for (size_t k = 0; k < st.stages[j].stage_clicks.size(); ++k) std::printf("%c%d", k ? ',' : ' ', st.stages[j].stage_clicks[k]);
        std::printf(" clean %d,%d grid %d,%d,%d", in.planned.cleaned.clean[j].max_hole, in.planned.cleaned.clean[j].max_island,
                    in.planned.grid[j].side, in.planned.grid[j].iou_permille, in.planned.grid[j].stability_permille);
        if (in.prior[j].any()) std::printf(" prior %d,%d", in.prior[j].entry, in.prior[j].strength_milli);
        LassoSpec const& l = plan.inner.inner.lasso[j];
        if (l.any()) std::printf(" lasso %d,%d,%d", l.entry, l.what, l.strength_milli);
        MatteSpec const& m = plan.inner.matte[j];
        if (m.any()) std::printf(" matte %d,%d,%d,%d", m.entry, m.radius, m.eps, m.channels);
        for (StrokeSpec const& s : plan.strokes[j]) {
            std::printf(" stroke %d,%d,%d:", s.entry, s.label, s.clicks);
            for (size_t c = 0; c < s.click_entry.size(); ++c) std::printf("%s%d", c ? "/" : "", s.click_entry[c]);
        }
        std::printf("\n");
    }
    std::printf("any_clean %d\nany_grid %d\n", (int)in.planned.cleaned.any_clean, (int)in.planned.any_grid);
    if (in.any_prior) std::printf("any_prior 1\n");
    if (plan.inner.inner.any_lasso) std::printf("any_lasso 1\n");
    if (plan.inner.any_matte) std::printf("any_matte 1\n");
    if (plan.any_stroke) {
        std::printf("any_stroke 1\nrewritten");
        for (size_t e = 0; e < plan.handles.size(); ++e)
            std::printf(" %c%d%s:%d,%d,%d,%d%s", plan.handles[e] ? 'h' : 'c', plan.entry_of[e], plan.derived[e] ? "*" : "", plan.regions[4 * e],
                        plan.regions[4 * e + 1], plan.regions[4 * e + 2], plan.regions[4 * e + 3], plan.pointers[e] ? "" : "!");
        std::printf("\n");
    }
    return 0;
}
