// Prints what csrc/matte_plan.hpp makes of one batch mask call that may hold matte marks, for tests/test_matte_plan.py to compare
// with what the rules say (built there with the host compiler).
//   matte_plan_cases <matte|lasso> <points given 0|1> <regions given 0|1> <mask branch 0|1> <device form 0|1> [<entry>]...
//       matte: plan_matte_prompts; lasso: plan_lasso_prompts on the same call (what a call without matte marks must equal)
//       entry: <h|c>:<a>,<b>,<c>,<d>[!]    h: the entry has a handle, c: it has none; the four ints of its region; `!`: its
//                                          out_masks pointer is NULL
//   Output: `error <message>` when the call is refused, else one line per prompt -- the line tests/lasso_plan_cases.cpp prints
//   (without its `packed` lines), with ` matte <entry>,<radius>,<eps>,<channels>` behind it for a prompt that has one -- then
//   `any_clean <0|1>`, `any_grid <0|1>`, in a call with prior marks `any_prior 1`, with lasso marks `any_lasso 1`, with matte
//   marks `any_matte 1`.
//   matte_plan_cases fuzz <calls> <seed>      plans that many random entry lists (what the sanitizer build runs) and checks
//       of every served call what the batch calls rely on; prints `ok`
#include "matte_plan.hpp"

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
    long served = 0, refused = 0;
    for (int c = 0; c < calls; ++c) {
        const int count = 1 + next(9);
        std::vector<char> has_handle(count), has_pointer(count);
        std::vector<int> regions((size_t)count * 4);
        for (int i = 0; i < count; ++i) {
            has_handle[i] = next(3) == 0 || (i == 0 && next(8) != 0);
            has_pointer[i] = next(10) != 0;
            int* r = &regions[(size_t)4 * i];
            if (has_handle[i]) {
                const bool empty = next(2) == 0;
                r[0] = empty ? 0 : next(50); r[1] = next(50); r[2] = empty ? -1 : r[0] + next(50); r[3] = r[1] + next(50);
                continue;
            }
            static const int kinds[] = {0, 1, 4, 6, 7, 8, 10, 11, 11, 11, 5};
            r[0] = kinds[next(11)];
            r[1] = r[2] = r[3] = 0;
            if (r[0] == 6) { r[1] = next(9); r[2] = next(9); }
            if (r[0] == 7) { r[1] = next(3) ? 4 : next(40); r[2] = next(1100); }
            if (r[0] == 8) r[1] = next(20) ? next(100001) : -1;
            if (r[0] == 10) { r[1] = next(3) ? 0 : next(5000); r[2] = next(9); }
            if (r[0] == 11) { r[1] = next(12) ? 1 + next(32) : next(40); r[2] = next(12) ? next(65026) : -next(3) + 65026 * next(2); r[3] = next(12) ? (next(2) ? 4 : (next(2) ? 3 : 1)) : next(6); }
        }
        const bool points = next(6) != 0, regs = next(12) != 0, branch = next(8) != 0, device = next(10) == 0;
        try {
            const MattePlannedPrompts plan = plan_matte_prompts(has_handle, points, regs ? regions.data() : nullptr, branch, has_pointer, device);
            ++served;
            StagedPrompts const& st = plan.inner.inner.planned.cleaned.staged;
            const size_t n = st.prompts.size();
            if (plan.matte.size() != n || plan.inner.lasso.size() != n || plan.inner.inner.prior.size() != n || st.stages.size() != n) return 3;
            int heads = 0;
            for (int i = 0; i < count; ++i) heads += has_handle[i] != 0;
            if ((int)n != heads) return 4;
            bool any = false;
            for (size_t j = 0; j < n; ++j) {
                PromptSpec const& p = st.prompts[j];
                if (p.head < 0 || p.head >= count || !has_handle[p.head]) return 5;
                const int end = j + 1 < n ? st.prompts[j + 1].head : count;
                for (int e : st.stages[j].click_entry)
                    if (e < p.head || e >= end) return 6;
                MatteSpec const& m = plan.matte[j];
                if (!m.any()) continue;
                any = true;
                if (device || !regs) return 7;
                if (m.entry != end - 1 || has_handle[m.entry] || regions[(size_t)4 * m.entry] != kMatteMark || !has_pointer[m.entry]) return 8;
                if (m.radius < 1 || m.radius > kMatteMaxRadius || m.eps < 1 || m.eps > kMatteMaxEps) return 9;
                if (m.channels != 1 && m.channels != 3 && m.channels != 4) return 10;
                if (plan.inner.inner.planned.grid[j].any() || (p.clicks == 0 && !p.box)) return 11;
                if (plan.inner.inner.prior[j].any() && regions[(size_t)4 * plan.inner.inner.prior[j].entry] != kPriorMark) return 12;
                if (plan.inner.lasso[j].any() && regions[(size_t)4 * plan.inner.lasso[j].entry] != kLassoMark) return 13;
            }
            if (any != plan.any_matte) return 14;
        } catch (std::invalid_argument const& e) {
            ++refused;
            if (std::strncmp(e.what(), "mask batch", 10) != 0) return 15;
        }
    }
    std::printf("served %ld refused %ld\nok\n", served, refused);
    return served > 0 && refused > 0 ? 0 : 16;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "fuzz")) return fuzz(std::atoi(argv[2]), (unsigned)std::atoi(argv[3]));
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <matte|lasso> <points given> <regions given> <mask branch> <device form> [<h|c>:<a>,<b>,<c>,<d>[!]]...\n",
                     argv[0]);
        return 2;
    }
    const bool matte = !std::strcmp(argv[1], "matte");
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
    MattePlannedPrompts plan;
    try {
        if (matte) {
            plan = plan_matte_prompts(has_handle, points, regions_given ? regions.data() : nullptr, branch, has_pointer, device);
        } else {
            plan.inner = plan_lasso_prompts(has_handle, points, regions_given ? regions.data() : nullptr, branch, has_pointer, device);
            plan.matte.resize(plan.inner.inner.planned.cleaned.staged.prompts.size());
        }
    } catch (std::exception const& e) {
        std::printf("error %s\n", e.what());
        return 0;
    }
    PriorPlannedPrompts const& in = plan.inner.inner;
    StagedPrompts const& st = in.planned.cleaned.staged;
    if (in.planned.cleaned.clean.size() != st.prompts.size() || in.planned.grid.size() != st.prompts.size() ||
        st.stages.size() != st.prompts.size() || in.prior.size() != st.prompts.size() || plan.inner.lasso.size() != st.prompts.size() ||
        plan.matte.size() != st.prompts.size())
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
        LassoSpec const& l = plan.inner.lasso[j];
        if (l.any()) std::printf(" lasso %d,%d,%d", l.entry, l.what, l.strength_milli);
        MatteSpec const& m = plan.matte[j];
        if (m.any()) std::printf(" matte %d,%d,%d,%d", m.entry, m.radius, m.eps, m.channels);
        std::printf("\n");
    }
    std::printf("any_clean %d\nany_grid %d\n", (int)in.planned.cleaned.any_clean, (int)in.planned.any_grid);
    if (in.any_prior) std::printf("any_prior 1\n");
    if (plan.inner.any_lasso) std::printf("any_lasso 1\n");
    if (plan.any_matte) std::printf("any_matte 1\n");
    return 0;
}
