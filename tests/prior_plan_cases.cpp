// Prints what csrc/prior_plan.hpp makes of one batch mask call that may hold prior marks, for tests/test_prior_ref.py to compare
// with what the rules say (built there with the host compiler).
//   prior_plan_cases <points given 0|1> <regions given 0|1> <mask branch 0|1> <device form 0|1> [<entry>]...
//       entry: <h|c>:<a>,<b>,<c>,<d>[!]    h: the entry has a handle, c: it has none; the four ints of its region; `!`: its
//                                          out_masks pointer is NULL
// Output: `error <message>` when the call is refused, else one line per prompt -- the line tests/grid_plan_cases.cpp prints,
// with ` prior <entry>,<strength_milli>` behind it for a prompt that has one --
//   prompt <head> clicks <n> box <0|1> points <n> entries <e0>,... stages <k0>,... clean <max_hole>,<max_island> grid <side>,<iou>,<stability>
// then `any_clean <0|1>`, `any_grid <0|1>` and, in a call with prior marks, `any_prior 1`.
#include "prior_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace dlimg;

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <points given> <regions given> <mask branch> <device form> [<h|c>:<a>,<b>,<c>,<d>[!]]...\n", argv[0]);
        return 2;
    }
    const bool points = std::atoi(argv[1]) != 0, regions_given = std::atoi(argv[2]) != 0, branch = std::atoi(argv[3]) != 0,
               device = std::atoi(argv[4]) != 0;
    std::vector<char> has_handle, has_pointer;
    std::vector<int> regions;
    for (int i = 5; i < argc; ++i) {
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
    PriorPlannedPrompts plan;
    try {
        plan = plan_prior_prompts(has_handle, points, regions_given ? regions.data() : nullptr, branch, has_pointer, device);
    } catch (std::exception const& e) {
        std::printf("error %s\n", e.what());
        return 0;
    }
    StagedPrompts const& st = plan.planned.cleaned.staged;
    if (plan.planned.cleaned.clean.size() != st.prompts.size() || plan.planned.grid.size() != st.prompts.size() ||
        st.stages.size() != st.prompts.size() || plan.prior.size() != st.prompts.size())
        return 3;
    for (size_t j = 0; j < st.prompts.size(); ++j) {
        PromptSpec const& p = st.prompts[j];
        std::printf("prompt %d clicks %d box %d points %d entries", p.head, p.clicks, (int)p.box, p.points());
        for (size_t c = 0; c < st.stages[j].click_entry.size(); ++c) std::printf("%c%d", c ? ',' : ' ', st.stages[j].click_entry[c]);
        std::printf(" stages");
        for (size_t k = 0; k < st.stages[j].stage_clicks.size(); ++k) std::printf("%c%d", k ? ',' : ' ', st.stages[j].stage_clicks[k]);
        std::printf(" clean %d,%d grid %d,%d,%d", plan.planned.cleaned.clean[j].max_hole, plan.planned.cleaned.clean[j].max_island,
                    plan.planned.grid[j].side, plan.planned.grid[j].iou_permille, plan.planned.grid[j].stability_permille);
        if (plan.prior[j].any()) std::printf(" prior %d,%d", plan.prior[j].entry, plan.prior[j].strength_milli);
        std::printf("\n");
    }
    std::printf("any_clean %d\nany_grid %d\n", (int)plan.planned.cleaned.any_clean, (int)plan.planned.any_grid);
    if (plan.any_prior) std::printf("any_prior 1\n");
    return 0;
}
