// Prints what csrc/prompt_plan.hpp makes of one batch mask call that may hold clean-up marks (and refinement marks), for
// tests/test_cleanup_oracle.py to compare with what the rules say (built there with the host compiler).
//   clean_plan_cases <points given 0|1> <regions given 0|1> <mask branch 0|1> [<entry>]...
//   entry: <h|c>:<a>,<b>,<c>,<d>      h: the entry has a handle, c: it has none; the four ints of its region
// Output: `error <message>` when the call is refused, else one line per prompt
//   prompt <head> clicks <n> box <0|1> points <n> entries <e0>,... labels <l0>,... stages <k0>,... clean <max_hole>,<max_island>
// then `any_clean <0|1>` and one line per decoder launch of the unstaged prompts (plan_prompt_chunks, 8 prompts per chunk)
//   chunk points <n> prompts <j0>,<j1>,...
#include "prompt_plan.hpp"

#include <cstdio>
#include <cstdlib>

using namespace dlimg;

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <points given> <regions given> <mask branch> [<h|c>:<a>,<b>,<c>,<d>]...\n", argv[0]);
        return 2;
    }
    const bool points = std::atoi(argv[1]) != 0, regions_given = std::atoi(argv[2]) != 0, branch = std::atoi(argv[3]) != 0;
    std::vector<char> has_handle;
    std::vector<int> regions;
    for (int i = 4; i < argc; ++i) {
        int r[4] = {0, 0, 0, 0};
        char kind = 0;
        if (std::sscanf(argv[i], "%c:%d,%d,%d,%d", &kind, &r[0], &r[1], &r[2], &r[3]) != 5 || (kind != 'h' && kind != 'c')) {
            std::fprintf(stderr, "bad entry %s\n", argv[i]);
            return 2;
        }
        has_handle.push_back(kind == 'h');
        regions.insert(regions.end(), r, r + 4);
    }
    int const* reg = regions_given ? regions.data() : nullptr;
    CleanedPrompts plan;
    try {
        plan = plan_cleaned_prompts(has_handle, points, reg, branch);
    } catch (std::exception const& e) {
        std::printf("error %s\n", e.what());
        return 0;
    }
    if (plan.clean.size() != plan.staged.prompts.size()) return 3;
    std::vector<int> plain;
    for (size_t j = 0; j < plan.staged.prompts.size(); ++j) {
        PromptSpec const& p = plan.staged.prompts[j];
        PromptStages const& s = plan.staged.stages[j];
        std::printf("prompt %d clicks %d box %d points %d entries", p.head, p.clicks, (int)p.box, p.points());
        for (size_t c = 0; c < s.click_entry.size(); ++c) std::printf("%c%d", c ? ',' : ' ', s.click_entry[c]);
        std::printf(" labels");
        for (int c = 0; c < p.clicks; ++c) std::printf("%c%d", c ? ',' : ' ', click_label(s, c, reg));
        std::printf(" stages");
        for (size_t k = 0; k < s.stage_clicks.size(); ++k) std::printf("%c%d", k ? ',' : ' ', s.stage_clicks[k]);
        std::printf(" clean %d,%d\n", plan.clean[j].max_hole, plan.clean[j].max_island);
        if (!s.staged()) plain.push_back((int)j);
    }
    std::printf("any_clean %d\n", (int)plan.any_clean);
    for (PromptChunk const& c : plan_prompt_chunks(plan.staged.prompts, plain, 8)) {
        std::printf("chunk points %d prompts", c.points);
        for (size_t k = 0; k < c.prompts.size(); ++k) std::printf("%c%d", k ? ',' : ' ', c.prompts[k]);
        std::printf("\n");
    }
    return 0;
}
