// Prints what csrc/prompt_plan.hpp makes of one batch mask call that may hold refinement marks, for
// tests/test_mask_input_oracle.py to compare with what the rules say (built there with the host compiler).
//   mask_input_plan_cases <points given 0|1> <regions given 0|1> <mask branch 0|1> [<entry>]...
//   entry: <h|c>:<a>,<b>,<c>,<d>     h: the entry has a handle, c: it has none; the four ints of its region
// Output: `error <message>` when the call is refused, else one line per prompt
//   prompt <head> clicks <n> box <0|1> points <n> entries <e0>,<e1>,... labels <l0>,<l1>,... stages <k0>,<k1>,...
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
    StagedPrompts plan;
    try {
        plan = plan_staged_prompts(has_handle, points, reg, branch);
    } catch (std::exception const& e) {
        std::printf("error %s\n", e.what());
        return 0;
    }
    for (size_t j = 0; j < plan.prompts.size(); ++j) {
        PromptSpec const& p = plan.prompts[j];
        PromptStages const& s = plan.stages[j];
        std::printf("prompt %d clicks %d box %d points %d entries", p.head, p.clicks, (int)p.box, p.points());
        for (size_t c = 0; c < s.click_entry.size(); ++c) std::printf("%c%d", c ? ',' : ' ', s.click_entry[c]);
        std::printf(" labels");
        for (int c = 0; c < p.clicks; ++c) std::printf("%c%d", c ? ',' : ' ', staged_click_label(s, c, reg));
        std::printf(" stages");
        for (size_t k = 0; k < s.stage_clicks.size(); ++k) std::printf("%c%d", k ? ',' : ' ', s.stage_clicks[k]);
        std::printf(" staged %d\n", (int)s.staged());
    }
    return 0;
}
