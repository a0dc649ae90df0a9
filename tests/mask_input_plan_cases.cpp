// Prints what csrc/prompt_plan.hpp makes of one batch mask call that may hold refinement marks, for
// tests/test_mask_input_oracle.py to compare with what the rules say (built there with the host compiler).
//   mask_input_plan_cases <points given 0|1> <regions given 0|1> <mask branch 0|1> [<entry>]...
//   entry: <h|c>:<a>,<b>,<c>,<d>[@<x>,<y>[@<width>x<height>]]
//          h: the entry has a handle, c: it has none; the four ints of its region; its point; the extent of its handle's image
// Output: `error <message>` when the call is refused, else one line per prompt
//   prompt <head> clicks <n> box <0|1> points <n> entries <e0>,<e1>,... labels <l0>,<l1>,... stages <k0>,<k1>,...
// and, when an entry names its point, one line per stage of every prompt with what pack_points makes of it
//   packed <head> stage <clicks> coords <x0>,<y0>;<x1>,<y1>;... labels <l0>,<l1>,...
#include "prompt_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace dlimg;

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <points given> <regions given> <mask branch> [<h|c>:<a>,<b>,<c>,<d>]...\n", argv[0]);
        return 2;
    }
    const bool points = std::atoi(argv[1]) != 0, regions_given = std::atoi(argv[2]) != 0, branch = std::atoi(argv[3]) != 0;
    std::vector<char> has_handle;
    std::vector<int> regions, xy;
    std::vector<Extent> extent;
    bool pack = false;
    for (int i = 4; i < argc; ++i) {
        int r[4] = {0, 0, 0, 0};
        char kind = 0;
        if (std::sscanf(argv[i], "%c:%d,%d,%d,%d", &kind, &r[0], &r[1], &r[2], &r[3]) != 5 || (kind != 'h' && kind != 'c')) {
            std::fprintf(stderr, "bad entry %s\n", argv[i]);
            return 2;
        }
        has_handle.push_back(kind == 'h');
        regions.insert(regions.end(), r, r + 4);
        int at[2] = {0, 0};
        Extent e{1024, 1024};
        if (const char* point = std::strchr(argv[i], '@')) {
            pack = true;
            const char* image = std::strchr(point + 1, '@');
            if (std::sscanf(point, "@%d,%d", &at[0], &at[1]) != 2 || (image && std::sscanf(image, "@%dx%d", &e.width, &e.height) != 2)) {
                std::fprintf(stderr, "bad entry %s\n", argv[i]);
                return 2;
            }
        }
        xy.insert(xy.end(), at, at + 2);
        extent.push_back(e);
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
        for (int c = 0; c < p.clicks; ++c) std::printf("%c%d", c ? ',' : ' ', click_label(s, c, reg));
        std::printf(" stages");
        for (size_t k = 0; k < s.stage_clicks.size(); ++k) std::printf("%c%d", k ? ',' : ' ', s.stage_clicks[k]);
        std::printf(" staged %d\n", (int)s.staged());
    }
    for (size_t j = 0; pack && j < plan.prompts.size(); ++j) {
        PromptSpec const& p = plan.prompts[j];
        ResizeLongestSide rs;
        rs.set(extent[p.head]);
        for (int clicks : plan.stages[j].stage_clicks) {
            // exactly the stage's points: a write past the end is a write past the allocation
            const int want = clicks + (p.box ? 2 : 1);
            std::vector<float> coords(2 * want), labels(want);
            const int n = pack_points(rs, p, plan.stages[j], clicks, points ? xy.data() : nullptr, reg, coords.data(), labels.data());
            if (n != want) return 3;
            std::printf("packed %d stage %d coords", p.head, clicks);
            for (int k = 0; k < n; ++k) std::printf("%c%.9g,%.9g", k ? ';' : ' ', coords[2 * k], coords[2 * k + 1]);
            std::printf(" labels");
            for (int k = 0; k < n; ++k) std::printf("%c%.9g", k ? ',' : ' ', labels[k]);
            std::printf("\n");
        }
    }
    return 0;
}
