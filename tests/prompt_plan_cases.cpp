// Prints what csrc/prompt_plan.hpp makes of one batch mask call, for tests/test_multi_click_oracle.py to compare with what the
// rules say (built there with the host compiler: the planner needs no HIP and no GPU).
//   prompt_plan_cases <points given 0|1> <regions given 0|1> <chunk> [<entry>]...
//   entry: <h|c><replica>:<x0>,<y0>,<x1>,<y1>     h: the entry has a handle, c: it has none; the four ints of its region
// Output: `error <message>` when the call is refused, else one line per prompt
//   prompt <head> clicks <n> box <0|1> points <n> labels <l0>,<l1>,...
// and, per replica in ascending order, one line per decoder chunk
//   chunk <replica> points <n> prompts <j0>,<j1>,...
#include "prompt_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>

using namespace dlimg;

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <points given> <regions given> <chunk> [<h|c><replica>:<x0>,<y0>,<x1>,<y1>]...\n", argv[0]);
        return 2;
    }
    const bool points = std::atoi(argv[1]) != 0, regions_given = std::atoi(argv[2]) != 0;
    const int chunk = std::atoi(argv[3]);
    std::vector<char> has_handle;
    std::vector<int> replica, regions;
    for (int i = 4; i < argc; ++i) {
        int rep = 0, r[4] = {0, 0, 0, 0};
        char kind = 0;
        if (std::sscanf(argv[i], "%c%d:%d,%d,%d,%d", &kind, &rep, &r[0], &r[1], &r[2], &r[3]) != 6 || (kind != 'h' && kind != 'c')) {
            std::fprintf(stderr, "bad entry %s\n", argv[i]);
            return 2;
        }
        has_handle.push_back(kind == 'h');
        replica.push_back(rep);
        regions.insert(regions.end(), r, r + 4);
    }
    std::vector<PromptSpec> prompts;
    try {
        prompts = plan_prompts(has_handle, points, regions_given ? regions.data() : nullptr);
    } catch (std::exception const& e) {
        std::printf("error %s\n", e.what());
        return 0;
    }
    std::set<int> replicas;
    for (PromptSpec const& p : prompts) {
        std::printf("prompt %d clicks %d box %d points %d labels", p.head, p.clicks, (int)p.box, p.points());
        for (int c = 0; c < p.clicks; ++c) std::printf("%c%d", c ? ',' : ' ', click_label(p, c, regions_given ? regions.data() : nullptr));
        std::printf("\n");
        replicas.insert(replica[p.head]);
    }
    for (int rep : replicas) {
        std::vector<int> mine;
        for (int j = 0; j < (int)prompts.size(); ++j)
            if (replica[prompts[j].head] == rep) mine.push_back(j);
        for (PromptChunk const& c : plan_prompt_chunks(prompts, mine, chunk)) {
            std::printf("chunk %d points %d prompts", rep, c.points);
            for (size_t k = 0; k < c.prompts.size(); ++k) std::printf("%c%d", k ? ',' : ' ', c.prompts[k]);
            std::printf("\n");
        }
    }
    return 0;
}
