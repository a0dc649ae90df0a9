// Prints what csrc/prompt_plan.hpp makes of one batch mask call, for tests/test_multi_click_oracle.py to compare with what the
// rules say (built there with the host compiler: the planner needs no HIP and no GPU).
//   prompt_plan_cases <points given 0|1> <regions given 0|1> <chunk> [<entry>]...
//   entry: <h|c><replica>:<x0>,<y0>,<x1>,<y1>[@<x>,<y>[@<width>x<height>]]
//          h: the entry has a handle, c: it has none; the four ints of its region; its point; the extent of its handle's image
// Output: `error <message>` when the call is refused, else one line per prompt
//   prompt <head> clicks <n> box <0|1> points <n> labels <l0>,<l1>,...
// and, per replica in ascending order, one line per decoder chunk
//   chunk <replica> points <n> prompts <j0>,<j1>,...
// and, when an entry names its point, one line per prompt with what pack_points makes of it in its image's frame
//   packed <head> coords <x0>,<y0>;<x1>,<y1>;... labels <l0>,<l1>,...
#include "prompt_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

using namespace dlimg;

static void print_packed(int head, int n, float const* coords, float const* labels) {
    std::printf("packed %d coords", head);
    for (int k = 0; k < n; ++k) std::printf("%c%.9g,%.9g", k ? ';' : ' ', coords[2 * k], coords[2 * k + 1]);
    std::printf(" labels");
    for (int k = 0; k < n; ++k) std::printf("%c%.9g", k ? ',' : ' ', labels[k]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <points given> <regions given> <chunk> [<h|c><replica>:<x0>,<y0>,<x1>,<y1>]...\n", argv[0]);
        return 2;
    }
    const bool points = std::atoi(argv[1]) != 0, regions_given = std::atoi(argv[2]) != 0;
    const int chunk = std::atoi(argv[3]);
    std::vector<char> has_handle;
    std::vector<int> replica, regions, xy;
    std::vector<Extent> extent;
    bool pack = false;
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
        for (int c = 0; c < p.clicks; ++c)
            std::printf("%c%d", c ? ',' : ' ', click_label(unmarked_stages(p), c, regions_given ? regions.data() : nullptr));
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
    for (PromptSpec const& p : prompts) {
        if (!pack) break;
        ResizeLongestSide rs;
        rs.set(extent[p.head]);
        // exactly points() entries: a write past the end is a write past the allocation
        std::vector<float> coords(2 * p.points()), labels(p.points());
        const int n = pack_points(rs, p, unmarked_stages(p), p.clicks, points ? xy.data() : nullptr, regions_given ? regions.data() : nullptr,
                                  coords.data(), labels.data());
        if (n != p.points()) return 3;
        print_packed(p.head, n, coords.data(), labels.data());
    }
    return 0;
}
