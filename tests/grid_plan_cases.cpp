// Prints what csrc/grid_plan.hpp makes of its inputs, for tests/test_grid_ref.py to compare with tests/grid_ref.py (built
// there with the host compiler; it is also the stand-alone program a sanitizer build of the header runs).
//   grid_plan_cases plan <points given 0|1> <regions given 0|1> <mask branch 0|1> [<entry>]...
//       entry: <h|c>:<a>,<b>,<c>,<d>      h: the entry has a handle, c: it has none; the four ints of its region
//       Output: `error <message>` when the call is refused, else one line per prompt
//         prompt <head> clicks <n> box <0|1> points <n> entries <e0>,... stages <k0>,... clean <max_hole>,<max_island> grid <side>,<iou>,<stability>
//       then `any_clean <0|1>` and `any_grid <0|1>`
//   grid_plan_cases pixels <width> <height> <side>
//       Output: one line `x,y` per grid prompt, in prompt order
//   grid_plan_cases select        (record sets on standard input)
//       `set <n> <iou_permille> <stability_permille>`, then n lines `<n_hi> <n_mid> <n_lo> <x0> <y0> <x1> <y1> <iou bits, hex>`
//       Output per set: `nms <c>,...` and `kept <c>,...` (a lone `nms` / `kept` when nothing is kept)
#include "grid_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace dlimg;

static void print_list(const char* name, std::vector<int> const& v) {
    std::printf("%s", name);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%c%d", i ? ',' : ' ', v[i]);
    std::printf("\n");
}

static int plan(int argc, char** argv) {
    if (argc < 5) return 2;
    const bool points = std::atoi(argv[2]) != 0, regions_given = std::atoi(argv[3]) != 0, branch = std::atoi(argv[4]) != 0;
    std::vector<char> has_handle;
    std::vector<int> regions;
    for (int i = 5; i < argc; ++i) {
        int r[4] = {0, 0, 0, 0};
        char kind = 0;
        if (std::sscanf(argv[i], "%c:%d,%d,%d,%d", &kind, &r[0], &r[1], &r[2], &r[3]) != 5 || (kind != 'h' && kind != 'c')) {
            std::fprintf(stderr, "bad entry %s\n", argv[i]);
            return 2;
        }
        has_handle.push_back(kind == 'h');
        regions.insert(regions.end(), r, r + 4);
    }
    GridPlannedPrompts plan;
    try {
        plan = plan_grid_prompts(has_handle, points, regions_given ? regions.data() : nullptr, branch);
    } catch (std::exception const& e) {
        std::printf("error %s\n", e.what());
        return 0;
    }
    StagedPrompts const& st = plan.cleaned.staged;
    if (plan.cleaned.clean.size() != st.prompts.size() || plan.grid.size() != st.prompts.size() || st.stages.size() != st.prompts.size()) return 3;
    for (size_t j = 0; j < st.prompts.size(); ++j) {
        PromptSpec const& p = st.prompts[j];
        std::printf("prompt %d clicks %d box %d points %d entries", p.head, p.clicks, (int)p.box, p.points());
        for (size_t c = 0; c < st.stages[j].click_entry.size(); ++c) std::printf("%c%d", c ? ',' : ' ', st.stages[j].click_entry[c]);
        std::printf(" stages");
        for (size_t k = 0; k < st.stages[j].stage_clicks.size(); ++k) std::printf("%c%d", k ? ',' : ' ', st.stages[j].stage_clicks[k]);
        std::printf(" clean %d,%d grid %d,%d,%d\n", plan.cleaned.clean[j].max_hole, plan.cleaned.clean[j].max_island, plan.grid[j].side,
                    plan.grid[j].iou_permille, plan.grid[j].stability_permille);
    }
    std::printf("any_clean %d\nany_grid %d\n", (int)plan.cleaned.any_clean, (int)plan.any_grid);
    return 0;
}

static int pixels(int argc, char** argv) {
    if (argc != 5) return 2;
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), side = std::atoi(argv[4]);
    if (w <= 0 || h <= 0 || side <= 0) return 2;
    for (int j = 0; j < side; ++j)
        for (int i = 0; i < side; ++i) {
            const Point p = grid_pixel(w, h, side, i, j);
            std::printf("%d,%d\n", p.x, p.y);
        }
    return 0;
}

static int select() {
    int n = 0, iou_permille = 0, stability_permille = 0;
    while (std::scanf(" set %d %d %d", &n, &iou_permille, &stability_permille) == 3) {
        if (n < 0) return 2;
        std::vector<GridRecord> records(n);
        std::vector<float> iou(n);
        for (int c = 0; c < n; ++c) {
            GridRecord& r = records[c];
            unsigned bits = 0;
            if (std::scanf("%d %d %d %d %d %d %d %x", &r.n_hi, &r.n_mid, &r.n_lo, &r.x0, &r.y0, &r.x1, &r.y1, &bits) != 8) return 2;
            r.cull = 0;
            std::memcpy(&iou[c], &bits, 4);
        }
        const GridSelection s = select_grid_segments(records.data(), iou.data(), n, iou_permille, stability_permille);
        print_list("nms", s.nms);
        print_list("kept", s.kept);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "plan")) return plan(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "pixels")) return pixels(argc, argv);
    if (argc == 2 && !std::strcmp(argv[1], "select")) return select();
    std::fprintf(stderr, "usage: %s plan|pixels|select ...\n", argv[0]);
    return 2;
}
