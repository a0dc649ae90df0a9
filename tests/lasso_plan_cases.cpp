// Prints what csrc/lasso_plan.hpp makes of one batch mask call that may hold lasso marks, for tests/test_lasso_ref.py to compare
// with what the rules say (built there with the host compiler).
//   lasso_plan_cases <lasso|prior> <points given 0|1> <regions given 0|1> <mask branch 0|1> <device form 0|1> [<entry>]...
//       lasso: plan_lasso_prompts; prior: plan_prior_prompts on the same call (what a call without lasso marks must equal)
//       entry: <h|c>:<a>,<b>,<c>,<d>[!]    h: the entry has a handle, c: it has none; the four ints of its region; `!`: its
//                                          out_masks pointer is NULL
//   Output: `error <message>` when the call is refused, else one line per prompt -- the line tests/prior_plan_cases.cpp prints,
//   with ` lasso <entry>,<what>,<strength_milli>` behind it for a prompt that has one -- then `any_clean <0|1>`, `any_grid
//   <0|1>`, in a call with prior marks `any_prior 1`, in one with lasso marks `any_lasso 1`.
//   lasso_plan_cases fold <width> <height> <pre_w> <pre_h>      reads 256 x 8 ints (the row records of k::lasso_derive) from
//       standard input and prints `record` and the 8 ints fold_lasso_rows makes of them
//   Behind the line of a lasso prompt, one line `  packed <x>,<y>,<label> ...` per stage: what pack_points packs from
//   lasso_prompt_arrays for an image of 1024 x 1024, with the record {1, box 10 20 30 40, click 15 25, d2 9} and the caller's
//   click of entry e at (100 e, 100 e + 1).
#include "lasso_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace dlimg;

static int fold(int argc, char** argv) {
    if (argc != 6) return 2;
    std::vector<int32_t> rows((size_t)kLassoRows * kLassoRowRecordInts);
    for (int32_t& v : rows)
        if (std::scanf("%d", &v) != 1) return 2;
    int32_t record[kLassoRecordInts];
    fold_lasso_rows(rows.data(), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), record);
    std::printf("record");
    for (int v : record) std::printf(" %d", v);
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "fold")) return fold(argc, argv);
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <lasso|prior> <points given> <regions given> <mask branch> <device form> [<h|c>:<a>,<b>,<c>,<d>[!]]...\n",
                     argv[0]);
        return 2;
    }
    const bool lasso = !std::strcmp(argv[1], "lasso");
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
    LassoPlannedPrompts plan;
    try {
        if (lasso) {
            plan = plan_lasso_prompts(has_handle, points, regions_given ? regions.data() : nullptr, branch, has_pointer, device);
        } else {
            plan.inner = plan_prior_prompts(has_handle, points, regions_given ? regions.data() : nullptr, branch, has_pointer, device);
            plan.lasso.resize(plan.inner.planned.cleaned.staged.prompts.size());
        }
    } catch (std::exception const& e) {
        std::printf("error %s\n", e.what());
        return 0;
    }
    PriorPlannedPrompts const& in = plan.inner;
    StagedPrompts const& st = in.planned.cleaned.staged;
    if (in.planned.cleaned.clean.size() != st.prompts.size() || in.planned.grid.size() != st.prompts.size() ||
        st.stages.size() != st.prompts.size() || in.prior.size() != st.prompts.size() || plan.lasso.size() != st.prompts.size())
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
        if (plan.lasso[j].any()) std::printf(" lasso %d,%d,%d", plan.lasso[j].entry, plan.lasso[j].what, plan.lasso[j].strength_milli);
        std::printf("\n");
        if (plan.lasso[j].any()) {
            // the prompt as pack_points packs it once a record is there: {1, box 10 20 30 40, click 15 25, 9}, at scale 1; the
            // caller's clicks are at (100 e, 100 e + 1) for entry e
            const int32_t record[kLassoRecordInts] = {1, 10, 20, 30, 40, 15, 25, 9};
            std::vector<int> pts(has_handle.size() * 2);
            for (size_t e = 0; e < has_handle.size(); ++e) {
                pts[2 * e] = 100 * (int)e;
                pts[2 * e + 1] = 100 * (int)e + 1;
            }
            const LassoPromptArrays own = lasso_prompt_arrays(p, st.stages[j], plan.lasso[j], points ? pts.data() : nullptr, regions.data(), record);
            ResizeLongestSide rs;
            rs.set(Extent{1024, 1024});
            for (int stage_clicks : own.stages.stage_clicks) {
                float coords[32], labels[16];
                const int n = pack_points(rs, own.spec, own.stages, stage_clicks, own.points.data(), own.regions.data(), coords, labels);
                std::printf("  packed");
                for (int q = 0; q < n; ++q) std::printf(" %d,%d,%d", (int)coords[2 * q], (int)coords[2 * q + 1], (int)labels[q]);
                std::printf("\n");
            }
        }
    }
    std::printf("any_clean %d\nany_grid %d\n", (int)in.planned.cleaned.any_clean, (int)in.planned.any_grid);
    if (in.any_prior) std::printf("any_prior 1\n");
    if (plan.any_lasso) std::printf("any_lasso 1\n");
    return 0;
}
