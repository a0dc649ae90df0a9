// "Segment everything" on the host: the grid mark of a batch mask call, the pixels of a point grid, and the selection of the
// segments a label map shows.  Pure host logic (no HIP, no environment), tested without a GPU (tests/grid_plan_cases.cpp,
// tests/test_grid_ref.py, against the numpy restatement tests/grid_ref.py).
//
// Grid marks (plan_grid_prompts).  A continuation entry whose four ints are {kGridMark, side, iou_permille, stability_permille}
// turns its prompt into a grid prompt: exactly two entries, the head (handle, out_masks, an EMPTY region) and the mark.  Neither
// entry's point is read.  The call without its grid prompts is an ordinary call, which plan_cleaned_prompts reads (as a call
// that held continuation entries: an empty head region is "no box"); a call without grid marks is plan_cleaned_prompts.  A grid
// prompt appears in the prompt list as a one-click prompt without a box (what every prompt of its grid is), in head order
// with the others; grid[j].side > 0 marks it.  Every refusal about a grid mark says "mark" and names the caller's entry.
//
// Grid pixels (grid_pixel).  Point (i, j), i, j in 0..side-1, is pixel (floor((2 i + 1) W / (2 side)), floor((2 j + 1) H /
// (2 side))); prompts are row-major, j outer: prompt p = j * side + i.
//
// Selection (select_grid_segments), over one record per candidate (kernels.hpp, k::grid_harvest; candidate c = 3 * prompt +
// plane - 1) and its IoU prediction:
//   filter   n_mid > 0, n_lo > 0, iou >= float(iou_permille) / float(1000) in fp32, n_hi * 1000 >= stability_permille * n_lo
//            in 64-bit integers; a threshold of 0 means SAM's default (880, 950)
//   NMS      the passing candidates by iou descending, ties by c ascending, greedily; a candidate is suppressed by a kept one
//            when inter * 10 > 7 * union in 64-bit integers, with torchvision's box area (x1 - x0) * (y1 - y0) on the inclusive
//            corners (a one-pixel box has area 0); union == 0 never suppresses; at most 255 are kept
//   labels   the kept ones by n_mid descending, ties by NMS order: label k is the k-th, so the smallest segment has the
//            largest label and lies on top
#pragma once

#include "prompt_plan.hpp"

#include <algorithm>
#include <cstdint>

namespace dlimg {

constexpr int kGridMark = 7;           // regions[4 i] of a grid mark
constexpr int kGridMaxSide = 32;
constexpr int kGridMaxSegments = 255;  // labels of a byte
constexpr int kGridDefaultIou = 880, kGridDefaultStability = 950;

struct GridSpec {
    int side = 0, iou_permille = 0, stability_permille = 0;
    bool any() const { return side > 0; }
};
struct GridPlannedPrompts {
    CleanedPrompts cleaned;            // every prompt of the call, the grid prompts as one-click prompts; caller's numbering
    std::vector<GridSpec> grid;        // [prompt]
    bool any_grid = false;
};

inline bool is_grid_mark_entry(int const* regions, int i) { return regions && regions[4 * i] == kGridMark; }

inline Point grid_pixel(int width, int height, int side, int i, int j) {
    return Point{int((int64_t)(2 * i + 1) * width / (2 * side)), int((int64_t)(2 * j + 1) * height / (2 * side))};
}

// had_continuation: as for plan_prompts -- the caller's list held continuation entries that are not in this one (prior marks,
// prior_plan.hpp).
inline GridPlannedPrompts plan_grid_prompts(std::vector<char> const& has_handle, bool points_given, int const* regions, bool mask_branch,
                                            bool had_continuation = false) {
    const int count = (int)has_handle.size();
    GridPlannedPrompts out;
    for (int i = 0; i < count; ++i) out.any_grid |= !has_handle[i] && is_grid_mark_entry(regions, i);
    if (!out.any_grid) {
        out.cleaned = plan_cleaned_prompts(has_handle, points_given, regions, mask_branch, had_continuation);
        out.grid.resize(out.cleaned.staged.prompts.size());
        return out;
    }
    std::vector<char> handles;
    std::vector<int> ints, entry_of;
    std::vector<std::pair<int, GridSpec>> grids;       // (head, what its mark asks for), in head order
    int head = -1;                                     // the nearest entry with a handle so far
    bool head_is_grid = false;
    const std::string alone = "a grid prompt is its head and its mark, no click and no other mark";
    for (int i = 0; i < count; ++i) {
        const std::string at = "mask batch: entry " + std::to_string(i) + ": ";
        if (has_handle[i] || !is_grid_mark_entry(regions, i)) {
            if (has_handle[i]) {
                head = i;
                head_is_grid = false;
            } else if (head_is_grid) {
                throw std::invalid_argument(at + "follows a grid mark: " + alone);
            }
            handles.push_back(has_handle[i]);
            ints.insert(ints.end(), regions + 4 * i, regions + 4 * i + 4);
            entry_of.push_back(i);
            continue;
        }
        const int* r = regions + 4 * i;
        const std::string who = at + "a grid mark ";
        if (r[1] < 1 || r[1] > kGridMaxSide)
            throw std::invalid_argument(who + "is {7, side, iou_permille, stability_permille} in regions[4 i ..]: side is 1.." +
                                        std::to_string(kGridMaxSide));
        if (head < 0) throw std::invalid_argument(who + "needs a prompt in front of it");
        if (head != i - 1) throw std::invalid_argument(who + "does not directly follow its head: " + alone);
        const int* h = regions + 4 * head;
        if (!(h[2] < h[0]))
            throw std::invalid_argument(who + "needs a head with an empty region (x1 < x0): a grid restricted to a box is not served");
        // the head was taken for an ordinary entry one step ago: it is the grid prompt's
        handles.pop_back();
        ints.resize(ints.size() - 4);
        entry_of.pop_back();
        grids.push_back({head, GridSpec{r[1], r[2], r[3]}});
        head_is_grid = true;
    }
    CleanedPrompts rest;
    if (!handles.empty()) {
        try {
            rest = plan_cleaned_prompts(handles, points_given, ints.data(), mask_branch, /*had_continuation*/ true);
        } catch (std::invalid_argument const& e) {
            throw std::invalid_argument(renumber_entry(e.what(), entry_of));
        }
    }
    // plan_cleaned_prompts numbers heads and click entries in the list it was given: back to the caller's through entry_of
    for (size_t j = 0; j < rest.staged.prompts.size(); ++j) {
        rest.staged.prompts[j].head = entry_of[rest.staged.prompts[j].head];
        for (int& e : rest.staged.stages[j].click_entry) e = entry_of[e];
    }
    // merge by head
    size_t a = 0, b = 0;
    out.cleaned.any_clean = rest.any_clean;
    while (a < rest.staged.prompts.size() || b < grids.size()) {
        const bool take_grid = a == rest.staged.prompts.size() || (b < grids.size() && grids[b].first < rest.staged.prompts[a].head);
        if (take_grid) {
            PromptSpec p;
            p.head = grids[b].first;
            p.clicks = 1;
            p.box = false;
            out.cleaned.staged.prompts.push_back(p);
            out.cleaned.staged.stages.push_back(unmarked_stages(p));
            out.cleaned.clean.push_back(CleanSpec{});
            out.grid.push_back(grids[b].second);
            ++b;
        } else {
            out.cleaned.staged.prompts.push_back(rest.staged.prompts[a]);
            out.cleaned.staged.stages.push_back(rest.staged.stages[a]);
            out.cleaned.clean.push_back(rest.clean[a]);
            out.grid.push_back(GridSpec{});
            ++a;
        }
    }
    return out;
}

// One candidate as k::grid_harvest leaves it (8 int32, kernels.hpp).
struct GridRecord {
    int32_t n_hi, n_mid, n_lo, x0, y0, x1, y1;
    uint32_t cull;
};
static_assert(sizeof(GridRecord) == 32, "a record is 32 bytes");

struct GridSelection {
    std::vector<int> nms;          // the candidates NMS keeps, in NMS order
    std::vector<int> kept;         // the same in label order: kept[k - 1] has label k
};

// iou[c]: the IoU prediction of candidate c
inline GridSelection select_grid_segments(GridRecord const* records, float const* iou, int candidates, int iou_permille, int stability_permille) {
    const float iou_threshold = float(iou_permille ? iou_permille : kGridDefaultIou) / float(1000);
    const int64_t stability = stability_permille ? stability_permille : kGridDefaultStability;
    std::vector<int> passing;
    for (int c = 0; c < candidates; ++c) {
        GridRecord const& r = records[c];
        if (r.n_mid > 0 && r.n_lo > 0 && iou[c] >= iou_threshold && (int64_t)r.n_hi * 1000 >= stability * (int64_t)r.n_lo) passing.push_back(c);
    }
    std::stable_sort(passing.begin(), passing.end(), [&](int a, int b) { return iou[a] > iou[b]; });
    GridSelection out;
    auto area = [](GridRecord const& r) { return (int64_t)(r.x1 - r.x0) * (r.y1 - r.y0); };
    for (int c : passing) {
        if ((int)out.nms.size() == kGridMaxSegments) break;
        GridRecord const& r = records[c];
        bool suppressed = false;
        for (int kc : out.nms) {
            GridRecord const& q = records[kc];
            const int64_t w = std::max(0, std::min(r.x1, q.x1) - std::max(r.x0, q.x0));
            const int64_t h = std::max(0, std::min(r.y1, q.y1) - std::max(r.y0, q.y0));
            const int64_t inter = w * h, uni = area(r) + area(q) - inter;
            if (uni != 0 && inter * 10 > 7 * uni) {
                suppressed = true;
                break;
            }
        }
        if (!suppressed) out.nms.push_back(c);
    }
    out.kept = out.nms;
    std::stable_sort(out.kept.begin(), out.kept.end(), [&](int a, int b) { return records[a].n_mid > records[b].n_mid; });
    return out;
}

}  // namespace dlimg
