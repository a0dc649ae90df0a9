// Edge marks of a batch mask call (table slot 14): grow, shrink, feather and border the mask a prompt delivers (kernels.hpp,
// k::mask_edge).  Pure host logic (no HIP, no environment), tested without a GPU (tests/edge_plan_cases.cpp,
// tests/test_edge_plan.py).
//
// A continuation entry whose four ints are {kEdgeMark, offset, feather, border} is an edge mark: neither a click nor a stage.
// Its point and its out_masks pointer are not read, and it does not count towards a prompt's clicks.  offset: -kEdgeMaxOffset ..
// kEdgeMaxOffset pixels, positive grows; feather: 0 .. kEdgeMaxFeather; border: 0 .. kEdgeMaxBorder; not all three 0.  A prompt
// has one at most.  It stands behind every click, stroke mark and refinement mark of its prompt and behind the clean-up mark when
// there is one; in front of the matte mark, and with that mark its cut-out mark, when there is one; otherwise it is the last
// entry of its prompt.  The stages run in that order: clean-up, edge, matte, cut-out.
//
// plan_edge_prompts is the outermost planner: it takes the marks out, remembers {entry, offset, feather, border} per prompt and
// hands the rest to plan_cutout_prompts, so to the planners under it the clean-up mark or the last click stands directly in front
// of the matte mark as ever; a call without edge marks is plan_cutout_prompts.  Every refusal about an edge mark says "mark" and
// names the caller's entry; refusals of the inner planners get the caller's entry numbers back, and so does what the plan says
// of the caller's entries.  The mark needs no pointer, so the device form serves it, as it serves clean-up marks.
#pragma once

#include "cutout_plan.hpp"

namespace dlimg {

constexpr int kEdgeMark = 14;                  // regions[4 i] of an edge mark
constexpr int kEdgeMaxOffset = 64;
constexpr int kEdgeMaxFeather = 32;
constexpr int kEdgeMaxBorder = 32;

struct EdgeSpec {
    int entry = -1;                    // the mark's entry, caller's numbering; -1: none
    int offset = 0, feather = 0, border = 0;
    bool any() const { return entry >= 0; }
};
struct EdgePlannedPrompts {
    CutoutPlannedPrompts inner;        // every prompt of the call, as plan_cutout_prompts numbers it (caller's entries behind it)
    std::vector<EdgeSpec> edge;        // [prompt]
    bool any_edge = false;
};

inline bool is_edge_mark_entry(int const* regions, int i) { return regions && regions[4 * i] == kEdgeMark; }

// has_pointer, device_form, same_as_head: as for plan_cutout_prompts (an edge mark's own pointer is not looked at).
inline EdgePlannedPrompts plan_edge_prompts(std::vector<char> const& has_handle, bool points_given, int const* regions, bool mask_branch,
                                            std::vector<char> const& has_pointer, bool device_form = false,
                                            std::vector<char> const& same_as_head = {}) {
    const int count = (int)has_handle.size();
    EdgePlannedPrompts out;
    for (int i = 0; i < count; ++i) out.any_edge |= !has_handle[i] && is_edge_mark_entry(regions, i);
    if (!out.any_edge) {
        out.inner = plan_cutout_prompts(has_handle, points_given, regions, mask_branch, has_pointer, device_form, same_as_head);
        out.edge.resize(out.inner.cutout.size());
        return out;
    }
    std::vector<char> handles, pointers, same;
    std::vector<int> ints, entry_of;
    std::vector<std::pair<int, EdgeSpec>> found;       // (head, its mark), in head order
    int head = -1;                                     // the head of the prompt entry i belongs to, caller's numbering
    bool edge_seen = false, matte_seen = false;        // of that prompt, in front of entry i
    for (int i = 0; i < count; ++i) {
        if (has_handle[i]) {
            head = i;
            edge_seen = matte_seen = false;
        }
        if (has_handle[i] || !is_edge_mark_entry(regions, i)) {
            if (!has_handle[i]) matte_seen |= is_matte_mark_entry(regions, i) || is_cutout_mark_entry(regions, i);
            handles.push_back(has_handle[i]);
            pointers.push_back(i < (int)has_pointer.size() && has_pointer[i]);
            same.push_back(i < (int)same_as_head.size() && same_as_head[i]);
            ints.insert(ints.end(), regions + 4 * i, regions + 4 * i + 4);
            entry_of.push_back(i);
            continue;
        }
        const int* r = regions + 4 * i;
        const std::string who = "mask batch: entry " + std::to_string(i) + ": an edge mark ";
        if (r[1] < -kEdgeMaxOffset || r[1] > kEdgeMaxOffset || r[2] < 0 || r[2] > kEdgeMaxFeather || r[3] < 0 || r[3] > kEdgeMaxBorder)
            throw std::invalid_argument(who + "is {14, offset, feather, border} in regions[4 i ..]: offset is -" + std::to_string(kEdgeMaxOffset) +
                                        " .. " + std::to_string(kEdgeMaxOffset) + ", feather is 0 .. " + std::to_string(kEdgeMaxFeather) +
                                        ", border is 0 .. " + std::to_string(kEdgeMaxBorder));
        if (r[1] == 0 && r[2] == 0 && r[3] == 0)
            throw std::invalid_argument(who + "with offset, feather and border all 0 is the identity: leave the mark out");
        if (head < 0) throw std::invalid_argument(who + "needs a prompt in front of it");
        if (edge_seen) throw std::invalid_argument(who + "is the second one of its prompt: a prompt has one edge mark at most");
        if (matte_seen)
            throw std::invalid_argument(who + "stands behind a matte mark: the matte filters what the edge mark delivers, so the edge mark "
                                              "comes in front of it");
        for (int e = i + 1; e < count && !has_handle[e]; ++e) {
            if (is_edge_mark_entry(regions, e))
                throw std::invalid_argument("mask batch: entry " + std::to_string(e) + ": an edge mark is the second one of its prompt: a "
                                            "prompt has one edge mark at most");
            if (is_matte_mark_entry(regions, e) || is_cutout_mark_entry(regions, e)) continue;
            throw std::invalid_argument(who + "stands in front of entry " + std::to_string(e) + ", which is neither a matte nor a cut-out "
                                              "mark: it comes behind every click, stroke mark and refinement mark and behind the clean-up "
                                              "mark of its prompt");
        }
        edge_seen = true;
        found.push_back({head, EdgeSpec{i, r[1], r[2], r[3]}});
    }
    try {
        out.inner = plan_cutout_prompts(handles, points_given, ints.data(), mask_branch, pointers, device_form, same);
    } catch (std::invalid_argument const& e) {
        throw std::invalid_argument(renumber_entry(e.what(), entry_of));
    }
    CutoutPlannedPrompts& with_cutouts = out.inner;
    StrokePlannedPrompts& with_strokes = with_cutouts.inner;
    MattePlannedPrompts& with_mattes = with_strokes.inner;
    PriorPlannedPrompts& with_priors = with_mattes.inner.inner;
    StagedPrompts& staged = with_priors.planned.cleaned.staged;
    // the caller's call held continuation entries, so an empty region is "no box" -- which the inner planners cannot know when
    // the call without its edge marks holds none: then they are plan_prompts alone, and this is the one thing to put right
    // (as in plan_stroke_prompts)
    bool continuation_left = false;
    for (char h : handles) continuation_left |= !h;
    if (!continuation_left)
        for (PromptSpec& p : staged.prompts)
            if (ints[4 * p.head + 2] < ints[4 * p.head]) p.box = false;
    // the inner planners number the caller's entries in the list they were given: back to the caller's through entry_of.  With
    // stroke marks the plan speaks of the rewritten call, and only what points from there to the caller is touched.
    for (int& e : with_strokes.entry_of) e = entry_of[e];
    for (std::vector<StrokeSpec>& marks : with_strokes.strokes)
        for (StrokeSpec& s : marks) s.entry = entry_of[s.entry];
    out.edge.resize(staged.prompts.size());
    size_t at = 0;
    for (size_t j = 0; j < staged.prompts.size(); ++j) {
        PromptSpec& p = staged.prompts[j];
        if (with_cutouts.cutout[j].any()) with_cutouts.cutout[j].entry = entry_of[with_cutouts.cutout[j].entry];
        if (!with_strokes.any_stroke) {
            p.head = entry_of[p.head];
            for (int& e : staged.stages[j].click_entry) e = entry_of[e];
            if (with_priors.prior[j].any()) with_priors.prior[j].entry = entry_of[with_priors.prior[j].entry];
            if (with_mattes.inner.lasso[j].any()) with_mattes.inner.lasso[j].entry = entry_of[with_mattes.inner.lasso[j].entry];
            if (with_mattes.matte[j].any()) with_mattes.matte[j].entry = entry_of[with_mattes.matte[j].entry];
        }
        if (at == found.size() || found[at].first != with_strokes.caller_entry(p.head)) continue;
        out.edge[j] = found[at++].second;
        if (with_priors.planned.grid[j].any())
            throw std::invalid_argument("mask batch: entry " + std::to_string(out.edge[j].entry) + ": an edge mark on a grid prompt: a label "
                                        "map has no edge to move");
        if (p.clicks == 0 && !p.box)
            throw std::invalid_argument("mask batch: entry " + std::to_string(out.edge[j].entry) + ": an edge mark is no prompt by itself: its "
                                        "prompt still needs a click or a box (an empty region is no box, and there are no `points`)");
    }
    return out;
}

}  // namespace dlimg
