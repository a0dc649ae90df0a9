// Cut-out marks of a batch mask call (table slot 14): a matte's foreground colours as RGBA (kernels.hpp, k::mask_cutout).  Pure
// host logic (no HIP, no environment), tested without a GPU (tests/cutout_plan_cases.cpp, tests/test_cutout_plan.py).
//
// A continuation entry whose four ints are {kCutoutMark, radius, 0, 0}, DIRECTLY BEHIND THE MATTE MARK OF ITS PROMPT and then the
// last entry of the prompt, is a cut-out mark: neither a click nor a stage.  Its point is not read; its out_masks pointer is
// WRITTEN: height * width * 4 bytes, tightly packed, the estimated foreground colour in the order of the guide's first three
// channels and the coverage the prompt delivers as the fourth.  The image is the matte mark's guide, so that mark's channels is
// 3 or 4.  radius: 1 .. kCutoutMaxRadius pixels, 0 = the default kCutoutDefaultRadius.  The pointer may be the guide itself when
// that has 4 channels (the guide is taken before anything is delivered); it is never the head's, which receives the coverage.
//
// plan_cutout_prompts is the outermost planner: it takes the marks out, remembers {entry, radius} per prompt and hands the rest
// to plan_stroke_prompts, so to the matte planner the matte mark is the last entry of its prompt as ever; a call without
// cut-out marks is plan_stroke_prompts.  Every refusal about a cut-out mark says "mark" and names the caller's entry; refusals of
// the inner planners get the caller's entry numbers back, and so does what the plan says of the caller's entries.
#pragma once

#include "stroke_plan.hpp"

namespace dlimg {

constexpr int kCutoutMark = 13;                // regions[4 i] of a cut-out mark (5 and 9 stay refused labels)
constexpr int kCutoutMaxRadius = 32;
constexpr int kCutoutDefaultRadius = 16;       // radius == 0: a choice, not a measurement

struct CutoutSpec {
    int entry = -1;                    // the mark's entry (whose out_masks pointer receives the RGBA), caller's numbering; -1: none
    int radius = 0;                    // 1 .. kCutoutMaxRadius once planned
    bool any() const { return entry >= 0; }
};
struct CutoutPlannedPrompts {
    StrokePlannedPrompts inner;        // every prompt of the call, as plan_stroke_prompts numbers it (caller's entries behind it)
    std::vector<CutoutSpec> cutout;    // [prompt]
    bool any_cutout = false;
};

inline bool is_cutout_mark_entry(int const* regions, int i) { return regions && regions[4 * i] == kCutoutMark; }

// has_pointer, device_form: as for plan_prior_prompts (the pointer of a cut-out mark's entry is its destination).
// same_as_head [entry] (may be shorter: 0): the entry's pointer is the very pointer of its prompt's head.
inline CutoutPlannedPrompts plan_cutout_prompts(std::vector<char> const& has_handle, bool points_given, int const* regions, bool mask_branch,
                                                std::vector<char> const& has_pointer, bool device_form = false,
                                                std::vector<char> const& same_as_head = {}) {
    const int count = (int)has_handle.size();
    CutoutPlannedPrompts out;
    for (int i = 0; i < count; ++i) out.any_cutout |= !has_handle[i] && is_cutout_mark_entry(regions, i);
    if (!out.any_cutout) {
        out.inner = plan_stroke_prompts(has_handle, points_given, regions, mask_branch, has_pointer, device_form);
        out.cutout.resize(out.inner.strokes.size());
        return out;
    }
    std::vector<char> handles, pointers;
    std::vector<int> ints, entry_of;
    std::vector<std::pair<int, CutoutSpec>> found;     // (head, its mark), in head order
    int head = -1;                                     // the head of the prompt entry i belongs to, caller's numbering
    for (int i = 0; i < count; ++i) {
        if (has_handle[i]) head = i;
        if (has_handle[i] || !is_cutout_mark_entry(regions, i)) {
            handles.push_back(has_handle[i]);
            pointers.push_back(i < (int)has_pointer.size() && has_pointer[i]);
            ints.insert(ints.end(), regions + 4 * i, regions + 4 * i + 4);
            entry_of.push_back(i);
            continue;
        }
        const int* r = regions + 4 * i;
        const std::string who = "mask batch: entry " + std::to_string(i) + ": a cut-out mark ";
        if (device_form)
            throw std::invalid_argument(who + "is not served by dlimg_amd_get_segmentation_masks_device: the device form has no per-entry "
                                              "pointer to write the RGBA to");
        if (r[1] < 0 || r[1] > kCutoutMaxRadius || r[2] != 0 || r[3] != 0)
            throw std::invalid_argument(who + "is {13, radius, 0, 0} in regions[4 i ..]: radius is 0 (the default, " +
                                        std::to_string(kCutoutDefaultRadius) + ") .. " + std::to_string(kCutoutMaxRadius) +
                                        ", the third and fourth int are 0");
        if (head < 0) throw std::invalid_argument(who + "needs a prompt in front of it");
        if (is_cutout_mark_entry(regions, i - 1) && !has_handle[i - 1])
            throw std::invalid_argument(who + "is the second one of its prompt: a prompt has one cut-out at most");
        if (has_handle[i - 1] || !is_matte_mark_entry(regions, i - 1))
            throw std::invalid_argument(who + "does not stand directly behind a matte mark: it cuts out what that mark's coverage covers, "
                                              "from that mark's guide");
        if (i + 1 < count && !has_handle[i + 1] && !is_cutout_mark_entry(regions, i + 1))
            throw std::invalid_argument(who + "is not the last entry of its prompt: it comes behind the matte mark, and nothing behind it");
        if (regions[4 * (i - 1) + 3] == 1)
            throw std::invalid_argument(who + "stands behind the matte mark of entry " + std::to_string(i - 1) + " whose guide has one channel: "
                                              "the colours are the guide's, so channels is 3 or 4");
        if (i >= (int)has_pointer.size() || !has_pointer[i])
            throw std::invalid_argument(who + "has no destination: out_masks[i] of the mark receives height * width * 4 bytes, and it is NULL");
        if (i < (int)same_as_head.size() && same_as_head[i])
            throw std::invalid_argument(who + "has the pointer of its prompt's head, entry " + std::to_string(head) + ": that one receives the "
                                              "coverage, height * width bytes");
        found.push_back({head, CutoutSpec{i, r[1] ? r[1] : kCutoutDefaultRadius}});
    }
    try {
        out.inner = plan_stroke_prompts(handles, points_given, ints.data(), mask_branch, pointers, device_form);
    } catch (std::invalid_argument const& e) {
        throw std::invalid_argument(renumber_entry(e.what(), entry_of));
    }
    // the inner planners number the caller's entries in the list they were given: back to the caller's through entry_of.  With
    // stroke marks the plan speaks of the rewritten call, and only what points from there to the caller is touched.
    StrokePlannedPrompts& with_strokes = out.inner;
    MattePlannedPrompts& with_mattes = with_strokes.inner;
    PriorPlannedPrompts& with_priors = with_mattes.inner.inner;
    StagedPrompts& staged = with_priors.planned.cleaned.staged;
    for (int& e : with_strokes.entry_of) e = entry_of[e];
    for (std::vector<StrokeSpec>& marks : with_strokes.strokes)
        for (StrokeSpec& s : marks) s.entry = entry_of[s.entry];
    out.cutout.resize(staged.prompts.size());
    size_t at = 0;
    for (size_t j = 0; j < staged.prompts.size(); ++j) {
        PromptSpec& p = staged.prompts[j];
        if (!with_strokes.any_stroke) {
            p.head = entry_of[p.head];
            for (int& e : staged.stages[j].click_entry) e = entry_of[e];
            if (with_priors.prior[j].any()) with_priors.prior[j].entry = entry_of[with_priors.prior[j].entry];
            if (with_mattes.inner.lasso[j].any()) with_mattes.inner.lasso[j].entry = entry_of[with_mattes.inner.lasso[j].entry];
            if (with_mattes.matte[j].any()) with_mattes.matte[j].entry = entry_of[with_mattes.matte[j].entry];
        }
        if (at == found.size() || found[at].first != with_strokes.caller_entry(p.head)) continue;
        out.cutout[j] = found[at++].second;
        // (directly behind a matte mark, which the matte planner has taken: the prompt has a matte, and is no grid prompt)
    }
    return out;
}

}  // namespace dlimg
