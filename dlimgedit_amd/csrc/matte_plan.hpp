// Matte marks of a batch mask call (table slot 14): an image-guided soft edge for the mask a prompt delivers.  Pure host logic
// (no HIP, no environment), tested without a GPU (tests/matte_plan_cases.cpp, tests/test_matte_plan.py).
//
// A continuation entry whose four ints are {kMatteMark, radius, eps, channels}, THE LAST ENTRY OF ITS PROMPT (behind the clean-up
// mark when the prompt has one), is a matte mark: neither a click nor a stage.  Its point is not read; its out_masks pointer is
// READ as the guide, the image the head's handle was made from: height * width * channels bytes, tightly packed.  radius: 1 ..
// kMatteMaxRadius pixels of the image; eps: 1 .. kMatteMaxEps squared grey levels, 0 = the default kMatteDefaultEps; channels:
// 1, 3 or 4.  The prompt delivers its one mask as coverage 0 .. 255: the matte (kernels.hpp, k::mask_matte) of the very mask it
// would deliver without the mark.  Everything in front of the mark is read as ever.
//
// plan_matte_prompts is the outermost planner: it takes the marks out, remembers {entry, radius, eps, channels} per prompt and
// hands the rest to plan_lasso_prompts as a call that held continuation entries; a call without matte marks is
// plan_lasso_prompts.  Every refusal about a matte mark says "mark" and names the caller's entry; refusals of the inner planners
// get the caller's entry numbers back.
#pragma once

#include "lasso_plan.hpp"

namespace dlimg {

constexpr int kMatteMark = 11;                 // regions[4 i] of a matte mark (5 and 9 stay refused labels)
constexpr int kMatteMaxRadius = 32;
constexpr int kMatteMaxEps = 65025;
constexpr int kMatteDefaultEps = 650;          // eps == 0: about 0.01 on the unit scale; a choice, not a measurement

struct MatteSpec {
    int entry = -1;                    // the mark's entry (whose out_masks pointer is the guide), caller's numbering; -1: none
    int radius = 0;                    // 1 .. kMatteMaxRadius once planned
    int eps = 0;                       // 1 .. kMatteMaxEps once planned
    int channels = 0;                  // 1, 3 or 4
    bool any() const { return entry >= 0; }
};
struct MattePlannedPrompts {
    LassoPlannedPrompts inner;         // every prompt of the call, caller's numbering
    std::vector<MatteSpec> matte;      // [prompt]
    bool any_matte = false;
};

inline bool is_matte_mark_entry(int const* regions, int i) { return regions && regions[4 * i] == kMatteMark; }

// has_pointer, device_form: as for plan_prior_prompts (the pointer of a matte mark's entry is its guide).
inline MattePlannedPrompts plan_matte_prompts(std::vector<char> const& has_handle, bool points_given, int const* regions, bool mask_branch,
                                              std::vector<char> const& has_pointer, bool device_form = false) {
    const int count = (int)has_handle.size();
    MattePlannedPrompts out;
    for (int i = 0; i < count; ++i) out.any_matte |= !has_handle[i] && is_matte_mark_entry(regions, i);
    if (!out.any_matte) {
        out.inner = plan_lasso_prompts(has_handle, points_given, regions, mask_branch, has_pointer, device_form);
        out.matte.resize(out.inner.inner.planned.cleaned.staged.prompts.size());
        return out;
    }
    std::vector<char> handles, pointers;
    std::vector<int> ints, entry_of;
    std::vector<std::pair<int, MatteSpec>> found;      // (head, its mark), in head order
    int head = -1;                                     // the head of the prompt entry i belongs to, caller's numbering
    for (int i = 0; i < count; ++i) {
        if (has_handle[i]) head = i;
        if (has_handle[i] || !is_matte_mark_entry(regions, i)) {
            handles.push_back(has_handle[i]);
            pointers.push_back(i < (int)has_pointer.size() && has_pointer[i]);
            ints.insert(ints.end(), regions + 4 * i, regions + 4 * i + 4);
            entry_of.push_back(i);
            continue;
        }
        const int* r = regions + 4 * i;
        const std::string who = "mask batch: entry " + std::to_string(i) + ": a matte mark ";
        if (device_form)
            throw std::invalid_argument(who + "is not served by dlimg_amd_get_segmentation_masks_device: the device form has no per-entry "
                                              "pointer to read a guide from");
        if (r[1] < 1 || r[1] > kMatteMaxRadius || r[2] < 0 || r[2] > kMatteMaxEps || (r[3] != 1 && r[3] != 3 && r[3] != 4))
            throw std::invalid_argument(who + "is {11, radius, eps, channels} in regions[4 i ..]: radius is 1 .. " + std::to_string(kMatteMaxRadius) +
                                        ", eps is 0 (the default) .. " + std::to_string(kMatteMaxEps) + ", channels is 1, 3 or 4");
        if (head < 0) throw std::invalid_argument(who + "needs a prompt in front of it");
        if (i + 1 < count && !has_handle[i + 1]) {
            if (is_matte_mark_entry(regions, i + 1))
                throw std::invalid_argument("mask batch: entry " + std::to_string(i + 1) + ": a matte mark is the second one of its prompt: a "
                                            "prompt has one guide at most");
            throw std::invalid_argument(who + "is not the last entry of its prompt: it comes behind the clicks and every other mark");
        }
        if (i >= (int)has_pointer.size() || !has_pointer[i])
            throw std::invalid_argument(who + "has no guide: out_masks[i] of the mark is the image, height * width * channels bytes, and it "
                                              "is NULL");
        found.push_back({head, MatteSpec{i, r[1], r[2] ? r[2] : kMatteDefaultEps, r[3]}});
    }
    try {
        out.inner = plan_lasso_prompts(handles, points_given, ints.data(), mask_branch, pointers, device_form, /*had_continuation*/ true);
    } catch (std::invalid_argument const& e) {
        throw std::invalid_argument(renumber_entry(e.what(), entry_of));
    }
    // the inner planners number entries in the list they were given: back to the caller's through entry_of
    PriorPlannedPrompts& with_priors = out.inner.inner;
    StagedPrompts& staged = with_priors.planned.cleaned.staged;
    out.matte.resize(staged.prompts.size());
    size_t at = 0;
    for (size_t j = 0; j < staged.prompts.size(); ++j) {
        PromptSpec& p = staged.prompts[j];
        p.head = entry_of[p.head];
        for (int& e : staged.stages[j].click_entry) e = entry_of[e];
        if (with_priors.prior[j].any()) with_priors.prior[j].entry = entry_of[with_priors.prior[j].entry];
        if (out.inner.lasso[j].any()) out.inner.lasso[j].entry = entry_of[out.inner.lasso[j].entry];
        if (at == found.size() || found[at].first != p.head) continue;
        out.matte[j] = found[at++].second;
        const std::string who = "mask batch: entry " + std::to_string(out.matte[j].entry) + ": a matte mark ";
        if (with_priors.planned.grid[j].any()) throw std::invalid_argument(who + "on a grid prompt: a label map is not a coverage");
        if (p.clicks == 0 && !p.box)
            throw std::invalid_argument(who + "is no prompt by itself: its prompt still needs a click or a box (an empty region is no box, "
                                              "and there are no `points`)");
    }
    return out;
}

}  // namespace dlimg
