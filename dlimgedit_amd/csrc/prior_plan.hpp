// Prior marks of a batch mask call (table slot 14): a caller's own mask as the mask input of a prompt.  Pure host logic (no HIP,
// no environment), tested without a GPU (tests/prior_plan_cases.cpp, tests/test_prior_ref.py, tests/sanitize/prior_plan_fuzz.cpp).
//
// A continuation entry whose four ints are {kPriorMark, strength_milli, 0, 0} DIRECTLY BEHIND ITS HEAD is a prior mark: neither
// a click nor a stage.  Its point is not read; its out_masks pointer is READ as the prior, width * height bytes of the head's
// image, values 0 .. 255 taken as coverage (kernels.hpp, k::mask_prior).  strength_milli: 1 .. kPriorMaxStrength, 0 = the
// default kPriorDefaultStrength.  The prior is the mask input of the prompt's FIRST stage (where a prompt without one has
// none); refinement marks, a clean-up mark and the prompt's clicks and box are read as ever.  The prompt still needs a click
// or a box.
//
// plan_prior_prompts takes the marks out, remembers {entry, strength} per prompt and hands the rest to plan_grid_prompts as a
// call that held continuation entries (an empty head region is "no box"); a call without prior marks is plan_grid_prompts.
// Every refusal about a prior mark says "mark" and names the caller's entry.
#pragma once

#include "grid_plan.hpp"

namespace dlimg {

constexpr int kPriorMark = 8;                  // regions[4 i] of a prior mark
constexpr int kPriorDefaultStrength = 8000;    // strength_milli == 0: a choice, not a measurement (no real checkpoint was at hand)
constexpr int kPriorMaxStrength = 100000;

struct PriorSpec {
    int entry = -1;                    // the mark's entry (whose out_masks pointer is the prior), caller's numbering; -1: none
    int strength_milli = 0;            // 1 .. kPriorMaxStrength once planned
    bool any() const { return entry >= 0; }
};
struct PriorPlannedPrompts {
    GridPlannedPrompts planned;        // every prompt of the call, caller's numbering
    std::vector<PriorSpec> prior;      // [prompt]
    bool any_prior = false;
};

inline bool is_prior_mark_entry(int const* regions, int i) { return regions && regions[4 * i] == kPriorMark; }

// has_pointer[i]: out_masks[i] of entry i is not NULL (read for prior marks only).  device_form: the call is
// dlimg_amd_get_segmentation_masks_device, which has no per-entry pointer a prior could be read from.  had_continuation: as
// for plan_prompts -- the caller's list held continuation entries that are not in this one (lasso marks, lasso_plan.hpp).
inline PriorPlannedPrompts plan_prior_prompts(std::vector<char> const& has_handle, bool points_given, int const* regions, bool mask_branch,
                                              std::vector<char> const& has_pointer, bool device_form = false,
                                              bool had_continuation = false) {
    const int count = (int)has_handle.size();
    PriorPlannedPrompts out;
    for (int i = 0; i < count; ++i) out.any_prior |= !has_handle[i] && is_prior_mark_entry(regions, i);
    if (!out.any_prior) {
        out.planned = plan_grid_prompts(has_handle, points_given, regions, mask_branch, had_continuation);
        out.prior.resize(out.planned.cleaned.staged.prompts.size());
        return out;
    }
    std::vector<char> handles;
    std::vector<int> ints, entry_of;
    std::vector<std::pair<int, PriorSpec>> priors;     // (head, its mark), in head order
    for (int i = 0; i < count; ++i) {
        if (has_handle[i] || !is_prior_mark_entry(regions, i)) {
            handles.push_back(has_handle[i]);
            ints.insert(ints.end(), regions + 4 * i, regions + 4 * i + 4);
            entry_of.push_back(i);
            continue;
        }
        const int* r = regions + 4 * i;
        const std::string who = "mask batch: entry " + std::to_string(i) + ": a prior mark ";
        if (device_form)
            throw std::invalid_argument(who + "is not served by dlimg_amd_get_segmentation_masks_device: the device form has no per-entry "
                                              "pointer to read a prior from");
        if (r[1] < 0 || r[1] > kPriorMaxStrength || r[2] != 0 || r[3] != 0)
            throw std::invalid_argument(who + "is {8, strength_milli, 0, 0} in regions[4 i ..]: strength_milli is 0 (the default) .. " +
                                        std::to_string(kPriorMaxStrength) + ", the other two ints are 0");
        if (!mask_branch)
            throw std::invalid_argument(who + "needs the prompt encoder's mask branch, and the model file has no pe.mask.* tensors");
        if (i == 0) throw std::invalid_argument(who + "needs a prompt in front of it");
        if (!has_handle[i - 1]) {
            if (!priors.empty() && priors.back().second.entry == i - 1)
                throw std::invalid_argument(who + "is the second one of its prompt: a prompt has one prior at most");
            throw std::invalid_argument(who + "does not directly follow its head");
        }
        if (i >= (int)has_pointer.size() || !has_pointer[i])
            throw std::invalid_argument(who + "has no prior: out_masks[i] of the mark is the prior mask, width * height bytes, and it is NULL");
        priors.push_back({i - 1, PriorSpec{i, r[1] ? r[1] : kPriorDefaultStrength}});
    }
    try {
        out.planned = plan_grid_prompts(handles, points_given, ints.data(), mask_branch, /*had_continuation*/ true);
    } catch (std::invalid_argument const& e) {
        throw std::invalid_argument(renumber_entry(e.what(), entry_of));
    }
    // plan_grid_prompts numbers heads and click entries in the list it was given: back to the caller's through entry_of
    StagedPrompts& staged = out.planned.cleaned.staged;
    out.prior.resize(staged.prompts.size());
    size_t at = 0;
    for (size_t j = 0; j < staged.prompts.size(); ++j) {
        PromptSpec& p = staged.prompts[j];
        p.head = entry_of[p.head];
        for (int& e : staged.stages[j].click_entry) e = entry_of[e];
        if (at == priors.size() || priors[at].first != p.head) continue;
        out.prior[j] = priors[at++].second;
        const std::string who = "mask batch: entry " + std::to_string(out.prior[j].entry) + ": a prior mark ";
        if (out.planned.grid[j].any()) throw std::invalid_argument(who + "on a grid prompt: a label map takes no prior");
        if (p.clicks == 0 && !p.box)
            throw std::invalid_argument(who + "is no prompt by itself: its prompt still needs a click or a box (an empty region is no box, "
                                              "and there are no `points`)");
    }
    return out;
}

}  // namespace dlimg
