// Lasso marks of a batch mask call (table slot 14): a caller's selection snapped to the object -- the prompt's box and its first
// click are DERIVED from the selection on the GPU (kernels.hpp, k::lasso_derive), and the selection may be the mask input of the
// first stage as well.  Pure host logic (no HIP, no environment), tested without a GPU (tests/lasso_plan_cases.cpp,
// tests/test_lasso_ref.py, tests/sanitize/lasso_plan_fuzz.cpp).
//
// A continuation entry whose four ints are {kLassoMark, strength_milli, what, 0} DIRECTLY BEHIND ITS HEAD is a lasso mark.  Its
// point is not read; its out_masks pointer is READ as the selection, width * height bytes of the head's image, 0 .. 255 taken as
// coverage, exactly as a prior mark's.  what is a bit set, 0 = all three:
//   kLassoBox    the prompt's box is the selection's box (the head's region must be empty)
//   kLassoClick  the prompt's FIRST click is a foreground click at the selection's most interior point; it counts towards the
//                8 clicks, the caller's clicks follow it in the order given
//   kLassoMask   the selection is the mask input of the first stage, as a prior mark of this strength_milli would make it
// strength_milli is 0 without kLassoMask; with it, 0 = kPriorDefaultStrength.
//
// plan_lasso_prompts takes the marks out, remembers {entry, what, strength} per prompt, hands the rest to plan_prior_prompts as a
// call that held continuation entries, and RESERVES the derived click and box in the PromptSpec (and the click in the stages: it
// belongs to the first one), so token counts, SAM-HQ limits and chunking are right before anything runs.  A call without lasso
// marks is plan_prior_prompts.  Every refusal about a lasso mark says "mark" and names the caller's entry.
//
// fold_lasso_rows folds the row records of k::lasso_derive into the prompt's record and maps cells to image pixels;
// lasso_prompt_arrays writes a record into the arrays pack_points reads, as a call of that one prompt.
#pragma once

#include "kernels/footprint.hpp"
#include "prior_plan.hpp"

namespace dlimg {

constexpr int kLassoMark = 10;                 // regions[4 i] of a lasso mark (5 and 9 stay refused labels)
constexpr int kLassoBox = 1, kLassoClick = 2, kLassoMask = 4;
constexpr int kLassoAll = kLassoBox | kLassoClick | kLassoMask;
constexpr int kLassoRecordInts = 8;            // {inside cells, box x0, y0, x1, y1, click x, click y, d2}
constexpr int kLassoRows = 256, kLassoRowRecordInts = 8;       // k::lasso_derive: one record per low-res row (kernels.hpp)

struct LassoSpec {
    int entry = -1;                    // the mark's entry (whose out_masks pointer is the selection), caller's numbering; -1: none
    int what = 0;                      // 1 .. 7 once planned, never 4
    int strength_milli = 0;            // with kLassoMask: 1 .. kPriorMaxStrength once planned; 0 without
    bool any() const { return entry >= 0; }
    bool box() const { return (what & kLassoBox) != 0; }
    bool click() const { return (what & kLassoClick) != 0; }
    bool mask() const { return (what & kLassoMask) != 0; }
};
struct LassoPlannedPrompts {
    PriorPlannedPrompts inner;         // every prompt of the call, caller's numbering, derived clicks and boxes reserved
    std::vector<LassoSpec> lasso;      // [prompt]
    bool any_lasso = false;
};

inline bool is_lasso_mark_entry(int const* regions, int i) { return regions && regions[4 * i] == kLassoMark; }

// has_pointer, device_form: as for plan_prior_prompts.  had_continuation: as for plan_prompts -- the caller's list held continuation
// entries that are not in this one (matte marks, matte_plan.hpp).
inline LassoPlannedPrompts plan_lasso_prompts(std::vector<char> const& has_handle, bool points_given, int const* regions, bool mask_branch,
                                              std::vector<char> const& has_pointer, bool device_form = false,
                                              bool had_continuation = false) {
    const int count = (int)has_handle.size();
    LassoPlannedPrompts out;
    for (int i = 0; i < count; ++i) out.any_lasso |= !has_handle[i] && is_lasso_mark_entry(regions, i);
    if (!out.any_lasso) {
        out.inner = plan_prior_prompts(has_handle, points_given, regions, mask_branch, has_pointer, device_form, had_continuation);
        out.lasso.resize(out.inner.planned.cleaned.staged.prompts.size());
        return out;
    }
    std::vector<char> handles, pointers;
    std::vector<int> ints, entry_of;
    struct Found { int head; LassoSpec spec; bool own_box; };
    std::vector<Found> found;                      // in head order
    for (int i = 0; i < count; ++i) {
        if (has_handle[i] || !is_lasso_mark_entry(regions, i)) {
            handles.push_back(has_handle[i]);
            pointers.push_back(i < (int)has_pointer.size() && has_pointer[i]);
            ints.insert(ints.end(), regions + 4 * i, regions + 4 * i + 4);
            entry_of.push_back(i);
            continue;
        }
        const int* r = regions + 4 * i;
        const std::string who = "mask batch: entry " + std::to_string(i) + ": a lasso mark ";
        if (device_form)
            throw std::invalid_argument(who + "is not served by dlimg_amd_get_segmentation_masks_device: the device form has no per-entry "
                                              "pointer to read a selection from");
        if (r[1] < 0 || r[1] > kPriorMaxStrength || r[2] < 0 || r[2] > kLassoAll || r[3] != 0)
            throw std::invalid_argument(who + "is {10, strength_milli, what, 0} in regions[4 i ..]: strength_milli is 0 (the default) .. " +
                                        std::to_string(kPriorMaxStrength) + ", what is 0 (all) .. 7, the fourth int is 0");
        if (r[2] == kLassoMask)
            throw std::invalid_argument(who + "with what == 4 derives nothing: the selection as a mask input alone is a prior mark");
        const int what = r[2] ? r[2] : kLassoAll;
        if (!(what & kLassoMask) && r[1] != 0)
            throw std::invalid_argument(who + "has a strength_milli without the mask bit (4) in what: the selection is not a mask input");
        if ((what & kLassoMask) && !mask_branch)
            throw std::invalid_argument(who + "with the mask bit (4) needs the prompt encoder's mask branch, and the model file has no "
                                              "pe.mask.* tensors");
        if (i == 0) throw std::invalid_argument(who + "needs a prompt in front of it");
        if (!has_handle[i - 1]) {
            if (!found.empty() && found.back().spec.entry == i - 1)
                throw std::invalid_argument(who + "is the second one of its prompt: a prompt has one selection at most");
            if (is_prior_mark_entry(regions, i - 1))
                throw std::invalid_argument(who + "follows a prior mark: a prompt takes a prior or a selection, not both");
            throw std::invalid_argument(who + "does not directly follow its head");
        }
        if (i + 1 < count && !has_handle[i + 1] && is_prior_mark_entry(regions, i + 1))
            throw std::invalid_argument(who + "is followed by a prior mark: a prompt takes a prior or a selection, not both");
        for (int e = i + 1; e < count && !has_handle[e]; ++e)
            if (is_grid_mark_entry(regions, e)) throw std::invalid_argument(who + "on a grid prompt: a label map takes no selection");
        if (i >= (int)has_pointer.size() || !has_pointer[i])
            throw std::invalid_argument(who + "has no selection: out_masks[i] of the mark is the selection, width * height bytes, and it is NULL");
        const int* h = regions + 4 * (i - 1);
        const bool own_box = !(h[2] < h[0]);
        if ((what & kLassoBox) && own_box)
            throw std::invalid_argument(who + "with the box bit (1) needs a head with an empty region (x1 < x0): the prompt's box is the "
                                              "selection's");
        // the inner planners see a prompt that has its box already (they refuse a prompt with neither a click nor a box)
        if (!own_box) {
            int* head_ints = ints.data() + ints.size() - 4;
            head_ints[0] = head_ints[1] = head_ints[2] = head_ints[3] = 0;
        }
        found.push_back(Found{i - 1, LassoSpec{i, what, (what & kLassoMask) ? (r[1] ? r[1] : kPriorDefaultStrength) : 0}, own_box});
    }
    try {
        out.inner = plan_prior_prompts(handles, points_given, ints.data(), mask_branch, pointers, device_form, /*had_continuation*/ true);
    } catch (std::invalid_argument const& e) {
        throw std::invalid_argument(renumber_entry(e.what(), entry_of));
    }
    // plan_prior_prompts numbers entries in the list it was given: back to the caller's through entry_of
    StagedPrompts& staged = out.inner.planned.cleaned.staged;
    out.lasso.resize(staged.prompts.size());
    size_t at = 0;
    for (size_t j = 0; j < staged.prompts.size(); ++j) {
        PromptSpec& p = staged.prompts[j];
        PromptStages& st = staged.stages[j];
        p.head = entry_of[p.head];
        for (int& e : st.click_entry) e = entry_of[e];
        if (out.inner.prior[j].any()) out.inner.prior[j].entry = entry_of[out.inner.prior[j].entry];
        if (at == found.size() || found[at].head != p.head) continue;
        Found const& f = found[at++];
        out.lasso[j] = f.spec;
        const std::string who = "mask batch: entry " + std::to_string(f.spec.entry) + ": a lasso mark ";
        if (out.inner.planned.grid[j].any()) throw std::invalid_argument(who + "on a grid prompt: a label map takes no selection");
        if (out.inner.prior[j].any()) throw std::invalid_argument(who + "and a prior mark on one prompt: a prompt takes a prior or a selection, not both");
        // what the derivation will deliver is reserved here: the box, and the click in front of the caller's
        p.box = f.spec.box() || f.own_box;
        if (f.spec.click()) {
            if (p.clicks + 1 > kMaxClicks)
                throw std::invalid_argument(who + "derives a click, and with it the prompt of entry " + std::to_string(p.head) + " has more than " +
                                            std::to_string(kMaxClicks) + " clicks");
            ++p.clicks;
            st.click_entry.insert(st.click_entry.begin(), f.spec.entry);       // (never read from the call's arrays)
            for (int& c : st.stage_clicks) ++c;
        }
    }
    return out;
}

// The row records of k::lasso_derive ([kLassoRows][kLassoRowRecordInts]: {inside cells, first inside column, last, column of the
// row's best cell, its d2, ...}) of an image width x height encoded at pre_w x pre_h -> record {inside cells, box x0, y0, x1,
// y1, click x, click y, d2} in image pixels: the box is the union of the inside cells' footprints (pixel-edge convention), the
// click the middle pixel of the footprint of the inside cell with the largest d2, ties to the smallest y, then the smallest
// x.  All zero when no cell is inside.
inline void fold_lasso_rows(int32_t const* rows, int width, int height, int pre_w, int pre_h, int32_t record[kLassoRecordInts]) {
    int64_t total = 0;
    int x_min = kLassoRows, x_max = -1, y_min = -1, y_max = -1, best_x = 0, best_y = 0, best_d2 = 0;
    for (int y = 0; y < kLassoRows; ++y) {
        int32_t const* r = rows + (size_t)y * kLassoRowRecordInts;
        if (r[0] <= 0) continue;
        total += r[0];
        x_min = r[1] < x_min ? r[1] : x_min;
        x_max = r[2] > x_max ? r[2] : x_max;
        if (y_min < 0) y_min = y;
        y_max = y;
        if (r[4] > best_d2) {
            best_d2 = r[4];
            best_x = r[3];
            best_y = y;
        }
    }
    for (int k = 0; k < kLassoRecordInts; ++k) record[k] = 0;
    if (total == 0) return;
    record[0] = (int32_t)total;
    record[1] = footprint_lo(x_min, width, pre_w);
    record[2] = footprint_lo(y_min, height, pre_h);
    record[3] = footprint_hi(x_max, width, pre_w);
    record[4] = footprint_hi(y_max, height, pre_h);
    record[5] = (footprint_lo(best_x, width, pre_w) + footprint_hi(best_x, width, pre_w) - 1) / 2;
    record[6] = (footprint_lo(best_y, height, pre_h) + footprint_hi(best_y, height, pre_h) - 1) / 2;
    record[7] = best_d2;
}

// One lasso prompt as a call of its own, the derived click and box written in: what pack_points (and with it every stage)
// reads instead of the call's arrays.  Entry 0 is the head (the first click, the box), entry c click c with its label.
struct LassoPromptArrays {
    PromptSpec spec;
    PromptStages stages;
    std::vector<int> points, regions;
};
inline LassoPromptArrays lasso_prompt_arrays(PromptSpec const& p, PromptStages const& st, LassoSpec const& l, int const* points,
                                             int const* regions, int32_t const record[kLassoRecordInts]) {
    LassoPromptArrays a;
    a.spec = p;
    a.spec.head = 0;
    a.stages.stage_clicks = st.stage_clicks;
    const int entries = p.clicks > 0 ? p.clicks : 1;
    a.points.assign((size_t)entries * 2, 0);
    a.regions.assign((size_t)entries * 4, 0);
    for (int c = 0; c < p.clicks; ++c) {
        a.stages.click_entry.push_back(c);
        if (c == 0 && l.click()) {
            a.points[0] = record[5];
            a.points[1] = record[6];
            continue;
        }
        const int e = st.click_entry[c];
        a.points[c * 2] = points[e * 2];
        a.points[c * 2 + 1] = points[e * 2 + 1];
        if (c > 0) a.regions[c * 4] = (e == p.head || !regions) ? 1 : regions[4 * e];      // the head's own click is foreground
    }
    for (int k = 0; k < 4; ++k) a.regions[k] = l.box() ? record[1 + k] : regions[4 * p.head + k];
    return a;
}

}  // namespace dlimg
