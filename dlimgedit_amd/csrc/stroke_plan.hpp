// Stroke marks of a batch mask call (table slot 14): clicks sampled from a caller's scribbles on the GPU (kernels.hpp,
// k::stroke_derive).  Pure host logic (no HIP, no environment), tested without a GPU (tests/stroke_plan_cases.cpp,
// tests/test_stroke_plan.py).
//
// A continuation entry whose four ints are {kStrokeMark, clicks, label, 0} is a stroke mark.  Its point is not read; its out_masks
// pointer is READ as the stroke map: width * height bytes of the head's image, tightly packed, a pixel belonging to the stroke
// when its byte is >= 128.  label: 1 foreground, 0 background; clicks: 1 .. 8, 0 = kStrokeDefaultClicks.  The mark may stand
// wherever a click entry may stand and STANDS FOR `clicks` click entries of its label at that position: they count towards the 8
// clicks and the SAM-HQ limit, a refinement mark behind them stages them like any click, a prompt may hold several stroke marks.
// Prior and lasso marks keep their place directly behind the head, in front of every stroke mark; clean-up and matte marks stay
// last, behind every stroke mark.  In a call without `points` the first foreground click a prompt's strokes stand for takes the
// place of the head's own click, so every prompt of such a call needs a foreground stroke.
//
// plan_stroke_prompts is the outermost planner: it REWRITES the call -- every stroke mark becomes its placeholder click entries,
// whose points the derivation fills in at run time -- and hands the rewritten call to plan_matte_prompts as one with `points`.
// The plan that comes back speaks of the REWRITTEN call's entries (its arrays are what the one packer reads); entry_of maps them
// back to the caller's, which every refusal names: the inner planners' refusals are renumbered through it.  A call without stroke
// marks is plan_matte_prompts, and nothing is rewritten.  Every refusal about a stroke mark says "mark" and names the caller's
// entry.
//
// stroke_cell_pixel maps a cell of the derivation's record to the middle pixel of its footprint, as fold_lasso_rows maps the
// lasso's click.
#pragma once

#include "matte_plan.hpp"

namespace dlimg {

constexpr int kStrokeMark = 12;                // regions[4 i] of a stroke mark (5 and 9 stay refused labels)
constexpr int kStrokeDefaultClicks = 3;        // clicks == 0: a choice, not a measurement
constexpr int kStrokeRecordInts = 20;          // k::stroke_derive: {ON cells, clicks, x0, y0 .. x7, y7, 0, 0}

struct StrokeSpec {
    int entry = -1;                    // the mark's entry (whose out_masks pointer is the map), CALLER's numbering
    int label = 1;                     // 1 foreground, 0 background
    int clicks = 0;                    // 1 .. kMaxClicks once planned
    std::vector<int> click_entry;      // [clicks]: the entry of the REWRITTEN call derived click c travels in (the head, for the click
                                       // that takes the place of the head's own)
};
struct StrokePlannedPrompts {
    MattePlannedPrompts inner;         // every prompt of the call; with any_stroke in the rewritten call's numbering
    std::vector<std::vector<StrokeSpec>> strokes;      // [prompt]: its stroke marks in the order given
    bool any_stroke = false;
    // the rewritten call (any_stroke only): what has_handle, regions and has_pointer became
    std::vector<char> handles, pointers;
    std::vector<int> regions;          // [entry][4]
    std::vector<int> entry_of;         // [entry]: the caller's entry it came from (a placeholder: its mark)
    std::vector<char> derived;         // [entry]: its point is a derived click's (never read from the caller's `points`)
    int caller_entry(int e) const { return any_stroke ? entry_of[e] : e; }
};

inline bool is_stroke_mark_entry(int const* regions, int i) { return regions && regions[4 * i] == kStrokeMark; }

// has_pointer, device_form: as for plan_prior_prompts (the pointer of a stroke mark's entry is its map).
inline StrokePlannedPrompts plan_stroke_prompts(std::vector<char> const& has_handle, bool points_given, int const* regions, bool mask_branch,
                                                std::vector<char> const& has_pointer, bool device_form = false) {
    const int count = (int)has_handle.size();
    StrokePlannedPrompts out;
    for (int i = 0; i < count; ++i) out.any_stroke |= !has_handle[i] && is_stroke_mark_entry(regions, i);
    if (!out.any_stroke) {
        out.inner = plan_matte_prompts(has_handle, points_given, regions, mask_branch, has_pointer, device_form);
        out.strokes.resize(out.inner.inner.inner.planned.cleaned.staged.prompts.size());
        return out;
    }
    auto push = [&](int from, int const* ints, bool handle, bool pointer, bool derived) {
        out.handles.push_back(handle);
        out.pointers.push_back(pointer);
        out.regions.insert(out.regions.end(), ints, ints + 4);
        out.entry_of.push_back(from);
        out.derived.push_back(derived);
    };
    int head = -1, head_rw = -1;       // the head of the prompt entry i belongs to: caller's entry, rewritten entry
    bool head_click_taken = false;     // (no `points`) a foreground stroke of this prompt has given the head its click
    bool tail_seen = false;            // a clean-up or matte mark of this prompt lies in front of entry i
    std::vector<int> heads;            // [prompt]: caller's entry
    std::vector<char> has_head_click;  // [prompt]
    for (int i = 0; i < count; ++i) {
        const bool pointer = i < (int)has_pointer.size() && has_pointer[i];
        if (has_handle[i] || !is_stroke_mark_entry(regions, i)) {
            if (has_handle[i]) {
                if (head >= 0) has_head_click.push_back(points_given || head_click_taken);
                head = i;
                head_rw = (int)out.handles.size();
                heads.push_back(i);
                head_click_taken = tail_seen = false;
                out.strokes.emplace_back();
            } else {
                tail_seen |= is_clean_mark_entry(regions, i) || is_matte_mark_entry(regions, i);
                // (the rewritten call has `points`, so plan_prompts no longer says this)
                if (!points_given && (regions[4 * i] == 0 || regions[4 * i] == 1))
                    throw std::invalid_argument("mask batch: entry " + std::to_string(i) + ": a continuation entry (null handle) is a click and "
                                                "needs `points`; only what a stroke mark stands for is derived");
            }
            push(i, regions + 4 * i, has_handle[i], pointer, !has_handle[i] ? false : !points_given);
            continue;
        }
        const int* r = regions + 4 * i;
        const std::string who = "mask batch: entry " + std::to_string(i) + ": a stroke mark ";
        if (device_form)
            throw std::invalid_argument(who + "is not served by dlimg_amd_get_segmentation_masks_device: the device form has no per-entry "
                                              "pointer to read a stroke map from");
        if (r[1] < 0 || r[1] > kMaxClicks || (r[2] != 0 && r[2] != 1) || r[3] != 0)
            throw std::invalid_argument(who + "is {12, clicks, label, 0} in regions[4 i ..]: clicks is 0 (the default, " +
                                        std::to_string(kStrokeDefaultClicks) + ") .. " + std::to_string(kMaxClicks) +
                                        ", label is 1 (foreground) or 0 (background), the fourth int is 0");
        if (head < 0) throw std::invalid_argument(who + "needs a prompt in front of it");
        if (!pointer)
            throw std::invalid_argument(who + "has no map: out_masks[i] of the mark is the stroke map, width * height bytes, and it is NULL");
        if (tail_seen)
            throw std::invalid_argument(who + "stands behind a clean-up or matte mark: those stay the last entries of their prompt");
        int clicks_in_all = points_given ? 1 : 0;      // of the whole prompt: the head's, the click entries, what the stroke marks stand for
        for (int e = head + 1; e < count && !has_handle[e]; ++e) {
            const int kind = regions[4 * e];
            if (is_grid_mark_entry(regions, e)) throw std::invalid_argument(who + "on a grid prompt: a label map takes no clicks");
            if (e > i && (kind == kPriorMark || kind == kLassoMark))
                throw std::invalid_argument(who + "stands in front of a " + (kind == kPriorMark ? "prior" : "lasso") +
                                            " mark: that one keeps its place directly behind the head, in front of every stroke mark");
            if (kind == 0 || kind == 1) ++clicks_in_all;
            if (kind == kStrokeMark && regions[4 * e + 1] >= 0 && regions[4 * e + 1] <= kMaxClicks)
                clicks_in_all += regions[4 * e + 1] ? regions[4 * e + 1] : kStrokeDefaultClicks;
        }
        if (clicks_in_all > kMaxClicks)
            throw std::invalid_argument(who + "stands for clicks that count: with them the prompt of entry " + std::to_string(head) + " has " +
                                        std::to_string(clicks_in_all) + " clicks, more than " + std::to_string(kMaxClicks));
        StrokeSpec spec;
        spec.entry = i;
        spec.label = r[2];
        spec.clicks = r[1] ? r[1] : kStrokeDefaultClicks;
        const int placeholder[4] = {spec.label, 0, 0, 0};
        for (int c = 0; c < spec.clicks; ++c) {
            if (!points_given && spec.label == 1 && !head_click_taken) {
                head_click_taken = true;               // the first derived foreground click of the prompt is the head's own
                spec.click_entry.push_back(head_rw);
                continue;
            }
            spec.click_entry.push_back((int)out.handles.size());
            push(i, placeholder, false, true, true);
        }
        out.strokes.back().push_back(std::move(spec));
    }
    if (head >= 0) has_head_click.push_back(points_given || head_click_taken);
    for (size_t j = 0; j < heads.size(); ++j) {
        if (has_head_click[j]) continue;
        if (out.strokes[j].empty())
            throw std::invalid_argument("mask batch: entry " + std::to_string(heads[j]) + ": in a call without `points` that holds a stroke mark "
                                        "every prompt takes its head's click from a foreground stroke mark, and this prompt has none");
        throw std::invalid_argument("mask batch: entry " + std::to_string(out.strokes[j][0].entry) + ": a stroke mark of background clicks is "
                                    "no prompt by itself: without `points` the prompt of entry " + std::to_string(heads[j]) +
                                    " needs a foreground stroke mark, whose first click is the head's");
    }
    try {
        out.inner = plan_matte_prompts(out.handles, /*points_given*/ true, out.regions.data(), mask_branch, out.pointers, device_form);
    } catch (std::invalid_argument const& e) {
        throw std::invalid_argument(renumber_entry(e.what(), out.entry_of));
    }
    StagedPrompts& staged = out.inner.inner.inner.planned.cleaned.staged;
    // the caller's call held continuation entries, so an empty region is "no box" -- which the inner planners cannot know when the
    // rewritten call holds none (every stroke click went to a head): then they are plan_prompts alone, and this is the one thing
    // to put right
    bool continuation_left = false;
    for (char h : out.handles) continuation_left |= !h;
    if (!continuation_left)
        for (PromptSpec& p : staged.prompts)
            if (out.regions[4 * p.head + 2] < out.regions[4 * p.head]) p.box = false;
    return out;
}

// cell (x, y) of a stroke record -> the middle pixel of its footprint in an image width x height encoded at pre_w x pre_h
inline void stroke_cell_pixel(int x, int y, int width, int height, int pre_w, int pre_h, int pixel[2]) {
    pixel[0] = (footprint_lo(x, width, pre_w) + footprint_hi(x, width, pre_w) - 1) / 2;
    pixel[1] = (footprint_lo(y, height, pre_h) + footprint_hi(y, height, pre_h) - 1) / 2;
}

}  // namespace dlimg
