// The entries of a batch mask call (table slot 14, dlimg_amd_get_segmentation_masks_device) as prompts, and the prompts of
// one GPU as decoder launches, and a prompt as the points the decoder takes (pack_points): pure host logic (no HIP, no
// environment), tested without a GPU (tests/prompt_plan_cases.cpp, tests/test_multi_click_oracle.py).
//
// Entries -> prompts.  An entry with a handle opens a prompt and is read as it always was: its point (regions == NULL), its
// region (points == NULL), or -- both arrays given -- its region refined by its foreground point.  An entry WITHOUT a handle
// is a continuation entry: points[i] is one more click of the prompt the nearest handle in front of it opened, its label
// regions[4 i] (1 foreground, 0 background; the other three ints 0), foreground when regions == NULL.  In a call with
// continuation entries a head whose region is empty (x1 < x0) has no box.  A prompt is its head's click, the further clicks
// in the order given (8 in all at most), then the box corners if there is a box; the padding point only without a box
// (SAM's PromptEncoder / SamOnnxModel._embed_points).  A call without continuation entries is today's call, entry = prompt.
//
// Prompts -> launches.  A decoder launch holds prompts of ONE point count.  The prompts of a GPU are grouped by their point
// count (groups in the order their first prompt appears, prompts in the caller's order inside a group) and every group is
// cut into chunks of `chunk` prompts, each chunk one decode on the next lane.  Prompts, never entries, are counted, so a
// prompt is never cut; a call whose prompts all have one count is cut as it always was.
//
// Marks -> stages (plan_staged_prompts).  A continuation entry whose four ints are {kRefineMark, 0, 0, 0} is a refinement
// mark, not a click: its point is not read and it does not count towards the 8 clicks.  A prompt with m marks is decoded in
// m + 1 stages: stage j takes the clicks in front of mark j (the head's included), the last stage all of them, every stage
// the prompt's box (or the padding point), packed exactly as an unmarked prompt of those clicks; from the second stage on a
// stage takes the low-res logits of the stage before it as SAM's mask input.  Every stage adds at least one click: a mark
// directly after a mark, and a mark as the last entry of a prompt, are refused.  plan_prompts itself knows no marks: the
// value 4 is one more label it refuses.
//
// Clean-up marks (plan_cleaned_prompts).  A continuation entry whose four ints are {kCleanMark, max_hole, max_island, 0} is a
// clean-up mark: neither a click nor a stage, but a modifier of the one mask its prompt delivers (small holes filled, small
// islands dropped: kernels.hpp, k::mask_cleanup).  A prompt has at most one, as the LAST entry of its prompt.  The call
// without its clean-up marks is an ordinary call, which plan_staged_prompts reads -- with one thing kept: a call that holds
// any continuation entry, a clean-up mark included, reads an empty head region as "no box", and the mark itself needs
// `regions` but not `points` (a box-only call may clean its masks).  A call without clean-up marks is plan_staged_prompts.
//
// Grid marks ({7, side, iou_permille, stability_permille}: "segment everything") are read one layer further out, in
// grid_plan.hpp (plan_grid_prompts), which hands the call without its grid prompts to plan_cleaned_prompts.
//
// Prior marks ({8, strength_milli, 0, 0} directly behind a head: the caller's own mask as the mask input of the prompt's first
// stage) are read one layer further out again, in prior_plan.hpp (plan_prior_prompts), which hands the call without its prior
// marks to plan_grid_prompts.
//
// Lasso marks ({10, strength_milli, what, 0} directly behind a head: a selection whose box and first click are derived on the
// GPU) are read one layer further out, in lasso_plan.hpp (plan_lasso_prompts), which hands the call without its lasso marks to
// plan_prior_prompts and reserves the derived click and box in the PromptSpec.
//
// Matte marks ({11, radius, eps, channels}, the last entry of a prompt: the mask delivered as coverage, its edge guided by the
// image) are read by the outermost layer, matte_plan.hpp (plan_matte_prompts), which hands the call without its matte marks to
// plan_lasso_prompts.
#pragma once

#include "prompt_geometry.hpp"

#include <stdexcept>
#include <string>
#include <vector>

namespace dlimg {

constexpr int kMaxClicks = 8;
constexpr int kRefineMark = 4;       // regions[4 i] of a mark: the first value SAM's labels (-1 pad, 0 / 1 clicks, 2 / 3 corners) leave free
constexpr int kCleanMark = 6;        // regions[4 i] of a clean-up mark (5 stays a refused label)

struct PromptSpec {
    int head = 0;            // entry that opened the prompt (its handle, its out_masks, its region)
    int clicks = 0;          // 0: a box alone; else the head's click and the clicks - 1 continuation entries behind it
    bool box = false;
    int points() const { return box ? clicks + 2 : clicks + 1; }       // packed points: the pad token takes the box's place
};

// has_handle[i]: entry i has a handle.  Throws std::invalid_argument with the message the caller reports.
// had_continuation: the caller's list held continuation entries that are not in this one (clean-up marks): an empty region is
// "no box" as in any call with continuation entries.
inline std::vector<PromptSpec> plan_prompts(std::vector<char> const& has_handle, bool points_given, int const* regions,
                                            bool had_continuation = false) {
    const int count = (int)has_handle.size();
    std::vector<PromptSpec> prompts;
    bool any_continuation = false;
    for (int i = 0; i < count; ++i) any_continuation |= !has_handle[i];
    const bool empty_is_no_box = any_continuation || had_continuation;
    if (!points_given && !regions) throw std::invalid_argument("mask batch: neither points nor regions given");
    if (any_continuation && !points_given) throw std::invalid_argument("mask batch: a continuation entry (null handle) is a click and needs `points`");
    prompts.reserve(count);
    for (int i = 0; i < count; ++i) {
        if (has_handle[i]) {
            PromptSpec p;
            p.head = i;
            p.clicks = points_given ? 1 : 0;
            p.box = regions != nullptr;
            // the empty region of a multi-click call: no box
            if (empty_is_no_box && regions && regions[4 * i + 2] < regions[4 * i]) p.box = false;
            prompts.push_back(p);
            continue;
        }
        if (prompts.empty()) throw std::invalid_argument("mask batch: entry 0 has no handle: a continuation entry needs a prompt in front of it");
        PromptSpec& p = prompts.back();
        if (regions) {
            const int* r = regions + 4 * i;
            if ((r[0] != 0 && r[0] != 1) || r[1] != 0 || r[2] != 0 || r[3] != 0)
                throw std::invalid_argument("mask batch: entry " + std::to_string(i) + ": the label of a click is 1 (foreground) or 0 (background), "
                                            "in regions[4 i] with the other three ints 0");
        }
        if (++p.clicks > kMaxClicks)
            throw std::invalid_argument("mask batch: the prompt of entry " + std::to_string(p.head) + " has more than " +
                                        std::to_string(kMaxClicks) + " clicks");
    }
    return prompts;
}

struct PromptChunk {
    int points = 0;                  // packed points of every prompt of the chunk
    std::vector<int> prompts;        // indices into the call's prompt list, caller's order
};

// The stages of one prompt of a call that may hold marks.  click_entry[c]: the entry click c travels in (the head for c = 0;
// marks skipped, so the clicks of a marked prompt are not consecutive entries); stage_clicks[j]: the clicks stage j takes,
// strictly increasing, the last one == PromptSpec::clicks.  A prompt without marks has one stage.
struct PromptStages {
    std::vector<int> click_entry;
    std::vector<int> stage_clicks;
    bool staged() const { return stage_clicks.size() > 1; }
};
struct StagedPrompts {
    std::vector<PromptSpec> prompts;
    std::vector<PromptStages> stages;        // [prompt]
};

inline bool is_mark_entry(int const* regions, int i) { return regions && regions[4 * i] == kRefineMark; }
inline bool is_clean_mark_entry(int const* regions, int i) { return regions && regions[4 * i] == kCleanMark; }

// A refusal that names "entry N" of a list some entries were taken out of, with N put back to the caller's numbering:
// entry_of[n] is the caller's entry that became entry n.
inline std::string renumber_entry(std::string msg, std::vector<int> const& entry_of) {
    const std::string key = "entry ";
    const size_t at = msg.find(key);
    if (at == std::string::npos) return msg;
    size_t end = at + key.size();
    while (end < msg.size() && msg[end] >= '0' && msg[end] <= '9') ++end;
    if (end == at + key.size()) return msg;
    const size_t n = std::stoul(msg.substr(at + key.size(), end - at - key.size()));
    if (n < entry_of.size()) msg = msg.substr(0, at + key.size()) + std::to_string(entry_of[n]) + msg.substr(end);
    return msg;
}

// the one stage of a prompt without marks: its clicks travel in consecutive entries
inline PromptStages unmarked_stages(PromptSpec const& p) {
    PromptStages s;
    for (int c = 0; c < p.clicks; ++c) s.click_entry.push_back(p.head + c);
    s.stage_clicks.push_back(p.clicks);
    return s;
}

// plan_prompts for a call that may hold marks; without one it is plan_prompts (same prompts, same refusals).  mask_branch: the
// model has the prompt encoder's mask branch (pe.mask.*), without which no stage can take a mask input.
inline StagedPrompts plan_staged_prompts(std::vector<char> const& has_handle, bool points_given, int const* regions, bool mask_branch,
                                         bool had_continuation = false) {
    const int count = (int)has_handle.size();
    bool any_mark = false;
    for (int i = 0; i < count; ++i) any_mark |= !has_handle[i] && is_mark_entry(regions, i);
    StagedPrompts out;
    if (!any_mark) {
        out.prompts = plan_prompts(has_handle, points_given, regions, had_continuation);
        for (PromptSpec const& p : out.prompts) out.stages.push_back(unmarked_stages(p));
        return out;
    }
    // the call without its marks is an ordinary call, which plan_prompts reads (a marked prompt has two clicks or more, so
    // the call keeps a continuation entry and with it the reading of an empty region as "no box")
    std::vector<char> handles;
    std::vector<int> ints, entry_of;
    bool last_was_mark = false;
    for (int i = 0; i < count; ++i) {
        const bool mark = !has_handle[i] && is_mark_entry(regions, i);
        if (mark) {
            const int* r = regions + 4 * i;
            const std::string who = "mask batch: entry " + std::to_string(i) + ": a refinement mark ";
            if (r[1] != 0 || r[2] != 0 || r[3] != 0) throw std::invalid_argument(who + "is {4, 0, 0, 0} in regions[4 i ..]: the other three ints are 0");
            if (!mask_branch)
                throw std::invalid_argument(who + "needs the prompt encoder's mask branch, and the model file has no pe.mask.* tensors");
            if (handles.empty()) throw std::invalid_argument(who + "needs a prompt in front of it");
            if (last_was_mark) throw std::invalid_argument(who + "directly follows another mark: every stage adds at least one click");
            if (i + 1 == count || has_handle[i + 1])
                throw std::invalid_argument(who + "is the last entry of its prompt: every stage adds at least one click");
        } else {
            handles.push_back(has_handle[i]);
            ints.insert(ints.end(), regions + 4 * i, regions + 4 * i + 4);
            entry_of.push_back(i);
        }
        last_was_mark = mark;
    }
    std::vector<PromptSpec> packed;
    try {
        packed = plan_prompts(handles, points_given, ints.data(), had_continuation);
    } catch (std::invalid_argument const& e) {
        // plan_prompts numbers the entries of the list without marks: name the caller's entry instead
        throw std::invalid_argument(renumber_entry(e.what(), entry_of));
    }
    for (PromptSpec p : packed) {
        PromptStages s;
        for (int c = 0; c < p.clicks; ++c) s.click_entry.push_back(entry_of[p.head + c]);
        p.head = entry_of[p.head];
        // the marks of this prompt: the entries between its clicks
        for (int c = 1; c < p.clicks; ++c)
            if (s.click_entry[c] != s.click_entry[c - 1] + 1) s.stage_clicks.push_back(c);
        s.stage_clicks.push_back(p.clicks);
        out.prompts.push_back(p);
        out.stages.push_back(s);
    }
    return out;
}

// What a clean-up mark asks for: both 0 = the prompt's mask is delivered as it is.
struct CleanSpec {
    int max_hole = 0, max_island = 0;
    bool any() const { return max_hole > 0 || max_island > 0; }
};
struct CleanedPrompts {
    StagedPrompts staged;                // the call without its clean-up marks; heads and click entries in the caller's numbering
    std::vector<CleanSpec> clean;      // [prompt]
    bool any_clean = false;
};

// plan_staged_prompts for a call that may hold clean-up marks; without one it is plan_staged_prompts (same prompts, same
// refusals).  Every refusal about a clean-up mark says "mark" and names the caller's entry.
// had_continuation: as for plan_prompts -- the caller's list held continuation entries that are not in this one (the marks of
// grid prompts, grid_plan.hpp).
inline CleanedPrompts plan_cleaned_prompts(std::vector<char> const& has_handle, bool points_given, int const* regions, bool mask_branch,
                                           bool had_continuation = false) {
    const int count = (int)has_handle.size();
    CleanedPrompts out;
    for (int i = 0; i < count; ++i) out.any_clean |= !has_handle[i] && is_clean_mark_entry(regions, i);
    if (!out.any_clean) {
        out.staged = plan_staged_prompts(has_handle, points_given, regions, mask_branch, had_continuation);
        out.clean.resize(out.staged.prompts.size());
        return out;
    }
    std::vector<char> handles;
    std::vector<int> ints, entry_of;
    std::vector<CleanSpec> by_head;        // [prompt of the list without clean-up marks]
    for (int i = 0; i < count; ++i) {
        if (has_handle[i] || !is_clean_mark_entry(regions, i)) {
            if (has_handle[i]) by_head.push_back(CleanSpec{});
            handles.push_back(has_handle[i]);
            ints.insert(ints.end(), regions + 4 * i, regions + 4 * i + 4);
            entry_of.push_back(i);
            continue;
        }
        const int* r = regions + 4 * i;
        const std::string who = "mask batch: entry " + std::to_string(i) + ": a clean-up mark ";
        if (r[1] < 0 || r[2] < 0 || (r[1] == 0 && r[2] == 0) || r[3] != 0)
            throw std::invalid_argument(who + "is {6, max_hole, max_island, 0} in regions[4 i ..]: thresholds >= 0 and not both 0, the fourth int 0");
        if (by_head.empty()) throw std::invalid_argument(who + "needs a prompt in front of it");
        if (i + 1 < count && !has_handle[i + 1])
            throw std::invalid_argument(who + "is the last entry of its prompt, and a prompt has one at most");
        by_head.back() = CleanSpec{r[1], r[2]};
    }
    try {
        out.staged = plan_staged_prompts(handles, points_given, ints.data(), mask_branch, /*had_continuation*/ true);
    } catch (std::invalid_argument const& e) {
        throw std::invalid_argument(renumber_entry(e.what(), entry_of));
    }
    // prompts come out in head order, one per handle
    out.clean = by_head;
    for (size_t j = 0; j < out.staged.prompts.size(); ++j) {
        PromptSpec& p = out.staged.prompts[j];
        p.head = entry_of[p.head];
        for (int& e : out.staged.stages[j].click_entry) e = entry_of[e];
        if (p.clicks == 0 && !p.box)
            throw std::invalid_argument("mask batch: entry " + std::to_string(p.head) + ": a prompt with a clean-up mark still needs a click or "
                                        "a box (an empty region is no box, and there are no `points`)");
    }
    return out;
}

// label of click c (0: the head's own) of a prompt, marked or not
inline int click_label(PromptStages const& s, int c, int const* regions) {
    return (c == 0 || !regions) ? 1 : regions[4 * s.click_entry[c]];
}
// the spellings programs written against the earlier header use: the same rule, by the prompt (unmarked) or by its stages
inline int click_label(PromptSpec const& p, int c, int const* regions) { return click_label(unmarked_stages(p), c, regions); }
inline int staged_click_label(PromptStages const& s, int c, int const* regions) { return click_label(s, c, regions); }

// The first n_clicks clicks of a prompt as the decoder takes them, from the call's arrays (points [count][2], regions
// [count][4]): the clicks in the order given with their labels, each from the entry it travels in, then the corners of the
// head's box (labels 2, 3), or the padding point (0, 0), label -1, when there is none (SAM's PromptEncoder.forward /
// SamOnnxModel._embed_points).  n_clicks == spec.clicks: the prompt itself; fewer: a stage of a marked prompt, packed exactly
// as an unmarked prompt of those clicks.  coords [n][2] in the frame of `rs`, labels [n]; returns n = n_clicks + 2 with a
// box, n_clicks + 1 without (PromptSpec::points() for the whole prompt).
inline int pack_points(ResizeLongestSide const& rs, PromptSpec const& spec, PromptStages const& stages, int n_clicks, int const* points,
                       int const* regions, float* coords, float* labels) {
    int n = 0;
    auto set = [&](Point p, int label) {
        const Point t = rs.transform(p);
        coords[n * 2 + 0] = float(t.x);
        coords[n * 2 + 1] = float(t.y);
        labels[n++] = float(label);
    };
    for (int c = 0; c < n_clicks; ++c) {
        const int e = stages.click_entry[c];
        set(Point{points[e * 2], points[e * 2 + 1]}, click_label(stages, c, regions));
    }
    if (spec.box) {
        int const* r = regions + 4 * spec.head;
        set(Point{r[0], r[1]}, 2);
        set(Point{r[2], r[3]}, 3);
    } else {
        set(Point{0, 0}, -1);
    }
    return n;
}

// `mine`: the prompts (indices) one GPU decodes, in the caller's order
inline std::vector<PromptChunk> plan_prompt_chunks(std::vector<PromptSpec> const& prompts, std::vector<int> const& mine, int chunk) {
    std::vector<int> counts;         // point counts in order of first appearance
    for (int i : mine) {
        const int n = prompts[i].points();
        bool seen = false;
        for (int c : counts) seen |= c == n;
        if (!seen) counts.push_back(n);
    }
    std::vector<PromptChunk> out;
    for (int n : counts) {
        PromptChunk cur;
        cur.points = n;
        for (int i : mine) {
            if (prompts[i].points() != n) continue;
            cur.prompts.push_back(i);
            if ((int)cur.prompts.size() == chunk) {
                out.push_back(cur);
                cur.prompts.clear();
            }
        }
        if (!cur.prompts.empty()) out.push_back(cur);
    }
    return out;
}

}  // namespace dlimg
