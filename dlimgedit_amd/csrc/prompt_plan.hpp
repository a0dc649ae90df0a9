// The entries of a batch mask call (table slot 14, dlimg_amd_get_segmentation_masks_device) as prompts, and the prompts of
// one GPU as decoder launches: pure host logic (no HIP, no environment), tested without a GPU (tests/prompt_plan_cases.cpp,
// tests/test_multi_click_oracle.py).
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
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

namespace dlimg {

constexpr int kMaxClicks = 8;

struct PromptSpec {
    int head = 0;            // entry that opened the prompt (its handle, its out_masks, its region)
    int clicks = 0;          // 0: a box alone; else the head's click and the clicks - 1 continuation entries behind it
    bool box = false;
    int points() const { return box ? clicks + 2 : clicks + 1; }       // packed points: the pad token takes the box's place
};

// has_handle[i]: entry i has a handle.  Throws std::invalid_argument with the message the caller reports.
inline std::vector<PromptSpec> plan_prompts(std::vector<char> const& has_handle, bool points_given, int const* regions) {
    const int count = (int)has_handle.size();
    std::vector<PromptSpec> prompts;
    bool any_continuation = false;
    for (int i = 0; i < count; ++i) any_continuation |= !has_handle[i];
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
            if (any_continuation && regions && regions[4 * i + 2] < regions[4 * i]) p.box = false;
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

// label of click c (0: the head's own) of a prompt
inline int click_label(PromptSpec const& p, int c, int const* regions) {
    return (c == 0 || !regions) ? 1 : regions[4 * (p.head + c)];
}

struct PromptChunk {
    int points = 0;                  // packed points of every prompt of the chunk
    std::vector<int> prompts;        // indices into the call's prompt list, caller's order
};

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
