// ASan + UBSan harness for csrc/prior_plan.hpp (tests/test_prior_ref.py): plan_prior_prompts on 120 000 random
// batch mask calls of 1 to 24 entries -- handles, clicks, refinement, clean-up, grid and prior marks, now and then a bad one or
// one out of place, NULL priors, with any combination of the two arrays -- with the invariants the batch calls rely on checked
// on every call that is served: a prior belongs to exactly the prompt whose head stands directly in front of its mark, its
// strength is in range, its pointer is there, a grid prompt has none, a prompt with one still has a click or a box, no prior
// mark is read as a click, and a call without prior marks is planned as plan_grid_prompts plans it.
#include "prior_plan.hpp"

#include <cstdint>
#include <cstdio>

using namespace dlimg;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % (n ? n : 1));
}

static bool same(GridPlannedPrompts const& a, GridPlannedPrompts const& b) {
    StagedPrompts const& x = a.cleaned.staged;
    StagedPrompts const& y = b.cleaned.staged;
    if (x.prompts.size() != y.prompts.size() || a.any_grid != b.any_grid || a.cleaned.any_clean != b.cleaned.any_clean) return false;
    for (size_t j = 0; j < x.prompts.size(); ++j) {
        if (x.prompts[j].head != y.prompts[j].head || x.prompts[j].clicks != y.prompts[j].clicks || x.prompts[j].box != y.prompts[j].box) return false;
        if (x.stages[j].click_entry != y.stages[j].click_entry || x.stages[j].stage_clicks != y.stages[j].stage_clicks) return false;
        if (a.cleaned.clean[j].max_hole != b.cleaned.clean[j].max_hole || a.cleaned.clean[j].max_island != b.cleaned.clean[j].max_island) return false;
        if (a.grid[j].side != b.grid[j].side || a.grid[j].iou_permille != b.grid[j].iou_permille || a.grid[j].stability_permille != b.grid[j].stability_permille) return false;
    }
    return true;
}

static const char* once(int* served, int* with_prior) {
    const int count = 1 + (int)rnd(24);
    std::vector<char> has_handle(count), has_pointer(count);
    std::vector<int> regions(4 * count, 0);
    const bool points_given = rnd(6) != 0, regions_given = rnd(8) != 0, branch = rnd(10) != 0, device = rnd(25) == 0;
    const bool priors = rnd(4) != 0;
    for (int i = 0; i < count; ++i) {
        has_handle[i] = i == 0 ? rnd(30) != 0 : rnd(3) == 0;
        has_pointer[i] = rnd(20) != 0;
        int* r = &regions[4 * i];
        if (has_handle[i]) {
            r[0] = (int)rnd(2000); r[1] = (int)rnd(2000);
            r[2] = rnd(2) ? r[0] + (int)rnd(2000) : -1; r[3] = rnd(2) ? r[1] + (int)rnd(2000) : -1;
            continue;
        }
        const uint32_t kind = rnd(16);
        const bool behind_head = i > 0 && has_handle[i - 1];
        if (priors && (behind_head ? kind < 8 : kind == 0)) {
            r[0] = kPriorMark;
            r[1] = rnd(4) == 0 ? 0 : rnd(30) ? 1 + (int)rnd(kPriorMaxStrength) : (int)rnd(400000) - 200000;
            if (!rnd(40)) r[2 + rnd(2)] = 1 + (int)rnd(3);
        } else if (kind == 8) {
            r[0] = kRefineMark;
        } else if (kind == 9) {
            r[0] = kCleanMark; r[1] = (int)rnd(50); r[2] = (int)rnd(50);
        } else if (kind == 10) {
            r[0] = kGridMark; r[1] = (int)rnd(36); r[2] = (int)rnd(1000); r[3] = (int)rnd(1000);
        } else {
            r[0] = rnd(40) ? (int)rnd(2) : (int)rnd(12) - 2;
            if (!rnd(60)) r[1 + rnd(3)] = 1 + (int)rnd(3);
        }
    }
    int const* reg = regions_given ? regions.data() : nullptr;
    bool any_prior = false;
    for (int i = 0; i < count; ++i) any_prior |= !has_handle[i] && reg && reg[4 * i] == kPriorMark;
    PriorPlannedPrompts plan;
    try {
        plan = plan_prior_prompts(has_handle, points_given, reg, branch, has_pointer, device);
    } catch (std::invalid_argument const& e) {
        // a call without prior marks is refused exactly where plan_grid_prompts refuses it, with the same words
        if (!any_prior) {
            try {
                plan_grid_prompts(has_handle, points_given, reg, branch);
                return "a call without prior marks is refused, and plan_grid_prompts serves it";
            } catch (std::invalid_argument const& g) {
                if (std::string(e.what()) != g.what()) return "a call without prior marks is refused in other words";
            }
        }
        return nullptr;
    }
    ++*served;
    StagedPrompts const& st = plan.planned.cleaned.staged;
    if (st.prompts.empty() || st.stages.size() != st.prompts.size() || plan.prior.size() != st.prompts.size() ||
        plan.planned.grid.size() != st.prompts.size() || plan.planned.cleaned.clean.size() != st.prompts.size())
        return "a vector per prompt has another length";
    if (plan.any_prior != any_prior) return "any_prior";
    if (!any_prior) {
        if (!same(plan.planned, plan_grid_prompts(has_handle, points_given, reg, branch))) return "a call without prior marks is planned differently";
        for (PriorSpec const& p : plan.prior)
            if (p.any()) return "a prior without a mark";
        return nullptr;
    }
    if (device || !branch) return "a prior mark is served by the device form or without the mask branch";
    int marks = 0, found = 0;
    for (int i = 0; i < count; ++i) marks += !has_handle[i] && reg[4 * i] == kPriorMark;
    for (size_t j = 0; j < st.prompts.size(); ++j) {
        PromptSpec const& p = st.prompts[j];
        if (p.head < 0 || p.head >= count || !has_handle[p.head] || (j && p.head <= st.prompts[j - 1].head)) return "heads";
        for (int e : st.stages[j].click_entry)
            if (e < p.head || e >= count || (e != p.head && (has_handle[e] || reg[4 * e] == kPriorMark))) return "a mark read as a click";
        PriorSpec const& pr = plan.prior[j];
        const bool marked = p.head + 1 < count && !has_handle[p.head + 1] && reg[4 * (p.head + 1)] == kPriorMark;
        if (pr.any() != marked) return "a prior without its mark, or a mark without its prior";
        if (!pr.any()) continue;
        ++found;
        ++*with_prior;
        if (pr.entry != p.head + 1 || !has_pointer[pr.entry]) return "the prior's entry";
        const int given = reg[4 * pr.entry + 1];
        if (pr.strength_milli != (given ? given : kPriorDefaultStrength) || pr.strength_milli < 1 || pr.strength_milli > kPriorMaxStrength) return "strength";
        if (reg[4 * pr.entry + 2] || reg[4 * pr.entry + 3]) return "trailing ints";
        if (plan.planned.grid[j].any()) return "a grid prompt with a prior";
        if (p.clicks == 0 && !p.box) return "a prior alone";
    }
    if (found != marks) return "a prior mark that belongs to no prompt";
    return nullptr;
}

int main() {
    int served = 0, with_prior = 0;
    for (int iter = 0; iter < 120000; ++iter)
        if (const char* bad = once(&served, &with_prior)) { std::printf("prior plan: %s (iteration %d)\n", bad, iter); return 1; }
    std::printf("served %d calls, %d priors\n", served, with_prior);
    if (served < 8000 || with_prior < 4000) { std::printf("prior plan: only %d calls served, %d priors\n", served, with_prior); return 1; }
    std::printf("ok\n");
    return 0;
}
