// ASan + UBSan harness for csrc/lasso_plan.hpp (tests/test_lasso_ref.py): plan_lasso_prompts on 120 000 random batch mask calls
// of 1 to 24 entries -- handles, clicks, refinement, clean-up, grid, prior and lasso marks, now and then a bad one or one out of
// place, NULL selections, with any combination of the two arrays -- with the invariants the batch calls rely on checked on every
// call that is served: a lasso belongs to exactly the prompt whose head stands directly in front of its mark, its `what` and
// strength are in range, its pointer is there, the derived click and box are reserved (and the click is the first of the first
// stage), the prompt stays within 8 clicks, no prompt has a prior and a lasso or a grid and a lasso, lasso_prompt_arrays and
// pack_points stay inside their arrays for every stage, fold_lasso_rows on random row records stays inside the image, and a call
// without lasso marks is planned (or refused) as plan_prior_prompts does it.
#include "lasso_plan.hpp"

#include <cstdint>
#include <cstdio>

using namespace dlimg;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % (n ? n : 1));
}

static bool same(PriorPlannedPrompts const& a, PriorPlannedPrompts const& b) {
    StagedPrompts const& x = a.planned.cleaned.staged;
    StagedPrompts const& y = b.planned.cleaned.staged;
    if (x.prompts.size() != y.prompts.size() || a.any_prior != b.any_prior || a.planned.any_grid != b.planned.any_grid ||
        a.planned.cleaned.any_clean != b.planned.cleaned.any_clean)
        return false;
    for (size_t j = 0; j < x.prompts.size(); ++j) {
        if (x.prompts[j].head != y.prompts[j].head || x.prompts[j].clicks != y.prompts[j].clicks || x.prompts[j].box != y.prompts[j].box) return false;
        if (x.stages[j].click_entry != y.stages[j].click_entry || x.stages[j].stage_clicks != y.stages[j].stage_clicks) return false;
        if (a.prior[j].entry != b.prior[j].entry || a.prior[j].strength_milli != b.prior[j].strength_milli) return false;
        if (a.planned.grid[j].side != b.planned.grid[j].side) return false;
        if (a.planned.cleaned.clean[j].max_hole != b.planned.cleaned.clean[j].max_hole) return false;
    }
    return true;
}

static const char* once(int* served, int* with_lasso) {
    const int count = 1 + (int)rnd(24);
    std::vector<char> has_handle(count), has_pointer(count);
    std::vector<int> regions(4 * count, 0), points(2 * count);
    for (int& v : points) v = (int)rnd(4000);
    const bool points_given = rnd(4) != 0, regions_given = rnd(8) != 0, branch = rnd(10) != 0, device = rnd(25) == 0;
    const bool lassos = rnd(4) != 0;
    for (int i = 0; i < count; ++i) {
        has_handle[i] = i == 0 ? rnd(30) != 0 : rnd(3) == 0;
        has_pointer[i] = rnd(20) != 0;
        int* r = &regions[4 * i];
        if (has_handle[i]) {
            r[0] = (int)rnd(2000); r[1] = (int)rnd(2000);
            r[2] = rnd(3) == 0 ? r[0] + (int)rnd(2000) : -1; r[3] = rnd(2) ? r[1] + (int)rnd(2000) : -1;
            continue;
        }
        const uint32_t kind = rnd(16);
        const bool behind_head = i > 0 && has_handle[i - 1];
        if (lassos && (behind_head ? kind < 8 : kind == 0)) {
            r[0] = kLassoMark;
            r[2] = rnd(30) ? (int)rnd(8) : (int)rnd(20) - 5;
            const bool mask_bit = r[2] == 0 || (r[2] > 0 && r[2] < 8 && (r[2] & kLassoMask));
            r[1] = (!mask_bit && rnd(12)) || rnd(4) == 0 ? 0 : rnd(30) ? 1 + (int)rnd(kPriorMaxStrength) : (int)rnd(400000) - 200000;
            if (!rnd(40)) r[3] = 1 + (int)rnd(3);
        } else if (kind == 8) {
            r[0] = kRefineMark;
        } else if (kind == 9) {
            r[0] = kCleanMark; r[1] = (int)rnd(50); r[2] = (int)rnd(50);
        } else if (kind == 10) {
            r[0] = kGridMark; r[1] = (int)rnd(36); r[2] = (int)rnd(1000); r[3] = (int)rnd(1000);
        } else if (kind == 11) {
            r[0] = kPriorMark; r[1] = (int)rnd(20000);
        } else {
            r[0] = rnd(40) ? (int)rnd(2) : (int)rnd(14) - 2;
            if (!rnd(60)) r[1 + rnd(3)] = 1 + (int)rnd(3);
        }
    }
    int const* reg = regions_given ? regions.data() : nullptr;
    bool any_lasso = false;
    for (int i = 0; i < count; ++i) any_lasso |= !has_handle[i] && reg && reg[4 * i] == kLassoMark;
    LassoPlannedPrompts plan;
    try {
        plan = plan_lasso_prompts(has_handle, points_given, reg, branch, has_pointer, device);
    } catch (std::invalid_argument const& e) {
        if (!any_lasso) {
            try {
                plan_prior_prompts(has_handle, points_given, reg, branch, has_pointer, device);
                return "a call without lasso marks is refused, and plan_prior_prompts serves it";
            } catch (std::invalid_argument const& g) {
                if (std::string(e.what()) != g.what()) return "a call without lasso marks is refused in other words";
            }
        }
        return nullptr;
    }
    ++*served;
    StagedPrompts const& st = plan.inner.planned.cleaned.staged;
    if (st.prompts.empty() || st.stages.size() != st.prompts.size() || plan.lasso.size() != st.prompts.size() ||
        plan.inner.prior.size() != st.prompts.size() || plan.inner.planned.grid.size() != st.prompts.size())
        return "a vector per prompt has another length";
    if (plan.any_lasso != any_lasso) return "any_lasso";
    if (!any_lasso) {
        if (!same(plan.inner, plan_prior_prompts(has_handle, points_given, reg, branch, has_pointer, device))) return "a call without lasso marks is planned differently";
        for (LassoSpec const& l : plan.lasso)
            if (l.any()) return "a lasso without a mark";
        return nullptr;
    }
    if (device) return "a lasso mark is served by the device form";
    int marks = 0, found = 0;
    for (int i = 0; i < count; ++i) marks += !has_handle[i] && reg[4 * i] == kLassoMark;
    for (size_t j = 0; j < st.prompts.size(); ++j) {
        PromptSpec const& p = st.prompts[j];
        PromptStages const& stages = st.stages[j];
        LassoSpec const& l = plan.lasso[j];
        if (p.head < 0 || p.head >= count || !has_handle[p.head] || (j && p.head <= st.prompts[j - 1].head)) return "heads";
        const bool marked = p.head + 1 < count && !has_handle[p.head + 1] && reg[4 * (p.head + 1)] == kLassoMark;
        if (l.any() != marked) return "a lasso without its mark, or a mark without its lasso";
        if (plan.inner.prior[j].any() && (plan.inner.prior[j].entry <= p.head || plan.inner.prior[j].entry >= count ||
                                          reg[4 * plan.inner.prior[j].entry] != kPriorMark))
            return "a prior's entry";
        if ((int)stages.click_entry.size() != p.clicks || stages.stage_clicks.empty() || stages.stage_clicks.back() != p.clicks) return "stages";
        for (size_t c = 0; c < stages.click_entry.size(); ++c) {
            const int e = stages.click_entry[c];
            if (l.any() && l.click() && c == 0) {
                if (e != l.entry) return "the derived click is not the first";
                continue;
            }
            if (e < p.head || e >= count || (e != p.head && (has_handle[e] || reg[4 * e] > 1 || reg[4 * e] < 0))) return "a mark read as a click";
        }
        if (!l.any()) continue;
        ++found;
        ++*with_lasso;
        if (l.entry != p.head + 1 || !has_pointer[l.entry]) return "the lasso's entry";
        const int* r = reg + 4 * l.entry;
        if (l.what < 1 || l.what > 7 || l.what == kLassoMask || l.what != (r[2] ? r[2] : 7) || r[3]) return "what";
        if (l.mask() ? (!branch || l.strength_milli != (r[1] ? r[1] : kPriorDefaultStrength) || l.strength_milli < 1 ||
                        l.strength_milli > kPriorMaxStrength)
                     : (l.strength_milli != 0 || r[1] != 0))
            return "strength";
        const bool own_box = !(reg[4 * p.head + 2] < reg[4 * p.head]);
        if (l.box() && own_box) return "two boxes";
        if (p.box != (l.box() || own_box)) return "the box is not reserved";
        if (p.clicks > kMaxClicks || p.clicks < (l.click() ? 1 : 0) || (p.clicks == 0 && !p.box)) return "clicks";
        if (l.click() && stages.stage_clicks.front() < (points_given ? 2 : 1)) return "the derived click is not in the first stage";
        if (plan.inner.planned.grid[j].any() || plan.inner.prior[j].any()) return "a grid prompt or a prior with a lasso";
        // the prompt as it is packed once a record is there
        const int32_t record[kLassoRecordInts] = {1, 3, 4, 50, 60, 20, 30, 9};
        const LassoPromptArrays own = lasso_prompt_arrays(p, stages, l, points_given ? points.data() : nullptr, reg, record);
        ResizeLongestSide rs;
        rs.set(Extent{4000, 3000});
        for (int k : own.stages.stage_clicks) {
            std::vector<float> coords(2 * (size_t)(k + 2)), labels((size_t)k + 2);       // exactly what the stage needs: ASan watches the rest
            const int n = pack_points(rs, own.spec, own.stages, k, own.points.data(), own.regions.data(), coords.data(), labels.data());
            if (n != k + (p.box ? 2 : 1)) return "packed points";
            if (l.click() && (labels[0] != 1.f || coords[0] != float(rs.transform(Point{20, 30}).x))) return "the derived click is not packed first";
            if (l.box() && (labels[n - 2] != 2.f || coords[2 * (n - 2)] != float(rs.transform(Point{3, 4}).x))) return "the derived box is not packed";
        }
    }
    if (found != marks) return "a lasso mark that belongs to no prompt";
    return nullptr;
}

static const char* fold_once() {
    const int W = 1 + (int)rnd(4000), H = 1 + (int)rnd(4000);
    const int longest = W > H ? W : H;
    const float scale = 1024.f / float(longest);
    const int pre_w = longest == 1024 ? W : int(float(W) * scale + 0.5f), pre_h = longest == 1024 ? H : int(float(H) * scale + 0.5f);
    if (pre_w < 1 || pre_h < 1) return nullptr;
    const int sw = (pre_w + 3) / 4, sh = (pre_h + 3) / 4;
    std::vector<int32_t> rows((size_t)kLassoRows * kLassoRowRecordInts, 0);
    bool any = false;
    for (int y = 0; y < sh; ++y) {
        if (rnd(3)) continue;
        const int a = (int)rnd(sw), b = a + (int)rnd(sw - a);
        int32_t* r = &rows[(size_t)y * kLassoRowRecordInts];
        r[0] = b - a + 1; r[1] = a; r[2] = b; r[3] = a + (int)rnd(b - a + 1); r[4] = 1 + (int)rnd(16384);
        any = true;
    }
    int32_t record[kLassoRecordInts];
    fold_lasso_rows(rows.data(), W, H, pre_w, pre_h, record);
    if (!any) return record[0] == 0 && record[7] == 0 ? nullptr : "an empty selection with a record";
    if (record[0] < 1 || record[7] < 1) return "a selection without a record";
    if (!(0 <= record[1] && record[1] <= record[5] && record[5] < record[3] && record[3] <= W)) return "the click or the box leaves the image (x)";
    if (!(0 <= record[2] && record[2] <= record[6] && record[6] < record[4] && record[4] <= H)) return "the click or the box leaves the image (y)";
    return nullptr;
}

int main() {
    int served = 0, with_lasso = 0;
    for (int iter = 0; iter < 120000; ++iter)
        if (const char* bad = once(&served, &with_lasso)) { std::printf("lasso plan: %s (iteration %d)\n", bad, iter); return 1; }
    for (int iter = 0; iter < 20000; ++iter)
        if (const char* bad = fold_once()) { std::printf("lasso fold: %s (iteration %d)\n", bad, iter); return 1; }
    std::printf("served %d calls, %d lassos\n", served, with_lasso);
    if (served < 8000 || with_lasso < 3000) { std::printf("lasso plan: only %d calls served, %d lassos\n", served, with_lasso); return 1; }
    std::printf("ok\n");
    return 0;
}
