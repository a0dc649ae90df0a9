"""Prior marks on the CPU: a caller's mask as SAM's mask input.

* the definition (tests/prior_ref.py, the numpy restatement of k::mask_prior): pushed through the oracle's post-processing the
  plane gives back the mask it was made from in all but 2e-3 of the pixels, at every extent the GPU test runs and two tiny ones;
  the footprints of an axis are never empty, never leave the mask and leave no source column out, for every width and every
  encoded width from 1 to 1100;
* the inputs of the GPU tests (tests/prior_cases.py): for every case the float64 reference mask with the prior differs from
  the reference of the same prompt without it in at least ten times what the GPU tests let a mask disagree in, so do two
  different priors on one prompt, and where the first stage is a two-point prompt its best plane among 1 .. 3 leads by at least
  ten times the tolerance the IoU predictions of this model are held to -- otherwise the GPU could pick another plane;
* the planner (csrc/prior_plan.hpp, printed by tests/prior_plan_cases.cpp, built with the host compiler): entry lists, every
  refusal with the caller's entry number, priors beside grid, clean-up and refinement marks, and a call without prior marks
  printing what tests/grid_plan_cases.cpp prints for it;
* the wrappers: dlimgedit_amd.api.click_entries with priors, and the C++ wrapper's Prior compiles against DLIMG_PRIOR_MARK == 8;
* csrc/prior_plan.hpp on random entry lists under ASan + UBSan, as a stand-alone program (tests/sanitize/prior_plan_fuzz.cpp).
"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import prior_cases as PC
import prior_ref
from conftest import IOU_PRED_TOL
from dlimgedit_amd import api
from dlimgedit_amd import weights as W
from dlimgedit_amd.sam_config import get_config
from oracle import sam_oracle as O

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dlimgedit_amd" / "csrc"
P = api.Point
ROUND_TRIP_LIMIT = 2e-3
EMPTY = "0,0,-1,-1"


# ---- the definition

@pytest.mark.parametrize("extent", [(1024, 1024), (800, 600), (600, 400), (333, 1000), (4000, 3000), (2047, 1025), (5, 3), (61, 47)],
                         ids=lambda e: f"{e[0]}x{e[1]}")
def test_round_trip_through_the_post_processing(extent):
    w, h = extent
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    mask = ((xx - 0.45 * w) / (0.3 * w)) ** 2 + ((yy - 0.5 * h) / (0.35 * h)) ** 2 <= 1.0
    mask |= (xx >= 0.6 * w) & (xx < 0.9 * w) & (yy >= 0.1 * h) & (yy < 0.45 * h)
    pre_w, pre_h = prior_ref.pre_extent(w, h)
    plane = prior_ref.prior_plane(np.where(mask, 255, 0).astype(np.uint8), pre_w, pre_h, prior_ref.DEFAULT_STRENGTH)
    assert plane.dtype == np.float32 and plane.shape == (256, 256) and not (plane.view(np.uint32) == 0x80000000).any()
    assert np.abs(plane).max() == np.float32(8.0)
    back = O.postprocess_logits(plane, (h, w)) > 0
    fraction = float((back != mask).mean())
    print(f"prior.round_trip.{w}x{h}: {int((back != mask).sum())} of {mask.size} pixels differ: fraction {fraction:.3g}")
    assert fraction <= ROUND_TRIP_LIMIT
    if max(w, h) < 100:
        assert fraction == 0.0


def test_footprints_are_never_empty_and_cover_every_column():
    sizes = np.arange(1, 1101, dtype=np.int64)[:, None]
    for pre in range(1, 1101):
        i = np.arange((pre + 3) // 4, dtype=np.int64)[None, :]
        lo = 4 * i * sizes // pre
        hi = (np.minimum(4 * i + 4, pre) * sizes + pre - 1) // pre
        assert (lo < hi).all() and (hi <= sizes).all(), pre
        # the union covers every column: it starts at 0, ends at the size, and no footprint starts behind the end of the one before
        assert (lo[:, 0] == 0).all() and (hi[:, -1] == sizes[:, 0]).all() and (lo[:, 1:] <= hi[:, :-1]).all(), pre
    lo, hi = prior_ref.footprints(4000, 1024)
    assert (hi - lo).max() == 17 and len(lo) == 256          # the largest footprint at 4000 x 3000
    lo, hi = prior_ref.footprints(800, 1024)
    assert (lo[1:] < hi[:-1]).any()                           # neighbouring footprints share a source column


def test_strength_and_padding():
    mask = np.zeros((600, 800), np.uint8)
    mask[100:300, 200:500] = 255
    mask[300:400, 200:500] = 128                              # coverage counts: about half
    for strength in (1, 2500, 100000):
        s = np.float32(strength) / np.float32(1000)
        plane = prior_ref.prior_plane(mask, 1024, 768, strength)
        assert (plane[192:] == -s).all() and plane[40, 90] == s and plane[20, 20] == -s
        assert plane[110, 90] == (np.float32(2 * 128 - 255) / np.float32(255)) * s
    assert prior_ref.pre_extent(800, 600) == (1024, 768)


# ---- the inputs of the GPU tests

@pytest.fixture(scope="module")
def oracle_segs():
    cfg = get_config("vit_test")
    params = W.synthetic_weights(cfg, 7, mask_branch=True)
    return {name: O.OracleSegmentation(params, cfg).process(PC.image(name), O.CH_RGBA) for name in PC.IMAGES}, params


@pytest.fixture(scope="module")
def references(oracle_segs):
    """case index -> (mask with the prior, its plane, the first stage's IoU predictions, mask without the prior)"""
    segs, params = oracle_segs
    out = {}
    for i, case in enumerate(PC.CASES):
        seg = segs[case[0]]
        w, h = seg.rs.original
        out[i] = PC.reference(seg.embedding, seg.rs, case, params, (h, w)) + (PC.reference_without(seg.embedding, seg.rs, case, params, (h, w)),)
    return out


def test_cases_cover_what_the_issue_names():
    rows = {PC.NAMES[i]: PC.token_rows(c) for i, c in enumerate(PC.CASES)}
    a, b, c, d, e, f, g = PC.CASES
    assert rows["a"] == [7] and a[0] == "square" and len(a[1]) == 1 and a[3] is None
    assert rows["b"] == [7] and len(b[1]) == 0 and b[3] is not None and b[4][5] > 0          # a box alone, soft-edged prior
    assert 0 < ((PC.draw_prior(b[0], b[4]) > 0) & (PC.draw_prior(b[0], b[4]) < 255)).mean() < 0.2
    assert rows["c"] == [7] and c[0] == "wide"
    assert rows["d"] == [9] and d[0] == "wide" and len(d[1]) == 3
    assert rows["e"] == [8] and e[0] == "wide" and len(e[1]) == 1 and e[3] is not None
    assert rows["f"] == [7, 8] and f[5] == (1,)
    assert g[:6] == a[:6] and g[6] is not None and a[6] is None
    assert PC.EXACT_LIMIT < PC.CHAIN_LIMIT < 2e-3


@pytest.mark.parametrize("i", range(len(PC.CASES)), ids=[PC.case_id(c) for c in PC.CASES])
def test_the_prior_moves_the_reference_mask(references, i):
    case = PC.CASES[i]
    mask, plane, iou, without = references[i]
    fraction = float((mask != without).mean())
    print(f"prior.with_without.{PC.case_id(case)}: fraction {fraction:.4g}, plane {plane}, first-stage IoU predictions {np.round(iou, 4)}")
    assert fraction >= 10 * PC.limit_of(case)
    assert 0.02 < mask.mean() < 0.98
    if PC.first_stage_is_two_point(case):
        best = np.sort(iou[1:])[::-1]
        assert best[0] - best[1] >= 10 * IOU_PRED_TOL, "another plane is too close: the GPU might pick it"
    assert plane == (0 if PC.token_rows(case)[-1] > 7 else int(np.argmax(iou[1:])) + 1)


def test_two_priors_on_one_prompt_differ(oracle_segs, references):
    segs, params = oracle_segs
    case = PC.CASES[0]
    seg = segs[case[0]]
    w, h = seg.rs.original
    other, _, iou = PC.reference(seg.embedding, seg.rs, case, params, (h, w), PC.OTHER_PRIOR)
    fraction = float((other != references[0][0]).mean())
    print(f"prior.two_priors: fraction {fraction:.4g}")
    assert fraction >= 10 * PC.EXACT_LIMIT
    best = np.sort(iou[1:])[::-1]
    assert best[0] - best[1] >= 10 * IOU_PRED_TOL


# ---- the planner

def _cxx():
    rocm_clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    cxx = str(rocm_clang) if rocm_clang.exists() else (shutil.which("c++") or shutil.which("g++") or shutil.which("clang++"))
    assert cxx, "no host C++ compiler found"
    return cxx


def _build(tmp, name):
    exe = tmp / name
    r = subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(ROOT / "tests" / f"{name}.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def planners(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("prior_plan")
    prior, grid = _build(tmp, "prior_plan_cases"), _build(tmp, "grid_plan_cases")

    def run(entries, points=1, regions=1, branch=1, device=0, exe="prior"):
        head = [str(prior), points, regions, branch, device] if exe == "prior" else [str(grid), "plan", points, regions, branch]
        r = subprocess.run([str(a) for a in head] + list(entries), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def test_planner_reads_prior_marks(planners):
    # one click and a prior; a box and a click without one
    assert planners([f"h:{EMPTY}", "c:8,0,0,0", "h:1,2,30,40"]) == [
        "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0 prior 1,8000",
        "prompt 2 clicks 1 box 1 points 3 entries 2 stages 1 clean 0,0 grid 0,0,0", "any_clean 0", "any_grid 0", "any_prior 1"]
    # a box alone with a prior needs no points; the strength travels
    assert planners(["h:1,2,30,40", "c:8,2500,0,0"], points=0) == [
        "prompt 0 clicks 0 box 1 points 2 entries stages 0 clean 0,0 grid 0,0,0 prior 1,2500", "any_clean 0", "any_grid 0", "any_prior 1"]
    # beside refinement, clean-up and grid marks: the click entries skip the prior mark, the stages are those of the marks
    assert planners([f"h:{EMPTY}", "c:8,100000,0,0", "c:4,0,0,0", "c:0,0,0,0", "c:6,5,7,0", f"h:{EMPTY}", "c:7,4,0,0", "h:3,3,9,9", "c:8,1,0,0",
                     "c:1,0,0,0"]) == [
        "prompt 0 clicks 2 box 0 points 3 entries 0,3 stages 1,2 clean 5,7 grid 0,0,0 prior 1,100000",
        "prompt 5 clicks 1 box 0 points 2 entries 5 stages 1 clean 0,0 grid 4,0,0",
        "prompt 7 clicks 2 box 1 points 4 entries 7,9 stages 2 clean 0,0 grid 0,0,0 prior 8,1", "any_clean 1", "any_grid 1", "any_prior 1"]
    # a prior mark makes the call one with continuation entries: the empty region of ANOTHER head is "no box" too
    assert planners([f"h:{EMPTY}", "h:1,1,5,5", "c:8,0,0,0"])[0] == "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0"


REFUSALS = [
    (["c:8,0,0,0", f"h:{EMPTY}"], {}, 0, "needs a prompt in front"),
    ([f"h:{EMPTY}", "c:1,0,0,0", "c:8,0,0,0"], {}, 2, "does not directly follow its head"),
    ([f"h:{EMPTY}", "c:4,0,0,0", "c:8,0,0,0", "c:1,0,0,0"], {}, 2, "does not directly follow its head"),
    ([f"h:{EMPTY}", "h:1,1,5,5", "c:8,0,0,0!"], {}, 2, "NULL"),
    ([f"h:{EMPTY}", "c:8,-1,0,0"], {}, 1, "strength_milli"),
    ([f"h:{EMPTY}", "c:8,100001,0,0"], {}, 1, "strength_milli"),
    ([f"h:{EMPTY}", "c:8,0,1,0"], {}, 1, "other two ints are 0"),
    ([f"h:{EMPTY}", "c:8,0,0,7"], {}, 1, "other two ints are 0"),
    ([f"h:{EMPTY}", "h:1,1,5,5", "c:8,0,0,0", "c:8,0,0,0"], {}, 3, "second"),
    ([f"h:{EMPTY}", "c:8,0,0,0"], {"branch": 0}, 1, r"pe\.mask"),
    ([f"h:{EMPTY}", "h:" + EMPTY, "c:8,0,0,0", "c:7,4,0,0"], {}, 2, "grid prompt"),
    ([f"h:{EMPTY}", "c:8,0,0,0"], {"device": 1}, 1, "dlimg_amd_get_segmentation_masks_device"),
    ([f"h:1,1,5,5", f"h:{EMPTY}", "c:8,0,0,0"], {"points": 0}, 2, "still needs a click or a box"),
]


@pytest.mark.parametrize("entries,how,entry,why", REFUSALS, ids=[f"{i}-{r[3][:24].replace(' ', '_')}" for i, r in enumerate(REFUSALS)])
def test_planner_refusals_name_the_mark_and_the_callers_entry(planners, entries, how, entry, why):
    import re
    out = planners(entries, **how)
    assert len(out) == 1 and out[0].startswith(f"error mask batch: entry {entry}: a prior mark "), out
    assert re.search(why, out[0]), out


def test_refusals_of_the_inner_planners_keep_the_callers_numbering(planners):
    # entries behind a prior mark are renumbered back: the bad label is the caller's entry 3, the misplaced grid mark its entry 4
    out = planners([f"h:{EMPTY}", "c:8,0,0,0", "c:1,0,0,0", "c:5,0,0,0"])
    assert out[0].startswith("error mask batch: entry 3:") and "label" in out[0]
    out = planners([f"h:{EMPTY}", "c:8,0,0,0", "h:" + EMPTY, "c:1,0,0,0", "c:7,4,0,0"])
    assert out[0].startswith("error mask batch: entry 4: a grid mark"), out
    out = planners([f"h:{EMPTY}", "c:8,0,0,0", "c:6,1,1,0", "c:1,0,0,0"])
    assert out[0].startswith("error mask batch: entry 2: a clean-up mark"), out


def test_a_call_without_prior_marks_is_planned_as_before(planners):
    calls = [([f"h:{EMPTY}", "c:1,0,0,0", "h:1,2,30,40", "c:0,0,0,0", "c:6,3,4,0"], {}),
             (["h:1,2,30,40", "h:5,5,1,1"], {}), (["h:1,2,30,40"], {"points": 0}), (["h:0,0,0,0", "h:0,0,0,0"], {"regions": 0}),
             ([f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0", f"h:{EMPTY}", "c:7,8,900,0"], {}),
             ([f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0"], {"branch": 0}), (["c:1,0,0,0"], {}), ([f"h:{EMPTY}", "c:9,0,0,0"], {}),
             ([f"h:{EMPTY}", "c:5,0,0,0"], {}), ([f"h:{EMPTY}", "c:1,0,0,0"], {"regions": 0})]
    for entries, how in calls:
        assert planners(entries, **how) == planners(entries, exe="grid", **how), (entries, how)
    # 8 is no label where there are no `regions` to hold a mark, and the device form serves every call without one
    assert planners([f"h:{EMPTY}", "c:1,0,0,0"], device=1) == planners([f"h:{EMPTY}", "c:1,0,0,0"], exe="grid")


# ---- the wrappers

def test_click_entries_with_priors():
    r = api.Region(P(10, 20), P(300, 400))
    m0, m2 = np.zeros((4, 6), np.uint8), np.ones((4, 6), np.uint8)
    e = api.click_entries([[P(1, 2), P(3, 4), P(5, 6)], [P(7, 8)], [P(9, 10), P(11, 12)]], [[1, 0, 1], None, [1, 0]], [None, r, r],
                          [[1], None, None], [None, None, (3, 4)], prior=[m0, None, m2], prior_strength=[0, 0, 2500])
    assert api.PRIOR_MARK == 8
    assert e.heads == [0, None, None, None, None, 1, 2, None, None, None]
    assert e.regions == [api.EMPTY_REGION, (8, 0, 0, 0), (4, 0, 0, 0), (0, 0, 0, 0), (1, 0, 0, 0), (10, 20, 300, 400), (10, 20, 300, 400),
                         (8, 2500, 0, 0), (0, 0, 0, 0), (6, 3, 4, 0)]
    assert e.points[1] == (0, 0) and e.points[3] == (3, 4) and e.prompt_heads == [0, 5, 6]
    assert e.token_rows == [9, 8, 9] and e.stage_clicks == [[1, 3], [1], [2]]
    assert e.priors[0] is m0 and e.priors[1] is None and e.priors[2] is m2
    # a prompt with a prior is decoded on its own, stage by stage, its first stage included
    assert e.launches == [(8, [1]), (7, [0]), (9, [0]), (9, [2])]
    assert api._entry_calls(e) == [(list(range(10)), True)]
    # a single click with a prior is a call with a continuation entry
    one = api.click_entries([[P(1, 2)]], prior=[m0])
    assert one.heads == [0, None] and one.regions == [api.EMPTY_REGION, (8, 0, 0, 0)] and api._entry_calls(one) == [([0, 1], True)]
    # entry lists without priors are what they were
    a = api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r])
    assert a == api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], prior=None) == api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], prior=[None])
    assert a.priors == []
    # the `points` / `regions` form: the prior mark directly behind its head, in front of the clean-up mark
    pr = api._checked_prior([m0, None], 700, 2)
    heads, pts, regs = api._marked_entries(2, None, [r, r], [(3, 0), None], None, pr)
    assert heads == [0, None, None, 1] and pts is None and regs == [(10, 20, 300, 400), (8, 700, 0, 0), (6, 3, 0, 0), (10, 20, 300, 400)]
    for bad in (dict(prior=[m0.astype(np.int32)]), dict(prior=[m0[:, ::2]]), dict(prior=[m0], prior_strength=-1),
                dict(prior=[m0], prior_strength=100001), dict(prior=[m0, m0]), dict(prior=[m0], prior_strength=[1, 2]),
                dict(prior=[np.zeros(24, np.uint8)])):
        with pytest.raises(api.Error):
            api.click_entries([[P(1, 2)]], **bad)
    with pytest.raises(api.Error):
        api.click_entries([None], grid=[(4, 0, 0)], prior=[m0])


def test_cpp_wrapper_compiles_with_a_prior(tmp_path):
    src = tmp_path / "consumer.cpp"
    src.write_text("""
#include <dlimgedit/dlimgedit.hpp>
static_assert(DLIMG_PRIOR_MARK == 8, "the prior mark of table slot 14");
dlimg::Image refine(dlimg::Segmentation const& seg, dlimg::Image& last) {
    dlimg::Prior prior{last.pixels(), 0};
    dlimg::Image once = seg.compute_mask({dlimg::Click{dlimg::Point{10, 20}, true}}, std::nullopt, {}, std::nullopt, prior);
    std::vector<std::optional<dlimg::Prior>> priors{dlimg::Prior{once.pixels(), 2500}, std::nullopt};
    auto both = dlimg::Segmentation::compute_mask_batch({&seg, &seg}, std::vector<std::vector<dlimg::Click>>{{{dlimg::Point{1, 2}}}, {{dlimg::Point{3, 4}}}},
                                                        {}, {}, {}, priors);
    return std::move(both[0]);
}
int main() { return 0; }
""")
    r = subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", "-DDLIMGEDIT_LOAD_DYNAMIC", f"-I{ROOT / 'include'}", "-fsyntax-only",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_planner_on_random_entry_lists_under_address_sanitizer(tmp_path):
    """csrc/prior_plan.hpp on 120 000 random batch mask calls with ASan + UBSan, every served call checked against what the
    batch calls rely on (tests/sanitize/prior_plan_fuzz.cpp): a stand-alone program on the CPU."""
    clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    if not clang.exists():
        pytest.skip("ROCm clang not found")
    exe = tmp_path / "prior_plan_fuzz"
    r = subprocess.run([str(clang), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", f"-I{CSRC}", str(ROOT / "tests" / "sanitize" / "prior_plan_fuzz.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and "sanitizer" in (r.stderr + r.stdout).lower() and "cannot find" in (r.stderr + r.stdout).lower():
        pytest.skip("this clang has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, errors="replace", timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
