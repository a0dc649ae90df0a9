"""Edge marks in the planner (csrc/edge_plan.hpp, printed by tests/edge_plan_cases.cpp, built with the host compiler): marks read
behind the clicks and the clean-up mark and in front of the matte mark, alone and with refinement, stroke, lasso, prior, matte and
cut-out marks in the same call; every refusal naming the mark and the caller's entry; the inner planners' refusals keeping the
caller's numbering; a call without edge marks printing what plan_cutout_prompts and tests/cutout_plan_cases.cpp print for it; the
device form accepted; the Python entry lists; the C++ wrapper's Edge; and the planner on random entry lists under ASan + UBSan, as
the stand-alone program it is.
"""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from dlimgedit_amd import api

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dlimgedit_amd" / "csrc"
EMPTY = "0,0,-1,-1"
P = api.Point


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
    tmp = tmp_path_factory.mktemp("edge_plan")
    edge, cutout = _build(tmp, "edge_plan_cases"), _build(tmp, "cutout_plan_cases")

    def run(entries, points=1, regions=1, branch=1, device=0, exe="edge"):
        head = {"edge": [str(edge), "edge"], "cutout": [str(edge), "cutout"], "cutout_cases": [str(cutout), "cutout"]}[exe]
        r = subprocess.run([str(a) for a in head + [points, regions, branch, device]] + list(entries), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def test_planner_reads_edge_marks(planners):
    # a click and an edge mark, the last entry of its prompt; the next prompt keeps the caller's numbers
    assert planners([f"h:{EMPTY}", "c:14,3,2,1", "h:1,2,30,40"]) == [
        "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0 edge 1,3,2,1",
        "prompt 2 clicks 1 box 1 points 3 entries 2 stages 1 clean 0,0 grid 0,0,0", "any_clean 0", "any_grid 0", "any_edge 1"]
    # on a box alone: the mark needs `regions` but no `points`, like a clean-up mark; the extremes of every value
    assert planners(["h:1,2,30,40", "c:14,-64,32,32"], points=0) == [
        "prompt 0 clicks 0 box 1 points 2 entries stages 0 clean 0,0 grid 0,0,0 edge 1,-64,32,32", "any_clean 0", "any_grid 0", "any_edge 1"]
    assert planners(["h:1,2,30,40", "c:14,64,0,0"], points=0)[0].endswith("edge 1,64,0,0")
    # the only continuation entry of its call: an empty region is still "no box"
    assert planners([f"h:{EMPTY}", "c:14,0,0,1"])[0] == "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0 edge 1,0,0,1"
    # behind clicks, a refinement mark and the clean-up mark; in front of the matte mark and its cut-out mark
    assert planners([f"h:{EMPTY}", "c:4,0,0,0", "c:0,0,0,0", "c:6,3,4,0", "c:14,5,0,0", "c:11,8,0,4", "c:13,0,0,0", f"h:{EMPTY}", "c:14,0,7,0",
                     "c:11,4,20,1"]) == [
        "prompt 0 clicks 2 box 0 points 3 entries 0,2 stages 1,2 clean 3,4 grid 0,0,0 matte 5,8,650,4 cutout 6,16 edge 4,5,0,0",
        "prompt 7 clicks 1 box 0 points 2 entries 7 stages 1 clean 0,0 grid 0,0,0 matte 9,4,20,1 edge 8,0,7,0",
        "any_clean 1", "any_grid 0", "any_matte 1", "any_cutout 1", "any_edge 1"]


def test_entries_keep_the_callers_numbers_with_every_other_mark_in_the_call(planners):
    # a prior, a lasso and a grid prompt beside prompts with edge marks
    out = planners([f"h:{EMPTY}", "c:14,1,0,0", f"h:{EMPTY}", "c:8,2500,0,0", "c:4,0,0,0", "c:1,0,0,0", "c:6,0,9,0", "c:14,-2,1,0", "c:11,16,650,4",
                    "c:13,7,0,0", f"h:{EMPTY}", "c:10,0,3,0", "c:14,2,2,2", "c:11,4,20,3", f"h:{EMPTY}", "c:7,8,900,0"])
    assert out[:4] == [
        "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0 edge 1,1,0,0",
        "prompt 2 clicks 2 box 0 points 3 entries 2,5 stages 1,2 clean 0,9 grid 0,0,0 prior 3,2500 matte 8,16,650,4 cutout 9,7 edge 7,-2,1,0",
        "prompt 10 clicks 2 box 1 points 4 entries 11,10 stages 2 clean 0,0 grid 0,0,0 lasso 11,3,0 matte 13,4,20,3 edge 12,2,2,2",
        "prompt 14 clicks 1 box 0 points 2 entries 14 stages 1 clean 0,0 grid 8,900,0"]
    # stroke marks: the plan speaks of the rewritten call (stroke_plan.hpp); the strokes', the cut-out's and the edge mark's entries
    # and entry_of are the caller's
    assert planners([f"h:{EMPTY}", "c:14,1,0,0", f"h:{EMPTY}", "c:1,0,0,0", "c:6,3,4,0", "c:14,5,0,0", "c:11,8,0,4", "c:13,0,0,0", f"h:{EMPTY}",
                     "c:12,2,1,0", "c:14,1,1,1"]) == [
        "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0 edge 1,1,0,0",
        "prompt 1 clicks 2 box 0 points 3 entries 1,2 stages 2 clean 3,4 grid 0,0,0 matte 4,8,650,4 cutout 7,16 edge 5,5,0,0",
        "prompt 5 clicks 3 box 0 points 4 entries 5,6,7 stages 3 clean 0,0 grid 0,0,0 stroke 9,1,2:6,7 edge 10,1,1,1",
        "any_clean 1", "any_grid 0", "any_matte 1", "any_stroke 1", "entry_of 0 2 3 4 6 8 9 9", "any_cutout 1", "any_edge 1"]
    # without `points` the first derived click is the head's own
    assert planners([f"h:{EMPTY}", "c:12,2,1,0", "c:14,-1,0,0", "c:11,4,0,3"], points=0)[0] == \
        "prompt 0 clicks 2 box 0 points 3 entries 0,1 stages 2 clean 0,0 grid 0,0,0 matte 2,4,650,3 stroke 1,1,2:0,1 edge 2,-1,0,0"


def test_the_device_form_serves_edge_marks(planners):
    assert planners([f"h:{EMPTY}", "c:1,0,0,0", "c:6,3,3,0", "c:14,3,0,0"], device=1) == [
        "prompt 0 clicks 2 box 0 points 3 entries 0,1 stages 2 clean 3,3 grid 0,0,0 edge 3,3,0,0", "any_clean 1", "any_grid 0", "any_edge 1"]
    # ... but not the matte mark behind one
    out = planners([f"h:{EMPTY}", "c:14,3,0,0", "c:11,8,0,4"], device=1)
    assert out[0].startswith("error mask batch: entry 2: a matte mark") and "dlimg_amd_get_segmentation_masks_device" in out[0], out


REFUSALS = [
    ([f"h:{EMPTY}", "c:14,65,0,0"], {}, 1, r"offset is -64 \.\. 64"),
    ([f"h:{EMPTY}", "c:14,-65,0,0"], {}, 1, r"offset is -64 \.\. 64"),
    ([f"h:{EMPTY}", "c:14,1,33,0"], {}, 1, r"feather is 0 \.\. 32"),
    ([f"h:{EMPTY}", "c:14,1,-1,0"], {}, 1, r"feather is 0 \.\. 32"),
    ([f"h:{EMPTY}", "c:14,1,0,33"], {}, 1, r"border is 0 \.\. 32"),
    ([f"h:{EMPTY}", "c:14,1,0,-1"], {}, 1, r"border is 0 \.\. 32"),
    ([f"h:{EMPTY}", "c:14,0,0,0"], {}, 1, "all 0"),
    ([f"h:{EMPTY}", "c:14,1,0,0", "c:14,2,0,0"], {}, 2, "second"),
    ([f"h:{EMPTY}", "c:14,1,0,0", "c:11,8,0,4", "c:14,2,0,0"], {}, 3, "second"),
    (["c:14,1,0,0", f"h:{EMPTY}"], {}, 0, "needs a prompt in front"),
    ([f"h:{EMPTY}", "c:14,1,0,0", "c:1,0,0,0"], {}, 1, "in front of entry 2"),                 # in front of a click
    ([f"h:{EMPTY}", "c:14,1,0,0", "c:12,2,1,0"], {}, 1, "in front of entry 2"),                # ... a stroke mark
    ([f"h:{EMPTY}", "c:1,0,0,0", "c:14,1,0,0", "c:4,0,0,0", "c:1,0,0,0"], {}, 2, "in front of entry 3"),      # ... a refinement mark
    ([f"h:{EMPTY}", "c:14,1,0,0", "c:6,3,3,0"], {}, 1, "in front of entry 2"),                 # ... the clean-up mark
    ([f"h:{EMPTY}", "c:14,1,0,0", "c:8,0,0,0"], {}, 1, "in front of entry 2"),                 # ... a prior mark
    ([f"h:{EMPTY}", "c:14,1,0,0", "c:7,4,0,0"], {}, 1, "in front of entry 2"),                 # ... a grid mark
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:14,1,0,0"], {}, 2, "behind a matte mark"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:13,0,0,0", "c:14,1,0,0"], {}, 3, "behind a matte mark"),
    ([f"h:{EMPTY}", "c:7,4,0,0", "c:14,1,0,0"], {}, 2, "grid prompt"),
    ([f"h:{EMPTY}", "c:7,4,0,0", "c:14,1,0,0"], {"device": 1}, 2, "grid prompt"),
    ([f"h:{EMPTY}", "c:14,1,0,0"], {"points": 0}, 1, "no prompt by itself"),
    ([f"h:{EMPTY}", "c:1,0,0,0", "h:1,2,30,40", "c:14,0,0,0"], {}, 3, "all 0"),
]


@pytest.mark.parametrize("entries,how,entry,why", REFUSALS, ids=[f"{i}-{re.sub('[^a-z0-9]+', '_', r[3][:24].lower())}" for i, r in enumerate(REFUSALS)])
def test_planner_refusals_name_the_mark_and_the_callers_entry(planners, entries, how, entry, why):
    out = planners(entries, **how)
    assert len(out) == 1 and out[0].startswith(f"error mask batch: entry {entry}: an edge mark "), out
    assert re.search(why, out[0]), out


def test_refusals_of_the_inner_planners_keep_the_callers_numbering(planners):
    out = planners([f"h:{EMPTY}", "c:14,1,0,0", f"h:{EMPTY}", "c:5,0,0,0"])
    assert out[0].startswith("error mask batch: entry 3:") and "label" in out[0], out
    out = planners([f"h:{EMPTY}", "c:14,1,0,0", f"h:{EMPTY}", "c:1,0,0,0", "c:8,0,0,0"])
    assert out[0].startswith("error mask batch: entry 4: a prior mark"), out
    out = planners([f"h:{EMPTY}", "c:14,1,0,0", "c:11,8,0,2"])
    assert out[0].startswith("error mask batch: entry 2: a matte mark") and "channels" in out[0], out
    out = planners([f"h:{EMPTY}", "c:14,1,0,0", "c:11,8,0,4!"])
    assert out[0].startswith("error mask batch: entry 2: a matte mark") and "NULL" in out[0], out
    # a cut-out mark directly behind the edge mark has no matte mark in front of it
    out = planners([f"h:{EMPTY}", "c:14,1,0,0", "c:13,8,0,0"])
    assert out[0].startswith("error mask batch: entry 2: a cut-out mark") and "directly behind a matte mark" in out[0], out
    out = planners([f"h:{EMPTY}", "c:14,1,0,0", "c:11,8,0,4", "c:13,8,0,0="])
    assert out[0].startswith("error mask batch: entry 3: a cut-out mark") and "head, entry 0" in out[0], out
    out = planners([f"h:{EMPTY}", "c:14,1,0,0", f"h:{EMPTY}", "c:12,2,1,0!"])
    assert out[0].startswith("error mask batch: entry 3: a stroke mark") and "NULL" in out[0], out
    out = planners([f"h:{EMPTY}", "c:14,1,0,0", f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0"], branch=0)
    assert out[0].startswith("error mask batch: entry 3:") and "mask" in out[0], out


def test_a_call_without_edge_marks_is_planned_as_before(planners):
    calls = [([f"h:{EMPTY}", "c:1,0,0,0", "h:1,2,30,40", "c:0,0,0,0", "c:6,3,4,0"], {}),
             (["h:1,2,30,40", "h:5,5,1,1"], {}), (["h:1,2,30,40"], {"points": 0}), (["h:0,0,0,0", "h:0,0,0,0"], {"regions": 0}),
             ([f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0", f"h:{EMPTY}", "c:7,8,900,0"], {}),
             ([f"h:{EMPTY}", "c:8,0,0,0", "c:1,0,0,0", "c:11,8,0,4"], {}), ([f"h:{EMPTY}", "c:10,0,0,0", "c:1,0,0,0", "c:6,2,2,0", "c:11,3,9,1"], {}),
             ([f"h:{EMPTY}", "c:10,0,0,0"], {"points": 0}), ([f"h:{EMPTY}", "c:11,8,0,4!"], {}), ([f"h:{EMPTY}", "c:11,8,0,4", "c:1,0,0,0"], {}),
             ([f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0"], {"branch": 0}), (["c:1,0,0,0"], {}), ([f"h:{EMPTY}", "c:9,0,0,0"], {}),
             ([f"h:{EMPTY}", "c:5,0,0,0"], {}), ([f"h:{EMPTY}", "c:1,0,0,0"], {"regions": 0}), ([f"h:{EMPTY}", "c:11,8,0,4"], {"device": 1}),
             ([f"h:{EMPTY}", "c:11,8,0,4", "c:13,0,0,0", "h:1,2,30,40"], {}), ([f"h:{EMPTY}", "c:13,8,0,0"], {}),
             ([f"h:{EMPTY}", "c:12,2,1,0", "c:11,8,0,4", "c:13,3,0,0"], {}), ([f"h:{EMPTY}", "c:12,0,1,0", "c:12,1,0,0"], {"points": 0}),
             ([f"h:{EMPTY}", "c:15,0,0,0"], {})]
    for entries, how in calls:
        assert planners(entries, **how) == planners(entries, exe="cutout", **how) == planners(entries, exe="cutout_cases", **how), (entries, how)
    # 14 is no label where there are no `regions` to hold a mark
    assert planners([f"h:{EMPTY}", "c:14,1,0,0"], regions=0) == planners([f"h:{EMPTY}", "c:14,1,0,0"], regions=0, exe="cutout")


def test_click_entries_with_edges():
    r = api.Region(P(10, 20), P(300, 400))
    rgba = np.zeros((4, 6, 4), np.uint8)
    assert api.EDGE_MARK == 14 and (api.EDGE_MAX_OFFSET, api.EDGE_MAX_FEATHER, api.EDGE_MAX_BORDER) == (64, 32, 32)
    e = api.click_entries([[P(1, 2), P(3, 4)], [P(7, 8)], [P(9, 10)]], [[1, 0], None, None], [None, r, None], [[1], None, None],
                          [(3, 4), None, None], matte=[(rgba, 8, 0), None, None], cutout=[5, None, None], edge=[(2, 1, 0), -3, None])
    assert e.heads == [0, None, None, None, None, None, None, 1, None, 2]
    assert e.regions == [api.EMPTY_REGION, (4, 0, 0, 0), (0, 0, 0, 0), (6, 3, 4, 0), (14, 2, 1, 0), (11, 8, 0, 4), (13, 5, 0, 0),
                         (10, 20, 300, 400), (14, -3, 0, 0), api.EMPTY_REGION]
    assert e.token_rows == api.click_entries([[P(1, 2), P(3, 4)], [P(7, 8)], [P(9, 10)]], [[1, 0], None, None], [None, r, None]).token_rows
    # behind the stroke marks
    stroke = np.zeros((4, 6), np.uint8)
    e = api.click_entries([None], strokes=[[(stroke, 1, 2)]], edge=[(0, 0, 2)])
    assert e.regions == [api.EMPTY_REGION, (12, 2, 1, 0), (14, 0, 0, 2)] and e.points is None
    # entry lists without edge marks are what they were
    a = api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], clean=[(1, 1)])
    assert a == api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], clean=[(1, 1)], edge=None) \
        == api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], clean=[(1, 1)], edge=[None])
    for bad in ([0], [(0, 0, 0)], [65], [-65], [(1, 33, 0)], [(1, -1, 0)], [(1, 0, 33)], [(1, 0)], ["1"], [1.5], [1, None], 3):
        with pytest.raises(api.Error, match="edge"):
            api.click_entries([[P(1, 2)]], edge=bad)
    with pytest.raises(api.Error, match="grid prompt"):
        api.click_entries([None], grid=[(4, 0, 0)], edge=[1])
    # the `points` / `regions` form: behind the clean-up mark, in front of the matte mark
    heads, pts, regs = api._marked_entries(2, [P(1, 2), P(3, 4)], None, [None, (1, 1)], matte=[None, (rgba, 4, 8, 650)],
                                           edge=[(5, 0, 0), (0, 2, 0)])
    assert heads == [0, None, 1, None, None, None]
    assert regs == [api.EMPTY_REGION, (14, 5, 0, 0), api.EMPTY_REGION, (6, 1, 1, 0), (14, 0, 2, 0), (11, 8, 650, 4)]


def test_cpp_wrapper_compiles_with_an_edge(tmp_path):
    """dlimgedit.hpp: Edge, the edge argument of both compute_mask forms, snap and scribble compile as a caller writes them."""
    src = tmp_path / "consumer.cpp"
    src.write_text('''#include <dlimgedit/dlimgedit.hpp>
static_assert(DLIMG_EDGE_MARK == 14, "the edge mark of table slot 14");
dlimg::Image modify(dlimg::Segmentation const& seg, dlimg::Image const& image, dlimg::Image& selection) {
    dlimg::Edge grow{3}, feather{0, 5}, band{-2, 1, 4};
    if (grow.offset != 3 || grow.feather != 0 || grow.border != 0 || feather.feather != 5 || band.border != 4)
        return dlimg::Image(dlimg::Extent{1, 1}, dlimg::Channels::mask);
    dlimg::Image grown = seg.compute_mask({dlimg::Click{dlimg::Point{10, 20}, true}}, std::nullopt, {}, std::nullopt, std::nullopt, std::nullopt,
                                          std::nullopt, {}, std::nullopt, grow);
    dlimg::Matte matte{image.pixels()};
    dlimg::Image soft = seg.compute_mask({dlimg::Click{dlimg::Point{10, 20}, true}}, std::nullopt, {}, dlimg::MaskCleanup{4, 4}, std::nullopt,
                                         std::nullopt, matte, {}, std::nullopt, dlimg::Edge{-2});
    dlimg::Image snapped = seg.snap(dlimg::Lasso{selection.pixels()}, {}, {}, std::nullopt, std::nullopt, std::nullopt, feather);
    seg.snap(dlimg::Lasso{selection.pixels()}, selection.pixels(), {}, {}, dlimg::MaskCleanup{0, 9}, matte, std::nullopt, band);
    dlimg::Image drawn = seg.scribble({dlimg::Stroke{selection.pixels()}}, std::nullopt, std::nullopt, std::nullopt, std::nullopt, band);
    std::vector<std::optional<dlimg::Edge>> edges{grow, std::nullopt};
    auto both = dlimg::Segmentation::compute_mask_batch({&seg, &seg}, std::vector<std::vector<dlimg::Click>>{{{dlimg::Point{1, 2}}}, {{dlimg::Point{3, 4}}}},
                                                        {}, {}, {}, {}, {}, {}, {}, {}, edges);
    return std::move(both[0]);
}
int main() { return 0; }
''')
    r = subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", "-DDLIMGEDIT_LOAD_DYNAMIC", f"-I{ROOT / 'include'}", "-fsyntax-only",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_planner_on_random_entry_lists_under_address_sanitizer(tmp_path):
    """csrc/edge_plan.hpp on 6000 random batch mask calls with ASan + UBSan, every served call checked against what the batch
    calls rely on (tests/edge_plan_cases.cpp, `fuzz`): a stand-alone program on the CPU, nothing loaded into Python."""
    clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    if not clang.exists():
        pytest.skip("ROCm clang not found")
    exe = tmp_path / "edge_plan_cases_san"
    r = subprocess.run([str(clang), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", f"-I{CSRC}", str(ROOT / "tests" / "edge_plan_cases.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and "sanitizer" in (r.stderr + r.stdout).lower() and "cannot find" in (r.stderr + r.stdout).lower():
        pytest.skip("this clang has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "fuzz", "6000", "17"], capture_output=True, text=True, errors="replace", timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    served, edged = int(re.search(r"served (\d+)", r.stdout).group(1)), int(re.search(r"edge mark (\d+)", r.stdout).group(1))
    assert 100 < served < 5900 and edged > 50, r.stdout
