"""Stroke marks in the planner (csrc/stroke_plan.hpp, printed by tests/stroke_plan_cases.cpp, built with the host compiler): marks
expanded into placeholder clicks at their positions; the first foreground click as the head's in a call without `points`; staging
across a refinement mark; every refusal naming the mark and the caller's entry; the inner planners' refusals keeping the caller's
numbering; a call without stroke marks printing what tests/matte_plan_cases.cpp prints for it; the Python entry lists; and the
planner on random entry lists under ASan + UBSan, as the stand-alone program it is.
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
    tmp = tmp_path_factory.mktemp("stroke_plan")
    stroke, matte = _build(tmp, "stroke_plan_cases"), _build(tmp, "matte_plan_cases")

    def run(entries, points=1, regions=1, branch=1, device=0, exe="stroke"):
        head = [str(stroke), "stroke"] if exe == "stroke" else ([str(stroke), "matte"] if exe == "inner" else [str(matte), "matte"])
        r = subprocess.run([str(a) for a in head + [points, regions, branch, device]] + list(entries), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def test_planner_expands_stroke_marks_where_they_stand(planners):
    # a head with its own click, a plain click, then a background stroke of 2 and a foreground stroke of the default 3
    assert planners([f"h:{EMPTY}", "c:1,0,0,0", "c:12,2,0,0", "c:12,0,1,0"]) == [
        "prompt 0 clicks 7 box 0 points 8 entries 0,1,2,3,4,5,6 stages 7 clean 0,0 grid 0,0,0 stroke 2,0,2:2/3 stroke 3,1,3:4/5/6",
        "any_clean 0", "any_grid 0", "any_stroke 1",
        f"rewritten h0:{EMPTY} c1:1,0,0,0 c2*:0,0,0,0 c2*:0,0,0,0 c3*:1,0,0,0 c3*:1,0,0,0 c3*:1,0,0,0"]
    # between plain clicks; a box; a second prompt without marks keeps its entries, renumbered
    assert planners(["h:1,2,30,40", "c:0,0,0,0", "c:12,1,1,0", "c:1,0,0,0", "h:5,6,70,80"]) == [
        "prompt 0 clicks 4 box 1 points 6 entries 0,1,2,3 stages 4 clean 0,0 grid 0,0,0 stroke 2,1,1:2",
        "prompt 4 clicks 1 box 1 points 3 entries 4 stages 1 clean 0,0 grid 0,0,0",
        "any_clean 0", "any_grid 0", "any_stroke 1", "rewritten h0:1,2,30,40 c1:0,0,0,0 c2*:1,0,0,0 c3:1,0,0,0 h4:5,6,70,80"]
    # behind a prior mark and behind a lasso mark, in front of clean-up and matte marks
    assert planners([f"h:{EMPTY}", "c:8,0,0,0", "c:12,2,1,0", "c:6,2,2,0", "c:11,8,0,4", f"h:{EMPTY}", "c:10,0,0,0", "c:12,1,0,0"])[:2] == [
        "prompt 0 clicks 3 box 0 points 4 entries 0,2,3 stages 3 clean 2,2 grid 0,0,0 prior 1,8000 matte 5,8,650,4 stroke 2,1,2:2/3",
        "prompt 6 clicks 3 box 1 points 5 entries 7,6,8 stages 3 clean 0,0 grid 0,0,0 lasso 7,7,8000 stroke 7,0,1:8"]
    # 8 clicks in all are served: the head's and 7 derived
    assert planners([f"h:{EMPTY}", "c:12,7,1,0"])[0].startswith("prompt 0 clicks 8 box 0 points 9 ")


def test_without_points_the_first_foreground_click_is_the_heads(planners):
    # the stroke alone: three clicks, the first in the head's entry, whose point is derived
    assert planners([f"h:{EMPTY}", "c:12,0,1,0"], points=0) == [
        "prompt 0 clicks 3 box 0 points 4 entries 0,1,2 stages 3 clean 0,0 grid 0,0,0 stroke 1,1,3:0/1/2",
        "any_clean 0", "any_grid 0", "any_stroke 1", f"rewritten h0*:{EMPTY} c1*:1,0,0,0 c1*:1,0,0,0"]
    # a background stroke in front: the head's click comes from the second mark; a box travels as ever
    assert planners(["h:1,2,30,40", "c:12,2,0,0", "c:12,2,1,0"], points=0) == [
        "prompt 0 clicks 4 box 1 points 6 entries 0,1,2,3 stages 4 clean 0,0 grid 0,0,0 stroke 1,0,2:1/2 stroke 2,1,2:0/3",
        "any_clean 0", "any_grid 0", "any_stroke 1", "rewritten h0*:1,2,30,40 c1*:0,0,0,0 c1*:0,0,0,0 c2*:1,0,0,0"]
    # one foreground click and nothing else: no continuation entry is left, and the empty region still is no box
    assert planners([f"h:{EMPTY}", "c:12,1,1,0"], points=0) == [
        "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0 stroke 1,1,1:0",
        "any_clean 0", "any_grid 0", "any_stroke 1", f"rewritten h0*:{EMPTY}"]
    # behind a lasso mark the lasso's click stays the first, the head's is the stroke's
    assert planners([f"h:{EMPTY}", "c:10,0,0,0", "c:12,2,1,0"], points=0)[0] == \
        "prompt 0 clicks 3 box 1 points 5 entries 1,0,2 stages 3 clean 0,0 grid 0,0,0 lasso 1,7,8000 stroke 2,1,2:0/2"
    # every prompt of such a call has a foreground stroke
    assert planners([f"h:{EMPTY}", "c:12,1,1,0", f"h:{EMPTY}", "c:12,2,1,0"], points=0)[:2] == [
        "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0 stroke 1,1,1:0",
        "prompt 1 clicks 2 box 0 points 3 entries 1,2 stages 2 clean 0,0 grid 0,0,0 stroke 3,1,2:1/2"]


def test_a_refinement_mark_stages_derived_clicks_like_any_click(planners):
    # stroke, refine, stroke: the first stage takes the head's click and the first stroke's two
    assert planners([f"h:{EMPTY}", "c:12,2,1,0", "c:4,0,0,0", "c:12,2,0,0"]) == [
        "prompt 0 clicks 5 box 0 points 6 entries 0,1,2,4,5 stages 3,5 clean 0,0 grid 0,0,0 stroke 1,1,2:1/2 stroke 3,0,2:4/5",
        "any_clean 0", "any_grid 0", "any_stroke 1", f"rewritten h0:{EMPTY} c1*:1,0,0,0 c1*:1,0,0,0 c2:4,0,0,0 c3*:0,0,0,0 c3*:0,0,0,0"]
    # without points: the head's click is in the first stage, whichever mark it came from
    assert planners([f"h:{EMPTY}", "c:12,1,0,0", "c:4,0,0,0", "c:12,2,1,0"], points=0)[0] == \
        "prompt 0 clicks 3 box 0 points 4 entries 0,1,3 stages 2,3 clean 0,0 grid 0,0,0 stroke 1,0,1:1 stroke 3,1,2:0/3"
    # a stroke mark is clicks enough between two refinement marks
    assert planners([f"h:{EMPTY}", "c:4,0,0,0", "c:12,1,1,0", "c:4,0,0,0", "c:12,1,0,0"])[0].startswith(
        "prompt 0 clicks 3 box 0 points 4 entries 0,2,4 stages 1,2,3 ")


REFUSALS = [
    ([f"h:{EMPTY}", "c:12,3,1,1"], {}, 1, "the fourth int is 0"),
    ([f"h:{EMPTY}", "c:12,3,2,0"], {}, 1, "label is 1 .foreground. or 0 .background."),
    ([f"h:{EMPTY}", "c:12,3,-1,0"], {}, 1, "label is 1 .foreground. or 0 .background."),
    ([f"h:{EMPTY}", "c:12,9,1,0"], {}, 1, r"clicks is 0 \(the default, 3\) \.\. 8"),
    ([f"h:{EMPTY}", "c:12,-1,1,0"], {}, 1, r"clicks is 0 \(the default, 3\) \.\. 8"),
    ([f"h:{EMPTY}", "c:1,0,0,0", "c:12,3,1,0!"], {}, 2, "NULL"),
    (["c:12,3,1,0", f"h:{EMPTY}"], {}, 0, "needs a prompt in front"),
    ([f"h:{EMPTY}", f"h:{EMPTY}", "c:12,3,1,0", "c:7,4,0,0"], {}, 2, "on a grid prompt"),
    ([f"h:{EMPTY}", "c:12,3,1,0"], {"device": 1}, 1, "dlimg_amd_get_segmentation_masks_device"),
    ([f"h:{EMPTY}", "c:12,3,0,0"], {"points": 0}, 1, "background clicks is no prompt by itself"),
    (["h:1,2,30,40", "c:12,3,0,0", "c:12,0,0,0"], {"points": 0}, 1, "background clicks is no prompt by itself"),
    ([f"h:{EMPTY}", "c:12,8,1,0"], {}, 1, "has 9 clicks, more than 8"),
    ([f"h:{EMPTY}", "c:12,8,1,0", "c:12,1,0,0"], {"points": 0}, 1, "has 9 clicks, more than 8"),
    ([f"h:{EMPTY}", "c:1,0,0,0", "c:12,3,1,0", "c:0,0,0,0", "c:12,0,0,0"], {}, 2, "has 9 clicks, more than 8"),
    ([f"h:{EMPTY}", "c:12,3,1,0", "c:10,0,0,0"], {}, 1, "in front of a lasso mark"),
    ([f"h:{EMPTY}", "c:12,1,1,0", "c:8,0,0,0"], {"points": 0}, 1, "in front of a prior mark"),
    ([f"h:{EMPTY}", "c:6,2,2,0", "c:12,1,1,0"], {"points": 0}, 2, "behind a clean-up or matte mark"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:12,1,1,0"], {}, 2, "behind a clean-up or matte mark"),
]


@pytest.mark.parametrize("entries,how,entry,why", REFUSALS, ids=[f"{i}-{re.sub('[^a-z0-9]+', '_', r[3][:24].lower())}" for i, r in enumerate(REFUSALS)])
def test_planner_refusals_name_the_mark_and_the_callers_entry(planners, entries, how, entry, why):
    out = planners(entries, **how)
    assert len(out) == 1 and out[0].startswith(f"error mask batch: entry {entry}: a stroke mark "), out
    assert re.search(why, out[0]), out


def test_a_call_without_points_has_a_foreground_stroke_in_every_prompt(planners):
    out = planners([f"h:{EMPTY}", "c:12,1,1,0", "h:1,2,30,40"], points=0)
    assert len(out) == 1 and out[0].startswith("error mask batch: entry 2:") and "stroke mark" in out[0], out
    # and a plain click entry still needs `points`
    out = planners([f"h:{EMPTY}", "c:12,1,1,0", "c:1,0,0,0"], points=0)
    assert len(out) == 1 and out[0].startswith("error mask batch: entry 2:") and "needs `points`" in out[0], out


def test_refusals_of_the_inner_planners_keep_the_callers_numbering(planners):
    # entries behind a stroke mark are renumbered back: three placeholders lie in front of the caller's entry 2
    out = planners([f"h:{EMPTY}", "c:12,3,1,0", "c:5,0,0,0"])
    assert out[0].startswith("error mask batch: entry 2:") and "label" in out[0], out
    out = planners([f"h:{EMPTY}", "c:12,3,1,0", f"h:{EMPTY}", "c:1,0,0,0", "c:8,0,0,0"])
    assert out[0].startswith("error mask batch: entry 4: a prior mark"), out
    out = planners([f"h:{EMPTY}", "c:12,3,1,0", f"h:{EMPTY}", "c:6,1,1,0", "c:1,0,0,0"])
    assert out[0].startswith("error mask batch: entry 3: a clean-up mark"), out
    out = planners([f"h:{EMPTY}", "c:12,2,1,0", "c:4,0,0,0"])
    assert out[0].startswith("error mask batch: entry 2: a refinement mark") and "last entry" in out[0], out
    out = planners([f"h:{EMPTY}", "c:12,2,1,0", "c:4,0,0,0", "c:12,1,1,0"], branch=0)
    assert out[0].startswith("error mask batch: entry 2: a refinement mark") and "pe.mask" in out[0], out
    out = planners([f"h:{EMPTY}", "c:12,2,1,0", f"h:{EMPTY}", "c:11,8,0,4!"])
    assert out[0].startswith("error mask batch: entry 3: a matte mark") and "NULL" in out[0], out
    # a lasso mark whose click is one too many: the lasso planner's own refusal, of the caller's entry
    out = planners([f"h:{EMPTY}", "c:10,0,2,0", "c:12,7,1,0"])
    assert out[0].startswith("error mask batch: entry 1: a lasso mark") and "more than 8" in out[0], out


def test_a_call_without_stroke_marks_is_planned_as_before(planners):
    calls = [([f"h:{EMPTY}", "c:1,0,0,0", "h:1,2,30,40", "c:0,0,0,0", "c:6,3,4,0"], {}),
             (["h:1,2,30,40", "h:5,5,1,1"], {}), (["h:1,2,30,40"], {"points": 0}), (["h:0,0,0,0", "h:0,0,0,0"], {"regions": 0}),
             ([f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0", f"h:{EMPTY}", "c:7,8,900,0"], {}),
             ([f"h:{EMPTY}", "c:8,0,0,0", "c:1,0,0,0", "c:11,8,0,4"], {}), ([f"h:{EMPTY}", "c:10,0,0,0", "c:1,0,0,0", "c:6,2,2,0"], {}),
             ([f"h:{EMPTY}", "c:10,0,0,0", "c:11,4,9,3"], {"points": 0}), ([f"h:{EMPTY}", "c:11,8,0,4!"], {}),
             ([f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0"], {"branch": 0}), (["c:1,0,0,0"], {}), ([f"h:{EMPTY}", "c:9,0,0,0"], {}),
             ([f"h:{EMPTY}", "c:13,0,0,0"], {}), ([f"h:{EMPTY}", "c:1,0,0,0"], {"regions": 0}), ([f"h:{EMPTY}", "c:11,8,0,4"], {"device": 1})]
    for entries, how in calls:
        assert planners(entries, **how) == planners(entries, exe="inner", **how) == planners(entries, exe="matte_cases", **how), (entries, how)
    # 12 is no label where there are no `regions` to hold a mark
    assert planners([f"h:{EMPTY}", "c:12,3,1,0"], regions=0) == planners([f"h:{EMPTY}", "c:12,3,1,0"], regions=0, exe="matte_cases")


def test_click_entries_with_strokes():
    fg, bg = np.full((4, 6), 255, np.uint8), np.zeros((4, 6), np.uint8)
    r = api.Region(P(10, 20), P(300, 400))
    assert api.STROKE_MARK == 12 and api.STROKE_DEFAULT_CLICKS == 3
    # clicks given: the stroke marks follow them, in front of the clean-up mark; None: a prompt without strokes
    e = api.click_entries([[P(1, 2), P(3, 4)], [P(7, 8)]], [[1, 0], None], [None, r], None, [(3, 4), None],
                          strokes=[[(fg, 1, 0), (bg, 0, 2)], None])
    assert e.heads == [0, None, None, None, None, 1]
    assert e.regions == [api.EMPTY_REGION, (0, 0, 0, 0), (12, 0, 1, 0), (12, 2, 0, 0), (6, 3, 4, 0), (10, 20, 300, 400)]
    assert e.strokes[0][0] is fg and e.strokes[0][1] is bg and e.strokes[1] == []
    assert e.token_rows == [5 + 2 + 3 + 2 + 1, 8] and e.stage_clicks == [[7], [1]]
    # no clicks: the first foreground click is the head's, the entry list holds no points
    only = api.click_entries([None], strokes=[[(fg, 1, 4)]])
    assert only.heads == [0, None] and only.points is None and only.regions == [api.EMPTY_REGION, (12, 4, 1, 0)]
    assert only.token_rows == [5 + 4 + 1] and only.stage_clicks == [[4]]
    # entry lists without strokes are what they were
    a = api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r])
    assert a == api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], strokes=None) == api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], strokes=[None])
    assert a.strokes == []
    for bad in ([[(fg.astype(np.int32), 1, 0)]], [[(fg[:, ::2], 1, 0)]], [[(fg, 2, 0)]], [[(fg, 1, 9)]], [[(fg, 1, -1)]], [[fg]], [(fg, 1, 0)],
                [[(fg, 1, 0)], None], [[(np.zeros(24, np.uint8), 1, 0)]]):
        with pytest.raises(api.Error):
            api.click_entries([[P(1, 2)]], strokes=bad)
    with pytest.raises(api.Error):          # background strokes alone are no prompt
        api.click_entries([None], strokes=[[(bg, 0, 2)]])
    with pytest.raises(api.Error):          # more than 8 clicks, the derived ones counted
        api.click_entries([[P(1, 2), P(3, 4)]], strokes=[[(fg, 1, 4), (bg, 0, 3)]])
    with pytest.raises(api.Error):
        api.click_entries([None], grid=[(4, 0, 0)], strokes=[[(fg, 1, 0)]])


def test_planner_on_random_entry_lists_under_address_sanitizer(tmp_path):
    """csrc/stroke_plan.hpp on 6000 random batch mask calls with ASan + UBSan, every served call checked against what the batch
    calls rely on (tests/stroke_plan_cases.cpp, `fuzz`): a stand-alone program on the CPU, nothing loaded into Python."""
    clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    if not clang.exists():
        pytest.skip("ROCm clang not found")
    exe = tmp_path / "stroke_plan_cases_san"
    r = subprocess.run([str(clang), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", f"-I{CSRC}", str(ROOT / "tests" / "stroke_plan_cases.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and "sanitizer" in (r.stderr + r.stdout).lower() and "cannot find" in (r.stderr + r.stdout).lower():
        pytest.skip("this clang has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "fuzz", "6000", "17"], capture_output=True, text=True, errors="replace", timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    served, strokes = (int(re.search(rf"{k} (\d+)", r.stdout).group(1)) for k in ("served", "strokes"))
    assert 200 < served < 5800 and strokes > 100, r.stdout


def test_the_cpp_wrapper_takes_strokes(tmp_path):
    """dlimgedit.hpp: Stroke, the strokes argument of both compute_mask forms and scribble compile as a caller writes them."""
    src = tmp_path / "strokes.cpp"
    src.write_text('''#include <dlimgedit/dlimgedit.hpp>
using namespace dlimg;
Image both(Segmentation const& s, uint8_t const* fg, uint8_t const* bg, uint8_t* out) {
    static_assert(DLIMG_STROKE_MARK == 12, "the mark");
    std::vector<Stroke> strokes{Stroke{fg, 1, 0}, Stroke{bg, 0, 2}};
    s.scribble(strokes, out, Region(Point{1, 2}, Point{30, 40}), MaskCleanup{4, 4});
    Image a = s.scribble({Stroke{fg}});
    Image b = s.compute_mask({Click{Point{5, 6}}}, std::nullopt, {}, std::nullopt, std::nullopt, std::nullopt, std::nullopt, strokes);
    return std::move(Segmentation::compute_mask_batch({&s}, {{Click{Point{5, 6}}}}, {}, {}, {}, {}, {}, {}, {strokes})[0]);
}
''')
    r = subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
