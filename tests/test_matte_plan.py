"""Matte marks in the planner (csrc/matte_plan.hpp, printed by tests/matte_plan_cases.cpp, built with the host compiler): marks
read alone and behind clean-up, lasso, prior and refinement marks; every refusal naming the mark and the caller's entry; the
inner planners' refusals keeping the caller's numbering; a call without matte marks printing what tests/lasso_plan_cases.cpp
prints for it; the Python entry lists; and the planner on random entry lists under ASan + UBSan, as the stand-alone program it is.
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
    tmp = tmp_path_factory.mktemp("matte_plan")
    matte, lasso = _build(tmp, "matte_plan_cases"), _build(tmp, "lasso_plan_cases")

    def run(entries, points=1, regions=1, branch=1, device=0, exe="matte"):
        head = [str(matte), "matte"] if exe == "matte" else ([str(matte), "lasso"] if exe == "inner" else [str(lasso), "lasso"])
        r = subprocess.run([str(a) for a in head + [points, regions, branch, device]] + list(entries), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return [l for l in r.stdout.splitlines() if not l.startswith("  packed")]
    return run


def test_planner_reads_matte_marks(planners):
    # one click and a matte; a box and a click without one; eps 0 is the default 650
    assert planners([f"h:{EMPTY}", "c:11,8,0,4", "h:1,2,30,40"]) == [
        "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0 matte 1,8,650,4",
        "prompt 2 clicks 1 box 1 points 3 entries 2 stages 1 clean 0,0 grid 0,0,0", "any_clean 0", "any_grid 0", "any_matte 1"]
    # a box alone needs no points; radius, eps and channels travel
    assert planners(["h:1,2,30,40", "c:11,32,65025,1"], points=0) == [
        "prompt 0 clicks 0 box 1 points 2 entries stages 0 clean 0,0 grid 0,0,0 matte 1,32,65025,1", "any_clean 0", "any_grid 0", "any_matte 1"]
    # behind a clean-up mark, which stays the last of the remaining entries
    assert planners([f"h:{EMPTY}", "c:0,0,0,0", "c:6,5,7,0", "c:11,1,1,3"]) == [
        "prompt 0 clicks 2 box 0 points 3 entries 0,1 stages 2 clean 5,7 grid 0,0,0 matte 3,1,1,3", "any_clean 1", "any_grid 0", "any_matte 1"]
    # behind a prior mark, refinement marks and a clean-up mark; a lasso prompt and a grid prompt beside it
    assert planners([f"h:{EMPTY}", "c:8,2500,0,0", "c:4,0,0,0", "c:1,0,0,0", "c:6,0,9,0", "c:11,16,650,4",
                     f"h:{EMPTY}", "c:10,0,3,0", "c:1,0,0,0", "c:11,4,20,3", f"h:{EMPTY}", "c:7,4,0,0"]) == [
        "prompt 0 clicks 2 box 0 points 3 entries 0,3 stages 1,2 clean 0,9 grid 0,0,0 prior 1,2500 matte 5,16,650,4",
        "prompt 6 clicks 3 box 1 points 5 entries 7,6,8 stages 3 clean 0,0 grid 0,0,0 lasso 7,3,0 matte 9,4,20,3",
        "prompt 10 clicks 1 box 0 points 2 entries 10 stages 1 clean 0,0 grid 4,0,0", "any_clean 1", "any_grid 1", "any_prior 1", "any_lasso 1",
        "any_matte 1"]
    # a lasso-only prompt with a matte lives in a call without points
    assert planners([f"h:{EMPTY}", "c:10,0,0,0", "c:11,8,0,4"], points=0)[0] == \
        "prompt 0 clicks 1 box 1 points 3 entries 1 stages 1 clean 0,0 grid 0,0,0 lasso 1,7,8000 matte 2,8,650,4"
    # a matte mark makes the call one with continuation entries: the empty region of ANOTHER head is "no box" too
    assert planners([f"h:{EMPTY}", "h:1,1,5,5", "c:11,8,0,4"])[0] == "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0"


REFUSALS = [
    (["c:11,8,0,4", f"h:{EMPTY}"], {}, 0, "needs a prompt in front"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:1,0,0,0"], {}, 1, "not the last entry of its prompt"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:6,3,3,0"], {}, 1, "not the last entry of its prompt"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:11,8,0,4"], {}, 2, "second"),
    ([f"h:{EMPTY}", "h:1,1,5,5", "c:11,8,0,4!"], {}, 2, "NULL"),
    ([f"h:{EMPTY}", "c:11,0,0,4"], {}, 1, r"radius is 1 \.\. 32"),
    ([f"h:{EMPTY}", "c:11,33,0,4"], {}, 1, r"radius is 1 \.\. 32"),
    ([f"h:{EMPTY}", "c:11,8,-1,4"], {}, 1, r"eps is 0 \(the default\) \.\. 65025"),
    ([f"h:{EMPTY}", "c:11,8,65026,4"], {}, 1, r"eps is 0 \(the default\) \.\. 65025"),
    ([f"h:{EMPTY}", "c:11,8,0,2"], {}, 1, "channels is 1, 3 or 4"),
    ([f"h:{EMPTY}", "c:11,8,0,0"], {}, 1, "channels is 1, 3 or 4"),
    ([f"h:{EMPTY}", "c:11,8,0,5"], {}, 1, "channels is 1, 3 or 4"),
    ([f"h:{EMPTY}", f"h:{EMPTY}", "c:7,4,0,0", "c:11,8,0,4"], {}, 3, "grid prompt: a label map is not a coverage"),
    ([f"h:{EMPTY}", "c:11,8,0,4"], {"device": 1}, 1, "dlimg_amd_get_segmentation_masks_device"),
    (["h:1,1,5,5", f"h:{EMPTY}", "c:11,8,0,4"], {"points": 0}, 2, "still needs a click or a box"),
]


@pytest.mark.parametrize("entries,how,entry,why", REFUSALS, ids=[f"{i}-{re.sub('[^a-z0-9]+', '_', r[3][:24].lower())}" for i, r in enumerate(REFUSALS)])
def test_planner_refusals_name_the_mark_and_the_callers_entry(planners, entries, how, entry, why):
    out = planners(entries, **how)
    assert len(out) == 1 and out[0].startswith(f"error mask batch: entry {entry}: a matte mark "), out
    assert re.search(why, out[0]), out


def test_refusals_of_the_inner_planners_keep_the_callers_numbering(planners):
    # entries behind a matte mark are renumbered back: the bad label is the caller's entry 3, the misplaced marks keep theirs
    out = planners([f"h:{EMPTY}", "c:11,8,0,4", f"h:{EMPTY}", "c:5,0,0,0"])
    assert out[0].startswith("error mask batch: entry 3:") and "label" in out[0], out
    out = planners([f"h:{EMPTY}", "c:11,8,0,4", f"h:{EMPTY}", "c:1,0,0,0", "c:8,0,0,0"])
    assert out[0].startswith("error mask batch: entry 4: a prior mark"), out
    out = planners([f"h:{EMPTY}", "c:11,8,0,4", f"h:{EMPTY}", "c:1,0,0,0", "c:10,0,0,0"])
    assert out[0].startswith("error mask batch: entry 4: a lasso mark"), out
    out = planners([f"h:{EMPTY}", "c:11,8,0,4", f"h:{EMPTY}", "c:6,1,1,0", "c:1,0,0,0", "c:11,8,0,4"])
    assert out[0].startswith("error mask batch: entry 3: a clean-up mark"), out
    out = planners([f"h:{EMPTY}", "c:11,8,0,4", f"h:{EMPTY}", "c:4,0,0,0", "c:11,8,0,4"])
    assert out[0].startswith("error mask batch: entry 3: a refinement mark"), out
    # the null selection of a lasso mark behind a matte prompt: the pointers travel with the entries
    out = planners([f"h:{EMPTY}", "c:11,8,0,4", f"h:{EMPTY}", "c:10,0,0,0!"])
    assert out[0].startswith("error mask batch: entry 3: a lasso mark") and "NULL" in out[0], out


def test_a_call_without_matte_marks_is_planned_as_before(planners):
    calls = [([f"h:{EMPTY}", "c:1,0,0,0", "h:1,2,30,40", "c:0,0,0,0", "c:6,3,4,0"], {}),
             (["h:1,2,30,40", "h:5,5,1,1"], {}), (["h:1,2,30,40"], {"points": 0}), (["h:0,0,0,0", "h:0,0,0,0"], {"regions": 0}),
             ([f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0", f"h:{EMPTY}", "c:7,8,900,0"], {}),
             ([f"h:{EMPTY}", "c:8,0,0,0", "c:1,0,0,0"], {}), ([f"h:{EMPTY}", "c:10,0,0,0", "c:1,0,0,0", "c:6,2,2,0"], {}),
             ([f"h:{EMPTY}", "c:10,0,0,0"], {"points": 0}), ([f"h:{EMPTY}", "c:10,0,0,0!"], {}),
             ([f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0"], {"branch": 0}), (["c:1,0,0,0"], {}), ([f"h:{EMPTY}", "c:9,0,0,0"], {}),
             ([f"h:{EMPTY}", "c:5,0,0,0"], {}), ([f"h:{EMPTY}", "c:1,0,0,0"], {"regions": 0}), ([f"h:{EMPTY}", "c:8,0,0,0"], {"device": 1})]
    for entries, how in calls:
        assert planners(entries, **how) == planners(entries, exe="inner", **how) == planners(entries, exe="lasso_cases", **how), (entries, how)
    # 11 is no label where there are no `regions` to hold a mark
    assert planners([f"h:{EMPTY}", "c:11,8,0,4"], regions=0) == planners([f"h:{EMPTY}", "c:11,8,0,4"], regions=0, exe="lasso_cases")


def test_click_entries_with_mattes():
    r = api.Region(P(10, 20), P(300, 400))
    rgba, grey, sel = np.zeros((4, 6, 4), np.uint8), np.zeros((4, 6), np.uint8), np.ones((4, 6), np.uint8)
    e = api.click_entries([[P(1, 2), P(3, 4)], [P(7, 8)], [P(9, 10)]], [[1, 0], None, None], [None, r, None], [[1], None, None],
                          [(3, 4), None, None], lasso=[None, None, sel], matte=[(rgba, 8, 0), None, (grey, 32, 65025)])
    assert api.MATTE_MARK == 11
    assert e.heads == [0, None, None, None, None, 1, 2, None, None]
    assert e.regions == [api.EMPTY_REGION, (4, 0, 0, 0), (0, 0, 0, 0), (6, 3, 4, 0), (11, 8, 0, 4), (10, 20, 300, 400), api.EMPTY_REGION,
                         (10, 0, 0, 0), (11, 32, 65025, 1)]
    assert e.mattes[0] is rgba and e.mattes[1] is None and e.mattes[2] is grey
    assert e.token_rows == [8, 8, 9] and e.stage_clicks == [[1, 2], [1], [2]]
    # a prompt with a matte is decoded on its own
    assert e.launches == [(8, [1]), (7, [0]), (8, [0]), (9, [2])]
    # a single click with a matte is a call with a continuation entry
    one = api.click_entries([[P(1, 2)]], matte=[(np.zeros((4, 6, 3), np.uint8), 5, 100)])
    assert one.heads == [0, None] and one.regions == [api.EMPTY_REGION, (11, 5, 100, 3)] and api._entry_calls(one) == [([0, 1], True)]
    # entry lists without mattes are what they were
    a = api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r])
    assert a == api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], matte=None) == api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], matte=[None])
    assert a.mattes == []
    # the `points` / `regions` form: the matte mark behind the clean-up mark
    mt = api._checked_matte([(rgba, 8, 0), None], 2)
    heads, pts, regs = api._marked_entries(2, None, [r, r], [(3, 0), None], None, None, None, mt)
    assert heads == [0, None, None, 1] and pts is None and regs == [(10, 20, 300, 400), (6, 3, 0, 0), (11, 8, 0, 4), (10, 20, 300, 400)]
    for bad in ([(rgba.astype(np.int32), 8, 0)], [(rgba[:, ::2], 8, 0)], [(rgba, 0, 0)], [(rgba, 33, 0)], [(rgba, 8, -1)], [(rgba, 8, 65026)],
                [(np.zeros((4, 6, 2), np.uint8), 8, 0)], [(rgba, 8, 0), None], [rgba], [(np.zeros(24, np.uint8), 8, 0)]):
        with pytest.raises(api.Error):
            api.click_entries([[P(1, 2)]], matte=bad)
    with pytest.raises(api.Error):
        api.click_entries([None], grid=[(4, 0, 0)], matte=[(rgba, 8, 0)])


def test_planner_on_random_entry_lists_under_address_sanitizer(tmp_path):
    """csrc/matte_plan.hpp on 6000 random batch mask calls with ASan + UBSan, every served call checked against what the batch
    calls rely on (tests/matte_plan_cases.cpp, `fuzz`): a stand-alone program on the CPU, nothing loaded into Python."""
    clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    if not clang.exists():
        pytest.skip("ROCm clang not found")
    exe = tmp_path / "matte_plan_cases_san"
    r = subprocess.run([str(clang), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", f"-I{CSRC}", str(ROOT / "tests" / "matte_plan_cases.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and "sanitizer" in (r.stderr + r.stdout).lower() and "cannot find" in (r.stderr + r.stdout).lower():
        pytest.skip("this clang has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "fuzz", "6000", "17"], capture_output=True, text=True, errors="replace", timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    served = int(re.search(r"served (\d+)", r.stdout).group(1))
    assert 200 < served < 5800, r.stdout
