"""Cut-out marks in the planner (csrc/cutout_plan.hpp, printed by tests/cutout_plan_cases.cpp, built with the host compiler):
marks read behind a matte mark, alone and with clean-up, refinement and stroke marks in front; every refusal naming the mark and
the caller's entry; the inner planners' refusals keeping the caller's numbering; a call without cut-out marks printing what
plan_stroke_prompts and tests/matte_plan_cases.cpp print for it; the Python entry lists; and the planner on random entry lists
under ASan + UBSan, as the stand-alone program it is.
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
    tmp = tmp_path_factory.mktemp("cutout_plan")
    cutout, matte = _build(tmp, "cutout_plan_cases"), _build(tmp, "matte_plan_cases")

    def run(entries, points=1, regions=1, branch=1, device=0, exe="cutout"):
        head = {"cutout": [str(cutout), "cutout"], "stroke": [str(cutout), "stroke"], "matte_cases": [str(matte), "matte"]}[exe]
        r = subprocess.run([str(a) for a in head + [points, regions, branch, device]] + list(entries), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def test_planner_reads_cutout_marks(planners):
    # a click, a matte and a cut-out; radius 0 is the default 16; the matte planner sees its mark as the last entry
    assert planners([f"h:{EMPTY}", "c:11,8,0,4", "c:13,0,0,0", "h:1,2,30,40"]) == [
        "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0 matte 1,8,650,4 cutout 2,16",
        "prompt 3 clicks 1 box 1 points 3 entries 3 stages 1 clean 0,0 grid 0,0,0", "any_clean 0", "any_grid 0", "any_matte 1", "any_cutout 1"]
    # behind clean-up + matte, on a box alone, 3 channels, the largest radius
    assert planners(["h:1,2,30,40", "c:6,5,7,0", "c:11,32,1,3", "c:13,32,0,0"], points=0) == [
        "prompt 0 clicks 0 box 1 points 2 entries stages 0 clean 5,7 grid 0,0,0 matte 2,32,1,3 cutout 3,32", "any_clean 1", "any_grid 0",
        "any_matte 1", "any_cutout 1"]
    # two prompts of which the SECOND has a cut-out, the first a matte alone; entries behind the first mark keep the caller's numbers
    assert planners([f"h:{EMPTY}", "c:11,8,0,4", "c:13,5,0,0", f"h:{EMPTY}", "c:0,0,0,0", "c:11,4,20,1", f"h:{EMPTY}", "c:1,0,0,0", "c:11,2,0,3",
                     "c:13,1,0,0"]) == [
        "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0 matte 1,8,650,4 cutout 2,5",
        "prompt 3 clicks 2 box 0 points 3 entries 3,4 stages 2 clean 0,0 grid 0,0,0 matte 5,4,20,1",
        "prompt 6 clicks 2 box 0 points 3 entries 6,7 stages 2 clean 0,0 grid 0,0,0 matte 8,2,650,3 cutout 9,1",
        "any_clean 0", "any_grid 0", "any_matte 1", "any_cutout 1"]
    # a prior, refinement marks and a lasso prompt in front: every entry in the caller's numbering
    assert planners([f"h:{EMPTY}", "c:11,8,0,4", "c:13,0,0,0", f"h:{EMPTY}", "c:8,2500,0,0", "c:4,0,0,0", "c:1,0,0,0", "c:6,0,9,0", "c:11,16,650,4",
                     "c:13,7,0,0", f"h:{EMPTY}", "c:10,0,3,0", "c:11,4,20,3", "c:13,2,0,0"])[:3] == [
        "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0 matte 1,8,650,4 cutout 2,16",
        "prompt 3 clicks 2 box 0 points 3 entries 3,6 stages 1,2 clean 0,9 grid 0,0,0 prior 4,2500 matte 8,16,650,4 cutout 9,7",
        "prompt 10 clicks 2 box 1 points 4 entries 11,10 stages 2 clean 0,0 grid 0,0,0 lasso 11,3,0 matte 12,4,20,3 cutout 13,2"]


def test_cutout_marks_with_stroke_marks_in_front(planners):
    # the plan speaks of the rewritten call (stroke_plan.hpp); the strokes' and the cut-out's entries and entry_of are the caller's
    with_cut = planners([f"h:{EMPTY}", "c:11,8,0,4", "c:13,3,0,0", f"h:{EMPTY}", "c:12,2,1,0", "c:6,1,1,0", "c:11,4,0,3", "c:13,9,0,0"])
    assert with_cut == [
        "prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 0,0,0 matte 1,8,650,4 cutout 2,3",
        "prompt 2 clicks 3 box 0 points 4 entries 2,3,4 stages 3 clean 1,1 grid 0,0,0 matte 6,4,650,3 stroke 4,1,2:3,4 cutout 7,9",
        "any_clean 1", "any_grid 0", "any_matte 1", "any_stroke 1", "entry_of 0 1 3 4 4 5 6", "any_cutout 1"]
    # without `points` the first derived click is the head's own
    assert planners([f"h:{EMPTY}", "c:12,2,1,0", "c:11,4,0,3", "c:13,9,0,0"], points=0)[0] == \
        "prompt 0 clicks 2 box 0 points 3 entries 0,1 stages 2 clean 0,0 grid 0,0,0 matte 2,4,650,3 stroke 1,1,2:0,1 cutout 3,9"


REFUSALS = [
    ([f"h:{EMPTY}", "c:13,8,0,0"], {}, 1, "directly behind a matte mark"),
    ([f"h:{EMPTY}", "c:1,0,0,0", "c:13,8,0,0"], {}, 2, "directly behind a matte mark"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:6,1,1,0", "c:13,8,0,0"], {}, 3, "directly behind a matte mark"),
    ([f"h:{EMPTY}", "c:11,8,0,4", f"h:{EMPTY}", "c:13,8,0,0"], {}, 3, "directly behind a matte mark"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:13,8,0,0", "c:1,0,0,0"], {}, 2, "not the last entry of its prompt"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:13,8,0,0", "c:11,8,0,4"], {}, 2, "not the last entry of its prompt"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:13,8,0,0", "c:13,8,0,0"], {}, 3, "second"),
    ([f"h:{EMPTY}", "c:11,8,0,1", "c:13,8,0,0"], {}, 2, "one channel"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:13,8,0,0!"], {}, 2, "NULL"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:13,8,0,0="], {}, 2, "pointer of its prompt's head, entry 0"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:13,33,0,0"], {}, 2, r"radius is 0 \(the default, 16\) \.\. 32"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:13,-1,0,0"], {}, 2, r"radius is 0 \(the default, 16\) \.\. 32"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:13,8,1,0"], {}, 2, "third and fourth int are 0"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:13,8,0,7"], {}, 2, "third and fourth int are 0"),
    (["c:13,8,0,0", f"h:{EMPTY}"], {}, 0, "needs a prompt in front"),
    (["c:11,8,0,4", "c:13,8,0,0", f"h:{EMPTY}"], {}, 1, "needs a prompt in front"),
    ([f"h:{EMPTY}", "c:11,8,0,4", "c:13,8,0,0"], {"device": 1}, 2, "dlimg_amd_get_segmentation_masks_device"),
]


@pytest.mark.parametrize("entries,how,entry,why", REFUSALS, ids=[f"{i}-{re.sub('[^a-z0-9]+', '_', r[3][:24].lower())}" for i, r in enumerate(REFUSALS)])
def test_planner_refusals_name_the_mark_and_the_callers_entry(planners, entries, how, entry, why):
    out = planners(entries, **how)
    assert len(out) == 1 and out[0].startswith(f"error mask batch: entry {entry}: a cut-out mark "), out
    assert re.search(why, out[0]), out


def test_refusals_of_the_inner_planners_keep_the_callers_numbering(planners):
    # a grid prompt is refused through its matte, by the matte's entry
    out = planners([f"h:{EMPTY}", "c:11,8,0,4", "c:13,0,0,0", f"h:{EMPTY}", "c:7,4,0,0", "c:11,8,0,4", "c:13,0,0,0"])
    assert out == [o for o in out if o.startswith("error mask batch: entry 5: a matte mark ") and "grid prompt" in o] and len(out) == 1, out
    # entries behind a cut-out mark are renumbered back
    out = planners([f"h:{EMPTY}", "c:11,8,0,4", "c:13,0,0,0", f"h:{EMPTY}", "c:5,0,0,0"])
    assert out[0].startswith("error mask batch: entry 4:") and "label" in out[0], out
    out = planners([f"h:{EMPTY}", "c:11,8,0,4", "c:13,0,0,0", f"h:{EMPTY}", "c:1,0,0,0", "c:8,0,0,0"])
    assert out[0].startswith("error mask batch: entry 5: a prior mark"), out
    out = planners([f"h:{EMPTY}", "c:11,8,0,4", "c:13,0,0,0", f"h:{EMPTY}", "c:11,8,0,2", "c:13,0,0,0"])
    assert out[0].startswith("error mask batch: entry 4: a matte mark") and "channels" in out[0], out
    out = planners([f"h:{EMPTY}", "c:11,8,0,4", "c:13,0,0,0", f"h:{EMPTY}", "c:11,8,0,4", "c:12,2,1,0"])
    assert out[0].startswith("error mask batch: entry 5: a stroke mark") and "behind a clean-up or matte mark" in out[0], out
    out = planners([f"h:{EMPTY}", "c:11,8,0,4", "c:13,0,0,0", f"h:{EMPTY}", "c:12,2,1,0!"])
    assert out[0].startswith("error mask batch: entry 4: a stroke mark") and "NULL" in out[0], out
    # the matte's own refusal comes through with its number: a null guide in front of a cut-out
    out = planners([f"h:{EMPTY}", "c:11,8,0,4!", "c:13,0,0,0"])
    assert out[0].startswith("error mask batch: entry 1: a matte mark") and "NULL" in out[0], out


def test_a_call_without_cutout_marks_is_planned_as_before(planners):
    calls = [([f"h:{EMPTY}", "c:1,0,0,0", "h:1,2,30,40", "c:0,0,0,0", "c:6,3,4,0"], {}),
             (["h:1,2,30,40", "h:5,5,1,1"], {}), (["h:1,2,30,40"], {"points": 0}), (["h:0,0,0,0", "h:0,0,0,0"], {"regions": 0}),
             ([f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0", f"h:{EMPTY}", "c:7,8,900,0"], {}),
             ([f"h:{EMPTY}", "c:8,0,0,0", "c:1,0,0,0", "c:11,8,0,4"], {}), ([f"h:{EMPTY}", "c:10,0,0,0", "c:1,0,0,0", "c:6,2,2,0", "c:11,3,9,1"], {}),
             ([f"h:{EMPTY}", "c:10,0,0,0"], {"points": 0}), ([f"h:{EMPTY}", "c:11,8,0,4!"], {}), ([f"h:{EMPTY}", "c:11,8,0,4", "c:1,0,0,0"], {}),
             ([f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0"], {"branch": 0}), (["c:1,0,0,0"], {}), ([f"h:{EMPTY}", "c:9,0,0,0"], {}),
             ([f"h:{EMPTY}", "c:5,0,0,0"], {}), ([f"h:{EMPTY}", "c:1,0,0,0"], {"regions": 0}), ([f"h:{EMPTY}", "c:11,8,0,4"], {"device": 1})]
    for entries, how in calls:
        assert planners(entries, **how) == planners(entries, exe="stroke", **how) == planners(entries, exe="matte_cases", **how), (entries, how)
    # with stroke marks: what plan_stroke_prompts makes of it, line for line
    for entries, how in [([f"h:{EMPTY}", "c:12,2,1,0", "c:11,8,0,4"], {}), ([f"h:{EMPTY}", "c:12,0,1,0", "c:12,1,0,0"], {"points": 0}),
                         ([f"h:{EMPTY}", "c:12,9,1,0"], {}), ([f"h:{EMPTY}", "c:11,8,0,4", "c:12,2,1,0"], {})]:
        assert planners(entries, **how) == planners(entries, exe="stroke", **how), (entries, how)
    # 13 is no label where there are no `regions` to hold a mark
    assert planners([f"h:{EMPTY}", "c:13,8,0,0"], regions=0) == planners([f"h:{EMPTY}", "c:13,8,0,0"], regions=0, exe="stroke")


def test_click_entries_with_cutouts():
    r = api.Region(P(10, 20), P(300, 400))
    rgba, rgb, grey = np.zeros((4, 6, 4), np.uint8), np.zeros((4, 6, 3), np.uint8), np.zeros((4, 6), np.uint8)
    dst = np.zeros((4, 6, 4), np.uint8)
    assert api.CUTOUT_MARK == 13 and api.CUTOUT_DEFAULT_RADIUS == 16 and api.CUTOUT_MAX_RADIUS == 32
    e = api.click_entries([[P(1, 2), P(3, 4)], [P(7, 8)], [P(9, 10)]], [[1, 0], None, None], [None, r, None], [[1], None, None],
                          [(3, 4), None, None], matte=[(rgba, 8, 0), (rgb, 2, 1), (grey, 32, 65025)], cutout=[5, None, None])
    assert e.heads == [0, None, None, None, None, None, 1, None, 2, None]
    assert e.regions == [api.EMPTY_REGION, (4, 0, 0, 0), (0, 0, 0, 0), (6, 3, 4, 0), (11, 8, 0, 4), (13, 5, 0, 0), (10, 20, 300, 400),
                         (11, 2, 1, 3), api.EMPTY_REGION, (11, 32, 65025, 1)]
    assert e.cutouts[0][0] == 5 and e.cutouts[0][1].shape == (4, 6, 4) and e.cutouts[1] is None and e.cutouts[2] is None
    # (radius, out): the destination travels; radius 0 is the library's default
    e = api.click_entries([[P(1, 2)]], matte=[(rgba, 8, 0)], cutout=[(0, dst)])
    assert e.regions == [api.EMPTY_REGION, (11, 8, 0, 4), (13, 0, 0, 0)] and e.cutouts[0][1] is dst
    # entry lists without cut-outs are what they were
    a = api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], matte=[(rgba, 8, 0)])
    assert a == api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], matte=[(rgba, 8, 0)], cutout=None) \
        == api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], matte=[(rgba, 8, 0)], cutout=[None])
    assert a.cutouts == []
    for bad, matte in (([5], None), ([5], [(grey, 8, 0)]), ([33], [(rgba, 8, 0)]), ([-1], [(rgba, 8, 0)]), ([(5, dst[:, :, :3])], [(rgba, 8, 0)]),
                       ([(5, dst.astype(np.int32))], [(rgba, 8, 0)]), ([(5, np.zeros((5, 6, 4), np.uint8))], [(rgba, 8, 0)]),
                       ([5, None], [(rgba, 8, 0)]), (["5"], [(rgba, 8, 0)])):
        with pytest.raises(api.Error):
            api.click_entries([[P(1, 2)]], matte=matte, cutout=bad)


def test_planner_on_random_entry_lists_under_address_sanitizer(tmp_path):
    """csrc/cutout_plan.hpp on 6000 random batch mask calls with ASan + UBSan, every served call checked against what the batch
    calls rely on (tests/cutout_plan_cases.cpp, `fuzz`): a stand-alone program on the CPU, nothing loaded into Python."""
    clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    if not clang.exists():
        pytest.skip("ROCm clang not found")
    exe = tmp_path / "cutout_plan_cases_san"
    r = subprocess.run([str(clang), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", f"-I{CSRC}", str(ROOT / "tests" / "cutout_plan_cases.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and "sanitizer" in (r.stderr + r.stdout).lower() and "cannot find" in (r.stderr + r.stdout).lower():
        pytest.skip("this clang has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "fuzz", "6000", "17"], capture_output=True, text=True, errors="replace", timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    served = int(re.search(r"served (\d+)", r.stdout).group(1))
    assert 100 < served < 5900, r.stdout
