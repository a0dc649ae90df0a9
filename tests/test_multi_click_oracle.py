"""Several clicks per prompt on the CPU.

* the inputs of the GPU tests (tests/test_gpu_multi_click.py), confirmed from the float64 reference alone: for every case of
  multi_click_cases the reference mask changes by at least ten times what the GPU parity test lets a mask disagree in, both
  when the last click is left out and when its label is flipped; the cases cover 9, 12 and 15 token rows, with and without a
  box, and a background click on each image;
* the Python wrapper's entry-list builder (dlimgedit_amd.api.click_entries / pack_clicks, pure host code): order of the
  entries, the padding-point rule, labels, grouping by token rows with the per-launch cuts, the 8-click cap, the refusals;
* the library's own reading of the entry lists, its grouping of prompts into decoder chunks and the points it packs for
  the decoder (csrc/prompt_plan.hpp, printed by tests/prompt_plan_cases.cpp, built here with the host compiler): the packed
  coordinates and labels equal the Python side's exactly.
Every expectation is worked out by hand from the rules; none is printed from the code under test."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import multi_click_cases as M
from dlimgedit_amd import api
from dlimgedit_amd import weights as W
from dlimgedit_amd.api import click_entries, pack_clicks      # fails to import without the feature
from dlimgedit_amd.sam_config import get_config
from oracle import sam_oracle as O

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dlimgedit_amd" / "csrc"
P = api.Point


def test_wrapper_has_the_click_form():
    assert callable(api.Segmentation.compute_mask_clicks)
    assert "dlimg_amd_get_segmentation_masks_device" in api.ext.EXPORTS and len(api.ext.EXPORTS) == 23


def test_cases_cover_what_the_gpu_tests_need():
    rows = [M.token_rows(c) for c in M.CASES]
    assert {9, 12, 15} <= set(rows) and min(rows) >= 8 and max(rows) == 15
    assert {(M.token_rows(c), c[3] is not None) for c in M.CASES} >= {(9, True), (9, False), (12, True), (12, False), (15, True)}
    for name in M.IMAGES:
        assert any(c[0] == name and 0 in c[2] for c in M.CASES), name
    assert {c[2][-1] for c in M.CASES} == {0, 1}          # the flipped click is a background click in some, foreground in others
    for _, clicks, labels, _ in M.CASES:
        assert 2 <= len(clicks) == len(labels) <= 8 and labels[0] == 1


def test_the_limit_is_three_times_the_measured_figures():
    assert M.PARENT_TWO_TOKEN_FRACTION > 0 and M.PARENT_THREE_TOKEN_FRACTION > 0
    assert M.DISAGREE_LIMIT == 3 * max(M.PARENT_TWO_TOKEN_FRACTION, M.PARENT_THREE_TOKEN_FRACTION)


@pytest.fixture(scope="module")
def oracle_segs():
    cfg = get_config("vit_test")
    params = W.synthetic_weights(cfg, 7)
    return {name: O.OracleSegmentation(params, cfg).process(M.image(name), O.CH_RGBA) for name in M.IMAGES}, params


def test_the_last_click_and_its_label_move_the_reference_mask(oracle_segs):
    segs, params = oracle_segs
    for case in M.CASES:
        seg = segs[case[0]]
        w, h = seg.rs.original
        masks = {}
        for kind, (c, l, b) in M.variants(case).items():
            masks[kind], plane = M.reference_mask(seg.embedding, seg.rs, c, l, b, params, (h, w))
            assert plane == 0 or len(c) + (2 if b is not None else 1) == 2, (M.case_id(case), kind, plane)
        allowed = M.DISAGREE_LIMIT * w * h
        for other in ("without_last", "flipped"):
            differing = int((masks["full"] != masks[other]).sum())
            print(f"multi_click.oracle.{M.case_id(case)}.{other}: {differing} pixels, {differing / (w * h):.3f}")
            assert differing >= 10 * allowed, (M.case_id(case), other, differing, allowed)


def test_packed_order_and_padding_point():
    r = api.Region(P(10, 20), P(300, 400))
    # clicks in the order given, then top-left and bottom-right (labels 2, 3); no padding point with a box
    assert pack_clicks([P(5, 6), P(7, 8), P(9, 1)], [1, 0, 1], r) == ([(5, 6), (7, 8), (9, 1), (10, 20), (300, 400)], [1, 0, 1, 2, 3])
    # the padding point (0, 0), label -1, only without a box
    assert pack_clicks([P(5, 6), P(7, 8)], [1, 0]) == ([(5, 6), (7, 8), (0, 0)], [1, 0, -1])
    assert pack_clicks([P(5, 6)], None) == ([(5, 6), (0, 0)], [1, -1])             # today's point prompt
    assert pack_clicks([P(5, 6)], None, r) == ([(5, 6), (10, 20), (300, 400)], [1, 2, 3])      # today's box + point prompt
    # the shared packer of the tests agrees (identity frame: a 1024 x 1024 image)
    rs = O.ResizeLongestSide()
    rs.target_extent(1024, 1024)
    coords, labels = M.pack(rs, ((5, 6), (7, 8)), (1, 0), (10, 20, 300, 400))
    assert coords.tolist() == [[5, 6], [7, 8], [10, 20], [300, 400]] and labels.tolist() == [1, 0, 2, 3]


def test_entry_lists():
    r = api.Region(P(10, 20), P(300, 400))
    e = click_entries([[P(1, 2), P(3, 4), P(5, 6)], [P(7, 8)], [P(9, 10), P(11, 12)]], [[1, 0, 1], None, [1, 0]], [None, r, r])
    # one entry per click; the head carries the handle and the box (an empty region: none), a further click its label
    assert e.heads == [0, None, None, 1, 2, None]
    assert e.points == [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12)]
    assert e.regions == [(0, 0, -1, -1), (0, 0, 0, 0), (1, 0, 0, 0), (10, 20, 300, 400), (10, 20, 300, 400), (0, 0, 0, 0)]
    assert e.prompt_heads == [0, 3, 4]
    assert e.token_rows == [9, 8, 9]                       # 6 + 3 clicks; 7 + 1 click; 7 + 2 clicks
    assert e.launches == [(9, [0, 2]), (8, [1])]           # grouped by token rows, groups in order of first appearance
    assert api._entry_calls(e) == [([0, 1, 2, 3, 4, 5], True)]
    # without a second click anywhere the entries are today's: prompts without a box in a call without regions
    e = click_entries([[P(1, 2)], [P(3, 4)], [P(5, 6)]], None, [None, r, None])
    assert e.heads == [0, 1, 2] and e.token_rows == [7, 8, 7]
    assert api._entry_calls(e) == [([0, 2], False), ([1], True)]


def test_launches_are_cut_at_112_token_rows():
    clicks = lambda n: [P(k, k) for k in range(n)]          # noqa: E731
    r = api.Region(P(0, 0), P(9, 9))
    # 8 clicks and a box: 15 rows, 7 prompts per launch; 3 clicks: 9 rows, 12 per launch; 5 clicks and a box: 12 rows, 9
    e = click_entries([clicks(8)] * 8 + [clicks(3)] * 13 + [clicks(5)] * 10, None, [r] * 8 + [None] * 13 + [r] * 10)
    assert e.token_rows == [15] * 8 + [9] * 13 + [12] * 10
    assert e.launches == [(15, list(range(7))), (15, [7]), (9, list(range(8, 20))), (9, [20]), (12, list(range(21, 30))), (12, [30])]
    assert len(e.heads) == 8 * 8 + 13 * 3 + 10 * 5 and e.prompt_heads[:3] == [0, 8, 16]


def test_builder_refusals():
    for bad in (dict(clicks=[[P(0, 0)] * 9]), dict(clicks=[[]]), dict(clicks=[[P(0, 0)] * 2], labels=[[1, 2]]),
                dict(clicks=[[P(0, 0)] * 2], labels=[[1, -1]]), dict(clicks=[[P(0, 0)] * 2], labels=[[1]]),
                dict(clicks=[[P(0, 0)] * 2], labels=[[0, 1]]), dict(clicks=[[P(0, 0)]], regions=[None, None])):
        with pytest.raises(api.Error):
            click_entries(**bad)
    assert click_entries([[P(0, 0)] * 8]).token_rows == [14]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    rocm_clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    cxx = str(rocm_clang) if rocm_clang.exists() else (shutil.which("c++") or shutil.which("g++") or shutil.which("clang++"))
    assert cxx, "no host C++ compiler found"
    exe = tmp_path_factory.mktemp("prompt_plan") / "prompt_plan_cases"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(ROOT / "tests" / "prompt_plan_cases.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(entries, points=True, regions=True, chunk=8):
        r = subprocess.run([str(exe), str(int(points)), str(int(regions)), str(chunk), *entries], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


EMPTY = "0,0,-1,-1"
BOX = "10,20,300,400"


def test_library_reads_the_entry_lists(plan):
    # three clicks without a box (labels 1, 0, 1), one click with a box, two clicks with a box
    out = plan([f"h0:{EMPTY}", "c0:0,0,0,0", "c0:1,0,0,0", f"h0:{BOX}", f"h0:{BOX}", "c0:0,0,0,0"])
    assert out == ["prompt 0 clicks 3 box 0 points 4 labels 1,0,1", "prompt 3 clicks 1 box 1 points 3 labels 1",
                   "prompt 4 clicks 2 box 1 points 4 labels 1,0",
                   "chunk 0 points 4 prompts 0,2", "chunk 0 points 3 prompts 1"]
    # regions == NULL: every click is a foreground click, nobody has a box
    out = plan([f"h0:{EMPTY}", "c0:0,0,0,0", f"h0:{EMPTY}"], regions=False)
    assert out == ["prompt 0 clicks 2 box 0 points 3 labels 1,1", "prompt 2 clicks 1 box 0 points 2 labels 1",
                   "chunk 0 points 3 prompts 0", "chunk 0 points 2 prompts 1"]


def test_calls_without_a_continuation_entry_are_read_as_before(plan):
    # an empty region means nothing special there: both arrays given is box + point, whatever the box
    assert plan([f"h0:{EMPTY}", f"h0:{BOX}"])[:2] == ["prompt 0 clicks 1 box 1 points 3 labels 1", "prompt 1 clicks 1 box 1 points 3 labels 1"]
    assert plan([f"h0:{BOX}"] * 2, points=False)[:2] == ["prompt 0 clicks 0 box 1 points 2 labels", "prompt 1 clicks 0 box 1 points 2 labels"]
    # 19 point prompts: chunks of 8 in the caller's order, as always
    out = plan([f"h0:{EMPTY}"] * 19, regions=False)
    assert out[19:] == ["chunk 0 points 2 prompts 0,1,2,3,4,5,6,7", "chunk 0 points 2 prompts 8,9,10,11,12,13,14,15",
                        "chunk 0 points 2 prompts 16,17,18"]


def test_library_counts_prompts_not_entries_and_keeps_a_prompt_on_its_replica(plan):
    three = [f"h0:{EMPTY}", "c0:1,0,0,0", "c0:0,0,0,0"]              # 3 clicks: 4 points
    other = [f"h1:{EMPTY}", "c1:0,0,0,0"]                            # 2 clicks on replica 1: 3 points
    out = plan(three * 9 + other + three * 1 + [f"h1:{BOX}"])
    prompts = [line for line in out if line.startswith("prompt")]
    assert len(prompts) == 12 and prompts[9] == "prompt 27 clicks 2 box 0 points 3 labels 1,0"
    # replica 0: ten prompts of 4 points -> chunks of 8 and 2 PROMPTS (30 entries); replica 1: 2 clicks, and 1 click with a
    # box, are 3 points each: one chunk
    assert [line for line in out if line.startswith("chunk")] == [
        "chunk 0 points 4 prompts 0,1,2,3,4,5,6,7", "chunk 0 points 4 prompts 8,10", "chunk 1 points 3 prompts 9,11"]


def test_library_refusals(plan):
    assert plan([f"h0:{EMPTY}"] + ["c0:1,0,0,0"] * 7)[0] == "prompt 0 clicks 8 box 0 points 9 labels 1,1,1,1,1,1,1,1"
    assert plan([f"h0:{EMPTY}"] + ["c0:1,0,0,0"] * 8)[0].startswith("error") and "more than 8 clicks" in plan([f"h0:{EMPTY}"] + ["c0:1,0,0,0"] * 8)[0]
    assert "continuation" in plan(["c0:1,0,0,0", f"h0:{EMPTY}"])[0] and plan(["c0:1,0,0,0", f"h0:{EMPTY}"])[0].startswith("error")
    for bad in ("c0:2,0,0,0", "c0:-1,0,0,0", "c0:1,0,0,7", "c0:0,1,0,0"):
        line = plan([f"h0:{EMPTY}", bad])[0]
        assert line.startswith("error") and "label" in line, bad
    # a click needs `points`; a call needs one of the arrays
    assert plan([f"h0:{BOX}", "c0:1,0,0,0"], points=False)[0].startswith("error")
    assert plan([f"h0:{BOX}"], points=False, regions=False)[0].startswith("error")


def test_library_packs_the_multi_click_cases_as_the_python_side_does(plan):
    """pack_points on the eight CASES, both images, in one call: exact equality with multi_click_cases.pack (integers held
    in floats: no tolerance)."""
    entries, heads = [], []
    for name, clicks, labels, box in M.CASES:
        heads.append(len(entries))
        extent = M.oracle_frame(name)[1]
        region = ",".join(map(str, box)) if box is not None else EMPTY
        entries.append(f"h0:{region}@{clicks[0][0]},{clicks[0][1]}@{extent}")
        entries += [f"c0:{l},0,0,0@{x},{y}" for (x, y), l in zip(clicks[1:], labels[1:])]
    rows = M.packed_lines(plan(entries))
    assert [r[0] for r in rows] == [[h] for h in heads]
    for (_, coords, labels), case in zip(rows, M.CASES):
        want_c, want_l = M.pack(M.oracle_frame(case[0])[0], *case[1:])
        assert coords == want_c.tolist() and labels == want_l.tolist(), M.case_id(case)
    assert any(c != [list(map(float, xy)) for xy in case[1]] + c[len(case[1]):] for (_, c, _), case in zip(rows, M.CASES)
               if case[0] == "wide")         # the image whose longest side is not 1024 is scaled


def test_library_packs_the_single_prompt_forms_as_the_oracle_does(plan):
    """A point, a box, a box and a point, on both images: oracle.sam_oracle.pack_prompt and box_point_cases.prompts."""
    import box_point_cases as B
    for name, box, point in B.PAIRS:
        rs, extent = M.oracle_frame(name)
        want, _ = B.prompts(rs, box, point)
        entry = f"h0:{','.join(map(str, box))}@{point[0]},{point[1]}@{extent}"
        for kind, given in (("point", dict(regions=False)), ("box", dict(points=False)), ("both", {})):
            rows = M.packed_lines(plan([entry], **given))
            assert len(rows) == 1 and rows[0][0] == [0]
            assert rows[0][1] == want[kind][0].tolist() and rows[0][2] == want[kind][1].tolist(), (name, kind)
    assert {p[0] for p in B.PAIRS} == set(M.IMAGES)
