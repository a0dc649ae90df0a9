"""Mask clean-up on the CPU.

* the reference (tests/cleanup_ref.py, run-based union-find) agrees on every named case with a second restatement of the rule
  through scipy.ndimage.label, where scipy is installed;
* the cases are not vacuous: apart from the empty, full and checkerboard masks the reference changes at least one pixel of
  every case, and hand-made masks come out as worked out by hand (the tie rule, the strict comparison, holes before islands);
* the library's planner (csrc/prompt_plan.hpp: plan_cleaned_prompts, printed by tests/clean_plan_cases.cpp, built with the
  host compiler): marks are read into per-prompt thresholds, prompts / stages / chunks are those of the call without its
  clean-up marks, every refusal says "mark" and names the caller's entry, a box-only call may carry marks, a click without
  `points` is refused with the text it always had;
* the wrapper's builder (dlimgedit_amd.api.click_entries with clean=) emits exactly those entry lists and refuses what the
  library refuses; CLEAN_MARK is the header's DLIMG_CLEAN_MARK, and the C++ wrapper's forms compile.
"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cleanup_cases as CC
from cleanup_ref import cleanup_ref, label8
from dlimgedit_amd import api

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dlimgedit_amd" / "csrc"
P = api.Point


def _cxx():
    rocm_clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    cxx = str(rocm_clang) if rocm_clang.exists() else (shutil.which("c++") or shutil.which("g++") or shutil.which("clang++"))
    assert cxx, "no host C++ compiler found"
    return cxx


# ---- the reference

def _scipy_cleanup(ndi, mask, max_hole, max_island):
    eight = np.ones((3, 3))
    m = mask > 0
    if max_hole > 0:
        lab, n = ndi.label(~m, structure=eight)
        areas = np.bincount(lab.ravel(), minlength=n + 1)
        fill = areas < max_hole
        fill[0] = False
        m = m | fill[lab]
    if max_island > 0:
        lab, n = ndi.label(m, structure=eight)       # scipy numbers components by their first pixel in raster order, too
        if n:
            areas = np.bincount(lab.ravel(), minlength=n + 1)
            keep = areas >= max_island
            keep[0] = False
            if not keep.any():
                flat = lab.ravel()
                idx = np.flatnonzero(flat)
                _, where = np.unique(flat[idx], return_index=True)
                first = idx[where]                   # first pixel of component 1 .. n
                best = max(range(1, n + 1), key=lambda c: (areas[c], -first[c - 1]))
                keep[best] = True
            m = keep[lab]
    return np.where(m, 255, 0).astype(np.uint8)


def test_reference_agrees_with_scipy_on_every_case():
    ndi = pytest.importorskip("scipy.ndimage")
    for case in CC.cases():
        name, mask, hole, island = case
        assert np.array_equal(CC.expected(case), _scipy_cleanup(ndi, mask, hole, island)), name


def test_cases_are_not_vacuous_and_cover_what_the_issue_names():
    names = [c[0] for c in CC.cases()]
    assert len(set(names)) == len(names)
    patterns = {CC.pattern_of(c) for c in CC.cases()}
    assert {"empty", "full", "spiral", "spiral_cut", "checkerboard", "comb", "comb_inverted", "noise1", "noise5", "noise9", "nested",
            "corner", "corner_anti", "largest_unique", "largest_tie", "equal_threshold"} <= patterns
    sizes = {c[1].shape[::-1] for c in CC.cases()}
    assert sizes == set(CC.SIZES)
    assert {(c[2] > 0, c[3] > 0) for c in CC.cases()} == {(True, False), (False, True), (True, True)}
    for case in CC.cases():
        name, mask, hole, island = case
        assert mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 255} and (hole > 0 or island > 0)
        out = CC.expected(case)
        if CC.pattern_of(case) in CC.UNCHANGED_PATTERNS:
            continue
        assert (out != mask).any(), f"{name}: the reference changes nothing"
    for case in CC.cases():
        if CC.pattern_of(case) == "checkerboard":
            assert np.array_equal(CC.expected(case), case[1])        # one component per polarity: nothing is small
    jobs = CC.multi_job_call()
    assert len({c[1].shape for c in jobs}) == 3


def test_reference_by_hand():
    X, o = 255, 0
    m = np.array([[X, o, X, X, o],
                  [o, o, o, o, o],
                  [X, X, o, o, X]], np.uint8)
    lab, areas = label8(m > 0)
    assert lab.tolist() == [[1, 0, 2, 2, 0], [0, 0, 0, 0, 0], [3, 3, 0, 0, 4]] and areas.tolist() == [0, 1, 2, 2, 1]
    # strict: area 2 is not below 2
    assert cleanup_ref(m, 0, 2).tolist() == [[o, o, X, X, o], [o, o, o, o, o], [X, X, o, o, o]]
    # all below 3: the largest stays, and of the two of area 2 the one that comes first in raster order
    assert cleanup_ref(m, 0, 3).tolist() == [[o, o, X, X, o], [o, o, o, o, o], [o, o, o, o, o]]
    # diagonal neighbours are connected, for the background too
    d = np.array([[X, o], [o, X]], np.uint8)
    assert label8(d > 0)[1].tolist() == [0, 2] and label8(d == 0)[1].tolist() == [0, 2]
    # holes first: filling the hole lifts the ring over the island threshold and swallows the pixel inside it
    ring = np.zeros((7, 7), np.uint8)
    ring[1:6, 1:6] = X
    ring[2:5, 2:5] = o
    ring[3, 3] = X
    both = cleanup_ref(ring, 9, 20)
    assert (both[1:6, 1:6] == X).all() and both.sum() == 25 * 255          # 16 + 8 + 1 = 25 >= 20
    assert cleanup_ref(ring, 8, 0).tolist() == ring.tolist()               # the hole has 8 pixels: not below 8
    islands_only = cleanup_ref(ring, 0, 20)                                # ring 16, centre 1: all below, the ring stays
    assert islands_only[3, 3] == o and islands_only.sum() == 16 * 255
    # nothing to label: left as it is
    assert cleanup_ref(np.zeros((3, 4), np.uint8), 0, 5).sum() == 0
    assert (cleanup_ref(np.full((3, 4), X, np.uint8), 5, 0) == X).all()


# ---- the planner

@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = tmp_path_factory.mktemp("clean_plan") / "clean_plan_cases"
    r = subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(ROOT / "tests" / "clean_plan_cases.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(entries, points=True, regions=True, branch=True):
        r = subprocess.run([str(exe), str(int(points)), str(int(regions)), str(int(branch)), *entries], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


EMPTY, BOX, MARK = "h:0,0,-1,-1", "h:10,20,300,400", "c:4,0,0,0"
FG, BG = "c:1,0,0,0", "c:0,0,0,0"


def CLEAN(a, b):
    return f"c:6,{a},{b},0"


def test_library_reads_clean_marks_into_thresholds(plan):
    # a point with a mark (the empty region is "no box" although the mark is the call's only continuation entry), a boxed
    # prompt of two clicks without one, a staged prompt with one, a box + point with one
    out = plan([EMPTY, CLEAN(40, 0), BOX, BG, EMPTY, MARK, BG, CLEAN(0, 7), BOX, CLEAN(5, 6)])
    assert out == ["prompt 0 clicks 1 box 0 points 2 entries 0 labels 1 stages 1 clean 40,0",
                   "prompt 2 clicks 2 box 1 points 4 entries 2,3 labels 1,0 stages 2 clean 0,0",
                   "prompt 4 clicks 2 box 0 points 3 entries 4,6 labels 1,0 stages 1,2 clean 0,7",
                   "prompt 8 clicks 1 box 1 points 3 entries 8 labels 1 stages 1 clean 5,6",
                   "any_clean 1",
                   "chunk points 2 prompts 0", "chunk points 4 prompts 1", "chunk points 3 prompts 3"]
    # a box-only call (no `points`) may clean its masks; an empty region there leaves nothing to decode
    assert plan([BOX, CLEAN(9, 9), BOX], points=False) == [
        "prompt 0 clicks 0 box 1 points 2 entries labels stages 0 clean 9,9",
        "prompt 2 clicks 0 box 1 points 2 entries labels stages 0 clean 0,0", "any_clean 1", "chunk points 2 prompts 0,1"]
    # marks do not count towards the 8 clicks
    out = plan([EMPTY] + [FG] * 7 + [CLEAN(1, 0)])
    assert out[0] == "prompt 0 clicks 8 box 0 points 9 entries 0,1,2,3,4,5,6,7 labels 1,1,1,1,1,1,1,1 stages 8 clean 1,0"


def _without_marks(entries):
    kept = [i for i, e in enumerate(entries) if not e.startswith("c:6,")]
    return [entries[i] for i in kept], kept


def _renumbered(lines, kept):
    """The lines of the call without clean-up marks, its entries numbered as in the caller's list, thresholds dropped."""
    out = []
    for line in lines:
        w = line.split()
        if w[0] == "prompt":
            w[1] = str(kept[int(w[1])])
            at = w.index("entries") + 1
            if w[at] != "labels":
                w[at] = ",".join(str(kept[int(e)]) for e in w[at].split(","))
            w = w[:w.index("clean")]
        out.append(" ".join(w))
    return out


def test_prompts_stages_and_chunks_are_those_of_the_call_without_clean_marks(plan):
    calls = [
        [EMPTY, CLEAN(40, 0), BOX, BG, EMPTY, MARK, BG, CLEAN(0, 7), BOX, CLEAN(5, 6)],
        [BOX, FG, BG, CLEAN(3, 3), EMPTY, FG, BOX, MARK, FG, MARK, BG, CLEAN(1, 1), EMPTY, BG, CLEAN(2, 0)],
        [EMPTY, FG, CLEAN(3, 3)] * 9 + [BOX, FG] * 9,            # more prompts than a chunk holds
    ]
    for entries in calls:
        stripped, kept = _without_marks(entries)
        assert any(e.startswith("c:") for e in stripped)          # the stripped call keeps a continuation entry: same box rule
        with_marks = plan(entries)
        assert not with_marks[0].startswith("error"), with_marks[0]
        mine = [" ".join(l.split()[:l.split().index("clean")]) if l.startswith("prompt") else l for l in with_marks]
        assert [l for l in mine if not l.startswith("any_clean")] == [l for l in _renumbered(plan(stripped), kept) if not l.startswith("any_clean")]
    # a call without clean-up marks: the thresholds are all 0 and nothing else is said
    out = plan([EMPTY, BG, BOX])
    assert out == ["prompt 0 clicks 2 box 0 points 3 entries 0,1 labels 1,0 stages 2 clean 0,0",
                   "prompt 2 clicks 1 box 1 points 3 entries 2 labels 1 stages 1 clean 0,0", "any_clean 0",
                   "chunk points 3 prompts 0,1"]


def test_refusals_say_mark_and_name_the_callers_entry(plan):
    refused = {
        "not the last entry of its prompt": ([EMPTY, CLEAN(3, 3), FG], 1),
        "two marks in one prompt": ([EMPTY, FG, CLEAN(3, 3), CLEAN(4, 4)], 2),
        "in front of any head": ([CLEAN(3, 3), EMPTY, FG], 0),
        "negative max_hole": ([EMPTY, FG, CLEAN(-1, 3)], 2),
        "negative max_island": ([EMPTY, FG, CLEAN(3, -2)], 2),
        "both thresholds 0": ([BOX, CLEAN(0, 0)], 1),
        "fourth int": ([BOX, "c:6,3,3,1"], 1),
        "second prompt's mark before its click": ([EMPTY, FG, CLEAN(1, 1), BOX, CLEAN(3, 3), FG], 4),
        "a refinement mark directly in front of a clean-up mark": ([EMPTY, CLEAN(2, 2), EMPTY, FG, MARK, CLEAN(3, 3)], 4),
        "a refinement mark of a model without the branch": ([EMPTY, CLEAN(2, 2), EMPTY, MARK, FG, CLEAN(3, 3)], 3),
    }
    for what, (entries, at) in refused.items():
        line = plan(entries, branch=what.find("without the branch") < 0)[0]
        assert line.startswith("error") and "mark" in line and f"entry {at}:" in line, (what, line)
    # the refinement mark keeps its own words
    line = plan([EMPTY, CLEAN(2, 2), EMPTY, FG, MARK, CLEAN(3, 3)])[0]
    assert "a refinement mark is the last entry of its prompt: every stage adds at least one click" in line
    # neither a click nor a box: no `points`, and the empty region is no box
    line = plan([BOX, CLEAN(3, 3), EMPTY, CLEAN(3, 3)], points=False)[0]
    assert line.startswith("error") and "mark" in line and "entry 2:" in line
    # refusals of the ordinary rules name the caller's entry too
    line = plan([EMPTY, CLEAN(3, 3), EMPTY, "c:2,0,0,0"])[0]
    assert line.startswith("error") and "entry 3:" in line and "label" in line
    line = plan([EMPTY, CLEAN(3, 3), BOX] + [FG] * 8)[0]
    assert line.startswith("error") and "the prompt of entry 2 has more than 8 clicks" in line


def test_old_refusals_keep_their_words(plan):
    # a click without `points`, with or without a clean-up mark in the call
    text = "error mask batch: a continuation entry (null handle) is a click and needs `points`"
    assert plan([BOX, FG], points=False) == [text]
    assert plan([BOX, FG, CLEAN(3, 3)], points=False) == [text]
    assert plan([BOX, CLEAN(3, 3), BOX, FG], points=False) == [text]
    # 5 is still a label, and a refused one
    for more in ([], [CLEAN(3, 3)]):
        line = plan([EMPTY, "c:5,0,0,0"] + more)[0]
        assert line.startswith("error") and "label" in line and "entry 1:" in line
    assert plan([], points=False, regions=False) == ["error mask batch: neither points nor regions given"]
    # without `regions` there are no marks: {6, ...} cannot be said, the entry is a foreground click
    assert plan([EMPTY, CLEAN(3, 3)], regions=False)[0] == "prompt 0 clicks 2 box 0 points 3 entries 0,1 labels 1,1 stages 2 clean 0,0"


# ---- the wrapper's builder

def test_entry_lists_with_clean_marks():
    r = api.Region(P(10, 20), P(300, 400))
    assert api.CLEAN_MARK == 6
    e = api.click_entries([[P(1, 2)], [P(3, 4), P(5, 6)], [P(7, 8), P(9, 10)]], [None, [1, 0], None], [None, r, None], [None, None, [1]],
                          clean=[(40, 0), None, (0, 7)])
    assert e.heads == [0, None, 1, None, 2, None, None, None]
    assert e.points == [(1, 2), (0, 0), (3, 4), (5, 6), (7, 8), (0, 0), (9, 10), (0, 0)]
    assert e.regions == [(0, 0, -1, -1), (6, 40, 0, 0), (10, 20, 300, 400), (0, 0, 0, 0), (0, 0, -1, -1), (4, 0, 0, 0), (1, 0, 0, 0),
                         (6, 0, 7, 0)]
    assert e.prompt_heads == [0, 2, 4] and e.token_rows == [7, 9, 8] and e.stage_clicks == [[1], [2], [1, 2]]
    assert api._entry_calls(e) == [(list(range(8)), True)]
    # launches are those of the same prompts without clean-up marks
    bare = api.click_entries([[P(1, 2)], [P(3, 4), P(5, 6)], [P(7, 8), P(9, 10)]], [None, [1, 0], None], [None, r, None], [None, None, [1]])
    assert e.launches == bare.launches and e.token_rows == bare.token_rows
    # one pair for all prompts
    e = api.click_entries([[P(1, 2)], [P(3, 4)]], clean=(5, 6))
    assert e.regions == [(0, 0, -1, -1), (6, 5, 6, 0), (0, 0, -1, -1), (6, 5, 6, 0)] and e.heads == [0, None, 1, None]
    # without clean the lists are what they were
    a, b = api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r]), api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], None, None)
    assert (a.heads, a.points, a.regions) == (b.heads, b.points, b.regions)
    # the points / regions form: entry i, then its mark; a box-only call has no points at all
    heads, pts, regs = api._marked_entries(2, None, [r, r], [(3, 0), None])
    assert heads == [0, None, 1] and pts is None and regs == [(10, 20, 300, 400), (6, 3, 0, 0), (10, 20, 300, 400)]
    heads, pts, regs = api._marked_entries(2, [P(1, 2), P(3, 4)], None, [None, (0, 9)])
    assert heads == [0, 1, None] and pts == [(1, 2), (3, 4), (0, 0)] and regs == [(0, 0, -1, -1), (0, 0, -1, -1), (6, 0, 9, 0)]


def test_builder_emits_what_the_library_reads(plan):
    r = api.Region(P(10, 20), P(300, 400))
    e = api.click_entries([[P(1, 2)], [P(3, 4), P(5, 6)], [P(7, 8), P(9, 10)]], [None, [1, 0], None], [None, r, None], [None, None, [1]],
                          clean=[(40, 0), None, (0, 7)])
    entries = [("h" if h is not None else "c") + ":" + ",".join(map(str, reg)) for h, reg in zip(e.heads, e.regions)]
    out = plan(entries)
    assert out[:3] == ["prompt 0 clicks 1 box 0 points 2 entries 0 labels 1 stages 1 clean 40,0",
                       "prompt 2 clicks 2 box 1 points 4 entries 2,3 labels 1,0 stages 2 clean 0,0",
                       "prompt 4 clicks 2 box 0 points 3 entries 4,6 labels 1,1 stages 1,2 clean 0,7"]
    assert [int(l.split()[1]) for l in out if l.startswith("prompt")] == e.prompt_heads


def test_builder_refuses_what_the_library_refuses():
    one = [[P(0, 0)]]
    for bad in ([(0, 0)], [(-1, 3)], [(3, -1)], [(3,)], [(1, 2, 3)], "ab", [(1.5, 2)], [(3, 3), (4, 4)], [None, None], (1.5, 2)):
        with pytest.raises(api.Error):
            api.click_entries(one, clean=bad)
    with pytest.raises(api.Error):
        api.click_entries(one, clean=(0, 0))
    with pytest.raises(api.Error):
        api.click_entries(one, clean=(2 ** 31, 1))
    with pytest.raises(api.Error):
        api.Segmentation.compute_mask_batch([], clean=(0, 0))


def test_headers_and_cpp_wrapper(tmp_path):
    """CLEAN_MARK == 6 == DLIMG_CLEAN_MARK == kCleanMark, and the wrapper's forms with a clean-up compile against the headers alone."""
    src = tmp_path / "clean.cpp"
    src.write_text('''#include <dlimgedit/dlimgedit.hpp>
static_assert(DLIMG_CLEAN_MARK == 6 && DLIMG_CLEAN_MARK != DLIMG_REFINE_MARK, "5 stays a refused label");
dlimg::Image one(dlimg::Segmentation const& s, std::vector<dlimg::Click> const& clicks) {
    return s.compute_mask(clicks, std::nullopt, {}, dlimg::MaskCleanup{4096, 4096});
}
dlimg::Image as_before(dlimg::Segmentation const& s, std::vector<dlimg::Click> const& clicks, dlimg::Region box) {
    return s.compute_mask(clicks, box, dlimg::Segmentation::refine_each(clicks.size()));
}
std::vector<dlimg::Image> many(dlimg::Segmentation const& s, std::vector<dlimg::Click> const& clicks, dlimg::Region box) {
    return dlimg::Segmentation::compute_mask_batch({&s, &s}, {clicks, clicks}, {box, std::nullopt}, {{1}, {}},
                                                   {dlimg::MaskCleanup{0, 64}, std::nullopt});
}
int main() { return 0; }
''')
    r = subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", "-DDLIMGEDIT_LOAD_DYNAMIC", f"-I{ROOT / 'include'}", "-fsyntax-only",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # the planner's constant is the header's (the library's own headers and the C++ wrapper do not share a translation unit)
    src = tmp_path / "planner.cpp"
    src.write_text('''#include <dlimgedit/dlimgedit.h>
#include "prompt_plan.hpp"
static_assert(dlimg::kCleanMark == DLIMG_CLEAN_MARK && dlimg::kRefineMark == DLIMG_REFINE_MARK, "one value on both sides");
int main() { return 0; }
''')
    r = subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{CSRC}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert api.CLEAN_MARK == 6
