"""Segment everything on the CPU.

* the reference itself (tests/grid_ref.py) on hand-made cases: strict comparisons at exactly 0 and +-1.0 (-0.0 included), an
  empty candidate, a zero-area box that never suppresses, an IoU tie broken by the candidate index, the cap of 255 kept
  segments, the smallest segment on top;
* the library's host logic (csrc/grid_plan.hpp, printed by tests/grid_plan_cases.cpp, built with the host compiler) gives the
  same NMS and label orders as the reference on the same records, hand-made and a few hundred seeded random sets; the same
  grid pixels; every refusal of a grid mark says "mark" and names the caller's entry; a call without grid marks is planned
  exactly as tests/clean_plan_cases.cpp (plan_cleaned_prompts) plans it;
* the wrapper's builder (dlimgedit_amd.api.click_entries with grid=) emits those entry lists; GRID_MARK is the header's
  DLIMG_GRID_MARK, and the C++ wrapper's forms compile.
"""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import grid_ref as G
from dlimgedit_amd import api

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dlimgedit_amd" / "csrc"
f32 = np.float32


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
def cases(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("grid_plan"), "grid_plan_cases")

    def run(*args, stdin=None):
        r = subprocess.run([str(exe), *[str(a) for a in args]], input=stdin, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def clean_plan(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("clean_plan"), "clean_plan_cases")

    def run(entries, points=True, regions=True, branch=True):
        r = subprocess.run([str(exe), str(int(points)), str(int(regions)), str(int(branch)), *entries], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def _select_compiled(cases, sets):
    """sets: [(records [n, >=7], iou [n], iou_permille, stability_permille)] -> [(nms, kept)]"""
    text = []
    for records, iou, ip, sp in sets:
        text.append(f"set {len(records)} {ip} {sp}")
        for r, v in zip(records, iou):
            bits = struct.unpack("<I", struct.pack("<f", float(f32(v))))[0]
            text.append(" ".join(str(int(x)) for x in r[:7]) + f" {bits:x}")
    lines = cases("select", stdin="\n".join(text) + "\n")
    assert len(lines) == 2 * len(sets)
    out = []
    for a, b in zip(lines[0::2], lines[1::2]):
        assert a.startswith("nms") and b.startswith("kept")
        out.append(([int(v) for v in a[3:].split(",") if v.strip()], [int(v) for v in b[4:].split(",") if v.strip()]))
    return out


def _plane(value=-5.0):
    return np.full((G.LOW, G.LOW), value, f32)


# ---- the reference on hand-made cases

def test_strict_comparisons_at_the_thresholds():
    p = _plane()
    p[0, 0:7] = [0.0, -0.0, 1.0, -1.0, np.nextafter(f32(0), f32(1)), np.nextafter(f32(1), f32(2)), np.nextafter(f32(-1), f32(0))]
    r = G.harvest([p], 1024, 1024)[0]
    # > +1: one (just above 1); > 0: 1.0, the smallest positive, just above 1; > -1: those, both zeros and just above -1
    assert list(r[:3]) == [1, 3, 6]
    assert list(r[3:7]) == [2, 0, 5, 0]


def test_scored_region_and_reach_box():
    p = _plane()
    p[100, 50] = 2.0       # just beyond the scored region of a 600 x 400 image (pre 1024 x 683: rows < 171)
    p[171, 10] = 2.0       # the one row beyond it that the taps reach
    p[172, 10] = 2.0       # beyond even that
    p[200, 255] = 2.0
    pre_w, pre_h = G.pre_extent(600, 400)
    assert (pre_w, pre_h) == (1024, 683)
    r = G.harvest([p], pre_w, pre_h)[0]
    assert list(r[:7]) == [1, 1, 1, 50, 100, 50, 100]
    assert int(r[7]) == 10 | 100 << 8 | 50 << 16 | 171 << 24


def test_an_empty_candidate_is_dropped():
    a, b = _plane(), _plane()
    b[10:20, 10:20] = 3.0
    rec = G.harvest([a, b], 1024, 1024)
    assert list(rec[0]) == [0, 0, 0, 0, 0, -1, -1, G.CULL_EMPTY]
    nms, kept = G.select(rec, [0.99, 0.99], 500, 500)
    assert nms == [1] and kept == [1]
    # n_lo > 0 alone does not make a candidate
    a[5, 5] = -0.5
    rec = G.harvest([a, b], 1024, 1024)
    assert list(rec[0][:3]) == [0, 0, 1]
    assert G.select(rec, [0.99, 0.99], 500, 500)[0] == [1]


def test_a_one_pixel_box_never_suppresses():
    one = np.array([[1, 1, 1, 7, 7, 7, 7, 0]] * 3)
    nms, kept = G.select(one, [0.9, 0.8, 0.7], 500, 500)
    assert nms == [0, 1, 2]              # identical boxes of area 0: union 0, nobody suppressed
    # a box inside a big one: inter / union is small, kept; an almost equal box: suppressed
    rec = np.array([[100, 100, 100, 0, 0, 10, 10, 0], [100, 100, 100, 0, 0, 10, 9, 0], [4, 4, 4, 2, 2, 4, 4, 0]])
    nms, kept = G.select(rec, [0.9, 0.8, 0.7], 500, 500)
    assert nms == [0, 2]
    # exactly at the threshold (inter 70, union 100): 700 > 700 is false, kept
    rec = np.array([[9, 9, 9, 0, 0, 10, 10, 0], [9, 9, 9, 0, 0, 10, 7, 0]])
    assert G.select(rec, [0.9, 0.8], 500, 500)[0] == [0, 1]
    rec[1, 6] = 8                        # inter 80, union 100
    assert G.select(rec, [0.9, 0.8], 500, 500)[0] == [0]


def test_an_iou_tie_goes_to_the_lower_index_and_labels_go_by_size():
    rec = np.array([[5, 5, 5, 0, 0, 4, 4, 0], [50, 50, 50, 20, 20, 40, 40, 0], [20, 20, 20, 60, 60, 70, 70, 0], [20, 20, 20, 80, 80, 90, 90, 0]])
    nms, kept = G.select(rec, [0.7, 0.9, 0.9, 0.9], 500, 500)
    assert nms == [1, 2, 3, 0]
    assert kept == [1, 2, 3, 0]          # n_mid descending, the tie 2 / 3 in NMS order: the smallest has the largest label
    # the two overlapping twins: the lower index survives
    rec = np.array([[9, 9, 9, 0, 0, 10, 10, 0], [9, 9, 9, 0, 0, 10, 10, 0]])
    assert G.select(rec, [0.9, 0.9], 500, 500)[0] == [0]


def test_thresholds_and_defaults():
    rec = np.array([[95, 100, 100, 0, 0, 9, 9, 0], [94, 100, 100, 20, 20, 29, 29, 0], [100, 100, 100, 40, 40, 49, 49, 0]])
    # defaults: 0.88 and 0.95 -- candidate 1 misses the stability (940 < 950), candidate 2 the IoU (fp32 0.88 is the bound)
    below = np.nextafter(f32(880) / f32(1000), f32(0))
    assert G.select(rec, [f32(880) / f32(1000), 0.99, below])[0] == [0]
    assert G.select(rec, [0.5, 0.5, 0.5], 500, 940)[0] == [0, 1, 2]
    assert G.select(rec, [0.5, 0.5, 0.5], 501, 1)[0] == []
    assert G.select(rec, [0.5, 0.5, 0.5], -1, -1)[0] == [0, 1, 2]


def test_the_cap_of_255():
    n = 300
    rec = np.array([[1, 1 + c, 2, 3 * c, 0, 3 * c + 1, 1, 0] for c in range(n)])        # disjoint boxes
    iou = np.linspace(0.99, 0.6, n).astype(f32)
    nms, kept = G.select(rec, iou, 500, 500)
    assert nms == list(range(255))
    assert kept == list(range(254, -1, -1))


def test_the_smallest_segment_lies_on_top():
    big, small = _plane(), _plane()
    big[40:200, 40:200] = 4.0
    small[100:120, 100:120] = 4.0
    planes4 = np.stack([np.stack([_plane(), big, small, _plane()])])
    out, rec, nms, kept = G.label_map(planes4, [[0.0, 0.9, 0.95, 0.1]], 1024, 1024, 500, 500)
    assert nms == [1, 0] and kept == [0, 1]
    assert out[440, 440] == 2 and out[300, 300] == 1 and out[10, 10] == 0
    assert set(np.unique(out)) == {0, 1, 2}
    assert np.array_equal(out == 2, G.mask_of(small, 1024, 1024) == 255)


# ---- csrc/grid_plan.hpp against the reference

def _random_set(rng):
    n = int(rng.integers(1, 60))
    rec = np.zeros((n, 8), np.int64)
    for c in range(n):
        x0, y0 = rng.integers(0, 40, 2)
        w, h = rng.integers(0, 24, 2)
        # mostly stable candidates (n_hi close to n_lo), some empty ones, some far from stable
        n_lo = int(rng.integers(0, 600))
        n_mid = int(rng.integers(0, n_lo + 1)) if rng.random() < 0.2 else n_lo - int(rng.integers(0, n_lo // 20 + 1))
        n_hi = int(rng.integers(0, n_mid + 1)) if rng.random() < 0.2 else n_mid - int(rng.integers(0, n_mid // 20 + 1))
        rec[c] = [n_hi, n_mid, n_lo, x0, y0, x0 + w, y0 + h, 0]
        if n_mid == 0:
            rec[c, 3:7] = [0, 0, -1, -1]
        if rng.random() < 0.15 and c:
            rec[c] = rec[int(rng.integers(0, c))]            # twins: IoU ties, equal sizes, full overlap
    iou = rng.choice(np.array([0.5, 0.7, 0.88, 0.9, 0.95], f32), n) if rng.random() < 0.3 else rng.uniform(0.4, 1.0, n).astype(f32)
    ip, sp = [(0, 0), (700, 800), (500, 500), (880, 0), (-5, 1), (950, 990)][int(rng.integers(0, 6))]
    return rec, iou, ip, sp


def test_compiled_selection_matches_the_reference(cases):
    rng = np.random.default_rng(20261019)
    sets = [_random_set(rng) for _ in range(300)]
    n = 300
    sets.append((np.array([[1, 1 + c, 2, 3 * c, 0, 3 * c + 1, 1, 0] for c in range(n)]), np.linspace(0.99, 0.6, n).astype(f32), 500, 500))
    sets.append((np.array([[1, 1, 1, 7, 7, 7, 7, 0]] * 3), np.array([0.9, 0.8, 0.7], f32), 500, 500))
    got = _select_compiled(cases, sets)
    kept_any = suppressed_any = 0
    for (rec, iou, ip, sp), (nms, kept) in zip(sets, got):
        want_nms, want_kept = G.select(rec, iou, ip, sp)
        assert nms == want_nms and kept == want_kept
        ok_iou, ok_stab, alive = G.passes(rec, iou, ip, sp)
        kept_any += len(nms) > 1
        suppressed_any += len(nms) < int((ok_iou & ok_stab & alive).sum())
    assert kept_any > 100 and suppressed_any > 100          # the sets exercise the ordering and the suppression


@pytest.mark.parametrize("w,h,side", [(1, 1, 1), (1, 1, 32), (1024, 1024, 1), (33, 17, 32), (600, 400, 5), (1024, 1024, 32), (4000, 3000, 7)])
def test_grid_pixels(cases, w, h, side):
    got = [tuple(int(v) for v in line.split(",")) for line in cases("pixels", w, h, side)]
    want = G.grid_pixels(w, h, side)
    assert got == want and len(got) == side * side
    assert all(0 <= x < w and 0 <= y < h for x, y in got)
    if side > 1:
        assert got[1][1] == got[0][1] and got[side][0] == got[0][0]          # row-major, rows outer


def test_grid_pixels_by_hand():
    assert G.grid_pixels(1024, 1024, 1) == [(512, 512)]
    assert G.grid_pixels(33, 17, 32)[:3] == [(0, 0), (1, 0), (2, 0)] and G.grid_pixels(33, 17, 32)[-1] == (32, 16)
    assert G.grid_pixels(600, 400, 4)[:5] == [(75, 50), (225, 50), (375, 50), (525, 50), (75, 150)]


# ---- the planner

EMPTY, BOX = "0,0,-1,-1", "10,20,300,200"


def _plan(cases, entries, points=True, regions=True, branch=True):
    return cases("plan", int(points), int(regions), int(branch), *entries)


def test_a_grid_prompt_is_planned_between_the_others(cases):
    lines = _plan(cases, [f"h:{EMPTY}", "c:1,0,0,0", "c:0,0,0,0", f"h:{EMPTY}", "c:7,5,700,-3", f"h:{BOX}", "c:6,8,16,0"])
    assert lines == ["prompt 0 clicks 3 box 0 points 4 entries 0,1,2 stages 3 clean 0,0 grid 0,0,0",
                     "prompt 3 clicks 1 box 0 points 2 entries 3 stages 1 clean 0,0 grid 5,700,-3",
                     "prompt 5 clicks 1 box 1 points 3 entries 5 stages 1 clean 8,16 grid 0,0,0",
                     "any_clean 1", "any_grid 1"]
    # grid prompts alone need no `points`; the other prompts of such a call are boxes
    lines = _plan(cases, [f"h:{EMPTY}", "c:7,32,0,0", f"h:{BOX}", f"h:{EMPTY}", "c:7,1,0,0"], points=False)
    assert lines == ["prompt 0 clicks 1 box 0 points 2 entries 0 stages 1 clean 0,0 grid 32,0,0",
                     "prompt 2 clicks 0 box 1 points 2 entries stages 0 clean 0,0 grid 0,0,0",
                     "prompt 3 clicks 1 box 0 points 2 entries 3 stages 1 clean 0,0 grid 1,0,0",
                     "any_clean 0", "any_grid 1"]
    # a refinement mark of another prompt keeps its stages, in the caller's numbering
    lines = _plan(cases, [f"h:{EMPTY}", "c:7,4,0,0", f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0"])
    assert lines[1] == "prompt 2 clicks 2 box 0 points 3 entries 2,4 stages 1,2 clean 0,0 grid 0,0,0"


REFUSALS = [
    ([f"h:{EMPTY}", "c:7,0,0,0"], "entry 1", "side is 1..32"),
    ([f"h:{EMPTY}", "c:7,33,0,0"], "entry 1", "side is 1..32"),
    ([f"h:{BOX}", f"h:{EMPTY}", "c:7,-1,0,0"], "entry 2", "side is 1..32"),
    ([f"h:{BOX}", "c:7,4,0,0"], "entry 1", "needs a head with an empty region"),
    ([f"h:{EMPTY}", "c:1,0,0,0", "c:7,4,0,0"], "entry 2", "does not directly follow its head"),
    ([f"h:{EMPTY}", "c:6,8,8,0", "c:7,4,0,0"], "entry 2", "does not directly follow its head"),
    ([f"h:{EMPTY}", "c:7,4,0,0", "c:7,4,0,0"], "entry 2", "does not directly follow its head"),
    ([f"h:{EMPTY}", "c:7,4,0,0", "c:1,0,0,0"], "entry 2", "follows a grid mark"),
    ([f"h:{EMPTY}", "c:7,4,0,0", "c:4,0,0,0", "c:1,0,0,0"], "entry 2", "follows a grid mark"),
    ([f"h:{BOX}", f"h:{EMPTY}", "c:7,4,0,0", "c:6,8,8,0"], "entry 3", "follows a grid mark"),
    (["c:7,4,0,0", f"h:{EMPTY}"], "entry 0", "needs a prompt in front of it"),
]


@pytest.mark.parametrize("entries,who,why", REFUSALS)
def test_refusals_say_mark_and_name_the_entry(cases, entries, who, why):
    for points in (True, False):
        lines = _plan(cases, entries, points=points)
        assert len(lines) == 1 and lines[0].startswith("error mask batch: "), lines
        assert who + ":" in lines[0] and "mark" in lines[0] and why in lines[0], lines


def test_refusals_of_the_rest_are_renumbered(cases):
    # the bad label of entry 4 is entry 2 of the call without the grid prompt
    lines = _plan(cases, [f"h:{EMPTY}", "c:7,4,0,0", f"h:{EMPTY}", "c:1,0,0,0", "c:5,0,0,0"])
    assert lines[0].startswith("error mask batch: entry 4: the label of a click")
    lines = _plan(cases, [f"h:{EMPTY}", "c:7,4,0,0", f"h:{EMPTY}", "c:6,0,0,0"])
    assert lines[0].startswith("error mask batch: entry 3: a clean-up mark")


CALLS_WITHOUT_GRID_MARKS = [
    ([f"h:{EMPTY}"], True, False), ([f"h:{BOX}"], False, True), ([f"h:{BOX}", f"h:{BOX}"], True, True),
    ([f"h:{EMPTY}", "c:1,0,0,0", "c:0,0,0,0", f"h:{BOX}"], True, True),
    ([f"h:{EMPTY}", "c:4,0,0,0", "c:1,0,0,0", "c:6,4,4,0"], True, True),
    ([f"h:{BOX}", "c:6,4,0,0"], False, True),
    ([f"h:{EMPTY}", "c:2,0,0,0"], True, True), ([f"h:{EMPTY}", "c:5,0,0,0"], True, True), ([f"h:{EMPTY}", "c:-1,0,0,0"], True, True),
    ([f"h:{EMPTY}", "c:1,0,0,5"], True, True), (["c:1,0,0,0", f"h:{EMPTY}"], True, True), ([f"h:{EMPTY}", "c:1,0,0,0"], False, True),
    ([f"h:{EMPTY}"] + ["c:1,0,0,0"] * 8, True, True), ([f"h:{EMPTY}", "c:6,0,0,0"], True, True), ([f"h:{EMPTY}"], False, False),
    ([f"h:{EMPTY}", "c:8,1,0,0"], True, True),
]


@pytest.mark.parametrize("entries,points,regions", CALLS_WITHOUT_GRID_MARKS)
def test_a_call_without_grid_marks_is_planned_as_before(cases, clean_plan, entries, points, regions):
    mine = _plan(cases, entries, points=points, regions=regions)
    before = clean_plan(entries, points=points, regions=regions)
    if before[0].startswith("error"):
        assert mine == before
        return
    prompts = [l for l in before if l.startswith("prompt")]
    assert [l for l in mine if l.startswith("prompt")] == [re_labels(l) + " grid 0,0,0" for l in prompts]
    assert mine[-2:] == [next(l for l in before if l.startswith("any_clean")), "any_grid 0"]


def re_labels(line):
    """clean_plan_cases prints the clicks' labels, grid_plan_cases does not"""
    head, _, rest = line.partition(" labels")
    return head + " stages" + rest.partition(" stages")[2]


# ---- the wrapper

def test_click_entries_with_grid():
    P = api.Point
    e = api.click_entries([[P(1, 2), P(3, 4)], None, [P(5, 6)]], labels=[[1, 0], None, None], grid=[None, (5, 700, 0), None])
    assert e.heads == [0, None, 1, None, 2]
    assert e.regions == [api.EMPTY_REGION, (0, 0, 0, 0), api.EMPTY_REGION, (api.GRID_MARK, 5, 700, 0), api.EMPTY_REGION]
    assert e.prompt_heads == [0, 2, 4] and e.grid_sides == [0, 5, 0]
    assert e.token_rows == [8, 7, 7]
    assert e.launches == [(8, [0]), (7, [2])]            # the grid prompt's launches are its own
    for bad in ([None, (0, 0, 0), None], [None, (33, 0, 0), None], [None, (4, 0), None], [(4, 0, 0), None, None]):
        with pytest.raises(api.Error, match="grid"):
            api.click_entries([[P(1, 2), P(3, 4)], None, [P(5, 6)]], labels=[[1, 0], None, None], grid=bad)
    with pytest.raises(api.Error, match="grid"):
        api.click_entries([None], grid=[(4, 0, 0)], clean=(3, 3))
    heads, pts, regs = api._marked_entries(2, None, None, [None, None], [(4, 0, 0), (2, 900, 900)])
    assert heads == [0, None, 1, None] and pts is None
    assert regs == [api.EMPTY_REGION, (7, 4, 0, 0), api.EMPTY_REGION, (7, 2, 900, 900)]


def test_constants_and_the_cpp_wrapper(tmp_path):
    assert api.GRID_MARK == 7
    src = tmp_path / "wrapper.cpp"
    src.write_text('''#include <dlimgedit/dlimgedit.hpp>
dlimg::Image everything(dlimg::Segmentation const& s) { return s.segment_everything(dlimg::GridOptions{16, 900, 0}); }
dlimg::Image defaults(dlimg::Segmentation const& s) { return s.segment_everything(); }
void into(dlimg::Segmentation const& s, uint8_t* out) { s.segment_everything(dlimg::GridOptions{}, out); }
int main() { return 0; }
''')
    r = subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", "-DDLIMGEDIT_LOAD_DYNAMIC", f"-I{ROOT / 'include'}", "-fsyntax-only",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    src = tmp_path / "planner.cpp"
    src.write_text('''#include <dlimgedit/dlimgedit.h>
#include "grid_plan.hpp"
static_assert(dlimg::kGridMark == DLIMG_GRID_MARK, "one value on both sides");
int main() { return 0; }
''')
    r = subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{CSRC}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
