"""Lasso marks without a GPU: the numpy restatement of the derivation (tests/lasso_ref.py), the planner (csrc/lasso_plan.hpp,
printed by tests/lasso_plan_cases.cpp, built with the host compiler) and the wrappers.

* the reference's separable distance transform equals a brute-force all-pairs minimum on a few thousand random planes up to
  24 x 24, the background around the plane included;
* inside == (prior_ref.prior_plane > 0) on every kernel case, and every derived click lies inside the image, inside the box and
  in an inside cell;
* the fold of the row records (fold_lasso_rows, the host's half of the derivation) gives the reference's record;
* the planner: every refusal with its entry number, token counts per `what` (+1 on a SAM-HQ file), the packed order, a call
  without lasso marks planned exactly as plan_prior_prompts plans it, 5 and 9 still refused labels;
* dlimgedit_amd.api.click_entries with lasso marks, and the C++ wrapper's Lasso / snap compile against DLIMG_LASSO_MARK == 10;
* the planner on random entry lists under ASan + UBSan (tests/sanitize/lasso_plan_fuzz.cpp, a stand-alone program).
"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lasso_cases as LC
import lasso_ref
import prior_ref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dlimgedit_amd" / "csrc"


def test_separable_transform_is_the_brute_force_minimum():
    rng = np.random.default_rng(20)
    planes = [np.ones((1, 1), bool), np.ones((24, 24), bool), np.ones((1, 24), bool), np.ones((24, 1), bool), np.zeros((5, 7), bool),
              np.ones((23, 24), bool), np.ones((24, 23), bool)]
    for _ in range(3000):
        sh, sw = rng.integers(1, 25, 2)
        kind = rng.integers(0, 3)
        if kind == 0:
            plane = rng.random((sh, sw)) < rng.random()
        elif kind == 1:                                   # mostly inside with a few holes: long distances, many ties
            plane = rng.random((sh, sw)) < 0.97
        else:                                             # blobs
            yy, xx = np.mgrid[0:sh, 0:sw]
            plane = np.zeros((sh, sw), bool)
            for _ in range(rng.integers(1, 4)):
                cx, cy, r = rng.integers(0, sw), rng.integers(0, sh), rng.integers(1, 9)
                plane |= (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
        planes.append(plane)
    for plane in planes:
        got, want = lasso_ref.squared_distance(plane), lasso_ref.brute_force_squared_distance(plane)
        assert np.array_equal(got, want), (plane.astype(int), got, want)
        assert ((got > 0) == plane).all()
    # a full plane: the distance is to the region's edge only, and the tie goes to the first of the middle cells
    for n in (23, 24):
        rec = lasso_ref.derive_from_inside(np.ones((n, n), bool), 4 * n, 4 * n, 4 * n, 4 * n)
        mid = (n - 1) // 2
        assert rec[7] == (mid + 1) ** 2 and (rec[5], rec[6]) == (4 * mid + 1, 4 * mid + 1)


@pytest.mark.parametrize("extent", LC.EXTENTS, ids=LC.EXTENT_IDS)
def test_inside_is_where_the_prior_plane_is_positive_and_the_click_lies_inside(extent):
    w, h = extent
    pre_w, pre_h = prior_ref.pre_extent(w, h)
    sw, sh = (pre_w + 3) // 4, (pre_h + 3) // 4
    c0, c1 = prior_ref.footprints(w, pre_w)
    r0, r1 = prior_ref.footprints(h, pre_h)
    names = set()
    for name, mask in LC.kernel_masks(w, h).items():
        names.add(name)
        inside = lasso_ref.inside_cells(mask, pre_w, pre_h)
        assert inside.shape == (sh, sw)
        for strength in (1, 8000):
            plane = prior_ref.prior_plane(mask, pre_w, pre_h, strength)
            assert np.array_equal(plane[:sh, :sw] > 0, inside), name
            assert not (plane[sh:] > 0).any() and not (plane[:, sw:] > 0).any()
        rec = lasso_ref.derive(mask, pre_w, pre_h)
        if name in ("zeros", "uniform_127"):
            assert not rec.any(), name
            continue
        assert rec[0] == inside.sum() > 0, name
        x0, y0, x1, y1, cx, cy = (int(v) for v in rec[1:7])
        assert 0 <= x0 <= cx < x1 <= w and 0 <= y0 <= cy < y1 <= h, (name, rec)
        # the click's pixel belongs to an inside cell with the record's distance
        cells = [(y, x) for y in range(sh) if r0[y] <= cy < r1[y] for x in range(sw) if c0[x] <= cx < c1[x]]
        d2 = lasso_ref.squared_distance(inside)
        assert any(inside[c] and d2[c] == rec[7] for c in cells), (name, rec)
        if name in ("full", "uniform_128"):
            assert inside.all() and (x0, y0, x1, y1) == (0, 0, w, h), name
        if name == "one_cell" and pre_w <= w and pre_h <= h:        # (scaled up, one source pixel is many cells)
            assert rec[0] == 1 and rec[7] == 1, rec
        if name == "two_discs" and min(w, h) >= 32:
            assert cx > w // 2 and cy < h // 2, rec             # the upper disc is the right one: the smallest y decides
    assert names >= {"full", "one_cell", "last_row_and_column", "ring", "two_discs", "l_shape", "checkerboard", "uniform_127",
                     "uniform_128", "soft_ellipse", "zeros", "random_blobs"}


def _cxx():
    rocm_clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    cxx = str(rocm_clang) if rocm_clang.exists() else (shutil.which("c++") or shutil.which("g++") or shutil.which("clang++"))
    assert cxx, "no host C++ compiler found"
    return cxx


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lasso_plan") / "lasso_plan_cases"
    r = subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(ROOT / "tests" / "lasso_plan_cases.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(entries, points=1, regions=1, branch=1, device=0, which="lasso", stdin=None):
        head = [str(exe), which, points, regions, branch, device] if which != "fold" else [str(exe), "fold"]
        r = subprocess.run([str(a) for a in head] + [str(e) for e in entries], capture_output=True, text=True, timeout=60, input=stdin)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def _rows_of(inside: np.ndarray) -> np.ndarray:
    """The row records k::lasso_derive writes for a plane (kernels.hpp), from the reference's distances."""
    d2 = lasso_ref.squared_distance(inside)
    rows = np.zeros((256, 8), np.int64)
    for y in range(inside.shape[0]):
        xs = np.nonzero(inside[y])[0]
        if len(xs):
            rows[y, :5] = [len(xs), xs.min(), xs.max(), int(np.argmax(d2[y])), d2[y].max()]
    return rows


@pytest.mark.parametrize("extent", [(1024, 1024), (600, 400), (37, 1024)], ids=["1024x1024", "600x400", "37x1024"])
def test_fold_of_the_row_records(planner, extent):
    w, h = extent
    pre_w, pre_h = prior_ref.pre_extent(w, h)
    for name, mask in LC.kernel_masks(w, h).items():
        inside = lasso_ref.inside_cells(mask, pre_w, pre_h)
        text = " ".join(str(v) for v in _rows_of(inside).ravel())
        out = planner([w, h, pre_w, pre_h], which="fold", stdin=text)
        assert out == ["record " + " ".join(str(int(v)) for v in lasso_ref.derive(mask, pre_w, pre_h))], name


H, L = "h:0,0,-1,-1", "c:10,0,0,0"


def test_planner_reads_lasso_marks(planner):
    # a lasso alone, in a call without `points`: the derived click, then the box
    assert planner([H, L], points=0) == ["prompt 0 clicks 1 box 1 points 3 entries 1 stages 1 clean 0,0 grid 0,0,0 lasso 1,7,8000",
                                         "  packed 15,25,1 10,20,2 30,40,3", "any_clean 0", "any_grid 0", "any_lasso 1"]
    # token rows per `what`: 5 + points -- 7, 7, 8, and the same with the mask bit
    for what, points, packed in ((1, 2, "10,20,2 30,40,3"), (2, 2, "15,25,1 0,0,-1"), (3, 3, "15,25,1 10,20,2 30,40,3")):
        for bits, strength, planned in ((what, 0, 0), (what | 4, 0, 8000), (what | 4, 2500, 2500)):
            out = planner([H, f"c:10,{strength},{bits},0"], points=0)
            assert out[0].startswith(f"prompt 0 clicks {1 if what & 2 else 0} box {what & 1} points {points} entries") and \
                out[0].endswith(f"lasso 1,{bits},{planned}"), out
            assert out[1] == "  packed " + packed and 5 + points == LC.token_rows(bits)
    # with `points` the head's click follows the derived one, then the further clicks; a refinement mark keeps the derived click
    # in the first stage, the box in both; a clean-up mark stays
    out = planner([H, "c:10,0,3,0", "c:0,0,0,0", "c:4,0,0,0", "c:1,0,0,0", "c:6,5,5,0"])
    assert out[:3] == ["prompt 0 clicks 4 box 1 points 6 entries 1,0,2,4 stages 3,4 clean 5,5 grid 0,0,0 lasso 1,3,0",
                       "  packed 15,25,1 0,1,1 200,201,0 10,20,2 30,40,3", "  packed 15,25,1 0,1,1 200,201,0 400,401,1 10,20,2 30,40,3"]
    # the click alone keeps the caller's box; a box-only prompt and a lasso prompt share a call without `points`
    out = planner(["h:5,5,50,50", "c:10,0,2,0", H, "c:1,0,0,0"])
    assert out[:3] == ["prompt 0 clicks 2 box 1 points 4 entries 1,0 stages 2 clean 0,0 grid 0,0,0 lasso 1,2,0",
                       "  packed 15,25,1 0,1,1 5,5,2 50,50,3", "prompt 2 clicks 2 box 0 points 3 entries 2,3 stages 2 clean 0,0 grid 0,0,0"]
    out = planner(["h:1,1,9,9", H, "c:10,0,2,0", "c:6,3,3,0"], points=0)
    assert out[:3] == ["prompt 0 clicks 0 box 1 points 2 entries stages 0 clean 0,0 grid 0,0,0",
                       "prompt 1 clicks 1 box 0 points 2 entries 2 stages 1 clean 3,3 grid 0,0,0 lasso 2,2,0", "  packed 15,25,1 0,0,-1"]
    # the box alone without the branch; eight clicks counting the derived one
    assert planner([H, "c:10,0,3,0"], branch=0)[0].endswith("lasso 1,3,0")
    assert planner([H, L] + ["c:1,0,0,0"] * 6)[0].startswith("prompt 0 clicks 8 box 1 points 10 entries 1,0,2,3,4,5,6,7 stages 8")


REFUSALS = [
    # (entries, how the call is made, the entry the message names, words of the message)
    ([L, H], {}, 0, "needs a prompt in front"),
    ([H, "c:1,0,0,0", L], {}, 2, "does not directly follow its head"),
    ([H, "c:4,0,0,0", L, "c:1,0,0,0"], {}, 2, "does not directly follow its head"),
    ([H, L, L], {}, 2, "second one"),
    ([H, "c:8,0,0,0", L], {}, 2, "prior"),
    ([H, L, "c:8,0,0,0"], {}, 1, "prior"),
    ([H, L + "!"], {}, 1, "NULL"),
    ([H, "c:10,0,8,0"], {}, 1, "what is 0"),
    ([H, "c:10,0,-1,0"], {}, 1, "what is 0"),
    ([H, "c:10,0,4,0"], {}, 1, "derives nothing"),
    ([H, "c:10,8000,4,0"], {}, 1, "derives nothing"),
    ([H, "c:10,0,0,1"], {}, 1, "fourth int"),
    ([H, "c:10,-1,0,0"], {}, 1, "strength_milli"),
    ([H, "c:10,100001,0,0"], {}, 1, "strength_milli"),
    ([H, "c:10,8000,3,0"], {}, 1, "without the mask bit"),
    (["h:5,5,50,50", "c:10,0,1,0"], {}, 1, "empty region"),
    (["h:5,5,50,50", L], {}, 1, "empty region"),
    ([H, L], {"branch": 0}, 1, "pe.mask"),
    ([H, "c:10,0,6,0"], {"branch": 0}, 1, "pe.mask"),
    ([H, L, "c:7,4,0,0"], {}, 1, "grid"),
    ([H, L], {"device": 1}, 1, "dlimg_amd_get_segmentation_masks_device"),
    ([H, L] + ["c:1,0,0,0"] * 7, {}, 1, "more than 8 clicks"),
    (["h:1,1,9,9", H, L, H, "c:10,0,9,0"], {"points": 0}, 4, "what is 0"),
]


@pytest.mark.parametrize("entries,how,entry,why", REFUSALS, ids=[f"{i}-{r[3][:24].replace(' ', '_')}" for i, r in enumerate(REFUSALS)])
def test_planner_refusals_name_the_mark_and_the_callers_entry(planner, entries, how, entry, why):
    out = planner(entries, **how)
    assert len(out) == 1 and out[0].startswith(f"error mask batch: entry {entry}: a lasso mark "), out
    assert "mark" in out[0] and why in out[0], out


def test_refusals_of_the_inner_planners_keep_the_callers_numbering(planner):
    # 5 and 9 stay refused labels, behind a lasso mark too; a caller's ninth click keeps the words of the click limit
    for label in (5, 9):
        assert planner([H, f"c:{label},0,0,0"]) == [f"error mask batch: entry 1: the label of a click is 1 (foreground) or 0 (background), "
                                                    "in regions[4 i] with the other three ints 0"]
        out = planner([H, "c:1,0,0,0", H, L, f"c:{label},0,0,0"])
        assert len(out) == 1 and out[0].startswith("error mask batch: entry 4: the label of a click"), out
    out = planner([H, "c:1,0,0,0", H, L] + ["c:1,0,0,0"] * 8)
    assert out == ["error mask batch: the prompt of entry 2 has more than 8 clicks"]
    out = planner([H, L, "c:1,0,0,0", "c:6,1,1,0", "c:1,0,0,0"])
    assert len(out) == 1 and out[0].startswith("error mask batch: entry 3: a clean-up mark"), out
    # a click without `points`
    assert "needs `points`" in planner([H, L, "c:1,0,0,0"], points=0)[0]


def test_a_call_without_lasso_marks_is_planned_as_before(planner):
    calls = [([H], {}), ([H, "c:1,0,0,0", "c:4,0,0,0", "c:0,0,0,0", "c:6,9,9,0"], {}), (["h:1,2,30,40", "c:8,0,0,0", H, "c:7,4,0,0"], {}),
             (["h:1,2,30,40", "h:3,4,50,60"], {"points": 0}), ([H, "c:8,0,0,0"], {"branch": 0}), (["h:1,2,3,4"], {"regions": 0}),
             ([H, "c:9,0,0,0"], {}), (["c:1,0,0,0"], {}), ([H, "c:8,5,0,0"], {"device": 1})]
    for entries, how in calls:
        assert planner(entries, **how) == planner(entries, which="prior", **how), entries


def test_click_entries_with_lasso_marks():
    from dlimgedit_amd import api
    P = api.Point
    m = np.zeros((6, 8), np.uint8)
    plain = api.click_entries([[P(1, 2), P(3, 4)]], labels=[[1, 0]])
    assert plain == api.click_entries([[P(1, 2), P(3, 4)]], labels=[[1, 0]], lasso=None) and plain.lassos == []
    assert (api.LASSO_MARK, api.LASSO_BOX, api.LASSO_CLICK, api.LASSO_MASK) == (10, 1, 2, 4)
    e = api.click_entries([[P(1, 2), P(3, 4)], [P(5, 6)]], labels=[[1, 0], None], refine_after=[[1], None], clean=[None, (3, 3)],
                          lasso=[m, None])
    assert e.heads == [0, None, None, None, 1, None]
    assert e.regions == [api.EMPTY_REGION, (10, 0, 0, 0), (4, 0, 0, 0), (0, 0, 0, 0), api.EMPTY_REGION, (6, 3, 3, 0)]
    assert e.token_rows == [10, 7] and e.stage_clicks == [[2, 3], [1]] and e.lassos[0] is m and e.lassos[1] is None
    assert e.launches == [(7, [1]), (9, [0]), (10, [0])]
    for what, rows in ((1, 8), (2, 8), (3, 9), (5, 8), (6, 8), (7, 9)):
        e = api.click_entries([[P(1, 2)]], lasso=[m], lasso_what=what, lasso_strength=2500 if what & 4 else 0)
        assert e.regions[1] == (10, 2500 if what & 4 else 0, what, 0) and e.token_rows == [rows] == [LC.token_rows(what, 1)]
    box = api.Region(P(0, 0), P(5, 5))
    assert api.click_entries([[P(1, 2)]], regions=[box], lasso=[m], lasso_what=2).token_rows == [9]
    for bad in (dict(lasso_what=4), dict(lasso_what=8), dict(lasso_what=3, lasso_strength=5), dict(lasso_strength=100001),
                dict(regions=[box]), dict(regions=[box], lasso_what=1), dict(prior=[m]), dict(lasso_what=[1, 2])):
        with pytest.raises(api.Error):
            api.click_entries([[P(1, 2)]], lasso=[m], **bad)
    with pytest.raises(api.Error):
        api.click_entries([[P(1, 2)]], lasso=[np.zeros((6, 8), np.float32)])
    with pytest.raises(api.Error):
        api.click_entries([None], grid=[(4, 0, 0)], lasso=[m])


def test_cpp_wrapper_compiles_with_a_lasso(tmp_path):
    src = tmp_path / "consumer.cpp"
    src.write_text("""
#include <dlimgedit/dlimgedit.hpp>
static_assert(DLIMG_LASSO_MARK == 10, "the lasso mark of table slot 14");
static_assert(DLIMG_LASSO_BOX == 1 && DLIMG_LASSO_CLICK == 2 && DLIMG_LASSO_MASK == 4, "the bits of its `what`");
static_assert(DLIMG_PRIOR_MARK == 8 && DLIMG_GRID_MARK == 7, "the other marks stay");
dlimg::Image snap(dlimg::Segmentation const& seg, dlimg::Image& selection) {
    dlimg::Lasso lasso{selection.pixels()};
    dlimg::Image a = seg.snap(lasso);
    dlimg::Image b = seg.snap(dlimg::Lasso{selection.pixels(), DLIMG_LASSO_BOX | DLIMG_LASSO_CLICK, 0},
                              {dlimg::Click{dlimg::Point{10, 20}, true}, dlimg::Click{dlimg::Point{30, 40}, false}}, {1},
                              dlimg::MaskCleanup{16, 16});
    seg.snap(lasso, selection.pixels());                                       // snapped in place
    seg.snap(lasso, selection.pixels(), {dlimg::Click{dlimg::Point{1, 2}}}, {}, std::nullopt);
    dlimg::Image c = seg.compute_mask({dlimg::Click{dlimg::Point{10, 20}, true}}, std::nullopt, {}, std::nullopt, std::nullopt, lasso);
    std::vector<std::optional<dlimg::Lasso>> lassos{dlimg::Lasso{a.pixels(), 7, 2500}, std::nullopt};
    auto both = dlimg::Segmentation::compute_mask_batch({&seg, &seg}, std::vector<std::vector<dlimg::Click>>{{{dlimg::Point{1, 2}}}, {{dlimg::Point{3, 4}}}},
                                                        {}, {}, {}, {}, lassos);
    return std::move(both[0]);
}
int main() { return 0; }
""")
    r = subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Werror", "-DDLIMGEDIT_LOAD_DYNAMIC", f"-I{ROOT / 'include'}", "-fsyntax-only",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_planner_on_random_entry_lists_under_address_sanitizer(tmp_path):
    """csrc/lasso_plan.hpp on random batch mask calls with ASan + UBSan, every served call checked against what the batch calls
    rely on (tests/sanitize/lasso_plan_fuzz.cpp): a stand-alone program on the CPU."""
    clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    if not clang.exists():
        pytest.skip("ROCm clang not found")
    exe = tmp_path / "lasso_plan_fuzz"
    r = subprocess.run([str(clang), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", f"-I{CSRC}", str(ROOT / "tests" / "sanitize" / "lasso_plan_fuzz.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and "sanitizer" in (r.stderr + r.stdout).lower() and "cannot find" in (r.stderr + r.stdout).lower():
        pytest.skip("this clang has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, errors="replace", timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
