"""Mask input for click-to-refine on the CPU.

* the staged float64 reference (mask_input_cases.staged_reference: oracle/decoder_ref.decode_fp64 per stage, the dense
  embedding of the previous stage's plane in pe.no_mask's place) against tests/golden/sam_vit_test_mask_input.npz --
  Hugging Face SamModel given input_masks stage by stage (tests/golden/make_mask_input_golden.py) -- within the logit and
  IoU tolerances test_oracle_golden.py holds this model to;
* the mask branch's reference is local: one 4 x 4 block of logits moves exactly one token's row;
* the weights: the branch round-trips through Hugging Face and Meta names, a model without it stays as it was, a partial
  set is refused, and no other tensor changes;
* the wrapper's builder (dlimgedit_amd.api.click_entries with refine_after) and the library's planner
  (csrc/prompt_plan.hpp: plan_staged_prompts, printed by tests/mask_input_plan_cases.cpp, built with the host compiler):
  entry lists and stage lists worked out by hand, and every refusal; the points it packs for every stage (pack_points) equal
  the Python side's stage prefixes exactly;
* the inputs of the GPU tests: for every case the reference mask with mask input differs from the reference of the same
  clicks without it in at least ten times what the GPU tests let a mask disagree in.
"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mask_input_cases as C
import multi_click_cases as M
from dlimgedit_amd import api
from dlimgedit_amd import weights as W
from dlimgedit_amd.sam_config import CONFIGS, get_config
from oracle import sam_oracle as O

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dlimgedit_amd" / "csrc"
GOLD = Path(__file__).resolve().parent / "golden" / "sam_vit_test_mask_input.npz"
EMB_STRIDE, LOW_STRIDE, MASK_ROW_STRIDE = 257, 61, 2
HF_LOGIT_TOL, HF_IOU_TOL = 5e-4, 1e-4          # test_oracle_golden.py, reduced model
P = api.Point


@pytest.fixture(scope="module")
def oracle_segs():
    cfg = get_config("vit_test")
    params = W.synthetic_weights(cfg, 7, mask_branch=True)
    return {name: O.OracleSegmentation(params, cfg).process(C.image(name), O.CH_RGBA) for name in C.IMAGES}, params


@pytest.fixture(scope="module")
def references(oracle_segs):
    """case index -> (staged mask, plane, unstaged mask), computed once"""
    segs, params = oracle_segs
    out = {}
    for i, case in enumerate(C.CASES):
        seg = segs[case[0]]
        w, h = seg.rs.original
        mask, plane, _ = C.staged_reference(seg.embedding, seg.rs, case, params, (h, w))
        out[i] = (mask, plane, C.unstaged_reference(seg.embedding, seg.rs, case, params, (h, w)))
    return out


def test_cases_cover_what_the_issue_names():
    rows = [C.token_rows(c) for c in C.CASES]
    assert [7, 8] in rows                                            # two stages, 7 -> 8
    assert any(len(r) == 2 and r[-1] == 9 for r in rows)             # two stages ending at the first count above 8
    assert any(len(r) == 3 for r in rows)                            # three stages
    assert any(c[3] is not None for c in C.CASES) and any(c[0] == "wide" for c in C.CASES)
    assert [7, 8, 9, 10, 11, 12, 13, 14] in rows                     # 8 clicks, "each", no box
    assert any(r[-1] == 15 and len(r) == 2 and len(c[1]) == 8 for r, c in zip(rows, C.CASES))      # 8 clicks, one mark, a box
    for case in C.CASES:
        ks = C.stage_clicks(case)
        assert ks == sorted(set(ks)) and ks[0] >= 1 and ks[-1] == len(case[1]) <= 8 and case[2][0] == 1


def test_staged_reference_matches_hugging_face(oracle_segs):
    segs, params = oracle_segs
    g = np.load(GOLD)
    assert int(g["seed"]) == 7
    seg = segs["square"]
    assert np.abs(seg.embedding.reshape(-1)[::EMB_STRIDE] - g["emb_samples"]).max() < 2e-4
    assert list(g["cases"]) == [i for i, c in enumerate(C.CASES) if c[0] == "square"] and len(g["cases"]) >= 3
    for n, i in enumerate(g["cases"]):
        case = C.CASES[i]
        _, clicks, labels, box, _ = case
        ks = C.stage_clicks(case)
        # the chain up to the last stage, then the last stage itself for all four planes
        prev = None
        if len(ks) > 1:
            head = (case[0], clicks[:ks[-2]], labels[:ks[-2]], box, tuple(ks[:-2]))
            _, _, planes = C.staged_reference(seg.embedding, seg.rs, head, params, (1024, 1024))
            prev = planes[-1]
        low, iou, plane = C.decode_stage(seg.embedding, seg.rs, clicks, labels, box, params, prev)
        d_low = np.abs(np.asarray(low, np.float64).reshape(4, -1)[:, ::LOW_STRIDE] - g["low_samples"][n]).max()
        d_iou = np.abs(np.asarray(iou, np.float64) - g["iou"][n]).max()
        print(f"mask_input.hf.{C.case_id(case)}: logits {d_low:.3g} (< {HF_LOGIT_TOL}), iou {d_iou:.3g} (< {HF_IOU_TOL})")
        assert d_low < HF_LOGIT_TOL, (C.case_id(case), d_low)
        assert d_iou < HF_IOU_TOL, (C.case_id(case), d_iou)
        assert plane == int(g["plane"][n]) == 0
        mask = O.postprocess_logits(np.asarray(low[plane], np.float32), (1024, 1024)) > 0
        want = np.unpackbits(g["mask_bits"][n]).reshape(1024 // MASK_ROW_STRIDE, 1024).astype(bool)
        assert (mask[::MASK_ROW_STRIDE] != want).mean() < 2e-5
        # ... and the fixture tells a decode with mask input from one without: the same clicks at once miss it by far
        low0, _, _ = C.decode_stage(seg.embedding, seg.rs, clicks, labels, box, params, None)
        assert np.abs(np.asarray(low0).reshape(4, -1)[:, ::LOW_STRIDE] - g["low_samples"][n]).max() > 100 * HF_LOGIT_TOL


def test_mask_embed_reference_is_local():
    """A token's 16 values depend on its own 4 x 4 block of logits and on nothing else."""
    params = W.synthetic_weights(get_config("vit_test"), 7, mask_branch=True)
    rng = np.random.default_rng(3)
    logits = rng.standard_normal((256, 256)) * 3
    base = C.mask_embed_ref(params, logits)
    assert base.shape == (4096, 16) and base.dtype == np.float64
    for ty, tx in ((0, 0), (17, 42), (63, 63), (5, 63)):
        changed = logits.copy()
        changed[4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4] += rng.standard_normal((4, 4))
        rows = np.flatnonzero((C.mask_embed_ref(params, changed) != base).any(axis=1))
        assert rows.tolist() == [ty * 64 + tx]
    # one pixel outside a token's block leaves it alone, the last pixel inside moves it
    changed = logits.copy()
    changed[4 * 17 + 3, 4 * 42 + 3] += 1.0
    assert np.flatnonzero((C.mask_embed_ref(params, changed) != base).any(axis=1)).tolist() == [17 * 64 + 42]
    assert C.dense_embedding_ref(params, logits).shape == (4096, 256)


def test_mask_branch_inventory_and_round_trips(tmp_path):
    cfg = CONFIGS["vit_test"]
    without, full = W.synthetic_weights(cfg, 5), W.synthetic_weights(cfg, 5, mask_branch=True)
    want = {"pe.mask.down1.w": (4, 1, 2, 2), "pe.mask.down1.b": (4,), "pe.mask.ln1.w": (4,), "pe.mask.ln1.b": (4,),
            "pe.mask.down2.w": (16, 4, 2, 2), "pe.mask.down2.b": (16,), "pe.mask.ln2.w": (16,), "pe.mask.ln2.b": (16,),
            "pe.mask.proj.w": (256, 16), "pe.mask.proj.b": (256,)}
    assert {n: tuple(full[n].shape) for n in full if n not in without} == want
    assert set(W.MASK_BRANCH) == set(want) and not any(W.f16_operand(n) for n in want)
    # the generator is a function of (seed, name): no other tensor changes
    assert all(np.array_equal(full[n], without[n]) for n in without)
    assert [n for n, _, _ in W.param_specs(cfg)] == [n for n, _, _ in W.param_specs(cfg, mask_branch=True) if n not in want]
    hf = {"down1": "conv1", "ln1": "layer_norm1", "down2": "conv2", "ln2": "layer_norm2", "proj": "conv3"}
    meta = {"down1": "0", "ln1": "1", "down2": "3", "ln2": "4", "proj": "6"}
    for params, has in ((full, True), (without, False)):
        sd = W.to_hf_state_dict(cfg, params)
        assert ("prompt_encoder.mask_embed.conv1.weight" in sd) == has
        if has:
            for ours, theirs in hf.items():
                assert np.array_equal(sd[f"prompt_encoder.mask_embed.{theirs}.bias"], params[f"pe.mask.{ours}.b"])
            assert sd["prompt_encoder.mask_embed.conv3.weight"].shape == (256, 16, 1, 1)
        back = W.from_hf_state_dict(cfg, sd)
        assert set(back) == set(params) and all(np.array_equal(back[n], params[n]) for n in params)
        sd = W.to_meta_state_dict(cfg, params)
        assert ("prompt_encoder.mask_downscaling.0.weight" in sd) == has
        if has:
            for ours, theirs in meta.items():
                assert np.array_equal(sd[f"prompt_encoder.mask_downscaling.{theirs}.bias"], params[f"pe.mask.{ours}.b"])
            assert sd["prompt_encoder.mask_downscaling.6.weight"].shape == (256, 16, 1, 1)
        back = W.from_meta_state_dict(cfg, sd)
        assert set(back) == set(params) and all(np.array_equal(back[n], params[n]) for n in params)
        # the file: with the branch or without it
        path = W.save_weights(tmp_path / f"m{int(has)}" / W.weight_file_name(cfg), cfg, params)
        _, loaded = W.load_weights(path)
        assert set(loaded) == set(params) and all(np.array_equal(loaded[n], params[n]) for n in params)
    # a part of the branch in a checkpoint is ignored on the way in ...
    sd = W.to_meta_state_dict(cfg, full)
    del sd["prompt_encoder.mask_downscaling.3.bias"]
    assert set(W.from_meta_state_dict(cfg, sd)) == set(without)
    sd = W.to_hf_state_dict(cfg, full)
    del sd["prompt_encoder.mask_embed.layer_norm2.weight"]
    assert set(W.from_hf_state_dict(cfg, sd)) == set(without)
    # ... and refused on the way out
    partial = dict(full)
    del partial["pe.mask.ln2.b"]
    with pytest.raises(ValueError, match="partial"):
        W.save_weights(tmp_path / "p.dlw", cfg, partial)
    with pytest.raises(ValueError, match="partial"):
        W.to_hf_state_dict(cfg, partial)
    wrong = dict(full)
    wrong["pe.mask.down2.w"] = np.zeros((16, 4, 2, 1), np.float32)
    with pytest.raises(ValueError, match="shape"):
        W.save_weights(tmp_path / "w.dlw", cfg, wrong)


def test_entry_lists_with_marks():
    r = api.Region(P(10, 20), P(300, 400))
    assert api.REFINE_MARK == 4
    # a mark after the first click and one after the third of four clicks; a second prompt without marks, with a box
    e = api.click_entries([[P(1, 2), P(3, 4), P(5, 6), P(7, 8)], [P(9, 10), P(11, 12)]], [[1, 0, 1, 0], [1, 0]], [None, r], [[1, 3], None])
    assert e.heads == [0, None, None, None, None, None, 1, None]
    assert e.points == [(1, 2), (0, 0), (3, 4), (5, 6), (0, 0), (7, 8), (9, 10), (11, 12)]
    assert e.regions == [(0, 0, -1, -1), (4, 0, 0, 0), (0, 0, 0, 0), (1, 0, 0, 0), (4, 0, 0, 0), (0, 0, 0, 0),
                         (10, 20, 300, 400), (0, 0, 0, 0)]
    assert e.prompt_heads == [0, 6] and e.token_rows == [10, 9] and e.stage_clicks == [[1, 3, 4], [2]]
    # the unmarked prompt's launch first, then one launch per stage: 6 + 1, 6 + 3, 6 + 4 rows
    assert e.launches == [(9, [1]), (7, [0]), (9, [0]), (10, [0])]
    assert api._entry_calls(e) == [(list(range(8)), True)]
    # "each": a mark behind every click but the last; with a box the stages have 7 + k rows
    e = api.click_entries([[P(1, 2), P(3, 4), P(5, 6)]], None, [r], "each")
    assert e.regions == [(10, 20, 300, 400), (4, 0, 0, 0), (1, 0, 0, 0), (4, 0, 0, 0), (1, 0, 0, 0)]
    assert e.stage_clicks == [[1, 2, 3]] and e.launches == [(8, [0]), (9, [0]), (10, [0])]
    # one click has nothing to refine: "each" leaves today's point entry
    e = api.click_entries([[P(1, 2)]], None, None, "each")
    assert e.heads == [0] and e.stage_clicks == [[1]] and api._entry_calls(e) == [([0], False)]
    # without refine_after the lists are what they were
    a, b = api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r]), api.click_entries([[P(1, 2), P(3, 4)]], [[1, 0]], [r], [None])
    assert (a.heads, a.points, a.regions, a.launches) == (b.heads, b.points, b.regions, b.launches) and a.launches == [(9, [0])]
    # marks do not count towards the 8 clicks
    assert len(api.click_entries([[P(k, k) for k in range(8)]], None, None, "each").heads) == 15


def test_builder_refusals():
    two = [[P(0, 0), P(1, 1)]]
    for bad in ([[0]], [[2]], [[1, 1]], [[-1]], ["all"], [[1], [1]]):
        with pytest.raises(api.Error):
            api.click_entries(two, None, None, bad)
    with pytest.raises(api.Error):
        api.click_entries([[P(0, 0), P(1, 1), P(2, 2)]], None, None, [[2, 1]])
    with pytest.raises(api.Error):
        api.Segmentation.compute_mask_batch([], points=[], refine_after="each")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    rocm_clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    cxx = str(rocm_clang) if rocm_clang.exists() else (shutil.which("c++") or shutil.which("g++") or shutil.which("clang++"))
    assert cxx, "no host C++ compiler found"
    exe = tmp_path_factory.mktemp("mask_input_plan") / "mask_input_plan_cases"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(ROOT / "tests" / "mask_input_plan_cases.cpp"),
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


def test_library_reads_marks_into_stages(plan):
    # entries 0..5: head, mark, background click, foreground click, mark, background click -> clicks in entries 0, 2, 3, 5;
    # stages of 1, 3 and 4 clicks.  entries 6, 7: a box and a second click, no mark: one stage
    out = plan([EMPTY, MARK, BG, FG, MARK, BG, BOX, BG])
    assert out == ["prompt 0 clicks 4 box 0 points 5 entries 0,2,3,5 labels 1,0,1,0 stages 1,3,4 staged 1",
                   "prompt 6 clicks 2 box 1 points 4 entries 6,7 labels 1,0 stages 2 staged 0"]
    # a boxed prompt keeps its box in every stage (points = clicks + 2); a mark right behind the head is fine
    assert plan([BOX, MARK, FG]) == ["prompt 0 clicks 2 box 1 points 4 entries 0,2 labels 1,1 stages 1,2 staged 1"]
    # marks do not count towards the 8 clicks: 8 clicks and 7 marks
    out = plan([EMPTY] + [MARK, FG] * 7)
    assert out == ["prompt 0 clicks 8 box 0 points 9 entries 0,2,4,6,8,10,12,14 labels 1,1,1,1,1,1,1,1 stages 1,2,3,4,5,6,7,8 staged 1"]
    assert "more than 8 clicks" in plan([EMPTY] + [MARK, FG] * 7 + [FG])[0]


def test_library_reads_calls_without_marks_as_before(plan):
    assert plan([EMPTY, BG, FG, BOX, BOX, BG]) == [
        "prompt 0 clicks 3 box 0 points 4 entries 0,1,2 labels 1,0,1 stages 3 staged 0",
        "prompt 3 clicks 1 box 1 points 3 entries 3 labels 1 stages 1 staged 0",
        "prompt 4 clicks 2 box 1 points 4 entries 4,5 labels 1,0 stages 2 staged 0"]
    assert plan([BOX, BOX], points=False) == ["prompt 0 clicks 0 box 1 points 2 entries labels stages 0 staged 0",
                                              "prompt 1 clicks 0 box 1 points 2 entries labels stages 0 staged 0"]
    # without the mask branch such calls are served as ever, and the old refusals keep their words
    assert plan([EMPTY, BG], branch=False) == ["prompt 0 clicks 2 box 0 points 3 entries 0,1 labels 1,0 stages 2 staged 0"]
    for bad in ("c:2,0,0,0", "c:-1,0,0,0", "c:1,0,0,5", "c:0,1,0,0", "c:3,0,0,0", "c:5,0,0,0"):
        for more in ([], [MARK, FG]):
            line = plan([EMPTY, bad] + more)[0]
            assert line.startswith("error") and "label" in line, (bad, more)


def test_refusals_of_a_marked_call_name_the_callers_entries(plan):
    # the bad label sits in entry 3 of the caller's list (entry 2 once the mark is taken out)
    line = plan([EMPTY, MARK, FG, "c:2,0,0,0"])[0]
    assert line.startswith("error") and "entry 3:" in line and "label" in line
    # nine clicks of the prompt whose head is entry 2 (entry 1 without the first prompt's mark)
    line = plan([EMPTY, MARK, BOX] + [MARK, FG] + [FG] * 7)[0]
    assert line.startswith("error") and "mark" in line                        # the first prompt's mark is its last entry
    line = plan([EMPTY, MARK, FG, BOX] + [MARK, FG] + [FG] * 7)[0]
    assert line.startswith("error") and "the prompt of entry 3 has more than 8 clicks" in line


def test_library_refusals_name_the_mark(plan):
    refused = {
        "mark after mark": [EMPTY, MARK, MARK, FG],
        "mark as the last entry of the call": [EMPTY, FG, MARK],
        "mark as the last entry of a prompt": [EMPTY, MARK, EMPTY, FG],
        "trailing ints": [EMPTY, "c:4,0,0,5", FG],
        "trailing ints (second)": [EMPTY, "c:4,1,0,0", FG],
        "mark in front": [MARK, EMPTY, FG],
    }
    for what, entries in refused.items():
        line = plan(entries)[0]
        assert line.startswith("error") and "mark" in line, (what, line)
    line = plan([EMPTY, MARK, FG], branch=False)[0]
    assert line.startswith("error") and "mark" in line and "pe.mask" in line


def test_library_packs_every_stage_as_the_python_side_does(plan):
    """pack_points on every stage of every case, both images, in one call: stage k is multi_click_cases.pack of the first k
    clicks with the prompt's box or the padding point; exact equality (integers held in floats: no tolerance)."""
    entries, heads = [], []
    for case in C.CASES:
        name, clicks, labels, box, _ = case
        marks = C.stage_clicks(case)[:-1]
        heads.append(len(entries))
        region = ",".join(map(str, box)) if box is not None else "0,0,-1,-1"
        entries.append(f"h:{region}@{clicks[0][0]},{clicks[0][1]}@{M.oracle_frame(name)[1]}")
        for c in range(1, len(clicks)):
            if c in marks:
                entries.append(MARK)
            entries.append(f"c:{labels[c]},0,0,0@{clicks[c][0]},{clicks[c][1]}")
    rows = M.packed_lines(plan(entries))
    want = [(head, k, case) for head, case in zip(heads, C.CASES) for k in C.stage_clicks(case)]
    assert [r[0] for r in rows] == [[head, k] for head, k, _ in want] and len(rows) == sum(len(C.stage_clicks(c)) for c in C.CASES)
    for (_, coords, labels), (_, k, case) in zip(rows, want):
        name, clicks, labs, box, _ = case
        want_c, want_l = M.pack(M.oracle_frame(name)[0], clicks[:k], labs[:k], box)
        assert coords == want_c.tolist() and labels == want_l.tolist(), (C.case_id(case), k)


def test_mask_input_moves_every_reference_mask(references):
    """Inputs of tests/test_gpu_mask_input.py, from the float64 reference alone."""
    assert len(C.WITHOUT_FRACTION) == len(C.CASES)
    limit = max(C.EXACT_LIMIT, C.CHAIN_LIMIT)
    assert C.EXACT_LIMIT == M.DISAGREE_LIMIT
    for i, case in enumerate(C.CASES):
        mask, plane, unstaged = references[i]
        fraction = float((mask != unstaged).mean())
        print(f"mask_input.oracle.{C.case_id(case)}: with / without mask input differ in {fraction:.4f} of the pixels")
        assert plane == 0                                   # every last stage has two clicks or more
        assert fraction >= 10 * limit, (C.case_id(case), fraction, limit)
        assert abs(fraction - C.WITHOUT_FRACTION[i]) < 2e-3, (C.case_id(case), fraction, C.WITHOUT_FRACTION[i])
    assert C.CHAIN_LIMIT <= min(C.WITHOUT_FRACTION) / 10
    if C.CHAIN_FRACTION:
        assert C.CHAIN_LIMIT == 3 * max(C.CHAIN_FRACTION)


def test_cpp_wrapper_takes_refine_after(tmp_path):
    """include/dlimgedit/dlimgedit.hpp: compute_mask(clicks, region, refine_after), refine_each and the batch form compile
    against the header alone, and the mark's value is the macro of dlimgedit.h."""
    rocm_clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    cxx = str(rocm_clang) if rocm_clang.exists() else (shutil.which("c++") or shutil.which("g++") or shutil.which("clang++"))
    assert cxx, "no host C++ compiler found"
    src = tmp_path / "refine.cpp"
    src.write_text('''#include <dlimgedit/dlimgedit.hpp>
static_assert(DLIMG_REFINE_MARK == 4, "the first value SAM's labels leave free");
dlimg::Image one(dlimg::Segmentation const& s, std::vector<dlimg::Click> const& clicks) {
    return s.compute_mask(clicks, std::nullopt, dlimg::Segmentation::refine_each(clicks.size()));
}
std::vector<dlimg::Image> many(dlimg::Segmentation const& s, std::vector<dlimg::Click> const& clicks, dlimg::Region box) {
    return dlimg::Segmentation::compute_mask_batch({&s, &s}, {clicks, clicks}, {box, std::nullopt}, {{1}, {}});
}
int main() { return dlimg::Segmentation::refine_each(4) == std::vector<int>{1, 2, 3} ? 0 : 1; }
''')
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-DDLIMGEDIT_LOAD_DYNAMIC", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
