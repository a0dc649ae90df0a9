"""Inputs shared by the prior-mark tests (tests/test_prior_ref.py, tests/test_gpu_prior.py): prompts that hand in a mask of the
caller's own as SAM's mask input, on the two images of box_point_cases (the second one takes the resize path).

A prompt with a prior is decoded like a prompt with refinement marks (csrc/prior_plan.hpp), except that its FIRST stage takes
a mask input too: the 256 x 256 plane k::mask_prior makes of the caller's mask (tests/prior_ref.py restates it).  The float64
reference of a case is therefore mask_input_cases.staged_reference(..., first_mask_logits=that plane, from_stage=0)."""
import numpy as np

import box_point_cases as B
import mask_input_cases as MI
import multi_click_cases as M
import prior_ref

IMAGES = B.IMAGES
image = B.image

# A prior is described by what draws it: ("ellipse", cx, cy, rx, ry, edge) in pixels of the image -- coverage 255 inside, 0
# outside, and with edge > 0 a linear ramp of that many pixels across the outline (a soft selection).
# (image, clicks (x, y), labels, box or None, prior, refine_after (click counts) or None, clean (max_hole, max_island) or None)
# The clicks and boxes are those of multi_click_cases / box_point_cases; the priors were placed on the CPU from the float64
# reference alone (test_prior_ref.py recomputes what is said about them here).
CASES = [
    ("square", (M.CASES[0][1][0],), (1,), None, ("ellipse", 330, 300, 260, 200, 0), None, None),                  # (a) 7 rows, masked
    ("square", (), (), M.CASES[1][3], ("ellipse", 520, 420, 260, 150, 24), None, None),                            # (b) a box alone, soft prior: 7 rows
    ("wide", (M.CASES[2][1][0],), (1,), None, ("ellipse", 420, 160, 220, 130, 0), None, None),                     # (c) resize path, 7 rows
    ("wide", M.CASES[2][1], M.CASES[2][2], None, ("ellipse", 430, 200, 240, 150, 0), None, None),                  # (d) three clicks: 9 rows
    ("wide", (B.PAIRS[3][2],), (1,), B.PAIRS[3][1], ("ellipse", 200, 330, 150, 80, 0), None, None),                # (e) a click and a box: 8 rows
    ("square", M.CASES[0][1], M.CASES[0][2], None, ("ellipse", 330, 300, 260, 200, 0), (1,), None),                # (f) prior -> 7 rows -> 8 rows
    ("square", (M.CASES[0][1][0],), (1,), None, ("ellipse", 330, 300, 260, 200, 0), None, (64, 64)),               # (g) (a) with a clean-up mark
]
NAMES = "abcdefg"
# another prior on the prompt of (a): the two reference masks differ (test_prior_ref.py)
OTHER_PRIOR = ("ellipse", 700, 640, 220, 260, 0)
STRENGTH = prior_ref.DEFAULT_STRENGTH


def draw_prior(name: str, spec) -> np.ndarray:
    """-> (h, w) uint8 coverage"""
    kind, cx, cy, rx, ry, edge = spec
    assert kind == "ellipse"
    _, w, h = IMAGES[name]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.sqrt(((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2)          # 1 on the outline
    if edge <= 0:
        return np.where(d <= 1.0, 255, 0).astype(np.uint8)
    return np.clip(np.rint(255.0 * (0.5 + (1.0 - d) * min(rx, ry) / edge)), 0, 255).astype(np.uint8)


def mi_case(case):
    """The case as mask_input_cases takes it: (image, clicks, labels, box, refine_after)."""
    name, clicks, labels, box, _, after, _ = case
    return (name, clicks, labels, box, () if after is None else after)


def token_rows(case) -> list:
    return MI.token_rows(mi_case(case))


def case_id(case) -> str:
    name, clicks, _, box, prior, after, clean = case
    return (f"{NAMES[CASES.index(case)]}-{name}-{len(clicks)}clicks-{'box' if box is not None else 'nobox'}-"
            f"{'soft' if prior[5] else 'hard'}-T" + "-".join(str(t) for t in token_rows(case)) + ("-clean" if clean else ""))


def plane_of(case, spec=None, strength=STRENGTH) -> np.ndarray:
    """The prior plane of a case (or of another prior on its image), as tests/prior_ref.py defines it."""
    name = case[0]
    _, w, h = IMAGES[name]
    pre_w, pre_h = prior_ref.pre_extent(w, h)
    return prior_ref.prior_plane(draw_prior(name, case[4] if spec is None else spec), pre_w, pre_h, strength)


def reference(emb, rs, case, params, hw, spec=None):
    """float64 chain of a case on a given embedding -> (boolean mask of the last stage BEFORE any clean-up, its plane, the IoU
    predictions [4] of the first stage)."""
    plane0 = plane_of(case, spec)
    mask, plane, _ = MI.staged_reference(emb, rs, mi_case(case), params, hw, first_mask_logits=plane0, from_stage=0)
    _, clicks, labels, box, _ = mi_case(case)
    k = MI.stage_clicks(mi_case(case))[0]
    _, iou, _ = MI.decode_stage(emb, rs, clicks[:k], labels[:k], box, params, plane0)
    return mask, plane, np.asarray(iou, np.float64)


def reference_without(emb, rs, case, params, hw):
    """The same prompt without the prior (refinement marks kept)."""
    return MI.staged_reference(emb, rs, mi_case(case), params, hw)[0]


def first_stage_is_two_point(case) -> bool:
    """The first stage has 7 token rows: its single mask is the best of planes 1 .. 3 by the IoU predictions."""
    return token_rows(case)[0] == 7


# Limits of the GPU tests (tests/test_gpu_prior.py): a single-stage case keeps the limit of the multi-click prompts -- the
# plane is bit-exact, and the mask adds to the keys in front of the one existing f16 rounding -- a case with a refinement mark
# the limit of the staged chains.
EXACT_LIMIT = MI.EXACT_LIMIT
CHAIN_LIMIT = MI.CHAIN_LIMIT


# Measured on MI355X, in the order of CASES: the fraction of pixels in which the delivered mask differs from the float64 chain
# on the GPU's own embedding (tests/test_gpu_prior.py prints them).
# (g) is (a) behind the clean-up: a few of (a)'s 191 pixels lie where a small hole or island is just above or just below the
# threshold of 64 pixels, and those components then differ as a whole.
MEASURED_FRACTION = [0.000182152, 0.000121117, 0.00023125, 0.000183333, 0.000145833, 0.000170708, 0.000652313]


def limit_of(case) -> float:
    return CHAIN_LIMIT if case[5] else EXACT_LIMIT
