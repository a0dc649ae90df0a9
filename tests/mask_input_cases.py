"""Inputs shared by the mask-input tests (tests/test_mask_input_oracle.py, tests/test_gpu_mask_input.py) and the fixture's
generator (tests/golden/make_mask_input_golden.py): the float64 reference of the prompt encoder's mask branch, the staged
reference built on oracle/decoder_ref.decode_fp64, and prompts with refinement marks on the two images of box_point_cases
(the second one takes the resize path).

A prompt with marks is decoded in stages (csrc/prompt_plan.hpp): stage j takes the clicks in front of mark j, the last stage
all of them, every stage the prompt's box or the padding point; from the second stage on a stage takes as SAM's mask input
the low-res logits plane the stage before it would deliver as its single mask."""
import math

import numpy as np

import box_point_cases as B
import multi_click_cases as M

IMAGES = B.IMAGES
image = B.image
f64 = np.float64
LN2D_EPS = 1e-6

# (image, clicks (x, y), labels, box or None, refine_after: click counts or "each").  Clicks, labels and boxes are those of
# multi_click_cases.CASES (cut to the wanted number of clicks), the marks were placed on the CPU from the float64 reference
# alone so that the reference mask with mask input differs from the reference of the same clicks without it in WITHOUT_FRACTION
# of the pixels (test_mask_input_oracle.py holds every one to ten times the limits below).  Covered: two stages 7 -> 8 token
# rows; two stages ending at 9 rows, the first count above 8; three stages; a boxed prompt; the "wide" image (resize path);
# 8 clicks with "each" (8 stages, 7 .. 14 rows); 8 clicks, one mark and a box (15 rows).
CASES = [
    ("square", M.CASES[0][1], M.CASES[0][2], None, (1,)),                                  # 7 -> 8
    ("wide", M.CASES[2][1], M.CASES[2][2], None, (1,)),                                    # 7 -> 9, resize path
    ("wide", M.CASES[2][1], M.CASES[2][2], None, (1, 2)),                                  # 7 -> 8 -> 9: three stages
    ("square", M.CASES[1][1], M.CASES[1][2], M.CASES[1][3], (1,)),                         # box: 8 -> 9
    ("wide", M.CASES[7][1], M.CASES[7][2], M.CASES[7][3], (2,)),                           # box: 9 -> 11
    ("square", M.CASES[6][1], M.CASES[6][2], None, "each"),                                # 8 stages, 7 .. 14
    ("wide", M.CASES[5][1], M.CASES[5][2], M.CASES[5][3], (4,)),                           # box, 8 clicks: 11 -> 15
]


def stage_clicks(case) -> list:
    """Clicks of each stage, worked out from the rule: a mark after the first k clicks ends a stage of k clicks."""
    _, clicks, _, _, after = case
    marks = list(range(1, len(clicks))) if after == "each" else list(after)
    return marks + [len(clicks)]


def token_rows(case) -> list:
    """Token rows of each stage: 5 output tokens + clicks + the padding point or the two corners."""
    return [5 + k + (2 if case[3] is not None else 1) for k in stage_clicks(case)]


def case_id(case) -> str:
    name, clicks, _, box, _ = case
    return f"{name}-{len(clicks)}clicks-{'box' if box is not None else 'nobox'}-T" + "-".join(str(t) for t in token_rows(case))


def first_stage_is_two_point_prompt(case) -> bool:
    """The first stage is a single click without a box: a two-point prompt, which dlimg_amd_get_logits decodes on its own."""
    return stage_clicks(case)[0] == 1 and case[3] is None


# ---- float64 reference of the mask branch (SAM's PromptEncoder.mask_downscaling / HF's SamMaskEmbedding)

def _gelu(x):
    from oracle.decoder_ref import _erf
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def _ln2d(x, w, b):
    """LayerNorm2d over the last (channel) axis."""
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    var = (xc * xc).mean(axis=-1, keepdims=True)
    return xc / np.sqrt(var + LN2D_EPS) * w + b


def _conv2x2s2(x, w, b):
    """x [H, W, Ci] -> [H / 2, W / 2, Co]; w [Co, Ci, 2, 2] (torch Conv2d, kernel 2, stride 2)."""
    H, W_, ci = x.shape
    blocks = x.reshape(H // 2, 2, W_ // 2, 2, ci).transpose(0, 2, 4, 1, 3)          # [H/2, W/2, Ci, ky, kx]
    return np.einsum("yxckl,ockl->yxo", blocks, w) + b


def mask_embed_ref(params, logits) -> np.ndarray:
    """Low-res logits [256, 256] -> h [4096, 16], float64: the branch in front of its last (1x1) convolution, token-major
    (token = row * 64 + column of the 64 x 64 grid)."""
    p = {k: np.asarray(v, f64) for k, v in params.items() if k.startswith("pe.mask.")}
    x = np.asarray(logits, f64).reshape(256, 256, 1)
    x = _gelu(_ln2d(_conv2x2s2(x, p["pe.mask.down1.w"], p["pe.mask.down1.b"]), p["pe.mask.ln1.w"], p["pe.mask.ln1.b"]))
    x = _gelu(_ln2d(_conv2x2s2(x, p["pe.mask.down2.w"], p["pe.mask.down2.b"]), p["pe.mask.ln2.w"], p["pe.mask.ln2.b"]))
    return x.reshape(4096, 16)


def dense_embedding_ref(params, logits) -> np.ndarray:
    """The dense prompt embedding of a mask input, token-major [4096, 256], float64."""
    return mask_embed_ref(params, logits) @ np.asarray(params["pe.mask.proj.w"], f64).T + np.asarray(params["pe.mask.proj.b"], f64)


# ---- the staged reference

def decode_stage(emb, rs, clicks, labels, box, params, mask_logits=None):
    """One stage in float64 -> (logits [4, 256, 256], iou [4], plane of the single-mask mode).  mask_logits: the stage's mask
    input [256, 256] or None.  The unchanged oracle forms keys = emb + pe.no_mask, so a masked stage passes
    emb + dense - pe.no_mask: the dense embedding takes no_mask's place."""
    from oracle import decoder_ref as R
    from oracle import sam_oracle as O
    coords, labs = M.pack(rs, clicks, labels, box)
    e = np.asarray(emb, f64)
    if mask_logits is not None:
        e = e + dense_embedding_ref(params, mask_logits) - np.asarray(params["pe.no_mask"], f64)[None, :]
    low, iou = R.decode_fp64(e, coords, labs, params)
    return low, iou, O.select_single(np.asarray(iou, np.float32), len(labs))


def staged_reference(emb, rs, case, params, hw, first_mask_logits=None, from_stage=0):
    """The pure float64 chain of a case -> (boolean mask [h, w] of the last stage, its plane, the low-res logits of every
    stage's delivered plane).  first_mask_logits / from_stage: start at a later stage with a given mask input."""
    from oracle import sam_oracle as O
    _, clicks, labels, box, _ = case
    prev, planes = first_mask_logits, []
    low = plane = None
    for k in stage_clicks(case)[from_stage:]:
        low, _, plane = decode_stage(emb, rs, clicks[:k], labels[:k], box, params, prev)
        prev = low[plane]
        planes.append(prev)
    return O.postprocess_logits(np.asarray(low[plane], np.float32), hw) > 0, plane, planes


def unstaged_reference(emb, rs, case, params, hw):
    """The same clicks without any mark: what the call answers without mask input."""
    _, clicks, labels, box, _ = case
    return M.reference_mask(emb, rs, clicks, labels, box, params, hw)[0]


# Fraction of pixels in which the float64 reference with mask input differs from the float64 reference of the same clicks
# without it, on the CPU oracle's embedding, in the order of CASES (test_mask_input_oracle.py recomputes them).
WITHOUT_FRACTION = [0.4382, 0.2479, 0.1487, 0.5210, 0.3355, 0.4464, 0.6768]

# Measured on MI355X, in the order of CASES (None: the case's first stage is not a two-point prompt):
#   exact stage: the GPU's own stage-1 plane (dlimg_amd_get_logits) fed to the float64 reference of the later stages
EXACT_STAGE_FRACTION = [0.000208855, 0.00025, 0.000245833, None, None, 0.000427246, None]
#   whole chain: the delivered mask against the pure float64 chain
CHAIN_FRACTION = [0.000273705, 0.00025, 0.00026875, 0.000265121, 0.000425, 0.000452995, 0.000266667]
# Exact stage keeps the limit of the multi-click prompts: the mask adds to the keys in front of the one existing f16 rounding
# and adds no rounding point.
EXACT_LIMIT = M.DISAGREE_LIMIT
# The whole chain also carries the error of every earlier stage's logits into the next stage's input: three times the largest
# measured fraction (the convention of tests/conftest.py), which has to stay at or below a tenth of the smallest with / without
# difference of the cases.
CHAIN_LIMIT = 3 * max(CHAIN_FRACTION)
