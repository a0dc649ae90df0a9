"""Inputs shared by the multi-click tests (tests/test_multi_click_oracle.py, tests/test_gpu_multi_click.py): the two synthetic
images of box_point_cases -- the second one's longest side is not 1024, so it takes the resize path -- and prompts of 2 .. 8
clicks on each, foreground and background, with and without a box, in original-image pixels."""
import numpy as np

import box_point_cases as B

IMAGES = B.IMAGES
image = B.image

# (image, clicks (x, y), labels 1 foreground / 0 background, box x0 y0 x1 y1 or None).  Chosen on the CPU from the float64
# reference alone so that the reference mask changes in 4.8 % of the pixels or more both when the last click is left out and
# when its label is flipped (test_multi_click_oracle.py holds both to ten times the limit of the GPU parity test).  Token rows
# T = 6 + clicks without a box, 7 + clicks with one: 8, 9, 9, 12, 12, 15, 14, 11 -- the first count above 8 with and without
# a box, 12 with and without, the largest; every case has a background click, the last click is background in five.
CASES = [
    ("square", ((137, 131), (816, 511)), (1, 0), None),
    ("square", ((497, 151), (411, 950)), (1, 0), (302, 307, 725, 519)),
    ("wide", ((438, 42), (434, 77), (603, 568)), (1, 1, 0), None),
    ("square", ((523, 454), (678, 1018), (281, 876), (141, 356), (806, 253)), (1, 1, 0, 1, 1), (318, 444, 635, 692)),
    ("wide", ((576, 141), (473, 481), (709, 520), (773, 77), (622, 280), (548, 166)), (1, 0, 0, 1, 1, 0), None),
    ("wide", ((686, 404), (61, 121), (450, 540), (796, 130), (489, 19), (139, 120), (353, 207), (581, 281)),
     (1, 0, 1, 1, 1, 1, 0, 0), (121, 128, 338, 274)),
    ("square", ((757, 27), (427, 824), (540, 194), (697, 95), (714, 18), (368, 300), (962, 744), (671, 505)),
     (1, 0, 1, 1, 0, 0, 0, 1), None),
    ("wide", ((294, 564), (402, 204), (748, 261), (619, 188)), (1, 0, 1, 1), (190, 77, 447, 373)),
]

# Fraction of pixels in which a mask of slot 14 may differ from the float64 reference's mask of the same prompt.
# Measured on MI355X with the decoder this change started from (its two-token and three-token kernels are unchanged by it,
# instruction for instruction), same images, same route (dlimg_amd_get_embedding -> oracle/decoder_ref.decode_fp64 ->
# select_single -> postprocess_logits -> > 0), on the parts of the cases above that decoder could take, in the order of CASES:
#   two tokens, the first click alone (all eight cases):
#       1.94e-4, 0.99e-4, 1.08e-4, 0.33e-4, 1.10e-4, 0.69e-4, 0.98e-4, 0.38e-4
#   two tokens, the box alone (the four cases with a box):
#       0.89e-4, 3.88e-4 (407 of 1024 x 1024), 0.33e-4, 1.06e-4
#   three tokens, the box refined by the first click (the same four):
#       1.32e-4, 1.01e-4, 0.96e-4, 1.79e-4 (86 of 800 x 600)
# The limit is three times the largest, the lower end of the "3-5x what was measured" convention of tests/conftest.py: further
# tokens add attention keys and no new f16 rounding point.  [The eight cases themselves then measured 1.23e-4 .. 3.81e-4.]
PARENT_TWO_TOKEN_FRACTION = 0.000388145
PARENT_THREE_TOKEN_FRACTION = 0.000179167
DISAGREE_LIMIT = 3 * max(PARENT_TWO_TOKEN_FRACTION, PARENT_THREE_TOKEN_FRACTION)        # 1.16e-3


def token_rows(case) -> int:
    _, clicks, _, box = case
    return 5 + len(clicks) + (2 if box is not None else 1)


def case_id(case) -> str:
    name, clicks, labels, box = case
    return f"{name}-{len(clicks)}clicks-{'box' if box is not None else 'nobox'}-T{token_rows(case)}"


def pack(rs, clicks, labels, box):
    """One prompt packed in the resized frame of `rs` (an oracle ResizeLongestSide whose target_extent was called), the way
    SamOnnxModel._embed_points wants it: the clicks in the order given, then the box corners (labels 2, 3); the padding point
    (0, 0), label -1, only without a box.  -> (coords f32 [n, 2], labels f32 [n])."""
    pts = [rs.transform(*c) for c in clicks]
    labs = list(labels)
    if box is not None:
        pts += [rs.transform(box[0], box[1]), rs.transform(box[2], box[3])]
        labs += [2, 3]
    else:
        pts.append((0, 0))
        labs.append(-1)
    return np.array(pts, np.float32), np.array(labs, np.float32)


def variants(case):
    """{"full": the case's prompt, "without_last": its last click left out, "flipped": the last click's label flipped}, each
    (clicks, labels, box)."""
    _, clicks, labels, box = case
    return {"full": (clicks, labels, box), "without_last": (clicks[:-1], labels[:-1], box),
            "flipped": (clicks, labels[:-1] + (1 - labels[-1],), box)}


def reference_mask(emb, rs, clicks, labels, box, params, hw):
    """float64 reference decode of one prompt on a given embedding -> (boolean mask [h, w] of the single-mask mode, plane)."""
    coords, labs = pack(rs, clicks, labels, box)
    return B.reference_mask(emb, coords, labs, len(labs), params, hw)


def packed_lines(out):
    """`packed <head> [stage <clicks>] coords x,y;... labels l,...` lines -> [(the ints in front, coords [[x, y], ...], labels)]"""
    rows = []
    for line in out:
        if not line.startswith("packed"):
            continue
        words = line.split()
        at = words.index("coords")
        coords = [[float(v) for v in xy.split(",")] for xy in words[at + 1].split(";")]
        rows.append(([int(w) for w in words[1:at] if w != "stage"], coords, [float(v) for v in words[at + 3].split(",")]))
    return rows


def oracle_frame(name):
    """-> (the oracle's ResizeLongestSide of image `name`, its extent as the case programs take it: <width>x<height>)"""
    from oracle import sam_oracle as O
    _, w, h = IMAGES[name]
    rs = O.ResizeLongestSide()
    rs.target_extent(w, h)
    return rs, f"{w}x{h}"
