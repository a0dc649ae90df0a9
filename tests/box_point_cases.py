"""Inputs shared by the box + point tests (tests/test_box_point_oracle.py, tests/test_gpu_box_point.py) and the fixture's
generator (tests/golden/make_box_point_golden.py): two synthetic images of different aspect ratio -- the second one's
longest side is not 1024, so it takes the resize path -- and box / point pairs on each, in original-image pixels."""
import numpy as np

from conftest import synthetic_image

# name -> (image seed, width, height)
IMAGES = {"square": (0, 1024, 1024), "wide": (5, 800, 600)}

# (image, box x0 y0 x1 y1, point x y).  Chosen on the CPU from the float64 reference alone so that the reference masks of
# box + point, box alone and point alone differ pairwise in 14 % of the pixels or more (test_box_point_oracle.py holds them
# to ten times the limit of the GPU parity test).
PAIRS = [
    ("square", (20, 69, 288, 322), (257, 199)),
    ("square", (257, 264, 580, 567), (312, 487)),
    ("square", (47, 597, 441, 826), (101, 668)),
    ("wide", (91, 278, 305, 372), (145, 344)),
    ("wide", (249, 134, 419, 237), (352, 202)),
    ("wide", (2, 245, 167, 458), (152, 336)),
]

# Fraction of pixels in which a mask of slot 14 may differ from the float64 reference's mask of the same prompt.
# Measured on MI355X with the two-token decoder this change started from, same images, boxes and points, same route
# (dlimg_amd_get_embedding -> oracle/decoder_ref.decode_fp64 -> select_single(iou, 2) -> postprocess_logits -> > 0):
#   box alone    3.38e-4 of the pixels at most (354 of 1024 x 1024; the six pairs: 3.13e-4, 1.34e-4, 3.38e-4, 1.33e-4, 1.44e-4, 0.98e-4)
#   point alone  2.00e-4 of the pixels at most (96 of 800 x 600;    the six pairs: 1.50e-4, 1.56e-4, 0.56e-4, 2.00e-4, 0.46e-4, 1.73e-4)
# The three-token limit is three times the larger of the two, the lower end of the "3-5x what was measured" convention of
# tests/conftest.py: the third token adds one attention key and no new f16 rounding point.
PARENT_BOX_FRACTION = 0.000337601
PARENT_POINT_FRACTION = 0.0002
DISAGREE_LIMIT = 3 * max(PARENT_BOX_FRACTION, PARENT_POINT_FRACTION)        # 1.01e-3


def image(name: str) -> np.ndarray:
    seed, w, h = IMAGES[name]
    return synthetic_image(seed, width=w, height=h)


def prompts(rs, box, point):
    """The three packed prompts of one pair in the resized frame of `rs` (an oracle ResizeLongestSide whose
    target_extent was called): {"both": (coords [3,2], labels [1,2,3]), "box": ..., "point": ...} and the number of prompt
    points each counts for select_single."""
    from oracle import sam_oracle as O
    cp, lp = O.pack_prompt(rs, point=point)
    cb, lb = O.pack_prompt(rs, region=box)
    both = (np.concatenate([cp[:1], cb]).astype(np.float32), np.array([1, 2, 3], np.float32))
    return {"both": both, "box": (cb, lb), "point": (cp, lp)}, {"both": 3, "box": 2, "point": 2}


def reference_mask(emb, coords, labels, num_points, params, hw):
    """float64 reference decode of one packed prompt on a given embedding -> boolean mask [h, w] of the single-mask mode."""
    from oracle import decoder_ref as R
    from oracle import sam_oracle as O
    low, iou = R.decode_fp64(emb, coords, labels, params)
    plane = O.select_single(np.asarray(iou, np.float32), num_points)
    return O.postprocess_logits(np.asarray(low[plane], np.float32), hw) > 0, plane
