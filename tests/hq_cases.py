"""Inputs shared by the SAM-HQ tests (tests/test_hq_oracle.py, tests/test_gpu_hq.py) and the fixture's generator
(tests/golden/make_hq_golden.py): the reduced geometry of the test model, two synthetic images -- the second one's longest
side is not 1024, so it takes the resize path -- and prompts on each, in original-image pixels.

The geometry is built here and not in sam_config.CONFIGS (the loader reads it from the file header): three blocks, the first
and the last with global attention.  SAM-HQ's early feature is the output of the FIRST global block, block 0, which is not the
last block: a build that taps the wrong one computes other HQ features."""
import numpy as np

from conftest import synthetic_image

from dlimgedit_amd.sam_config import SamConfig

CFG = SamConfig("vit_hqtest", 128, 3, 2, (0, 2))
# Seed of the synthetic weights.  Chosen on the CPU from the float64 reference alone (test_hq_oracle.py asserts it): with it
# the HQ mask of every case differs from the plain mask of the same prompt in a visible share of the pixels.
SEED = 11

# name -> (image seed, width, height)
IMAGES = {"square": (0, 1024, 1024), "small": (5, 640, 480)}


def image(name: str) -> np.ndarray:
    seed, w, h = IMAGES[name]
    return synthetic_image(seed, width=w, height=h)


# (image, clicks (x, y), labels 1 foreground / 0 background, box x0 y0 x1 y1 or None, refine_after: click counts or None)
CASES = [
    ("square", ((512, 512),), (1,), None, None),                                               # one point: 8 token rows
    ("small", (), (), (91, 178, 305, 372), None),                                              # a box: 8
    ("square", ((312, 487),), (1,), (257, 264, 580, 567), None),                               # box plus point: 9
    ("small", ((438, 42), (434, 77), (303, 368)), (1, 1, 0), (150, 30, 520, 400), None),       # 3 clicks with a box: 11
    ("square", ((686, 404), (61, 121), (450, 540), (796, 130), (489, 19), (139, 120), (353, 207)),
     (1, 0, 1, 1, 1, 1, 0), (121, 128, 838, 674), None),                                       # 7 clicks with a box: 9 points, 15 rows
    ("small", ((557, 27), (427, 424), (540, 194), (97, 95), (314, 18), (368, 300), (562, 444), (71, 405)),
     (1, 0, 1, 1, 0, 0, 0, 1), None, None),                                                    # 8 clicks without a box: 9 points
    ("square", ((137, 131), (816, 511)), (1, 0), None, (1,)),                                  # a marked prompt of 2 stages: 8 -> 9
]
# what no SAM-HQ model takes: 8 clicks and a box, 10 points
TOO_MANY = ("square", CASES[5][1], CASES[5][2], (121, 128, 838, 674), None)


def points_of(case) -> int:
    """Packed points of the case's (last) prompt: clicks + the padding point or the two corners."""
    return len(case[1]) + (2 if case[3] is not None else 1)


def stage_clicks(case) -> list:
    return list(case[4] or ()) + [len(case[1])]


def case_id(case) -> str:
    name, clicks, _, box, after = case
    return f"{name}-{len(clicks)}clicks-{'box' if box is not None else 'nobox'}-{points_of(case)}pts" + ("-marked" if after else "")


def pack(rs, clicks, labels, box):
    """One prompt packed in the resized frame of `rs` (an oracle ResizeLongestSide whose target_extent was called): the clicks
    in the order given, then the box corners (labels 2, 3); the padding point (0, 0), label -1, only without a box."""
    pts = [rs.transform(*c) for c in clicks]
    labs = list(labels)
    if box is not None:
        pts += [rs.transform(box[0], box[1]), rs.transform(box[2], box[3])]
        labs += [2, 3]
    else:
        pts.append((0, 0))
        labs.append(-1)
    return np.array(pts, np.float32).reshape(-1, 2), np.array(labs, np.float32)


def resize_geometry(name):
    """(oracle ResizeLongestSide of the image, (h, w))"""
    from oracle import sam_oracle as O
    _, w, h = IMAGES[name]
    rs = O.ResizeLongestSide()
    rs.target_extent(w, h)
    return rs, (h, w)
