"""Inputs shared by the end-to-end tests of grid prompts (tests/test_gpu_grid.py): the synthetic images, the cases, and the
rule that takes a case's two thresholds from its data.

Synthetic weights put IoU predictions and stabilities anywhere, so SAM's defaults would keep everything or nothing.  A threshold
is the midpoint of the widest gap between consecutive sorted values in the middle half of the candidates, rounded to the int
the mark carries: some candidates pass, some do not, and none sits at the threshold (asserted).
"""
import numpy as np

import grid_ref as G

f32 = np.float32

# name -> (image seed, width, height): without a padded band, and with one (pre 1024 x 683)
IMAGES = {"square": (0, 1024, 1024), "band": (3, 600, 400)}
# (image, side): one full chunk of 16 prompts, a ragged last chunk (25 = 16 + 9), four chunks
CASES = [("square", 4), ("band", 5), ("band", 8), ("square", 5)]
IDS = [f"{n}-side{s}" for n, s in CASES]


# Seed of the synthetic weights, and how their masks are made sparse.  Randomly initialised weights give masks that are speckle
# over the whole image -- logits of about N(0.1, 1.1) everywhere -- so the box of every candidate is the whole scored region
# and NMS leaves one segment whatever the seed, the image or the thresholds.  sparse_mask_weights() therefore sharpens the
# decoder's last step: every plane becomes LOGIT_SCALE * logits - LOGIT_OFFSET, i.e. a pixel is in the mask where the random
# logit exceeds 3.0 (one pixel in a few hundred), in the stability band where it lies within 0.1 of that.  The masks are then a
# handful of scattered pixels whose boxes differ from candidate to candidate, which is what the selection needs to have work
# to do.  Chosen on the CPU from the oracle's own planes for these images: 3 / 8 / 9 / 3 segments kept in the four cases, and
# every one of the three steps rejects candidates in every case.
SEED = 7
LOGIT_SCALE, LOGIT_OFFSET = 10.0, 30.0
CONST_CHANNEL, CONST_BIAS = 0, 3.0


def sparse_mask_weights(cfg, seed=SEED):
    """Seeded synthetic weights (with the mask branch) whose four logit planes are LOGIT_SCALE * p - LOGIT_OFFSET of the planes p
    the same weights would give with up-scaling channel CONST_CHANNEL taken out: the hypernetworks' last layers are scaled, and
    the offset travels through that channel, which is made the constant gelu(CONST_BIAS)."""
    import math
    from dlimgedit_amd import weights as W
    p = W.synthetic_weights(cfg, seed, mask_branch=True)
    const = 0.5 * CONST_BIAS * (1.0 + math.erf(CONST_BIAS / math.sqrt(2.0)))
    p["dec.up2.w"][:, CONST_CHANNEL] = 0
    p["dec.up2.b"][CONST_CHANNEL] = CONST_BIAS
    for m in range(4):
        p[f"dec.hyper{m}.2.w"] *= f32(LOGIT_SCALE)
        p[f"dec.hyper{m}.2.b"] *= f32(LOGIT_SCALE)
        p[f"dec.hyper{m}.2.w"][CONST_CHANNEL] = 0
        p[f"dec.hyper{m}.2.b"][CONST_CHANNEL] = f32(-LOGIT_OFFSET / const)
    return p


def write_model_dir(model_dir, cfg, seed=SEED):
    """`<model_dir>/segmentation/sam_<variant>.dlw` with sparse_mask_weights(); returns them."""
    from pathlib import Path
    from dlimgedit_amd import weights as W
    p = sparse_mask_weights(cfg, seed)
    W.save_weights(Path(model_dir) / "segmentation" / W.weight_file_name(cfg), cfg, p)
    return p


def widest_gap_threshold(values):
    """int t strictly between two consecutive sorted values of the middle half with the widest gap between them"""
    v = np.sort(np.asarray(values, np.float64))
    n = len(v)
    lo, hi = n // 4, max(n // 4 + 2, 3 * n // 4)
    mid = v[lo:hi]
    k = int(np.argmax(np.diff(mid)))
    a, b = float(mid[k]), float(mid[k + 1])
    t = int(round((a + b) / 2))
    assert a < t < b, f"no int strictly inside the widest gap ({a}, {b}): pick another seed"
    return t


def thresholds(records, iou):
    """(iou_permille, stability_permille) of a case from the reference's records and the IoU predictions of its candidates"""
    records = np.asarray(records, np.int64)
    iou = np.asarray(iou, f32)
    ip = widest_gap_threshold(iou.astype(np.float64) * 1000)
    sp = widest_gap_threshold([int(r[0]) * 1000 / int(r[2]) if r[2] > 0 else 0.0 for r in records])
    assert ip != 0 and sp != 0, "0 means SAM's default: pick another seed"
    # none sits at a threshold, in the arithmetic the filter uses
    t = f32(ip) / f32(1000)
    assert not np.any(iou == t)
    assert not any(int(r[0]) * 1000 == sp * int(r[2]) for r in records if r[2] > 0)
    return ip, sp


def rejections(records, iou, ip, sp):
    """(rejected by the IoU threshold, rejected by the stability threshold among those that pass it, suppressed by NMS, kept)"""
    ok_iou, ok_stab, alive = G.passes(records, iou, ip, sp)
    nms, kept = G.select(records, iou, ip, sp)
    return int((alive & ~ok_iou).sum()), int((alive & ok_iou & ~ok_stab).sum()), int((alive & ok_iou & ok_stab).sum()) - len(nms), len(kept)
