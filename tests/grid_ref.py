"""Numpy restatement of what a grid prompt ("segment everything") delivers, from given planes, IoU predictions and extents:
scoring on the low-res plane, filter, NMS, ranking, and painting through the oracle's own post-processing of every kept plane
(oracle.sam_oracle.postprocess_logits).  The definition the library is held to (csrc/grid_plan.hpp, kernels/mask_grid.hip).

Candidates: planes 1..3 of every prompt, c = 3 * prompt + (plane - 1).
"""
import numpy as np

from oracle import sam_oracle as O

LOW = 256
MAX_KEPT = 255
DEFAULT_IOU, DEFAULT_STABILITY = 880, 950
CULL_EMPTY = 0x0000FFFF
f32 = np.float32


def pre_extent(width, height):
    """(pre_w, pre_h): the extent an image of width x height is encoded at."""
    return O.ResizeLongestSide().target_extent(width, height)


def grid_pixels(width, height, side):
    """[(x, y)] of the side * side prompts, row-major, j (rows) outer."""
    return [((2 * i + 1) * width // (2 * side), (2 * j + 1) * height // (2 * side)) for j in range(side) for i in range(side)]


def candidates_of(planes4):
    """[P, 4, 256, 256] -> [3 P, 256, 256]: planes 1..3 of every prompt."""
    planes4 = np.asarray(planes4, f32)
    return planes4[:, 1:4].reshape(-1, LOW, LOW)


def _box(pos):
    ys, xs = np.nonzero(pos)
    if len(ys) == 0:
        return None
    return int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())


def harvest(planes, pre_w, pre_h):
    """planes [C, 256, 256] -> records int64 [C, 8]: n_hi, n_mid, n_lo, x0, y0, x1, y1 over the scored region (x < ceil(pre_w / 4),
    y < ceil(pre_h / 4); an empty box is 0, 0, -1, -1) and the cull word: the box of the logits > 0 over one low-res row and
    column more, x0 | y0 << 8 | x1 << 16 | y1 << 24 (CULL_EMPTY when there is none).  All comparisons strict."""
    sw, sh = -(-pre_w // 4), -(-pre_h // 4)
    rw, rh = min(sw + 1, LOW), min(sh + 1, LOW)
    out = np.zeros((len(planes), 8), np.int64)
    for c, plane in enumerate(planes):
        s = np.asarray(plane, f32)[:sh, :sw]
        box = _box(s > f32(0))
        reach = _box(np.asarray(plane, f32)[:rh, :rw] > f32(0))
        out[c, :3] = (s > f32(1)).sum(), (s > f32(0)).sum(), (s > f32(-1)).sum()
        out[c, 3:7] = box if box else (0, 0, -1, -1)
        out[c, 7] = CULL_EMPTY if reach is None else reach[0] | reach[1] << 8 | reach[2] << 16 | reach[3] << 24
    return out


def passes(records, iou, iou_permille=0, stability_permille=0):
    """(passes the IoU threshold, passes the stability threshold, is non-empty) per candidate, as boolean arrays."""
    records = np.asarray(records, np.int64)
    threshold = f32(iou_permille or DEFAULT_IOU) / f32(1000)
    stability = int(stability_permille or DEFAULT_STABILITY)
    ok_iou = np.asarray(iou, f32) >= threshold
    ok_stab = np.array([int(r[0]) * 1000 >= stability * int(r[2]) for r in records], bool)
    alive = (records[:, 1] > 0) & (records[:, 2] > 0)
    return ok_iou, ok_stab, alive


def select(records, iou, iou_permille=0, stability_permille=0):
    """-> (nms, kept): the candidates NMS keeps in NMS order, and the same in label order (kept[k - 1] has label k)."""
    records = np.asarray(records, np.int64)
    iou = np.asarray(iou, f32)
    ok_iou, ok_stab, alive = passes(records, iou, iou_permille, stability_permille)
    passing = [c for c in range(len(records)) if alive[c] and ok_iou[c] and ok_stab[c]]
    passing.sort(key=lambda c: (-float(iou[c]), c))
    nms = []
    for c in passing:
        if len(nms) == MAX_KEPT:
            break
        x0, y0, x1, y1 = (int(v) for v in records[c, 3:7])
        area = (x1 - x0) * (y1 - y0)
        suppressed = False
        for q in nms:
            qx0, qy0, qx1, qy1 = (int(v) for v in records[q, 3:7])
            inter = max(0, min(x1, qx1) - max(x0, qx0)) * max(0, min(y1, qy1) - max(y0, qy0))
            union = area + (qx1 - qx0) * (qy1 - qy0) - inter
            if union != 0 and inter * 10 > 7 * union:
                suppressed = True
                break
        if not suppressed:
            nms.append(c)
    order = sorted(range(len(nms)), key=lambda n: (-int(records[nms[n], 1]), n))
    return nms, [nms[n] for n in order]


def mask_of(plane, width, height):
    """what the post-processing delivers for one plane: 255 where the two-stage bilinear sample is > 0"""
    return np.where(O.postprocess_logits(np.asarray(plane, f32), (height, width)) > 0, 255, 0).astype(np.uint8)


def paint(planes, kept, width, height):
    """label map [height, width] u8: the largest k whose mask is 255, 0 where none is"""
    out = np.zeros((height, width), np.uint8)
    for k, c in enumerate(kept, start=1):
        out[mask_of(planes[c], width, height) == 255] = k
    return out


def label_map(planes4, iou4, width, height, iou_permille=0, stability_permille=0):
    """planes4 [P, 4, 256, 256], iou4 [P, 4] as the decoder leaves them for the grid's prompts -> (map, records, nms, kept)"""
    planes = candidates_of(planes4)
    iou = np.asarray(iou4, f32)[:, 1:4].reshape(-1)
    pre_w, pre_h = pre_extent(width, height)
    records = harvest(planes, pre_w, pre_h)
    nms, kept = select(records, iou, iou_permille, stability_permille)
    return paint(planes, kept, width, height), records, nms, kept
