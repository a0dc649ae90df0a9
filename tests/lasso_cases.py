"""Inputs shared by the lasso-mark tests (tests/test_lasso_ref.py, tests/test_gpu_lasso_kernel.py, tests/test_gpu_lasso.py).

Kernel cases: extents and selections for the derivation alone -- every record must EQUAL tests/lasso_ref.py.
End-to-end cases: the images and ellipse priors of tests/prior_cases.py as selections; the yardstick is the library's own
explicit path: the mask delivered for a lasso prompt is byte-equal to the mask delivered for the prompt built from
lasso_ref's box and click (with a prior mark on the same buffer when the mark's mask bit is set)."""
import numpy as np

import lasso_ref
import prior_cases as PC
import prior_ref

# (width, height): the identity; up-scaling, footprints share source columns, sh = 171 with a 3-row last footprint; down-scaling;
# sw = 10; a region smaller than one wave's row of source pixels
EXTENTS = [(1024, 1024), (600, 400), (1800, 1200), (37, 1024), (5, 3)]
EXTENT_IDS = [f"{w}x{h}" for w, h in EXTENTS]

WHATS = [1, 2, 3, 5, 6, 7]          # every valid `what` (0 is 7; 4 is refused)


def from_cells(cells: np.ndarray, w: int, h: int, pre_w: int, pre_h: int) -> np.ndarray:
    """A mask (h, w) uint8 whose pixels are 255 in the footprint of every low-res cell set in `cells` [sh, sw] (where
    neighbouring footprints share source pixels, a set cell also covers a part of its neighbours)."""
    c0, c1 = prior_ref.footprints(w, pre_w)
    r0, r1 = prior_ref.footprints(h, pre_h)
    m = np.zeros((h, w), np.uint8)
    for y, x in zip(*np.nonzero(cells)):
        m[r0[y]:r1[y], c0[x]:c1[x]] = 255
    return m


def soft_ellipse(w: int, h: int, edge: float) -> np.ndarray:
    """prior_cases.draw_prior's soft ellipse for an image of any extent: a linear ramp of `edge` pixels across the outline."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rx, ry = 0.3 * w, 0.27 * h
    d = np.sqrt(((xx - 0.45 * w) / rx) ** 2 + ((yy - 0.55 * h) / ry) ** 2)
    return np.clip(np.rint(255.0 * (0.5 + (1.0 - d) * min(rx, ry) / max(edge, 1e-9))), 0, 255).astype(np.uint8)


def kernel_masks(w: int, h: int) -> dict:
    """name -> selection (h, w) uint8 for an image of w x h, what the issue lists."""
    pre_w, pre_h = prior_ref.pre_extent(w, h)
    sw, sh = (pre_w + 3) // 4, (pre_h + 3) // 4
    yy, xx = np.mgrid[0:sh, 0:sw]
    cells = lambda c: from_cells(c, w, h, pre_w, pre_h)      # noqa: E731
    r = max(1, min(sw, sh) // 6)
    out = {
        "full": np.full((h, w), 255, np.uint8),                                           # the distance is to the region's edge only
        "one_cell": cells((xx == sw // 2) & (yy == sh // 2)),
        "last_row_and_column": cells((xx >= max(0, sw - 3)) & (yy >= max(0, sh - 2))),
        "ring": cells(((xx - sw // 2) ** 2 + (yy - sh // 2) ** 2 <= (2 * r) ** 2) & ((xx - sw // 2) ** 2 + (yy - sh // 2) ** 2 > r * r)),
        # two discs of one radius: the upper one is the right one, so the smallest y decides, not the smallest x
        "two_discs": cells(((xx - (3 * sw) // 4) ** 2 + (yy - sh // 3) ** 2 <= r * r) | ((xx - sw // 4) ** 2 + (yy - (2 * sh) // 3) ** 2 <= r * r)),
        "l_shape": cells(((xx >= sw // 8) & (xx < sw // 8 + max(2, sw // 5)) & (yy >= sh // 8) & (yy < (7 * sh) // 8)) |
                         ((xx >= sw // 8) & (xx < (7 * sw) // 8) & (yy >= (7 * sh) // 8 - max(2, sh // 5)) & (yy < (7 * sh) // 8))),
        "checkerboard": cells(((xx + yy) & 1) == 1),
        "uniform_127": np.full((h, w), 127, np.uint8),                                    # 2 * 127 < 255: empty
        "uniform_128": np.full((h, w), 128, np.uint8),                                    # 2 * 128 > 255: full
        "soft_ellipse": PC.draw_prior("square", PC.CASES[1][4]) if (w, h) == (1024, 1024) else soft_ellipse(w, h, 0.05 * min(w, h)),
        "zeros": np.zeros((h, w), np.uint8),
    }
    rng = np.random.default_rng(1000 * w + h)
    blobs = np.zeros((sh, sw), bool)
    for _ in range(12):
        cx, cy, rr = rng.integers(0, sw), rng.integers(0, sh), rng.integers(1, max(2, min(sw, sh) // 5))
        blobs |= (xx - cx) ** 2 + (yy - cy) ** 2 <= rr * rr
    out["random_blobs"] = cells(blobs)
    return out


# ---- end to end -----------------------------------------------------------------------------------------------------------------
IMAGES = PC.IMAGES
image = PC.image
# image name -> the ellipse that is its selection (those of prior_cases (a) and (d))
SELECTIONS = {"square": PC.CASES[0][4], "wide": PC.CASES[3][4]}
# further clicks behind the derived one: (x, y), label
EXTRA_CLICKS = {"square": (((523, 454), 1), ((816, 511), 0)), "wide": (((438, 42), 1), ((603, 568), 0))}


def selection(name: str) -> np.ndarray:
    return PC.draw_prior(name, SELECTIONS[name])


def record_of(name: str, sel: np.ndarray) -> np.ndarray:
    _, w, h = IMAGES[name]
    return lasso_ref.derive(sel, *prior_ref.pre_extent(w, h))


def token_rows(what: int, extra_clicks: int = 0, hq: bool = False) -> int:
    what = what or 7
    clicks = extra_clicks + (1 if what & lasso_ref.CLICK else 0)
    return 5 + clicks + (2 if what & lasso_ref.BOX else 1) + (1 if hq else 0)
