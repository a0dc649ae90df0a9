"""Numpy restatement of k::mask_prior (csrc/kernels/kernels.hpp, K19): a caller's full-resolution u8 mask as the 256 x 256 fp32
plane the prompt encoder's mask branch takes.  Integers up to the one division (a summed-area table in int64), then the same
fp32 operations in the same order: two exact conversions, one correctly rounded division, one multiply.

    sw = ceil(pre_w / 4), sh = ceil(pre_h / 4)
    x < sw:  c0 = floor(4 x W / pre_w),  c1 = ceil(min(4 x + 4, pre_w) W / pre_w)
    y < sh:  r0 = floor(4 y H / pre_h),  r1 = ceil(min(4 y + 4, pre_h) H / pre_h)
    sum = sum of mask[r0:r1, c0:c1],  area = (r1 - r0) (c1 - c0),  s = float32(strength_milli) / float32(1000)
    plane[y, x] = (float32(2 sum - 255 area) / float32(255 area)) * s      inside the scored region
    plane[y, x] = -1 * s                                                   elsewhere: padding is background
"""
import numpy as np

LOW = 256
DEFAULT_STRENGTH = 8000      # strength_milli == 0 of a prior mark (csrc/prior_plan.hpp: kPriorDefaultStrength)
MAX_STRENGTH = 100000


def footprints(size: int, pre: int):
    """-> (lo, hi) int64 arrays over the ceil(pre / 4) low-res indices of one axis: source indices lo[i] .. hi[i] - 1."""
    i = np.arange((pre + 3) // 4, dtype=np.int64)
    lo = 4 * i * size // pre
    hi = (np.minimum(4 * i + 4, pre) * size + pre - 1) // pre
    return lo, hi


def pre_extent(width: int, height: int):
    """The extent an image of width x height is encoded at (the library's ResizeLongestSide)."""
    from oracle import sam_oracle as O
    return O.ResizeLongestSide().target_extent(width, height)


def coverage_quotient(mask: np.ndarray, pre_w: int, pre_h: int) -> np.ndarray:
    """The scored region in front of the multiply: float32(2 sum - 255 area) / float32(255 area), [sh, sw] float32."""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim == 2
    H, W = mask.shape
    c0, c1 = footprints(W, pre_w)
    r0, r1 = footprints(H, pre_h)
    assert (c0 < c1).all() and c1.max() <= W and (r0 < r1).all() and r1.max() <= H
    sat = np.zeros((H + 1, W + 1), np.int64)
    sat[1:, 1:] = mask.astype(np.int64).cumsum(0).cumsum(1)
    total = sat[r1][:, c1] - sat[r0][:, c1] - sat[r1][:, c0] + sat[r0][:, c0]
    area = (r1 - r0)[:, None] * (c1 - c0)[None, :]
    num, den = 2 * total - 255 * area, 255 * area
    assert np.abs(num).max() < 2 ** 24 and den.max() < 2 ** 24          # the conversions below are exact
    return num.astype(np.float32) / den.astype(np.float32)


def plane_from_quotient(quotient: np.ndarray, strength_milli: int) -> np.ndarray:
    assert quotient.dtype == np.float32 and 1 <= strength_milli <= MAX_STRENGTH
    s = np.float32(strength_milli) / np.float32(1000)
    plane = np.full((LOW, LOW), np.float32(-1) * s, np.float32)
    plane[:quotient.shape[0], :quotient.shape[1]] = quotient * s
    return plane


def prior_plane(mask: np.ndarray, pre_w: int, pre_h: int, strength_milli: int) -> np.ndarray:
    return plane_from_quotient(coverage_quotient(mask, pre_w, pre_h), strength_milli)
