"""Geometries, weights, images and model files of the encoder-chain tests (tests/test_gpu_encoder.py on the GPU,
tests/test_encoder_ref.py on the CPU).  No test functions here."""
from pathlib import Path
from typing import Dict

import numpy as np

# The smallest geometries that take the product path (sam_model.cpp: the f16-pair stream needs D % 256 == 0):
#   d512   two statistics groups, head dimension 64, a windowed block behind a global one
#   d1280  five groups, head dimension 80 (1280 is the smallest width that is a multiple of both 80 and 256)
GEOMETRIES = {"d512": (512, 3, 8, (1,)), "d1280": (1280, 2, 16, (1,))}
# trained-like weights (dlimgedit_amd.weights.trained_like_weights): four massive channels, rows with |mean| >> sigma
FAMILIES = [("d512", "synthetic"), ("d512", "trained"), ("d1280", "synthetic")]
SEEDS = {"synthetic": 7, "trained": 3}
IMAGES = ("sinusoids", "hard_edges", "short")      # "short": 1024 x 683, grid rows 43 .. 63 are zero patches
FAMILY_IMAGES = {family: IMAGES for family in FAMILIES}      # every image through every stage of every family
YARDSTICK_ROWS = 512


def config(geometry: str, depth: int = 0):
    """The geometry cut to its first `depth` blocks (0: all of them); a prefix keeps the global blocks it still holds."""
    from dlimgedit_amd.sam_config import SamConfig
    D, full, heads, global_blocks = GEOMETRIES[geometry]
    depth = depth or full
    return SamConfig(f"enc_{geometry}_{depth}", D, depth, heads, tuple(g for g in global_blocks if g < depth))


def parameters(geometry: str, kind: str, depth: int = 0) -> Dict[str, np.ndarray]:
    from dlimgedit_amd import weights as W
    cfg = config(geometry, depth)
    return W.synthetic_weights(cfg, SEEDS[kind]) if kind == "synthetic" else W.trained_like_weights(cfg, SEEDS[kind])


def hard_edged_image(seed: int, width: int = 1024, height: int = 1024) -> np.ndarray:
    """A second family of synthetic inputs (every other test uses low-frequency sinusoids + noise): flat-coloured rectangles
    and discs with hard edges on a gradient, saturated regions (0 and 255), a one-pixel checkerboard patch -- step
    edges, clipping and the highest spatial frequency a patch embedding can see."""
    rng = np.random.default_rng(5000 + seed)
    yy, xx = np.mgrid[0:height, 0:width]
    img = np.zeros((height, width, 4), np.uint8)
    for c in range(3):
        img[:, :, c] = (xx * (c + 1) * 255 // (3 * max(1, width - 1)) + yy * 40 // max(1, height - 1)).astype(np.uint8)
    for _ in range(14):
        x0, y0 = rng.integers(0, width - 40), rng.integers(0, height - 40)
        w, h = rng.integers(30, 400), rng.integers(30, 400)
        img[y0:y0 + h, x0:x0 + w, :3] = rng.integers(0, 256, 3)
    for _ in range(8):
        cx, cy, r = rng.integers(0, width), rng.integers(0, height), rng.integers(20, 180)
        img[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r, :3] = rng.integers(0, 256, 3)
    img[100:260, 700:900, :3] = 255
    img[800:960, 80:300, :3] = 0
    img[400:528, 400:528, :3] = (((xx[400:528, 400:528] + yy[400:528, 400:528]) & 1) * 255)[:, :, None]
    img[:, :, 3] = 255
    return img


def image(name: str) -> np.ndarray:
    from conftest import synthetic_image
    if name == "sinusoids":
        return synthetic_image(0)
    if name == "hard_edges":
        return hard_edged_image(0)
    assert name == "short", name
    return synthetic_image(3, 1024, 683)


def twin(params: Dict[str, np.ndarray], depth: int, bare: bool = False) -> Dict[str, np.ndarray]:
    """The depth-`depth` prefix with its last block's fc2 zeroed: its final stream is the value behind the attention half
    (x_mid), since hi + lo is exact in fp32 and splits into the same pair again.  bare: proj zeroed too, which leaves the
    block's INPUT stream (depth 1: stream 0, the patch embedding's result)."""
    p = dict(params)
    last = f"enc.L{depth - 1}"
    for lin in ("fc2", "proj") if bare else ("fc2",):
        p[f"{last}.{lin}.w"] = np.zeros_like(params[f"{last}.{lin}.w"])
        p[f"{last}.{lin}.b"] = np.zeros_like(params[f"{last}.{lin}.b"])
    return p


def write_model(directory, geometry: str, depth: int, params: Dict[str, np.ndarray]) -> str:
    """<directory>/segmentation/sam_<name>.dlw with the first `depth` blocks of `params`."""
    from dlimgedit_amd import weights as W
    cfg = config(geometry, depth)
    W.save_weights(Path(directory) / "segmentation" / W.weight_file_name(cfg), cfg, params)
    return str(directory)
