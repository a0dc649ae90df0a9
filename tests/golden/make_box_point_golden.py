"""Generates tests/golden/sam_vit_test_box_point.npz: box + point prompts through Hugging Face SamModel.

Runs ONLY where Hugging Face `transformers` is importable, like make_golden.py, whose helpers it uses.  The reduced test
variant's synthetic weights go into HF SamModel through dlimgedit_amd.weights.to_hf_state_dict; the "square" image of
tests/box_point_cases.py is encoded by HF's vision encoder, and its three box / point pairs are decoded in one call with
input_points AND input_boxes -- HF's prompt encoder then puts the point embedding in front of the two corner embeddings
and adds no padding point, which is the order and the labels (1, 2, 3) the fixture pins.

    python tests/golden/make_box_point_golden.py

Stored: the pairs, strided samples of the embedding and of all four low-res logit planes per pair, all four IoU
predictions per pair, and the packed bits of plane 0's final mask (torch F.interpolate post-processing).
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))

import box_point_cases as B  # noqa: E402
from dlimgedit_amd import weights as W  # noqa: E402
from dlimgedit_amd.sam_config import get_config  # noqa: E402
from make_golden import EMB_STRIDE, LOW_STRIDE, OUT, hf_model, torch_post  # noqa: E402
from oracle import sam_oracle as O  # noqa: E402

VARIANT, SEED, IMAGE = "vit_test", 7, "square"


def main():
    torch.manual_seed(0)
    cfg = get_config(VARIANT)
    model = hf_model(cfg, W.synthetic_weights(cfg, SEED))
    img = B.image(IMAGE)
    h, w = img.shape[:2]
    assert (w, h) == (1024, 1024)            # no resize: prompt coordinates are image coordinates
    x = O.preprocess(O.create_image_tensor(img, O.CH_RGBA))
    pairs = [(box, pt) for name, box, pt in B.PAIRS if name == IMAGE]
    boxes = torch.tensor([[[float(v) for v in box] for box, _ in pairs]])            # [1, n, 4]
    points = torch.tensor([[[[float(pt[0]), float(pt[1])]] for _, pt in pairs]])     # [1, n, 1, 2]
    labels = torch.ones((1, len(pairs), 1), dtype=torch.int64)
    with torch.no_grad():
        emb = model.get_image_embeddings(torch.from_numpy(x)[None])
        kw = dict(image_embeddings=emb, input_points=points, input_labels=labels, input_boxes=boxes)
        o3 = model(multimask_output=True, **kw)
        o1 = model(multimask_output=False, **kw)
    low = torch.cat([o1.pred_masks[0], o3.pred_masks[0]], 1).numpy()          # [n, 4, 256, 256], token 0 first
    iou = torch.cat([o1.iou_scores[0], o3.iou_scores[0]], 1).numpy()          # [n, 4]
    emb_tok = emb[0].reshape(256, -1).T.contiguous().numpy()
    out = {"seed": SEED, "boxes": np.array([b for b, _ in pairs], np.int32), "points": np.array([p for _, p in pairs], np.int32),
           "emb_samples": emb_tok.reshape(-1)[::EMB_STRIDE].copy(),
           "low_samples": low.reshape(len(pairs), 4, -1)[:, :, ::LOW_STRIDE].copy(), "iou": iou,
           "mask0_bits": np.stack([np.packbits(torch_post(low[i, 0], h, w) > 0) for i in range(len(pairs))])}
    path = OUT / f"sam_{VARIANT}_box_point.npz"
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
