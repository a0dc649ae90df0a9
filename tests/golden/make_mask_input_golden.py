"""Generates tests/golden/sam_vit_test_mask_input.npz: prompts with a mask input through Hugging Face SamModel.

Runs ONLY where Hugging Face `transformers` is importable, like make_golden.py, whose helpers it uses.  The reduced test
variant's synthetic weights, WITH the mask branch, go into HF SamModel through dlimgedit_amd.weights.to_hf_state_dict
(prompt_encoder.mask_embed.*); the "square" image of tests/mask_input_cases.py is encoded by HF's vision encoder, and every
case on that image is decoded stage by stage the way SAM's interactive predictor does: the clicks of the stage (and the
box) as input_points / input_labels / input_boxes, and from the second stage on input_masks = the low-res logits plane the
stage before delivered (select_single's rule on HF's own IoU predictions).

    python tests/golden/make_mask_input_golden.py

Stored per case: strided samples of all four low-res logit planes and all four IoU predictions of the LAST stage, the plane
it delivers, and the packed bits of every second row of its final mask (torch F.interpolate post-processing); once,
strided samples of the embedding.
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))

import mask_input_cases as C  # noqa: E402
from dlimgedit_amd import weights as W  # noqa: E402
from dlimgedit_amd.sam_config import get_config  # noqa: E402
from make_golden import EMB_STRIDE, LOW_STRIDE, OUT, hf_model, torch_post  # noqa: E402
from oracle import sam_oracle as O  # noqa: E402

VARIANT, SEED, IMAGE = "vit_test", 7, "square"
MASK_ROW_STRIDE = 2      # every second row of the final mask: the fixture stays below the box + point one


def hf_stage(model, emb, clicks, labels, box, mask):
    """One stage -> (low [4, 256, 256], iou [4]), token 0 first.  HF pads a point prompt without a box itself."""
    kw = dict(image_embeddings=emb,
              input_points=torch.tensor([[[[float(x), float(y)] for x, y in clicks]]]),              # [1, 1, n, 2]
              input_labels=torch.tensor([[[int(v) for v in labels]]], dtype=torch.int64))            # [1, 1, n]
    if box is not None:
        kw["input_boxes"] = torch.tensor([[[float(v) for v in box]]])                                # [1, 1, 4]
    if mask is not None:
        kw["input_masks"] = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32))[None, None]     # [1, 1, 256, 256]
    with torch.no_grad():
        o3 = model(multimask_output=True, **kw)
        o1 = model(multimask_output=False, **kw)
    low = torch.cat([o1.pred_masks[0, 0], o3.pred_masks[0, 0]], 0).numpy()
    iou = torch.cat([o1.iou_scores[0, 0], o3.iou_scores[0, 0]], 0).numpy()
    return low, iou


def main():
    torch.manual_seed(0)
    cfg = get_config(VARIANT)
    params = W.synthetic_weights(cfg, SEED, mask_branch=True)
    model = hf_model(cfg, params)
    assert any(k.startswith("prompt_encoder.mask_embed.") for k in W.to_hf_state_dict(cfg, params))
    img = C.image(IMAGE)
    h, w = img.shape[:2]
    assert (w, h) == (1024, 1024)            # no resize: prompt coordinates are image coordinates
    x = O.preprocess(O.create_image_tensor(img, O.CH_RGBA))
    with torch.no_grad():
        emb = model.get_image_embeddings(torch.from_numpy(x)[None])
    emb_tok = emb[0].reshape(256, -1).T.contiguous().numpy()
    index = [i for i, c in enumerate(C.CASES) if c[0] == IMAGE]
    lows, ious, planes, bits = [], [], [], []
    for i in index:
        _, clicks, labels, box, _ = C.CASES[i]
        mask = low = plane = None
        for k in C.stage_clicks(C.CASES[i]):
            low, iou = hf_stage(model, emb, clicks[:k], labels[:k], box, mask)
            plane = O.select_single(iou.astype(np.float32), k + (2 if box is not None else 1))
            mask = low[plane]
        lows.append(low.reshape(4, -1)[:, ::LOW_STRIDE].copy())
        ious.append(iou)
        planes.append(plane)
        bits.append(np.packbits((torch_post(low[plane], h, w) > 0)[::MASK_ROW_STRIDE]))
    out = {"seed": SEED, "cases": np.array(index, np.int32), "emb_samples": emb_tok.reshape(-1)[::EMB_STRIDE].copy(),
           "low_samples": np.stack(lows), "iou": np.stack(ious), "plane": np.array(planes, np.int32), "mask_bits": np.stack(bits)}
    path = OUT / f"sam_{VARIANT}_mask_input.npz"
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
