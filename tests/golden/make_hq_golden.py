"""Generates tests/golden/sam_vit_hqtest.npz: SAM-HQ prompts through Hugging Face SamHQModel.

Runs ONLY where Hugging Face `transformers` (with models/sam_hq) is importable, like make_golden.py, whose helpers it uses.
The reduced geometry of tests/hq_cases.py with seeded synthetic weights, WITH the mask branch and the SAM-HQ group, goes into
HF SamHQModel through dlimgedit_amd.weights.to_hf_state_dict; the "square" image of hq_cases is encoded by HF's vision encoder
(which also returns intermediate_embeddings[0], the output of the first global-attention block), and every case on that image
is decoded stage by stage as make_mask_input_golden.py does.  HF runs in float64, so what the fixture pins is the published
model and not HF's fp32 rounding.

    python tests/golden/make_hq_golden.py

The SamHQMaskDecoder of the transformers release this was generated with drops the image half of the two-way transformer's
result: its forward binds the transformer's second return value to a name it overwrites, and up-scales the embedding it was
GIVEN (transposed in space by a transpose(2, 3) meant for the flattened keys) instead of the keys the transformer returns, as
sam-hq's MaskDecoderHQ.predict_masks and HF's own SamMaskDecoder do.  The fixture pins the published model: `use_transformer_keys`
wraps two sub-modules of the loaded HF model so that upscale_conv1 receives the transformer's keys; every module, weight and
every other line of HF's forward (prompt encoder, transformer, HQ features, 3x3 path, MLPs, the sum, the sorting) runs as it is.

HF delivers masks_sam + masks_hq and sorts the three multimask planes by their IoU predictions; the generator undoes the
sorting (the planes are stored in token order 0..3, as the library delivers them).

Stored once: strided samples of the embedding, of intermediate_embeddings[0] and of hq_features.  Per case: strided samples of
the four delivered planes, the four IoU predictions, the plane of the single-mask mode and the packed bits of every second row
of the final mask (torch F.interpolate post-processing) of the LAST stage.
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))

import hq_cases as H  # noqa: E402
from dlimgedit_amd import weights as W  # noqa: E402
from make_golden import EMB_STRIDE, LOW_STRIDE, OUT, torch_post  # noqa: E402
from oracle import sam_oracle as O  # noqa: E402

IMAGE = "square"
MASK_ROW_STRIDE = 2
EARLY_STRIDE = 131       # every 131st value of the [4096][128] early feature
FEAT_STRIDE = 509        # every 509th value of the [256][256][32] HQ features


def hf_hq_model(cfg, params):
    from transformers import SamHQConfig, SamHQMaskDecoderConfig, SamHQModel, SamHQVisionConfig
    vc = SamHQVisionConfig(hidden_size=cfg.embed_dim, num_hidden_layers=cfg.depth, num_attention_heads=cfg.num_heads,
                           global_attn_indexes=list(cfg.global_attn_indexes), mlp_dim=cfg.mlp_dim)
    dc = SamHQMaskDecoderConfig(layer_norm_eps=O.DEC_LN_EPS, vit_dim=cfg.embed_dim)
    model = SamHQModel(SamHQConfig(vision_config=vc, mask_decoder_config=dc)).eval()
    sd = {k: torch.from_numpy(np.array(v)) for k, v in W.to_hf_state_dict(cfg, params).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return use_transformer_keys(model.double())


class _KeepKeys(torch.nn.Module):
    """The two-way transformer, remembering the keys it returns."""
    def __init__(self, inner):
        super().__init__()
        self.inner, self.keys = inner, None

    def forward(self, **kw):
        queries, keys = self.inner(**kw)
        self.keys = keys                                   # [batch, prompts, 4096, 256]
        return queries, keys


class _UpscaleKeys(torch.nn.Module):
    """upscale_conv1 on the transformer's keys, whatever it is handed."""
    def __init__(self, inner, transformer):
        super().__init__()
        self.inner, self.transformer = inner, transformer

    def forward(self, given):
        k = self.transformer.keys
        b, p, n, c = k.shape
        g = int(round(n ** 0.5))
        assert given.shape == (b * p, c, g, g)
        return self.inner(k.reshape(b * p, g, g, c).permute(0, 3, 1, 2).contiguous())


def use_transformer_keys(model):
    d = model.mask_decoder
    d.transformer = _KeepKeys(d.transformer)
    d.upscale_conv1 = _UpscaleKeys(d.upscale_conv1, d.transformer)
    return model


def hf_stage(model, emb, inter, clicks, labels, box, mask):
    """One stage -> (delivered low [4, 256, 256], iou [4]) in token order."""
    kw = dict(image_embeddings=emb, intermediate_embeddings=inter)
    if len(clicks):
        kw["input_points"] = torch.tensor([[[[float(x), float(y)] for x, y in clicks]]], dtype=torch.float64)
        kw["input_labels"] = torch.tensor([[[int(v) for v in labels]]], dtype=torch.int64)
    if box is not None:
        kw["input_boxes"] = torch.tensor([[[float(v) for v in box]]], dtype=torch.float64)
    if mask is not None:
        kw["input_masks"] = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float64))[None, None]
    # the decoder alone, through its own forward: multimask_output sorts the three planes, which is undone by evaluating the
    # unsorted IoU predictions the same way
    with torch.no_grad():
        o1 = model(multimask_output=False, **kw)
        o3 = model(multimask_output=True, **kw)
    iou3 = o3.iou_scores[0, 0].numpy()                    # sorted, descending
    low3 = o3.pred_masks[0, 0].numpy()
    return o1.pred_masks[0, 0].numpy(), o1.iou_scores[0, 0].numpy(), low3, iou3


def unsort(model, kw_iou, low3, iou3):
    """HF sorted planes 1..3 by descending IoU prediction (a stable sort); kw_iou: the same three predictions in token order."""
    order = torch.sort(torch.from_numpy(np.asarray(kw_iou)), descending=True, stable=True).indices.numpy()
    low = np.empty_like(low3)
    iou = np.empty_like(iou3)
    for rank, tok in enumerate(order):
        low[tok], iou[tok] = low3[rank], iou3[rank]
    return low, iou


def token_order_iou(model, emb, inter, clicks, labels, box, mask):
    """The four IoU predictions in token order, from the mask decoder called directly (no sorting on this path)."""
    pts = torch.tensor([[[[float(x), float(y)] for x, y in clicks]]], dtype=torch.float64) if len(clicks) else None
    labs = torch.tensor([[[int(v) for v in labels]]], dtype=torch.int64) if len(clicks) else None
    boxes = torch.tensor([[[float(v) for v in box]]], dtype=torch.float64) if box is not None else None
    masks = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float64))[None, None] if mask is not None else None
    with torch.no_grad():
        sparse, dense = model.prompt_encoder(input_points=pts, input_labels=labs, input_boxes=boxes, input_masks=masks)
        tok = model.mask_decoder.iou_prediction_head
        # run the transformer as the decoder does and read the IoU head on token 0
        d = model.mask_decoder
        output_tokens = torch.cat([d.iou_token.weight, d.mask_tokens.weight, d.hq_token.weight], dim=0)[None, None]
        tokens = torch.cat([output_tokens, sparse], dim=2) if sparse is not None else output_tokens
        pos = model.get_image_wide_positional_embeddings()
        point_embedding, _ = d.transformer(point_embeddings=tokens, image_embeddings=emb + dense,
                                           image_positional_embeddings=pos, attention_similarity=None, target_embedding=None)
        return tok(point_embedding[:, :, 0, :])[0, 0].numpy()


def main():
    torch.manual_seed(0)
    cfg = H.CFG
    params = W.synthetic_weights(cfg, H.SEED, mask_branch=True, hq=True)
    model = hf_hq_model(cfg, params)
    img = H.image(IMAGE)
    h, w = img.shape[:2]
    assert (w, h) == (1024, 1024)            # no resize: prompt coordinates are image coordinates
    x = O.preprocess(O.create_image_tensor(img, O.CH_RGBA))
    with torch.no_grad():
        emb, inter = model.get_image_embeddings(torch.from_numpy(x)[None].double())
    emb_tok = emb[0].reshape(256, -1).T.contiguous().numpy()
    early = inter[0][0].reshape(-1, cfg.embed_dim).numpy()
    with torch.no_grad():
        d = model.mask_decoder
        feat = d.encoder_conv2(d.activation(d.encoder_norm(d.encoder_conv1(emb))))
        v = inter[0].permute(0, 3, 1, 2).contiguous()
        feat = feat + d.compress_vit_conv2(d.activation(d.compress_vit_norm(d.compress_vit_conv1(v))))
    feat = feat[0].permute(1, 2, 0).contiguous().numpy()          # [256][256][32]
    index = [i for i, c in enumerate(H.CASES) if c[0] == IMAGE]
    lows, ious, planes, bits = [], [], [], []
    for i in index:
        _, clicks, labels, box, _ = H.CASES[i]
        mask = low = iou = plane = None
        for k in H.stage_clicks(H.CASES[i]):
            low1, iou1, low3, iou3 = hf_stage(model, emb, inter, clicks[:k], labels[:k], box, mask)
            iou4 = token_order_iou(model, emb, inter, clicks[:k], labels[:k], box, mask)
            assert abs(iou4[0] - iou1[0]) < 1e-9 and np.allclose(np.sort(iou4[1:])[::-1], iou3, atol=1e-9)
            l3, i3 = unsort(model, iou4[1:], low3, iou3)
            low, iou = np.concatenate([low1, l3], 0), np.concatenate([iou1, i3], 0)
            plane = O.select_single(iou.astype(np.float32), k + (2 if box is not None else 1))
            mask = low[plane]
        lows.append(low.reshape(4, -1)[:, ::LOW_STRIDE].astype(np.float32))
        ious.append(iou.astype(np.float32))
        planes.append(plane)
        bits.append(np.packbits((torch_post(low[plane].astype(np.float32), h, w) > 0)[::MASK_ROW_STRIDE]))
    out = {"seed": H.SEED, "cases": np.array(index, np.int32),
           "emb_samples": emb_tok.reshape(-1)[::EMB_STRIDE].astype(np.float32),
           "early_samples": early.reshape(-1)[::EARLY_STRIDE].astype(np.float32),
           "feat_samples": feat.reshape(-1)[::FEAT_STRIDE].astype(np.float32),
           "low_samples": np.stack(lows), "iou": np.stack(ious), "plane": np.array(planes, np.int32), "mask_bits": np.stack(bits)}
    path = OUT / "sam_vit_hqtest.npz"
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
