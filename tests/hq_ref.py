"""Float64 numpy reference of the SAM-HQ decode  --  TEST INFRASTRUCTURE ONLY.

Restates SAM-HQ's mask decoder (sam-hq: MaskDecoderHQ, Hugging Face: SamHQMaskDecoder) on top of the helpers of
oracle/decoder_ref.py, every operation in float64:

* `encoder_stream`   the image encoder's residual stream after a given block (oracle/sam_oracle.encoder_block in a loop):
                     the early feature SAM-HQ taps is the stream after the FIRST global-attention block.
* `hq_features`      compress_vit_feat(early feature) + embedding_encoder(embedding): two transposed convolutions (kernel 2,
                     stride 2) each with LayerNorm2d + GELU between them and NO activation behind the second, [256, 256, 32].
* `decode_hq`        the two-way transformer with the HQ token at ROW 5, directly behind the four mask tokens, as Hugging Face
                     and sam-hq place it (the product carries it as the LAST row: the two orders are checked against each
                     other), embedding_maskfeature (two 3x3 convolutions, zero padding 1) on the up-scaled embedding, the HQ
                     plane hyper_hq . (maskfeature + hq_features) and the delivered logits masks_sam + masks_hq: the HQ plane
                     added to each of the four SAM planes.
* `staged_mask`      a prompt with refinement marks, stage by stage: the delivered plane (with the HQ plane in it) is the next
                     stage's mask input.

`wrong=` names deliberate mistakes, one at a time, for the tests that show the fixture can tell right from wrong."""
from __future__ import annotations

import numpy as np

from oracle import decoder_ref as R
from oracle import sam_oracle as O

f64 = np.float64
GRID = R.GRID
LN2D_EPS = 1e-6
WRONG = ("no_hq_plane", "no_vit_feature", "gelu_after_emb_conv2", "hq_token_with_pe")


def first_global_block(cfg) -> int:
    return min(cfg.global_attn_indexes)


def encoder_stream(chw, params, cfg, after_block: int) -> np.ndarray:
    """Preprocessed [3, S, S] -> the residual stream [g * g, D] after block `after_block` (the oracle's own arithmetic)."""
    g = cfg.grid
    x = O.patchify(chw, cfg.patch_size) @ params["enc.patch.w"].T + params["enc.patch.b"] + params["enc.pos"]
    x = x.reshape(g, g, cfg.embed_dim).astype(np.float32)
    for i in range(after_block + 1):
        x = O.encoder_block(x, params, i, cfg)
    return np.ascontiguousarray(x.reshape(g * g, cfg.embed_dim))


def _conv_t(x, w, b):
    """ConvTranspose2d(kernel 2, stride 2): x [H, W, Ci], w [Ci, Co, 2, 2] -> [2 H, 2 W, Co]."""
    H, W_, _ = x.shape
    co = w.shape[1]
    y = x.reshape(H * W_, -1) @ w.reshape(w.shape[0], -1)
    return y.reshape(H, W_, co, 2, 2).transpose(0, 3, 1, 4, 2).reshape(2 * H, 2 * W_, co) + b


def _conv3x3(x, w, b):
    """Conv2d(kernel 3, padding 1): x [H, W, Ci], w [Co, Ci, 3, 3] -> [H, W, Co]."""
    H, W_, _ = x.shape
    xp = np.pad(x, ((1, 1), (1, 1), (0, 0)))
    y = np.zeros((H, W_, w.shape[0]), f64)
    for ky in range(3):
        for kx in range(3):
            y += xp[ky:ky + H, kx:kx + W_] @ w[:, :, ky, kx].T
    return y + b


def _branch(x, p, pre, gelu_after=False):
    y = _conv_t(x, p[pre + ".conv1.w"], p[pre + ".conv1.b"])
    y = R._gelu(R._layer_norm(y, p[pre + ".ln.w"], p[pre + ".ln.b"], LN2D_EPS))
    y = _conv_t(y, p[pre + ".conv2.w"], p[pre + ".conv2.b"])
    return R._gelu(y) if gelu_after else y


def _hq_params(params):
    return {k: np.asarray(v, f64) for k, v in params.items() if k.startswith("dec.hq.")}


def hq_features(early, emb, params, wrong=()) -> np.ndarray:
    """early [4096, D] (stream after the first global block), emb [4096, 256] -> [256, 256, 32], float64."""
    p = _hq_params(params)
    f = _branch(np.asarray(emb, f64).reshape(GRID, GRID, -1), p, "dec.hq.emb", "gelu_after_emb_conv2" in wrong)
    if "no_vit_feature" not in wrong:
        f = f + _branch(np.asarray(early, f64).reshape(GRID, GRID, -1), p, "dec.hq.vit")
    return f


def decode_hq(emb, features, coords, labels, params, wrong=(), dense=None, parts=None, hq_row_last=False):
    """Embedding [4096, 256], hq_features [256, 256, 32], packed prompt -> (delivered logits [4, 256, 256] = SAM planes + HQ
    plane, iou [4]).  dense: the dense embedding of a mask input [4096, 256] in place of pe.no_mask.  parts (dict): receives
    "sam" [4, 256, 256], "hq" [256, 256] and "hyper_hq" [32].  hq_row_last: the HQ token behind the prompt tokens instead."""
    unknown = set(wrong) - set(WRONG)
    if unknown:
        raise ValueError(f"unknown wrong forms {sorted(unknown)}")
    p = {k: np.asarray(v, f64) for k, v in params.items() if k.startswith(("pe.", "dec."))}
    sparse = R.embed_prompt(coords, labels, p)
    hq_tok = p["dec.hq.token"][None, :]
    if "hq_token_with_pe" in wrong:
        hq_tok = hq_tok + R.embed_prompt(np.zeros((1, 2)), np.array([1.0]), p)
    hq_row = 5 + len(sparse) if hq_row_last else 5                                            # Hugging Face: row 5
    rows = [p["dec.iou_token"][None, :], p["dec.mask_tokens"]] + ([sparse, hq_tok] if hq_row_last else [hq_tok, sparse])
    tokens = np.concatenate(rows, axis=0)
    keys = np.asarray(emb, f64) + (p["pe.no_mask"][None, :] if dense is None else np.asarray(dense, f64))
    pos = R.image_pe(p["pe.gauss"])

    queries, qpe = tokens, tokens
    for i in range(2):
        pre = f"dec.L{i}"
        if i == 0:
            queries = R._token_attention(queries, queries, queries, p, pre + ".self")
        else:
            qq = queries + qpe
            queries = queries + R._token_attention(qq, qq, queries, p, pre + ".self")
        queries = R._layer_norm(queries, p[pre + ".ln1.w"], p[pre + ".ln1.b"], R.DEC_LN_EPS)
        kp = keys + pos
        att = R._attend(R._lin(queries + qpe, p, pre + ".t2i.q"), R._lin(kp, p, pre + ".t2i.k"), R._lin(keys, p, pre + ".t2i.v"))
        queries = queries + R._lin(att, p, pre + ".t2i.o")
        queries = R._layer_norm(queries, p[pre + ".ln2.w"], p[pre + ".ln2.b"], R.DEC_LN_EPS)
        h = np.maximum(R._lin(queries, p, pre + ".mlp.fc1"), 0)
        queries = queries + R._lin(h, p, pre + ".mlp.fc2")
        queries = R._layer_norm(queries, p[pre + ".ln3.w"], p[pre + ".ln3.b"], R.DEC_LN_EPS)
        att = R._attend(R._lin(kp, p, pre + ".i2t.q"), R._lin(queries + qpe, p, pre + ".i2t.k"), R._lin(queries, p, pre + ".i2t.v"))
        keys = R._layer_norm(keys + R._lin(att, p, pre + ".i2t.o"), p[pre + ".ln4.w"], p[pre + ".ln4.b"], R.DEC_LN_EPS)
    att = R._attend(R._lin(queries + qpe, p, "dec.final.q"), R._lin(keys + pos, p, "dec.final.k"), R._lin(keys, p, "dec.final.v"))
    queries = queries + R._lin(att, p, "dec.final.o")
    queries = R._layer_norm(queries, p["dec.ln_final.w"], p["dec.ln_final.b"], R.DEC_LN_EPS)

    y = _conv_t(keys.reshape(GRID, GRID, -1), p["dec.up1.w"], p["dec.up1.b"])
    y = R._gelu(R._layer_norm(y, p["dec.up_ln.w"], p["dec.up_ln.b"], R.UP_LN_EPS))
    up = R._gelu(_conv_t(y, p["dec.up2.w"], p["dec.up2.b"]))                                   # [256, 256, 32]

    def mlp3(x, pre):
        x = np.maximum(R._lin(x, p, pre + ".0"), 0)
        x = np.maximum(R._lin(x, p, pre + ".1"), 0)
        return R._lin(x, p, pre + ".2")

    hyper = np.stack([mlp3(queries[1 + m], f"dec.hyper{m}") for m in range(4)], axis=0)
    sam = (hyper @ up.reshape(-1, up.shape[-1]).T).reshape(4, 4 * GRID, 4 * GRID)
    iou = mlp3(queries[0], "dec.iou")
    hyper_hq = mlp3(queries[hq_row], "dec.hq.mlp")
    m = _conv3x3(up, p["dec.hq.mask.conv1.w"], p["dec.hq.mask.conv1.b"])
    m = R._gelu(R._layer_norm(m, p["dec.hq.mask.ln.w"], p["dec.hq.mask.ln.b"], LN2D_EPS))
    m = _conv3x3(m, p["dec.hq.mask.conv2.w"], p["dec.hq.mask.conv2.b"]) + np.asarray(features, f64)
    hq = m @ hyper_hq                                                                         # [256, 256]
    if parts is not None:
        parts.update(sam=sam, hq=hq, hyper_hq=hyper_hq)
    if "no_hq_plane" in wrong:
        return sam, iou
    return sam + hq[None], iou


def decode_case_stage(emb, features, rs, clicks, labels, box, params, mask_logits=None, wrong=()):
    """One stage -> (delivered logits [4, 256, 256], iou [4], plane of the single-mask mode)."""
    import hq_cases as H
    import mask_input_cases as MI
    coords, labs = H.pack(rs, clicks, labels, box)
    dense = None if mask_logits is None else MI.dense_embedding_ref(params, mask_logits)
    low, iou = decode_hq(emb, features, coords, labs, params, wrong, dense)
    return low, iou, O.select_single(np.asarray(iou, np.float32), len(labs))


def staged(emb, features, rs, case, params, hw, wrong=(), first_mask_logits=None, from_stage=0):
    """A case, stage by stage -> (boolean mask [h, w], plane, delivered low-res logits [4, 256, 256] and iou of the last stage)."""
    import hq_cases as H
    _, clicks, labels, box, _ = case
    prev = first_mask_logits
    low = iou = plane = None
    for k in H.stage_clicks(case)[from_stage:]:
        low, iou, plane = decode_case_stage(emb, features, rs, clicks[:k], labels[:k], box, params, prev, wrong)
        prev = low[plane]
    return O.postprocess_logits(np.asarray(low[plane], np.float32), hw) > 0, plane, low, iou


def plain_mask(emb, rs, case, params, hw):
    """The plain twin: the same prompt through oracle/decoder_ref.decode_fp64 (marks as mask_input_cases stages them)."""
    import mask_input_cases as MI
    _, clicks, labels, box, _ = case
    import hq_cases as H
    prev = None
    low = plane = None
    for k in H.stage_clicks(case):
        low, _, plane = MI.decode_stage(emb, rs, clicks[:k], labels[:k], box, params, prev)
        prev = low[plane]
    return O.postprocess_logits(np.asarray(low[plane], np.float32), hw) > 0
