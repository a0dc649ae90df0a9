"""High-precision reference of the SAM prompt encoder + mask decoder  --  TEST INFRASTRUCTURE ONLY.

`oracle/sam_oracle.decode_masks` states the decoder in fp32, the way the reference's ONNX graph computes it.  This module
states the same decoder in float64, so that the HIP decoder can be checked on its own (tests/test_gpu_decoder.py) with a
tolerance set by the decoder's own error and not by the encoder's:

* `decode_fp64`  the published decoder, every operation in float64.
* `decode_f16`   the same, with values rounded to f16 (numpy astype(float16): round to nearest even) at every point
                 where the HIP decoder stores or consumes f16, and nowhere else.  What is left between this and the GPU
                 is fp32 accumulation, fp32 transcendental functions and the order of sums.
* `decode`       the common body: `round_at` names the rounding points to apply (`decode(..., round_at=())` IS
                 `decode_fp64`), `taps` receives the intermediates that `dlimg_amd_decoder_state` exposes.

Rounding points (F16_POINTS), read off csrc/sam_model.cpp and csrc/kernels/decoder*.hip:

  keys_h   the f16 copy of the keys that every image-side MFMA reads: f16(embedding + no_mask) (decoder_start_kernel),
           and f16 of each LayerNorm(norm4) output (image_update_kernel).  The fp32 keys themselves stay unrounded: they
           are the residual of image_update and what keys_head shows.
  weight_h the f16 weights of the image side (SamWeights: fused_h / linear_h / conv_transpose_h): the fused
           [t2i.k ; i2t.q ; t2i.v] projection of each layer, i2t.o, the fused [final.k ; final.v], up1 and up2.
           Biases stay fp32; every token-side weight is fp32.
  pos_h    the dense positional encoding, rounded to f16 on the host before `pos_term` multiplies it with the f16
           projection weights (fp32 accumulation, stored as an fp32 addend of the image-side GEMM).
  kqv_h    the f16 output of the image-side GEMMs (kqv_h_): the keys and values the tokens attend to, and the queries
           of the image -> token attention.
  attn_h   the image -> token attention output, cast to f16 as the A operand of the Wo MFMA (image_update_kernel).
  gelu_h   GELU(LayerNorm2d(ConvT1)) cast to f16 as the A operand of the ConvT2 MFMA (upscale_logits_kernel).

Taps (names of `dlimg_amd_decoder_state` and of the state of `dlimg_amd_test_decode_prompts`, one prompt of n points,
T = 5 + n token rows: 7 for the two-point prompts, up to 15):
  tokens     [T,256]  iou token, 4 mask tokens, the n prompt tokens in the order of the packed prompt (tokens_)
  queries    [T,256]  the last two-way block's token rows after the MLP residual, before norm3 (queries_)
  keys_head  [16,256] the first 16 rows of the final fp32 keys (keys_), after the last block's norm4
  hyper      [4,32]   the hyper-network outputs (hyper_)
  iou        [4]      the IoU predictions (iou_)
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional

import numpy as np

try:
    from scipy.special import erf as _erf
except Exception:  # pragma: no cover
    _erf = np.vectorize(math.erf, otypes=[np.float64])

f64 = np.float64

F16_POINTS = ("keys_h", "weight_h", "pos_h", "kqv_h", "attn_h", "gelu_h")

IMAGE_SIZE = 1024
GRID = 64
HEADS = 8
DEC_LN_EPS = 1e-5      # norm1..4, norm_final_attn (sam_oracle.DEC_LN_EPS)
UP_LN_EPS = 1e-6       # LayerNorm2d of the upscaling path


def _f16(x: np.ndarray) -> np.ndarray:
    return np.asarray(x).astype(np.float16).astype(f64)


def _layer_norm(x, w, b, eps):
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    var = (xc * xc).mean(axis=-1, keepdims=True)
    return xc / np.sqrt(var + eps) * w + b


def _gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def _softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _pe_encoding(coords01, gauss):
    c = 2.0 * math.pi * ((2.0 * coords01 - 1.0) @ gauss)
    return np.concatenate([np.sin(c), np.cos(c)], axis=-1)


def image_pe(gauss) -> np.ndarray:
    """Dense positional encoding of the 64 x 64 grid, token-major [4096,256], float64."""
    t = (np.arange(GRID, dtype=f64) + 0.5) / GRID
    yy, xx = np.meshgrid(t, t, indexing="ij")
    return _pe_encoding(np.stack([xx, yy], axis=-1), gauss).reshape(GRID * GRID, -1)


def embed_prompt(coords, labels, p) -> np.ndarray:
    """SamOnnxModel._embed_points in float64: coords [n,2] in resized-image pixels, labels [n] (0 / 1: a background / foreground
    click, 2 / 3: box corners, -1: the padding point) -> [n,256]."""
    c = (np.asarray(coords, f64).reshape(-1, 2) + 0.5) / IMAGE_SIZE
    e = _pe_encoding(c, p["pe.gauss"])
    lab = np.asarray(labels, f64).reshape(-1)[:, None]
    e = e * (lab != -1) + p["pe.not_a_point"][None, :] * (lab == -1)
    for i in range(4):
        e = e + p["pe.point"][i][None, :] * (lab == i)
    return e


def _heads(x):
    n, d = x.shape
    return x.reshape(n, HEADS, d // HEADS).transpose(1, 0, 2)


def _attend(q, k, v):
    """q [nq,D'], k [nk,D'], v [nk,D'] (already projected) -> [nq,D'] over 8 heads."""
    hd = q.shape[-1] // HEADS
    a = _softmax((_heads(q) @ _heads(k).transpose(0, 2, 1)) / math.sqrt(hd))
    return (a @ _heads(v)).transpose(1, 0, 2).reshape(q.shape[0], -1)


def _lin(x, p, pre):
    return x @ p[pre + ".w"].T + p[pre + ".b"]


def _token_attention(q_in, k_in, v_in, p, pre):
    return _lin(_attend(_lin(q_in, p, pre + ".q"), _lin(k_in, p, pre + ".k"), _lin(v_in, p, pre + ".v")), p, pre + ".o")


def decode(emb, coords, labels, params, round_at: Iterable[str] = (), taps: Optional[dict] = None):
    """Embedding [4096,256] + packed prompt (coords [n,2], labels [n], any n) -> (logits [4,256,256], iou [4]), float64, with
    f16 rounding at the points named in `round_at` (a subset of F16_POINTS)."""
    round_at = frozenset(round_at)
    unknown = round_at - set(F16_POINTS)
    if unknown:
        raise ValueError(f"unknown rounding points {sorted(unknown)}")

    def rnd(point, x):
        return _f16(x) if point in round_at else x

    p = {k: np.asarray(v, f64) for k, v in params.items() if k.startswith(("pe.", "dec."))}
    wh = lambda name: rnd("weight_h", p[name])                                     # noqa: E731

    sparse = embed_prompt(coords, labels, p)
    tokens = np.concatenate([p["dec.iou_token"][None, :], p["dec.mask_tokens"], sparse], axis=0)
    keys = np.asarray(emb, f64) + p["pe.no_mask"][None, :]
    pos_h = rnd("pos_h", image_pe(p["pe.gauss"]))

    def image_projection(parts, with_pos):
        """kqv_h = f16(keys_h W^T + b + pos_h W[:with_pos]^T): the fused image-side GEMM of csrc/sam_model.cpp."""
        w = np.concatenate([wh(n + ".w") for n in parts], axis=0)
        b = np.concatenate([p[n + ".b"] for n in parts], axis=0)
        y = rnd("keys_h", keys) @ w.T + b
        y[:, :with_pos] += pos_h @ w[:with_pos].T
        return rnd("kqv_h", y)

    queries, qpe = tokens, tokens
    for i in range(2):
        pre = f"dec.L{i}"
        if i == 0:
            queries = _token_attention(queries, queries, queries, p, pre + ".self")
        else:
            qq = queries + qpe
            queries = queries + _token_attention(qq, qq, queries, p, pre + ".self")
        queries = _layer_norm(queries, p[pre + ".ln1.w"], p[pre + ".ln1.b"], DEC_LN_EPS)
        kqv = image_projection([pre + ".t2i.k", pre + ".i2t.q", pre + ".t2i.v"], 256)
        # tokens -> image: q from the tokens (fp32 side), k / v from the f16 projection of the keys
        att = _attend(_lin(queries + qpe, p, pre + ".t2i.q"), kqv[:, :128], kqv[:, 256:])
        queries = queries + _lin(att, p, pre + ".t2i.o")
        queries = _layer_norm(queries, p[pre + ".ln2.w"], p[pre + ".ln2.b"], DEC_LN_EPS)
        h = np.maximum(_lin(queries, p, pre + ".mlp.fc1"), 0)
        queries = queries + _lin(h, p, pre + ".mlp.fc2")
        if i == 1 and taps is not None:
            taps["queries"] = queries.copy()
        queries = _layer_norm(queries, p[pre + ".ln3.w"], p[pre + ".ln3.b"], DEC_LN_EPS)
        # image -> tokens: q from the f16 projection, token k / v on the fp32 side, output projection on f16 operands
        att = _attend(kqv[:, 128:256], _lin(queries + qpe, p, pre + ".i2t.k"), _lin(queries, p, pre + ".i2t.v"))
        out = rnd("attn_h", att) @ wh(pre + ".i2t.o.w").T + p[pre + ".i2t.o.b"]
        keys = _layer_norm(keys + out, p[pre + ".ln4.w"], p[pre + ".ln4.b"], DEC_LN_EPS)
    kv = image_projection(["dec.final.k", "dec.final.v"], 128)
    att = _attend(_lin(queries + qpe, p, "dec.final.q"), kv[:, :128], kv[:, 128:])
    queries = queries + _lin(att, p, "dec.final.o")
    queries = _layer_norm(queries, p["dec.ln_final.w"], p["dec.ln_final.b"], DEC_LN_EPS)

    # upscaling: ConvT 2x2/2 -> LayerNorm2d -> GELU -> ConvT 2x2/2 -> GELU, pixel-major [256*256, 32]
    w1 = wh("dec.up1.w")                                                          # [256,64,2,2]
    c1 = w1.shape[1]
    y = rnd("keys_h", keys) @ w1.reshape(w1.shape[0], -1)
    y = y.reshape(GRID, GRID, c1, 2, 2).transpose(0, 3, 1, 4, 2).reshape(2 * GRID, 2 * GRID, c1) + p["dec.up1.b"]
    y = rnd("gelu_h", _gelu(_layer_norm(y, p["dec.up_ln.w"], p["dec.up_ln.b"], UP_LN_EPS)))
    w2 = wh("dec.up2.w")                                                          # [64,32,2,2]
    c2 = w2.shape[1]
    z = y.reshape(-1, c1) @ w2.reshape(c1, -1)
    z = z.reshape(2 * GRID, 2 * GRID, c2, 2, 2).transpose(0, 3, 1, 4, 2).reshape(4 * GRID, 4 * GRID, c2) + p["dec.up2.b"]
    up = _gelu(z).reshape(-1, c2)

    def mlp3(x, pre):
        x = np.maximum(_lin(x, p, pre + ".0"), 0)
        x = np.maximum(_lin(x, p, pre + ".1"), 0)
        return _lin(x, p, pre + ".2")

    hyper = np.stack([mlp3(queries[1 + m], f"dec.hyper{m}") for m in range(4)], axis=0)
    logits = (hyper @ up.T).reshape(4, 4 * GRID, 4 * GRID)
    iou = mlp3(queries[0], "dec.iou")
    if taps is not None:
        taps.update(tokens=tokens, keys_head=keys[:16].copy(), hyper=hyper, iou=iou)
    return logits, iou


def decode_fp64(emb, coords, labels, params, taps: Optional[dict] = None):
    """The published decoder in float64."""
    return decode(emb, coords, labels, params, (), taps)


def decode_f16(emb, coords, labels, params, taps: Optional[dict] = None):
    """The float64 decoder with the HIP decoder's f16 storage emulated (every point of F16_POINTS)."""
    return decode(emb, coords, labels, params, F16_POINTS, taps)


def perturbed(params: Dict[str, np.ndarray], no_mask_scale: float = 0.99, iou_bias_shift: float = 0.002):
    """The decoder's bug stand-ins as a weight change: pe.no_mask scaled (an error of 1 % in one addend of the keys) and
    the IoU head's last bias shifted.  Every other tensor is the same object."""
    q = dict(params)
    q["pe.no_mask"] = (np.asarray(params["pe.no_mask"], np.float32) * np.float32(no_mask_scale)).astype(np.float32)
    q["dec.iou.2.b"] = (np.asarray(params["dec.iou.2.b"], np.float32) + np.float32(iou_bias_shift)).astype(np.float32)
    return q
