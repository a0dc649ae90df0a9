"""Float64 references, a rounding model and input builders for the two encoder attention kernels
(kernels/attention_global.hip, kernels/attention_window.hip), shared by tests/test_attention_ref.py (CPU) and
tests/test_gpu_attention.py (GPU).  No test functions here.

Everything is written from the kernels' CONTRACTS (kernels.hpp, the header comments of the two kernels, and what
dlimg_amd_test_attention does on the host before it launches them), not from their code:

  * global:   q' = f16(f32(q) * qs), qs = f32(log2 e) / sqrt(f32(hd)); tables R' = f16(rel * sqrt(f32(hd)));
              S[i,j] = q'_i.k_j + q'_i.R'h[qy_i - ky_j + 63] + q'_i.R'w[qx_i - kx_j + 63]   (units of log2)
  * windowed: qkv f16, qkv bias and tables rounded to f16; 25 windows of 14x14 over the 64x64 grid padded to 70x70;
              a zero-padding token carries qkv == bias and is an un-masked key / value; pad queries are dropped;
              S[i,j] = log2(e) * (q_i.k_j / sqrt(hd) + q_i.Rh[ty_i - ty_j + 13] + q_i.Rw[tx_i - tx_j + 13])
  * both:     out = f16(softmax2(S) @ v), where the probabilities are taken relative to a lazily raised reference
              maximum (never more than 8 log2 units below the running row maximum) and rounded to f16 as operands of
              the second MFMA.

A "score matrix" below is S in units of log2, float64, [queries, keys]; for the windowed kernel the key axis is in SLOT
order (slot = ty * 16 + tx, tx = 14, 15 are dummies with S = -inf and v = 0), so that a key tile is 32 consecutive slots.
"""
from typing import Callable, Dict, List, Optional

import numpy as np

f16, f32, f64 = np.float16, np.float32, np.float64

GRID = 64
TOKENS = GRID * GRID
WS = 14                     # window size
NW = 5                      # windows per axis
SLOTS = 224                 # 14 rows x 16 slots (14 tokens + 2 dummies)
GLOBAL_TILE = 64            # keys per tile of the global kernel: one grid row
WINDOW_TILE = 32            # slots per tile of the windowed kernel: two window rows
RAISE = 8.0                 # log2 units a key may lie above the reference before the reference must be raised
LOG2E = 1.44269504088896341

RMS_MARGIN = 1.5
MAX_MARGIN = 2.0


# ------------------------------------------------------------------------------------------ roundings

def round_f16(x: np.ndarray) -> np.ndarray:
    """x -> nearest f16 (ties to even, subnormals kept: numpy's conversion), back in float64."""
    return np.asarray(x, f64).astype(f16).astype(f64)


def round_bf16(x: np.ndarray) -> np.ndarray:
    """x -> nearest bfloat16 (ties to even), back in float64.  (Only a modified model uses it.)"""
    b = np.asarray(x, f64).astype(f32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(f32).astype(f64)


def rms(x: np.ndarray) -> float:
    x = np.asarray(x, f64)
    return float(np.sqrt(np.mean(x * x)))


# ------------------------------------------------------------------- softmax, rounding model, raise rule

def softmax2(S: np.ndarray, V: np.ndarray, want_p: bool = False):
    """out = softmax over keys of 2^S, times V; float64.  With want_p also the normalised P."""
    m = S.max(axis=1, keepdims=True)
    P = np.exp2(S - m)
    P /= P.sum(axis=1, keepdims=True)
    out = P @ V
    return (out, P) if want_p else out


def reference_track(S: np.ndarray, tile: int):
    """The documented raise rule, from a SUFFICIENT condition only.  Per query: the reference starts as the maximum of key
    tile 0; at tile t it must be raised when one single key of the tile lies more than RAISE log2 units above it (that
    key alone makes the tile's probabilities outgrow 2^8, whichever keys a lane happens to sum), and then becomes that
    tile's maximum.  Returns (m [queries, tiles]: the reference in force at each tile, raises: per query the tiles)."""
    nq, nk = S.shape
    assert nk % tile == 0
    nt = nk // tile
    tmax = S.reshape(nq, nt, tile).max(axis=2)
    m = np.empty((nq, nt), f64)
    cur = tmax[:, 0].copy()
    m[:, 0] = cur
    raises: List[List[int]] = [[] for _ in range(nq)]
    for t in range(1, nt):
        up = tmax[:, t] > cur + RAISE
        for i in np.nonzero(up)[0]:
            raises[i].append(t)
        cur = np.where(up, tmax[:, t], cur)
        m[:, t] = cur
    return m, raises


def forced_raises(S_log2: np.ndarray, tile: int) -> List[List[int]]:
    """Per query (row of S_log2) the list of key tiles at which the kernel MUST raise its reference maximum."""
    return reference_track(S_log2, tile)[1]


def rounding_model(S: np.ndarray, V: np.ndarray, tile: int, round_p: Callable = round_f16) -> np.ndarray:
    """What the kernels' contracts state and nothing more: P relative to the lazily raised reference (reference_track:
    at most 8 log2 units below the running maximum, so P <= 2^8), rounded to f16; products, sums and the quotient
    exact (float64); the output rounded to f16."""
    nq, nk = S.shape
    nt = nk // tile
    m, _ = reference_track(S, tile)
    P = round_p(np.exp2(S.reshape(nq, nt, tile) - m[:, :, None]))
    P *= np.exp2(m - m[:, -1:])[:, :, None]                 # every tile brought to the final reference
    P = P.reshape(nq, nk)
    return round_f16((P @ V) / P.sum(axis=1, keepdims=True))


def check(name: str, got: np.ndarray, ref: np.ndarray, model: np.ndarray) -> Dict[str, float]:
    """got (the kernel, or a modified model) against ref (float64), in units of the rounding model's own error:
    finite, rms <= 1.5 units, max <= 2 units.  Both ratios are logged through conftest.within."""
    from conftest import within
    got, ref, model = np.asarray(got, f64), np.asarray(ref, f64), np.asarray(model, f64)
    assert got.shape == ref.shape == model.shape, (got.shape, ref.shape, model.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    unit_rms, unit_max = rms(model - ref), float(np.abs(model - ref).max())
    assert unit_rms > 0 and unit_max > 0, f"{name}: the rounding model has no error on this input, nothing to measure in"
    r_rms = rms(got - ref) / unit_rms
    r_max = float(np.abs(got - ref).max()) / unit_max
    print(f"{name}: rms {rms(got - ref):.3g} = {r_rms:.3f} x model ({unit_rms:.3g}); "
          f"max {np.abs(got - ref).max():.3g} = {r_max:.3f} x model ({unit_max:.3g})")
    # within() asserts strictly below; the margins are inclusive, hence the nextafter
    ok_rms = r_rms <= RMS_MARGIN
    ok_max = r_max <= MAX_MARGIN
    try:
        within(name + " rms/model", r_rms, np.nextafter(RMS_MARGIN, 2.0))
    finally:
        within(name + " max/model", r_max, np.nextafter(MAX_MARGIN, 3.0))
    assert ok_rms and ok_max
    return {"rms": r_rms, "max": r_max}


# ---------------------------------------------------------------------------------------- global kernel

def global_operands(qkv, rel_h, rel_w, batch: int, heads: int, hd: int) -> Dict[str, np.ndarray]:
    """The f16 operands dlimg_amd_test_attention hands attention_global, as float64: q', k, v [batch, heads, 4096, hd],
    tables R'h, R'w [127, hd].  The scalings are done in float32 as the hook does them, so the bits match."""
    qkv = np.asarray(qkv, f16).reshape(batch, TOKENS, 3, heads, hd)
    qs = f32(1.44269504088896341) / np.sqrt(f32(hd))
    rs = np.sqrt(f32(hd))
    assert qs.dtype == f32 and rs.dtype == f32
    q = (qkv[:, :, 0].astype(f32) * qs).astype(f16)
    t = lambda x: np.ascontiguousarray(x.transpose(0, 2, 1, 3)).astype(f64)
    return {"q": t(q), "k": t(qkv[:, :, 1]), "v": t(qkv[:, :, 2]),
            "rh": (np.asarray(rel_h, f32) * rs).astype(f16).astype(f64),
            "rw": (np.asarray(rel_w, f32) * rs).astype(f16).astype(f64)}


def global_scores(ops, b: int = 0, h: int = 0, queries: Optional[np.ndarray] = None,
                  variant: Optional[str] = None) -> np.ndarray:
    """S [queries, 4096] in float64 from the f16 operands.  `variant` names a MODIFIED computation (a shortcut or an
    indexing mistake a kernel might make; tests/test_attention_ref.py shows that check() rejects each)."""
    queries = np.arange(TOKENS) if queries is None else np.asarray(queries)
    q, k = ops["q"][b, h][queries], ops["k"][b, h]
    rh, rw = (ops["rw"], ops["rh"]) if variant == "tables_swapped" else (ops["rh"], ops["rw"])
    nq = len(queries)
    qy, qx = queries // GRID, queries % GRID
    kk = np.arange(GRID)
    kx = np.minimum(kk, GRID - 2) if variant == "clamp_kx63" else kk        # key column 63 takes column 62's entry
    row = np.take_along_axis(q @ rh.T, qy[:, None] - kk[None, :] + GRID - 1, axis=1)       # [nq, ky]
    col = np.take_along_axis(q @ rw.T, qx[:, None] - kx[None, :] + GRID - 1, axis=1)       # [nq, kx]
    if variant == "row_bias_f16":
        row = round_f16(row)
    if variant == "col_bias_f16":
        col = round_f16(col)
    S = (q @ k.T).reshape(nq, GRID, GRID)
    S += row[:, :, None]
    S += col[:, None, :]
    S = S.reshape(nq, TOKENS)
    if variant == "scores_f16":
        S = round_f16(S)
    assert variant in (None, "tables_swapped", "clamp_kx63", "row_bias_f16", "col_bias_f16", "scores_f16"), variant
    return S


def global_reference(qkv, rel_h, rel_w, batch: int, heads: int, hd: int, b: int = 0, h: int = 0,
                     queries: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """ref, model [queries, hd] and S [queries, 4096] of one (image, head)."""
    ops = global_operands(qkv, rel_h, rel_w, batch, heads, hd)
    S = global_scores(ops, b, h, queries)
    V = ops["v"][b, h]
    return {"ref": softmax2(S, V), "model": rounding_model(S, V, GLOBAL_TILE), "S": S, "V": V}


def head_columns(got: np.ndarray, batch: int, heads: int, hd: int, b: int, h: int,
                 queries: Optional[np.ndarray] = None) -> np.ndarray:
    """The [queries, hd] block of one (image, head) out of a kernel result [batch * 4096, heads * hd]."""
    x = np.asarray(got).reshape(batch, TOKENS, heads, hd)[b, :, h].astype(f64)
    return x if queries is None else x[np.asarray(queries)]


# -------------------------------------------------------------------------------------- windowed kernel

def window_slots():
    """token [25, 224]: the grid token of every slot of every window, -1 for a zero-padding token, -2 for a dummy slot;
    ty, tx [224]."""
    slot = np.arange(SLOTS)
    ty, tx = slot >> 4, slot & 15
    token = np.empty((NW * NW, SLOTS), np.int64)
    for w in range(NW * NW):
        gy, gx = (w // NW) * WS + ty, (w % NW) * WS + tx
        token[w] = np.where(tx >= WS, -2, np.where((gy >= GRID) | (gx >= GRID), -1, gy * GRID + gx))
    return token, ty, tx


def window_operands(qkv, bias, rel_h, rel_w, batch: int, heads: int, hd: int) -> Dict[str, np.ndarray]:
    """Operands of attention_window as float64, in slot order: q, k, v [batch, heads, 25, 224, hd] (pad slots carry the
    f16-rounded bias, dummy slots zeros), tables [27, hd]."""
    qkv = np.asarray(qkv, f16).reshape(batch, TOKENS, 3, heads, hd).astype(f64)
    b16 = np.asarray(bias, f32).astype(f16).astype(f64).reshape(3, heads, hd)
    token, _, _ = window_slots()
    x = qkv[:, np.maximum(token, 0)]                                    # [batch, 25, 224, 3, heads, hd]
    x = np.where((token == -1)[None, :, :, None, None, None], b16[None, None, None], x)
    x = np.where((token == -2)[None, :, :, None, None, None], 0.0, x)
    x = x.transpose(3, 0, 4, 1, 2, 5)                                    # [3, batch, heads, 25, 224, hd]
    return {"q": x[0], "k": x[1], "v": x[2], "token": token,
            "rh": np.asarray(rel_h, f32).astype(f16).astype(f64), "rw": np.asarray(rel_w, f32).astype(f16).astype(f64)}


def window_scores(ops, b: int = 0, h: int = 0, variant: Optional[str] = None) -> np.ndarray:
    """S [25, 224 query slots, 224 key slots]; dummy key slots are -inf.  Rows of pad / dummy query slots are computed
    like any other and dropped by the callers."""
    q, k = ops["q"][b, h], ops["k"][b, h]                               # [25, 224, hd]
    hd = q.shape[-1]
    token, ty, tx = window_slots()
    rh, rw = (ops["rw"], ops["rh"]) if variant == "tables_swapped" else (ops["rh"], ops["rw"])
    txk = np.minimum(tx, WS - 1)                                        # (a dummy's index is never used: -inf below)
    ih = ty[:, None] - ty[None, :] + WS - 1                             # [224 q, 224 k]
    iw = np.minimum(tx, WS - 1)[:, None] - txk[None, :] + WS - 1
    gh = q @ rh.T                                                       # [25, 224, 27]
    gw = q @ rw.T
    row = np.take_along_axis(gh, np.broadcast_to(ih, (NW * NW, SLOTS, SLOTS)), axis=2)
    col = np.take_along_axis(gw, np.broadcast_to(iw, (NW * NW, SLOTS, SLOTS)), axis=2)
    if variant == "row_bias_f16":
        row = round_f16(row)
    if variant == "col_bias_f16":
        col = round_f16(col)
    kk = k
    if variant == "dummies_are_keys":           # the two dummy slots of a row read the K row of its last token
        kk = k[:, (ty * 16 + txk)]
    S = LOG2E * (q @ kk.transpose(0, 2, 1) / np.sqrt(f64(hd)) + row + col)
    if variant == "scores_f16":
        S = round_f16(S)
    if variant != "dummies_are_keys":
        S[:, :, tx >= WS] = -np.inf
    if variant == "pad_keys_masked":
        S = np.where((token == -1)[:, None, :], -np.inf, S)
    assert variant in (None, "tables_swapped", "row_bias_f16", "col_bias_f16", "scores_f16", "dummies_are_keys",
                       "pad_keys_masked"), variant
    return S


def window_gather(per_window: np.ndarray) -> np.ndarray:
    """[25, 224, hd] in slot order -> [4096, hd] in token order (pad and dummy query slots dropped)."""
    token, _, _ = window_slots()
    real = token >= 0
    out = np.empty((TOKENS, per_window.shape[-1]), f64)
    out[token[real]] = per_window[real]
    return out


def window_apply(S: np.ndarray, V: np.ndarray, fn: Callable) -> np.ndarray:
    """fn(S_w, V_w) per window, gathered to token order."""
    return window_gather(np.stack([fn(S[w], V[w]) for w in range(NW * NW)]))


def window_reference(qkv, bias, rel_h, rel_w, batch: int, heads: int, hd: int, b: int = 0, h: int = 0):
    """ref, model [4096, hd] in token order, S [25, 224, 224], V [25, 224, hd], token [25, 224] of one (image, head)."""
    ops = window_operands(qkv, bias, rel_h, rel_w, batch, heads, hd)
    S, V = window_scores(ops, b, h), ops["v"][b, h]
    return {"ref": window_apply(S, V, softmax2),
            "model": window_apply(S, V, lambda s, v: rounding_model(s, v, WINDOW_TILE)),
            "S": S, "V": V, "token": ops["token"]}


def window_forced_raises(S: np.ndarray) -> Dict[int, List[int]]:
    """token -> tiles at which the windowed kernel must raise, for every real query that must raise at all."""
    token, _, _ = window_slots()
    out = {}
    for w in range(NW * NW):
        for slot, tiles in enumerate(forced_raises(S[w], WINDOW_TILE)):
            if tiles and token[w, slot] >= 0:
                out[int(token[w, slot])] = tiles
    return out


# ------------------------------------------------------------------------------------------ input builders
# Every builder returns a dict with the arguments of ext.test_attention (qkv, bias, rel_h, rel_w, batch, heads, hd) and
# whatever its conditions are stated on.  The conditions themselves are asserted in tests/test_attention_ref.py and
# again, on the very inputs the kernel gets, in tests/test_gpu_attention.py -- always on the float64 reference alone.

def gaussian_qkv(seed: int, heads: int, hd: int, batch: int = 1):
    """The existing attention tests' inputs (tests/test_gpu_kernels.py, _qkv)."""
    rng = np.random.default_rng(seed)
    D = heads * hd
    qkv = rng.standard_normal((batch * TOKENS, 3 * D)).astype(f16)
    bias = (0.5 * rng.standard_normal(3 * D)).astype(f32)
    return qkv, bias


def gaussian_tables(seed: int, span: int, hd: int, sigma: float = 0.2):
    rng = np.random.default_rng(seed)
    rel_h = (sigma * rng.standard_normal((2 * span - 1, hd))).astype(f32)
    rel_w = (sigma * rng.standard_normal((2 * span - 1, hd))).astype(f32)
    return rel_h, rel_w


def diffuse_case(is_global: bool, hd: int, heads: int = 1, batch: int = 1, seed: int = 21):
    qkv, bias = gaussian_qkv(seed, heads, hd, batch)
    rel_h, rel_w = gaussian_tables(seed + 1, GRID if is_global else WS, hd)
    return {"qkv": qkv, "bias": None if is_global else bias, "rel_h": rel_h, "rel_w": rel_w,
            "batch": batch, "heads": heads, "hd": hd}


# the cases of tests/test_gpu_attention.py (and of the builders' CPU tests)
ROUTING_GLOBAL = [(2731, 1234, 1), (4093, 63, 2)]           # (a, b, heads): perm(i) = (a * i + b) mod 4096, a odd
ROUTING_WINDOW = [(45, 17), (137, 100)]                     # (a, b): (a * i + b) mod 196, gcd(a, 196) = 1
SHIFT_GLOBAL = [(0, 63), (63, 126), (126, 0), (40, 90)]     # (d*, e*): table rows of rel_h, rel_w
SHIFT_WINDOW = [(0, 13), (13, 26), (26, 0), (8, 20)]


def code_words(n: int, hd: int) -> np.ndarray:
    """n <= 4096 words of +-1 in hd >= 64 dimensions, any two of which correlate at most 0.6: words of the second-order
    Reed-Muller code RM(2, 6) (length 64, minimum distance 16, so the correlation of two words is at most 1/2) with
    12 message bits -- the six linear and six of the quadratic monomials; dimensions past 64 repeat the first ones."""
    assert n <= 4096 and 64 <= hd <= 128
    x = (np.arange(64)[:, None] >> np.arange(6)[None, :]) & 1                                # [64 points, 6 bits]
    mono = np.concatenate([x, np.stack([x[:, i] * x[:, (i + 1) % 6] for i in range(6)], axis=1)], axis=1)   # [64, 12]
    msg = (np.arange(n)[:, None] >> np.arange(12)[None, :]) & 1                              # [n, 12]
    bits = (msg @ mono.T) & 1                                                                # [n, 64]
    w = 1.0 - 2.0 * bits
    return np.concatenate([w, w[:, :hd - 64]], axis=1)


def _aligned(q_row16: np.ndarray, target_log2: float, per_unit: float) -> np.ndarray:
    """A key row along q_row16 (f16) whose score with that query is target_log2; per_unit = score of k == q."""
    return (q_row16.astype(f64) * (target_log2 / per_unit)).astype(f16)


def routing_global_case(hd: int, a: int, b: int, heads: int = 1, peak: float = 32.0, seed: int = 31):
    """Query i is routed to key perm(i) = (a * i + b) mod 4096 (head h: b + 977 h) by the q.k term alone, tables zero:
    k_j = beta * word(j), q_i = alpha * word(perm(i)), scaled so that the designated score is `peak` log2 units and
    every other key lies at most at 0.6 * peak.  V rows are Gaussian, different for every key, head and image."""
    assert a % 2 == 1
    rng = np.random.default_rng(seed)
    D = heads * hd
    words = code_words(TOKENS, hd)
    qkv = np.zeros((TOKENS, 3, heads, hd), f16)
    perm = np.empty((heads, TOKENS), np.int64)
    qs = float(f32(1.44269504088896341) / np.sqrt(f32(hd)))
    alpha = 2.0
    qprime = float(f16(f32(alpha) * f32(qs)))
    beta = peak / (hd * qprime)
    for h in range(heads):
        perm[h] = (a * np.arange(TOKENS) + b + 977 * h) % TOKENS
        qkv[:, 0, h] = (alpha * words[perm[h]]).astype(f16)
        qkv[:, 1, h] = (beta * words).astype(f16)
    qkv[:, 2] = rng.standard_normal((TOKENS, heads, hd)).astype(f16)
    zero = np.zeros((2 * GRID - 1, hd), f32)
    return {"qkv": qkv.reshape(TOKENS, 3 * D), "bias": None, "rel_h": zero, "rel_w": zero, "batch": 1, "heads": heads,
            "hd": hd, "perm": perm}


def routing_window_case(hd: int, a: int, b: int, peak: float = 32.0, seed: int = 33):
    """The windowed analogue: inside every window, the query at window position i (= ty * 14 + tx) is routed to the key
    at position (a * i + b) mod 196.  All zero-padding tokens share one key row (the bias's k part, a code word of its
    own), so a query whose designated position is a pad token attends to the pad tokens and returns the bias's v part."""
    assert np.gcd(a, WS * WS) == 1
    rng = np.random.default_rng(seed)
    words = code_words(256, hd)
    token, ty, tx = window_slots()
    alpha = 2.0
    beta = peak * np.sqrt(hd) / (LOG2E * hd * alpha)
    qkv = np.zeros((TOKENS, 3, hd), f16)
    # [window, query slot] -> slot of the designated key; -1: it is a pad token (all pad slots); -2: not a real query
    target_slot = np.full((NW * NW, SLOTS), -2, np.int64)
    pos = ty * WS + tx
    for w in range(NW * NW):
        pos_token = np.full(WS * WS, -1, np.int64)
        real_or_pad = tx < WS
        pos_token[pos[real_or_pad]] = token[w, real_or_pad]
        for s in np.nonzero(token[w] >= 0)[0]:
            target = (a * pos[s] + b) % (WS * WS)
            t = token[w, s]
            target_slot[w, s] = (target // WS) * 16 + target % WS if pos_token[target] >= 0 else -1
            qkv[t, 0] = (alpha * words[target if pos_token[target] >= 0 else 255]).astype(f16)
            qkv[t, 1] = (beta * words[pos[s]]).astype(f16)
    qkv[:, 2] = rng.standard_normal((TOKENS, hd)).astype(f16)
    bias = np.concatenate([np.zeros(hd), beta * words[255], rng.standard_normal(hd)]).astype(f16).astype(f32)
    zero = np.zeros((2 * WS - 1, hd), f32)
    return {"qkv": qkv.reshape(TOKENS, 3 * hd), "bias": bias, "rel_h": zero, "rel_w": zero, "batch": 1, "heads": 1,
            "hd": hd, "target_slot": target_slot}


def shift_case(is_global: bool, hd: int, d_star: int, e_star: int, height: float = 18.0, seed: int = 35):
    """All queries equal, all keys zero (windowed: the bias's k part too), so a score is the rel-pos bias alone; rel_h is
    zero but for row d_star and rel_w but for row e_star, both aligned with the query: a key scores `height` log2 units
    for each axis on which its offset from the query hits the entry, so every query attends to the key at
    (qy + span - 1 - d_star, qx + span - 1 - e_star) where that key exists; where it does not, the reference decides."""
    rng = np.random.default_rng(seed)
    span = GRID if is_global else WS
    u = rng.choice([-1.0, 1.0], hd) * rng.uniform(0.5, 1.5, hd)
    qkv = np.zeros((TOKENS, 3, hd), f16)
    qkv[:, 0] = u.astype(f16)
    qkv[:, 2] = rng.standard_normal((TOKENS, hd)).astype(f16)
    u16 = u.astype(f16).astype(f64)
    entry = (u16 * (height / (LOG2E * float(u16 @ u16)))).astype(f32)      # log2(e) * q.entry == height
    rel_h = np.zeros((2 * span - 1, hd), f32)
    rel_w = np.zeros((2 * span - 1, hd), f32)
    rel_h[d_star] = entry
    rel_w[e_star] = entry
    bias = None if is_global else np.concatenate([rng.standard_normal(hd), np.zeros(hd), rng.standard_normal(hd)]).astype(f32)
    return {"qkv": qkv.reshape(TOKENS, 3 * hd), "bias": bias, "rel_h": rel_h, "rel_w": rel_w, "batch": 1, "heads": 1,
            "hd": hd, "offset": (span - 1 - d_star, span - 1 - e_star)}


# designated query token -> [(key tile, key column, planted score in log2 units)]: ascending staircases, each step well
# above 8 and at most 40.  Token 5 and 17 share wave 0 of block 0 (group A: token % 256 < 128), 198 sits in wave 6
# (group B), 1300 in wave 0 of block 5, 4095 in wave 7 of the last block.
GLOBAL_STAIRS = {
    5:    [(1, 3, 16.0), (2, 40, 30.0), (63, 10, 44.0)],        # tile 1, consecutive tiles, tile 63; residues 1, 2, 0
    17:   [(30, 50, 16.0), (45, 7, 30.0)],                      # same wave as token 5, other tiles
    198:  [(7, 33, 15.0), (8, 2, 28.0), (9, 63, 41.0), (63, 31, 54.0)],
    1300: [(1, 62, 16.0), (62, 0, 30.0), (63, 32, 44.0)],
    4095: [(3, 20, 16.0), (4, 45, 30.0), (5, 12, 44.0)],
}


def rescale_global_case(hd: int, seed: int = 37):
    """The existing rescale test's recipe (Gaussian qkv, queries and keys scaled by 0.3) with non-zero tables and staircase
    keys: for each designated query, key (tile, column) is set along the query so that its q.k score is the planted
    height -- each step far above everything the query has seen so far."""
    qkv, _ = gaussian_qkv(seed, 1, hd)
    qkv = (qkv.astype(f32) * f32(0.3)).astype(f16)
    rel_h, rel_w = gaussian_tables(seed + 1, GRID, hd)
    qs = f32(1.44269504088896341) / np.sqrt(f32(hd))
    planted = {}
    for tok, steps in GLOBAL_STAIRS.items():
        q16 = qkv[tok, :hd]
        qp = (q16.astype(f32) * qs).astype(f16).astype(f64)
        per_unit = float(qp @ q16.astype(f64))
        for tile, kx, height in steps:
            key = tile * GLOBAL_TILE + kx
            assert key not in planted
            planted[key] = tok
            qkv[key, hd:2 * hd] = _aligned(q16, height, per_unit)
    return {"qkv": qkv, "bias": None, "rel_h": rel_h, "rel_w": rel_w, "batch": 1, "heads": 1, "hd": hd,
            "stairs": GLOBAL_STAIRS}


def _profile_case(hd: int, levels: np.ndarray, gains: np.ndarray, seed: int):
    """Global-kernel inputs whose score matrix is an outer product: S[i, j] = gains[i] * levels[j] (log2 units, up to the
    f16 rounding of the operands), tables zero.  q_i = gains[i] * u, k_j = levels[j] * w with q'(u).w == 1."""
    rng = np.random.default_rng(seed)
    u = rng.choice([-1.0, 1.0], hd) * rng.uniform(0.75, 1.5, hd)
    qs = f32(1.44269504088896341) / np.sqrt(f32(hd))
    up = (u.astype(f16).astype(f32) * qs).astype(f16).astype(f64)
    w = up / float(up @ up)
    qkv = np.zeros((TOKENS, 3, hd), f16)
    qkv[:, 0] = (gains[:, None] * u[None, :]).astype(f16)
    qkv[:, 1] = (levels[:, None] * w[None, :]).astype(f16)
    qkv[:, 2] = rng.standard_normal((TOKENS, hd)).astype(f16)
    zero = np.zeros((2 * GRID - 1, hd), f32)
    return {"qkv": qkv.reshape(TOKENS, 3 * hd), "bias": None, "rel_h": zero, "rel_w": zero, "batch": 1, "heads": 1, "hd": hd}


def no_raise_limit_case(hd: int, seed: int = 41):
    """No raise at the limit: key 9 (tile 0) scores 0 and is tile 0's maximum, the background lies 4 to 10 log2 units
    below it, and one planted key in each of 48 tiles lies 7.8 to 7.9 above it; with query gains of 0.9, 0.95 and 1 the
    planted keys sit 7.02 to 7.9 log2 units above every query's tile-0 maximum: nothing forces a raise, P reaches
    2^7.9 and the row sum several thousand times the reference's own term."""
    rng = np.random.default_rng(seed)
    levels = -rng.uniform(4.0, 10.0, TOKENS)
    levels[9] = 0.0
    tiles = np.sort(rng.choice(np.arange(1, 64), 48, replace=False))
    if 63 not in tiles:
        tiles[-1] = 63
    if 1 not in tiles:
        tiles[0] = 1
    planted = tiles * GLOBAL_TILE + rng.integers(0, GLOBAL_TILE, len(tiles))
    levels[planted] = rng.uniform(7.8, 7.88, len(planted))
    gains = np.array([1.0, 0.95, 0.9])[np.arange(TOKENS) % 3]
    case = _profile_case(hd, levels, gains, seed)
    case["planted"] = planted
    return case


def f16_edge_case(hd: int, seed: int = 43):
    """P at the edge of f16's normal range: key 21 (tile 0) scores 0 and is the row maximum; every other key lies 13 to
    16 log2 units below it (P between 2^-13 and 2^-16: around f16's smallest normal 2^-14, about a sixth of them subnormal),
    crowded towards 13 so that together they carry a quarter of the softmax mass."""
    rng = np.random.default_rng(seed)
    levels = -(13.0 + 3.0 * rng.uniform(0.0, 1.0, TOKENS) ** 6)
    levels[21] = 0.0
    return _profile_case(hd, levels, np.ones(TOKENS), seed)


# windowed rescale coverage: (window, query (ty, tx), [(key (ty, tx), planted q.k score in log2 units)]).
# key tile = ty // 2.  Window 6 = (1, 1) is interior; its second entry's key is the last real token of a window row (tx
# = 13: the two dummy slots after it read its K row).  Window 20 = (4, 0) has zero padding in rows 8-13 only (tiles 4-6):
# its raise comes from the bias's k part, aligned with the query at (1, 2).
WINDOW_STAIRS = [
    (0,  (0, 1),  [((2, 5), 16.0)]),                       # tile 1
    (1,  (3, 4),  [((5, 0), 16.0)]),                       # tile 2
    (2,  (13, 13), [((6, 9), 16.0)]),                      # tile 3
    (3,  (7, 7),  [((9, 12), 16.0)]),                      # tile 4
    (5,  (2, 0),  [((11, 3), 16.0)]),                      # tile 5
    (7,  (10, 6), [((13, 13), 16.0)]),                     # tile 6, last slot of the window
    (6,  (4, 4),  [((4, 2), 16.0), ((10, 11), 30.0)]),     # two raises for one query: tiles 2 and 5
    (6,  (9, 1),  [((5, 13), 16.0)]),                      # forced by the last real token of a row (tile 2)
    (12, (0, 0),  [((3, 13), 16.0), ((8, 0), 29.0), ((13, 7), 42.0)]),
]
WINDOW_PAD_RAISE = (20, (1, 2), 16.0)                      # window (4, 0): the first pad keys are in tile 4


def rescale_window_case(hd: int, seed: int = 45):
    """The existing windowed rescale test's recipe (Gaussian qkv scaled by 0.3, Gaussian bias and tables) with planted keys
    aligned with designated queries (WINDOW_STAIRS) and the bias's k part aligned with one query of a border window."""
    qkv, bias = gaussian_qkv(seed, 1, hd)
    qkv = (qkv.astype(f32) * f32(0.3)).astype(f16)
    rel_h, rel_w = gaussian_tables(seed + 1, WS, hd)
    token, _, _ = window_slots()
    per = lambda q16: float(q16.astype(f64) @ q16.astype(f64)) * LOG2E / np.sqrt(hd)
    designated = {}
    for w, (qty, qtx), steps in WINDOW_STAIRS:
        qt = int(token[w, qty * 16 + qtx])
        assert qt >= 0
        q16 = qkv[qt, :hd]
        designated[qt] = [kty // 2 for (kty, _), _ in steps]
        for (kty, ktx), height in steps:
            kt = int(token[w, kty * 16 + ktx])
            assert kt >= 0
            qkv[kt, hd:2 * hd] = _aligned(q16, height, per(q16))
    w, (qty, qtx), height = WINDOW_PAD_RAISE
    qt = int(token[w, qty * 16 + qtx])
    q16 = qkv[qt, :hd]
    bias[hd:2 * hd] = _aligned(q16, height, per(q16)).astype(f32)
    designated[qt] = [4]
    return {"qkv": qkv, "bias": bias, "rel_h": rel_h, "rel_w": rel_w, "batch": 1, "heads": 1, "hd": hd,
            "designated": designated, "pad_query": qt}


# ------------------------------------------------------------------------ the builders' stated conditions
# Asserted on the float64 reference alone (score matrices from global_scores / window_scores on the builder's inputs).

def assert_routing_global(S: np.ndarray, perm_rows: np.ndarray):
    """Row r of S is routed to key perm_rows[r]: it leads every other key by >= 12 log2 units, and all |S| <= 64."""
    assert np.abs(S).max() <= 64.0, np.abs(S).max()
    rows = np.arange(len(S))
    lead = S[rows, perm_rows].copy()
    rest = S.copy()
    rest[rows, perm_rows] = -np.inf
    gap = lead - rest.max(axis=1)
    assert gap.min() >= 12.0, gap.min()
    return float(gap.min())


def assert_routing_window(S: np.ndarray, target_slot: np.ndarray):
    """S [25, 224, 224]: every real query's designated key (the pad keys together, where it is a pad token) leads every
    other key by >= 12 log2 units; all finite |S| of real queries <= 64."""
    token, _, _ = window_slots()
    worst = np.inf
    for w in range(NW * NW):
        for s in np.nonzero(target_slot[w] > -2)[0]:
            row = S[w, s]
            mine = (token[w] == -1) if target_slot[w, s] == -1 else (np.arange(SLOTS) == target_slot[w, s])
            assert mine.any()
            assert np.abs(row[np.isfinite(row)]).max() <= 64.0
            worst = min(worst, row[mine].min() - row[~mine].max())
    assert worst >= 12.0, worst
    return float(worst)


def assert_rescale_global(S_rows: Dict[int, np.ndarray], stairs) -> Dict[int, List[int]]:
    """S_rows: designated query token -> its row of S [4096].  The designated queries together cover every raise
    position of the global kernel that the issue lists; every step is at most 40 log2 units."""
    toks = sorted(S_rows)
    S = np.stack([S_rows[t] for t in toks])
    m, raises = reference_track(S, GLOBAL_TILE)
    got = dict(zip(toks, raises))
    for tok, steps in stairs.items():
        assert [t for t, _, _ in steps] == got[tok], (tok, got[tok])       # exactly the planted staircase, nothing else
        for t, kx, _ in steps:                                             # ... and the planted key is what forces it
            assert int(np.argmax(S_rows[tok][t * GLOBAL_TILE:(t + 1) * GLOBAL_TILE])) == kx, (tok, t)
    assert np.diff(m, axis=1).max() <= 40.0 and np.diff(m, axis=1).min() >= 0.0
    every = [t for r in raises for t in r]
    assert 1 in every and 63 in every
    assert {t % 3 for t in every} == {0, 1, 2}
    assert any(b == a + 1 for r in raises for a, b in zip(r, r[1:])), "two consecutive tiles"
    assert max(len(r) for r in raises) >= 3
    assert any(t % 256 < 128 for t in toks) and any(t % 256 >= 128 for t in toks), "both groups of four waves"
    assert any(a != b and a // 32 == b // 32 and set(got[a]) != set(got[b]) for a in toks for b in toks), \
        "two queries of one wave raising at different tiles"
    forcing = [kx for steps in stairs.values() for _, kx, _ in steps]
    assert min(forcing) < 32 <= max(forcing), "both halves of the key columns"
    return got


def assert_no_forced_raise(S: np.ndarray, planted: np.ndarray):
    """No raise at the limit: planted keys 7 to 7.9 log2 units above the tile-0 maximum, nothing else above it; the rule
    forces nothing; P (relative to the tile-0 maximum) reaches 2^7.8 and the row sum exceeds 2^12."""
    m0 = S[:, :GLOBAL_TILE].max(axis=1, keepdims=True)
    rel = S - m0
    assert rel[:, planted].min() >= 7.0 and rel[:, planted].max() <= 7.9, (rel[:, planted].min(), rel[:, planted].max())
    other = np.delete(rel, planted, axis=1)
    assert other.max() <= 0.0
    assert len(set(int(p) // GLOBAL_TILE for p in planted)) >= 32, "planted in many tiles"
    assert all(r == [] for r in forced_raises(S, GLOBAL_TILE))
    assert np.exp2(rel).max() >= 2.0 ** 7.8 and np.exp2(rel).sum(axis=1).min() >= 2.0 ** 12


def assert_f16_edge(S: np.ndarray):
    """The row maximum is in tile 0; the keys 13 to 16 log2 units below it carry at least a quarter of the mass, and there
    is nothing else but the maximum itself."""
    m = S.max(axis=1, keepdims=True)
    assert (S[:, :GLOBAL_TILE].max(axis=1, keepdims=True) == m).all()
    rel = S - m
    low = (rel <= -13.0) & (rel >= -16.0)
    assert ((rel == 0.0) | low).all() and ((rel == 0.0).sum(axis=1) == 1).all()
    P = np.exp2(rel)
    share = (P * low).sum(axis=1) / P.sum(axis=1)
    assert share.min() >= 0.25, share.min()
    assert (rel < -14.0).mean() > 0.1, "a good part of P is below f16's smallest normal"
    assert all(r == [] for r in forced_raises(S, GLOBAL_TILE))
    return float(share.min())


def assert_shift(S: np.ndarray, queries: np.ndarray, offset, span: int, lead: float = 12.0) -> int:
    """Global (span 64, S [queries, 4096]): wherever the key at (qy + dy, qx + dx) exists it leads every other key by
    `lead` log2 units.  Returns how many of the queries have such a key."""
    dy, dx = offset
    qy, qx = queries // GRID, queries % GRID
    ky, kx = qy + dy, qx + dx
    ok = (ky >= 0) & (ky < span) & (kx >= 0) & (kx < span)
    rows = np.nonzero(ok)[0]
    key = ky[rows] * GRID + kx[rows]
    rest = S[rows].copy()
    rest[np.arange(len(rows)), key] = -np.inf
    assert (S[rows, key] - rest.max(axis=1)).min() >= lead
    return int(ok.sum())


def assert_shift_window(S: np.ndarray, offset, lead: float = 12.0) -> int:
    """Windowed (S [25, 224, 224]): wherever the slot at (ty + dy, tx + dx) is a key of the window (a real or a pad token) it
    leads every other key of a real query by `lead` log2 units."""
    token, ty, tx = window_slots()
    dy, dx = offset
    n = 0
    for w in range(NW * NW):
        for s in np.nonzero(token[w] >= 0)[0]:
            ky, kx = ty[s] + dy, tx[s] + dx
            if 0 <= ky < WS and 0 <= kx < WS:
                row = S[w, s].copy()
                top = row[ky * 16 + kx]
                row[ky * 16 + kx] = -np.inf
                assert top - row.max() >= lead, (w, s)
                n += 1
    return n


def assert_rescale_window(S: np.ndarray, case) -> Dict[int, List[int]]:
    """Every designated query is forced to raise exactly at its planted tiles; together: each of tiles 1 to 6, two or more
    raises for one query, a raise forced by a zero-padding key, one forced by the last real token of a window row."""
    token, ty, tx = window_slots()
    got = window_forced_raises(S)
    for tok, tiles in case["designated"].items():
        assert got.get(tok) == tiles, (tok, got.get(tok), tiles)
    every = {t for tok in case["designated"] for t in got[tok]}
    assert every >= {1, 2, 3, 4, 5, 6}
    assert max(len(got[tok]) for tok in case["designated"]) >= 2
    w, (qty, qtx), _ = WINDOW_PAD_RAISE                        # the forcing key of the pad raise is a pad token
    row = S[w, qty * 16 + qtx]
    assert token[w, int(np.argmax(row[4 * WINDOW_TILE:5 * WINDOW_TILE])) + 4 * WINDOW_TILE] == -1
    assert (token[w, :4 * WINDOW_TILE] != -1).all()
    last = [(w, q, k) for w, q, steps in WINDOW_STAIRS for k, _ in steps if k[1] == WS - 1 and w % NW < NW - 1]
    assert last, "a forcing key at tx = 13 of a window without padding on the right"
    for w, (qty, qtx), (kty, ktx) in last:
        row = S[w, qty * 16 + qtx]
        t = kty // 2
        assert int(np.argmax(row[t * WINDOW_TILE:(t + 1) * WINDOW_TILE])) + t * WINDOW_TILE == kty * 16 + ktx
    return got
