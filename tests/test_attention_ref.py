"""CPU tests of tests/attention_ref.py: the float64 references against the fp32 oracle, check() against modified models
(the evidence that tests/test_gpu_attention.py would fail on a subtly wrong kernel), and every input builder's stated
conditions on the reference alone.  Nothing here touches a GPU.

How the residual against the fp32 oracle is bounded.  If every logit of a softmax row is perturbed by at most d (natural
units), every probability changes by a factor inside [e^-2d, e^2d], so the output moves by at most
(e^2d - 1) * sum_j p_j |v_j - o| per column (A).  For the fp32 oracle, d is the rounding of its three fp32 dot products and
the additions, d <= 2^-24 * ((hd + 4) * sum|terms| + 8 max|S|); its exponentials, row sum, quotient and the n-term
fp32 product P @ V add at most (n + 64) * 2^-24 * sum_j p_j |v_j| (B).  The test asserts |ref64 - oracle| <= A + B per
element.  The windowed kernel's operands are the oracle's, so that is the whole residual.  The global kernel's contract
re-rounds its operands (q' = f16(q * qs), R' = f16(R * sqrt(hd)), 2^-11 relative each), which the oracle's raw operands
lack: that part is bounded by (A) with d = ln 2 * (2^-11 |q'|.|k| + 2^-10 (|q'|.|R'h| + |q'|.|R'w|)), against a float64
evaluation on the oracle's own operands.  Both bounds are worst-case sums, so the measured residuals (printed) sit one to
two orders of magnitude below them."""
import numpy as np
import pytest

import attention_ref as A
from attention_ref import f16, f32, f64

SUB = np.arange(0, A.TOKENS, 8)             # "every 8th query" of the issue's table


def _oracle():
    from oracle import sam_oracle as O
    return O


def _spread(P, V, out):
    """sum_j p_j |v_j - o| per (query, column), without the [q, k, d] cube: sum p|v - o| <= sum p|v| + |o|."""
    return P @ np.abs(V) + np.abs(out)


# ---------------------------------------------------------------------- the references against the oracle

@pytest.fixture(scope="module")
def global_parity_inputs():
    """test_attention_global_parity's inputs (seed 3 / 4), head 0 of its two heads."""
    out = {}
    for hd in (64, 80):
        qkv, _ = A.gaussian_qkv(3, 2, hd)
        rel_h, rel_w = A.gaussian_tables(4, A.GRID, hd)
        D = 2 * hd
        one = np.ascontiguousarray(np.concatenate([qkv[:, 0:hd], qkv[:, D:D + hd], qkv[:, 2 * D:2 * D + hd]], axis=1))
        out[hd] = (one, rel_h, rel_w)
    return out


@pytest.mark.parametrize("hd", [64, 80])
def test_global_reference_agrees_with_fp32_oracle(global_parity_inputs, hd):
    O = _oracle()
    qkv, rel_h, rel_w = global_parity_inputs[hd]
    rh16, rw16 = rel_h.astype(f16).astype(f32), rel_w.astype(f16).astype(f32)
    oracle = O.attention_from_qkv(qkv.astype(f32)[None], rh16, rw16, 1, 64)[0][SUB].astype(f64)

    # float64 on the ORACLE's operands: raw q, scale on q.k only, tables f16(rel)
    q, k, v = (qkv[:, i * hd:(i + 1) * hd].astype(f64) for i in range(3))
    qq = q[SUB]
    kk = np.arange(64)
    row = np.take_along_axis(qq @ rh16.astype(f64).T, (SUB // 64)[:, None] - kk[None, :] + 63, axis=1)
    col = np.take_along_axis(qq @ rw16.astype(f64).T, (SUB % 64)[:, None] - kk[None, :] + 63, axis=1)
    S_nat = ((qq @ k.T) / np.sqrt(f64(hd))).reshape(-1, 64, 64) + row[:, :, None] + col[:, None, :]
    S_nat = S_nat.reshape(len(SUB), A.TOKENS)
    raw, P = A.softmax2(S_nat * A.LOG2E, v, want_p=True)

    a_qk = (np.abs(qq) @ np.abs(k).T) / np.sqrt(f64(hd))
    a_h = (np.abs(qq) @ np.abs(rh16.astype(f64)).T).max(axis=1, keepdims=True)
    a_w = (np.abs(qq) @ np.abs(rw16.astype(f64)).T).max(axis=1, keepdims=True)
    d = 2.0 ** -24 * ((hd + 4) * (a_qk + a_h + a_w).max(axis=1, keepdims=True) + 8 * np.abs(S_nat).max(axis=1, keepdims=True))
    bound_fp32 = np.expm1(2 * d) * _spread(P, v, raw) + (A.TOKENS + 64) * 2.0 ** -24 * (P @ np.abs(v))
    res = np.abs(raw - oracle)
    print(f"global hd {hd}: float64 on the oracle's operands vs oracle: max {res.max():.3g}, bound {bound_fp32.max():.3g}")
    assert (res <= bound_fp32).all()

    # the contract's operands against the oracle's: 2^-11 per re-rounded operand
    ops = A.global_operands(qkv, rel_h, rel_w, 1, 1, hd)
    S = A.global_scores(ops, 0, 0, SUB)
    ref = A.softmax2(S, ops["v"][0, 0])
    qp = np.abs(ops["q"][0, 0][SUB])
    d_ops = np.log(2.0) * (2.0 ** -11 * (qp @ np.abs(k).T).max(axis=1, keepdims=True)
                           + 2.0 ** -10 * ((qp @ np.abs(ops["rh"]).T).max(axis=1, keepdims=True)
                                           + (qp @ np.abs(ops["rw"]).T).max(axis=1, keepdims=True))) * (1 + 2.0 ** -10)
    bound_ops = np.expm1(2 * d_ops) * _spread(P, v, raw)
    res = np.abs(ref - raw)
    print(f"global hd {hd}: contract operands vs the oracle's operands: max {res.max():.3g}, bound {bound_ops.max():.3g}")
    assert (res <= bound_ops).all()
    assert (np.abs(ref - oracle) <= bound_ops + bound_fp32).all()


@pytest.mark.parametrize("hd", [64, 80])
def test_window_reference_agrees_with_fp32_oracle(hd):
    """test_attention_window_parity's inputs (seed 1 / 2), head 0 of its two heads; same operands on both sides."""
    O = _oracle()
    qkv2, bias2 = A.gaussian_qkv(1, 2, hd)
    rel_h, rel_w = A.gaussian_tables(2, A.WS, hd)
    D = 2 * hd
    cols = np.r_[0:hd, D:D + hd, 2 * D:2 * D + hd]
    qkv, bias = np.ascontiguousarray(qkv2[:, cols]), bias2[cols]
    rh16, rw16 = rel_h.astype(f16).astype(f32), rel_w.astype(f16).astype(f32)
    oracle = O.windowed_attention_from_qkv(qkv.astype(f32), bias.astype(f16).astype(f32), rh16, rw16, 1).astype(f64)
    r = A.window_reference(qkv, bias, rel_h, rel_w, 1, 1, hd)
    ops = A.window_operands(qkv, bias, rel_h, rel_w, 1, 1, hd)
    q, k = np.abs(ops["q"][0, 0]), np.abs(ops["k"][0, 0])
    terms = (q @ k.transpose(0, 2, 1)) / np.sqrt(f64(hd)) + (q @ np.abs(ops["rh"]).T).max(axis=2, keepdims=True) \
        + (q @ np.abs(ops["rw"]).T).max(axis=2, keepdims=True)
    S_nat = np.where(np.isfinite(r["S"]), r["S"], 0.0) / A.LOG2E
    d = 2.0 ** -24 * ((hd + 4) * terms.max(axis=2, keepdims=True) + 8 * np.abs(S_nat).max(axis=2, keepdims=True))

    def bound_w(w):
        out, P = A.softmax2(r["S"][w], r["V"][w], want_p=True)
        return np.expm1(2 * d[w]) * _spread(P, r["V"][w], out) + (196 + 64) * 2.0 ** -24 * (P @ np.abs(r["V"][w]))
    bound = A.window_gather(np.stack([bound_w(w) for w in range(25)]))
    res = np.abs(r["ref"] - oracle)
    print(f"window hd {hd}: float64 vs oracle: max {res.max():.3g}, bound {bound.max():.3g}")
    assert (res <= bound).all()


# ------------------------------------------------------------------------ check() against modified models

def _verdict(name, got, ref, model):
    """check()'s verdict with the figures printed beside the margins."""
    r_rms = A.rms(got - ref) / A.rms(model - ref)
    r_max = np.abs(got - ref).max() / np.abs(model - ref).max()
    print(f"{name}: rms ratio {r_rms:.3f} (margin {A.RMS_MARGIN}), max ratio {r_max:.3f} (margin {A.MAX_MARGIN})")
    try:
        A.check("cpu model " + name, got, ref, model)
    except AssertionError:
        return False
    return True


@pytest.fixture(scope="module")
def global_base(global_parity_inputs):
    qkv, rel_h, rel_w = global_parity_inputs[64]
    ops = A.global_operands(qkv, rel_h, rel_w, 1, 1, 64)
    S, V = A.global_scores(ops, 0, 0, SUB), ops["v"][0, 0]
    return ops, S, V, A.softmax2(S, V), A.rounding_model(S, V, A.GLOBAL_TILE)


def test_rounding_model_matches_the_issue_figures(global_base):
    """The issue's numpy figures for "the kernel's roundings" on these inputs: 4.7e-4 max, 3.6e-5 rms."""
    _, _, _, ref, model = global_base
    print(f"global model: max {np.abs(model - ref).max():.3g}, rms {A.rms(model - ref):.3g}")
    assert 3.5e-4 < np.abs(model - ref).max() < 6e-4 and 3e-5 < A.rms(model - ref) < 4.2e-5


def test_check_accepts_the_model_itself(global_base):
    _, _, _, ref, model = global_base
    assert _verdict("global plain model", model, ref, model)


GLOBAL_VARIANTS = ["row_bias_f16", "col_bias_f16", "scores_f16", "p_bf16", "one_key_dropped", "last_tile_dropped",
                   "tables_swapped", "clamp_kx63"]


@pytest.mark.parametrize("variant", GLOBAL_VARIANTS)
def test_check_rejects_modified_global_model(global_base, variant):
    ops, S, V, ref, model = global_base
    if variant == "p_bf16":
        got = A.rounding_model(S, V, A.GLOBAL_TILE, round_p=A.round_bf16)
    elif variant == "one_key_dropped":
        S2 = S.copy()
        S2[:, 2077] = -np.inf
        got = A.rounding_model(S2, V, A.GLOBAL_TILE)
    elif variant == "last_tile_dropped":
        S2 = S.copy()
        S2[:, -A.GLOBAL_TILE:] = -np.inf
        got = A.rounding_model(S2, V, A.GLOBAL_TILE)
    else:
        got = A.rounding_model(A.global_scores(ops, 0, 0, SUB, variant=variant), V, A.GLOBAL_TILE)
    assert not _verdict("global " + variant, got, ref, model)


@pytest.fixture(scope="module")
def window_base():
    qkv2, bias2 = A.gaussian_qkv(1, 2, 64)
    rel_h, rel_w = A.gaussian_tables(2, A.WS, 64)
    cols = np.r_[0:64, 128:192, 256:320]
    qkv, bias = np.ascontiguousarray(qkv2[:, cols]), bias2[cols]
    ops = A.window_operands(qkv, bias, rel_h, rel_w, 1, 1, 64)
    r = A.window_reference(qkv, bias, rel_h, rel_w, 1, 1, 64)
    return ops, r


def test_window_model_figures_and_self_acceptance(window_base):
    """The issue's figures for the windowed kernel's modelled rounding error: 6e-4 max, 7.5e-5 rms
    (here, over all queries of head 0: 1.1e-3 and 8.4e-5)."""
    _, r = window_base
    print(f"window model: max {np.abs(r['model'] - r['ref']).max():.3g}, rms {A.rms(r['model'] - r['ref']):.3g}")
    assert 4e-4 < np.abs(r["model"] - r["ref"]).max() < 1.5e-3 and 6e-5 < A.rms(r["model"] - r["ref"]) < 1e-4
    assert _verdict("window plain model", r["model"], r["ref"], r["model"])


WINDOW_VARIANTS = ["pad_keys_masked", "dummies_are_keys", "row_bias_f16", "col_bias_f16", "p_bf16", "one_key_dropped",
                   "last_tile_dropped", "tables_swapped"]


@pytest.mark.parametrize("variant", WINDOW_VARIANTS)
def test_check_rejects_modified_window_model(window_base, variant):
    ops, r = window_base
    model_fn = lambda s, v: A.rounding_model(s, v, A.WINDOW_TILE)
    S, V = r["S"], r["V"]
    if variant == "p_bf16":
        got = A.window_apply(S, V, lambda s, v: A.rounding_model(s, v, A.WINDOW_TILE, round_p=A.round_bf16))
    elif variant == "one_key_dropped":
        S2 = S.copy()
        S2[:, :, 5 * 16 + 6] = -np.inf
        got = A.window_apply(S2, V, model_fn)
    elif variant == "last_tile_dropped":
        S2 = S.copy()
        S2[:, :, -A.WINDOW_TILE:] = -np.inf
        got = A.window_apply(S2, V, model_fn)
    else:
        got = A.window_apply(A.window_scores(ops, 0, 0, variant=variant), V, model_fn)
    assert not _verdict("window " + variant, got, r["ref"], r["model"])


# ---------------------------------------------------------------- the builders' conditions, reference alone

def _global_S(case, queries=None, h=0):
    ops = A.global_operands(case["qkv"], case["rel_h"], case["rel_w"], case["batch"], case["heads"], case["hd"])
    return A.global_scores(ops, 0, h, queries)


def _window_S(case):
    ops = A.window_operands(case["qkv"], case["bias"], case["rel_h"], case["rel_w"], 1, 1, case["hd"])
    return A.window_scores(ops, 0, 0)


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("a,b,heads", A.ROUTING_GLOBAL)
def test_routing_global_conditions(hd, a, b, heads):
    case = A.routing_global_case(hd, a, b, heads)
    for h in range(heads):
        assert sorted(case["perm"][h]) == list(range(A.TOKENS))
        print("lead", A.assert_routing_global(_global_S(case, SUB, h), case["perm"][h][SUB]))


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("a,b", A.ROUTING_WINDOW)
def test_routing_window_conditions(hd, a, b):
    case = A.routing_window_case(hd, a, b)
    ts = case["target_slot"]
    assert (ts == -1).any(), "some designated keys are pad tokens"
    for w in range(25):                                     # a bijection of the window's real and pad positions
        real = ts[w][ts[w] >= 0]
        assert len(set(real)) == len(real)
    print("lead", A.assert_routing_window(_window_S(case), ts))


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("d,e", A.SHIFT_GLOBAL)
def test_shift_global_conditions(hd, d, e):
    case = A.shift_case(True, hd, d, e)
    assert d != e and case["offset"][0] != case["offset"][1]
    q = np.arange(0, A.TOKENS, 3)
    n = A.assert_shift(_global_S(case, q), q, case["offset"], A.GRID)
    assert n > 0
    assert np.abs(case["qkv"][:, hd:2 * hd]).max() == 0 and (case["qkv"][:, :hd] == case["qkv"][0, :hd]).all()


def test_shift_offsets_cover_the_table_ends():
    for pairs, span in ((A.SHIFT_GLOBAL, A.GRID), (A.SHIFT_WINDOW, A.WS)):
        for axis in (0, 1):
            assert {0, span - 1, 2 * span - 2} <= {p[axis] for p in pairs}


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("d,e", A.SHIFT_WINDOW)
def test_shift_window_conditions(hd, d, e):
    case = A.shift_case(False, hd, d, e)
    assert A.assert_shift_window(_window_S(case), case["offset"]) > 0
    assert np.abs(case["bias"][hd:2 * hd]).max() == 0


@pytest.mark.parametrize("hd", [64, 80])
def test_rescale_global_conditions(hd):
    case = A.rescale_global_case(hd)
    assert np.abs(case["rel_h"]).max() > 0 and np.abs(case["rel_w"]).max() > 0
    toks = np.array(sorted(case["stairs"]))
    S = _global_S(case, toks)
    print(A.assert_rescale_global(dict(zip(toks.tolist(), S)), case["stairs"]))


@pytest.mark.parametrize("hd", [64, 80])
def test_no_raise_limit_conditions(hd):
    case = A.no_raise_limit_case(hd)
    A.assert_no_forced_raise(_global_S(case, np.arange(0, A.TOKENS, 7)), case["planted"])


@pytest.mark.parametrize("hd", [64, 80])
def test_f16_edge_conditions(hd):
    case = A.f16_edge_case(hd)
    print("share", A.assert_f16_edge(_global_S(case, np.arange(0, A.TOKENS, 16))))


def test_check_rejects_flushed_subnormal_p():
    """On the f16-edge inputs a kernel that flushed f16-subnormal P to zero would lose 1.8 % of the mass: ~90 units."""
    case = A.f16_edge_case(64)
    ops = A.global_operands(case["qkv"], case["rel_h"], case["rel_w"], 1, 1, 64)
    S, V = A.global_scores(ops, 0, 0, np.arange(0, A.TOKENS, 16)), ops["v"][0, 0]
    flush = lambda x: np.where(A.round_f16(x) < 2.0 ** -14, 0.0, A.round_f16(x))
    got = A.rounding_model(S, V, A.GLOBAL_TILE, round_p=flush)
    assert not _verdict("global f16-edge, subnormal P flushed", got, A.softmax2(S, V), A.rounding_model(S, V, A.GLOBAL_TILE))


@pytest.mark.parametrize("hd", [64, 80])
def test_rescale_window_conditions(hd):
    case = A.rescale_window_case(hd)
    print(A.assert_rescale_window(_window_S(case), case))


def test_forced_raises_rule():
    """The rule itself on a hand-made row: reference = tile-0 maximum; > 8 above forces, exactly 8 does not; the reference
    then is the tile's maximum."""
    S = np.zeros((1, 5 * 4))
    S[0, 4] = 8.0           # tile 1: exactly 8 above: not forced
    S[0, 9] = 8.5           # tile 2: forced, reference 8.5
    S[0, 13] = 16.0         # tile 3: 7.5 above the new reference: not forced
    S[0, 17] = 17.0         # tile 4: 8.5 above: forced
    assert A.forced_raises(S, 4) == [[2, 4]]
    m, _ = A.reference_track(S, 4)
    assert m.tolist() == [[0.0, 0.0, 8.5, 8.5, 17.0]]
