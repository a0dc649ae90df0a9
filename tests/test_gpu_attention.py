"""The two encoder attention kernels against float64 references on their own f16 operands, in units of the rounding the
kernels' contracts allow (tests/attention_ref.py: check() asserts rms <= 1.5 and max <= 2 times the rounding model's own
error), over every path of the lazy-maximum rescale.  The builders' conditions (what a case is meant to force) are
asserted on the float64 reference of the very inputs the kernel gets; tests/test_attention_ref.py shows on the CPU that
check() rejects the shortcuts and indexing mistakes a faster kernel might make.

Measured on an MI355X at the commit that added this file: rms(got - ref) / rms(model - ref) and
max|got - ref| / max|model - ref| (margins 1.5 and 2; every run logs them through conftest.within, with the other parity margins).

    case                                   hd 64: rms    max      hd 80: rms    max
    global diffuse, 1 image x 3 heads            1.065  1.000           1.075  1.083
    global diffuse, 2 images x 1 head            1.061  1.593           1.070  1.789
    window diffuse, 2 images x 3 heads           1.082  1.203           1.089  1.765
    global routing a = 2731 / a = 4093           1.000  1.000           1.000  1.000
    window routing a = 45 / a = 137              1.000  1.000           1.000  0.996
    global and window rel-pos shift, all 8       1.000  1.000           1.000  1.000
    global rescale coverage                      1.147  1.269           1.113  1.741
    global, no raise at the limit                1.000  1.000           0.993  1.000
    global, P at the edge of f16                 1.000  1.000           1.000  1.000
    window rescale coverage                      1.006  1.126           1.006  1.000

No rounding had to be added to the model, and no test exposed a kernel error.  Where one key carries the row (routing,
shift, the planted-key cases) the only error left is the f16 rounding of the output, and the kernels agree with the model
bit for bit almost everywhere.  On diffuse rows the kernels sit 6 to 9 % above the model in rms (figures above: from the
commit that added this file).  Most of that was one rounding the model's "exact quotient" leaves out: both kernels summed the
row's l from the fp32 probabilities BEFORE these are rounded to f16 for the second MFMA, so the rounding of a p did not cancel
between numerator and denominator as it does in the model.  Inside these margins -- but behind the output's own f16 rounding
the error it leaves grows with |output| / spread of V, and the encoder chain's staged check (tests/test_gpu_encoder.py, S2)
measured 1.5 to 3.1 times the model's error where V has a mean of order one.  The kernels now sum the ROUNDED probabilities
(v_dot2_f32_f16 with ones); test_row_sum_is_that_of_the_rounded_probabilities holds them to it on such values.
f16-subnormal P is KEPT by the GPU (v_cvt_f16_f32 and the f16 MFMA both honour subnormals
here): test_global_p_at_the_edge_of_f16 puts 1.8 % of the softmax mass on P below 2^-14 and measures 1.000.
"""
import numpy as np
import pytest

import attention_ref as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from dlimgedit_amd import api
    assert api.ext.device_count() >= 1, "no HIP device visible"
    assert api.Environment.is_supported(api.Backend.gpu), "GPU backend must be supported on the GPU box"
    return api.ext


def _run(ext, is_global, case):
    got = ext.test_attention(is_global, case["qkv"], case["bias"], case["rel_h"], case["rel_w"], case["batch"],
                             case["heads"], case["hd"])
    assert np.isfinite(got.astype(np.float32)).all()
    return got


def _global_ops(case):
    return A.global_operands(case["qkv"], case["rel_h"], case["rel_w"], case["batch"], case["heads"], case["hd"])


def _global_parts(case, ops, got, b, h, queries=None):
    """(got, ref, model, S) of one (image, head) on a subset of its queries."""
    S, V = A.global_scores(ops, b, h, queries), ops["v"][b, h]
    return (A.head_columns(got, case["batch"], case["heads"], case["hd"], b, h, queries), A.softmax2(S, V),
            A.rounding_model(S, V, A.GLOBAL_TILE), S)


def _window_parts(case, ops, got, b, h):
    S, V = A.window_scores(ops, b, h), ops["v"][b, h]
    return (A.head_columns(got, case["batch"], case["heads"], case["hd"], b, h), A.window_apply(S, V, A.softmax2),
            A.window_apply(S, V, lambda s, v: A.rounding_model(s, v, A.WINDOW_TILE)), S)


def _window_ops(case):
    return A.window_operands(case["qkv"], case["bias"], case["rel_h"], case["rel_w"], case["batch"], case["heads"],
                             case["hd"])


# ------------------------------------------------------------------------------- 1. diffuse parity

@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("batch,heads", [(1, 3), (2, 1)])
def test_global_diffuse(ext, hd, batch, heads):
    """Gaussian qkv, 0.2-sigma tables.  Reference on every (image, head), each on a quarter of its queries (every 4th,
    starting at a different token, so every lane and wave position is covered across the heads)."""
    case = A.diffuse_case(True, hd, heads, batch)
    got, ops = _run(ext, True, case), _global_ops(case)
    parts = [_global_parts(case, ops, got, b, h, np.arange((b * heads + h) % 4, A.TOKENS, 4))[:3]
             for b in range(batch) for h in range(heads)]
    A.check(f"attn global diffuse hd{hd} b{batch} h{heads}", *(np.concatenate(x) for x in zip(*parts)))


@pytest.mark.parametrize("hd", [64, 80])
def test_window_diffuse(ext, hd):
    """Gaussian qkv, bias and tables; two images, three heads, every window and query of all six."""
    case = A.diffuse_case(False, hd, heads=3, batch=2)
    got, ops = _run(ext, False, case), _window_ops(case)
    parts = [_window_parts(case, ops, got, b, h)[:3] for b in range(2) for h in range(3)]
    A.check(f"attn window diffuse hd{hd} b2 h3", *(np.concatenate(x) for x in zip(*parts)))


# --------------------------------------------------------------------------------------- 2. routing

@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("a,b,heads", A.ROUTING_GLOBAL)
def test_global_routing(ext, hd, a, b, heads):
    """Every query attends to one key, perm(i) = (a i + b) mod 4096 (another b per head); V rows are all different, so
    a misrouted key, tile, lane or head is an error of order one."""
    case = A.routing_global_case(hd, a, b, heads)
    got, ops = _run(ext, True, case), _global_ops(case)
    parts = []
    for h in range(heads):
        g, ref, model, S = _global_parts(case, ops, got, 0, h)
        A.assert_routing_global(S, case["perm"][h])
        assert np.abs(ref - ops["v"][0, h][case["perm"][h]]).max() < 0.05      # the reference IS the routed row (a wrong row: order one)
        parts.append((g, ref, model))
    A.check(f"attn global routing hd{hd} a{a} h{heads}", *(np.concatenate(x) for x in zip(*parts)))


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("a,b", A.ROUTING_WINDOW)
def test_window_routing(ext, hd, a, b):
    """A bijection inside each window's 196 positions; where the designated position is a zero-padding token the query
    attends to the pad tokens (they share the bias's k part) and the expected output is the bias's v part."""
    case = A.routing_window_case(hd, a, b)
    got, ops = _run(ext, False, case), _window_ops(case)
    g, ref, model, S = _window_parts(case, ops, got, 0, 0)
    A.assert_routing_window(S, case["target_slot"])
    to_pad = ops["token"][case["target_slot"] == -1]
    bias_v = case["bias"][2 * hd:].astype(np.float64)
    assert len(to_pad) > 0 and np.abs(ref[to_pad] - bias_v).max() < 0.05
    A.check(f"attn window routing hd{hd} a{a}", g, ref, model)


# -------------------------------------------------------------------------------- 3. rel-pos shift

@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("d,e", A.SHIFT_GLOBAL)
def test_global_relpos_shift(ext, hd, d, e):
    """Equal queries, zero keys: the bias alone routes every query to the key at a fixed offset (table rows d of rel_h, e
    of rel_w: the table ends 0 and 126, the centre 63, and an interior pair); at the borders the reference decides.
    Reference on every third query (3 is coprime to 64: every row, column, lane and wave)."""
    case = A.shift_case(True, hd, d, e)
    got, ops = _run(ext, True, case), _global_ops(case)
    q = np.arange(0, A.TOKENS, 3)
    g, ref, model, S = _global_parts(case, ops, got, 0, 0, q)
    assert A.assert_shift(S, q, case["offset"], A.GRID) > 0
    A.check(f"attn global shift hd{hd} d{d} e{e}", g, ref, model)


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("d,e", A.SHIFT_WINDOW)
def test_window_relpos_shift(ext, hd, d, e):
    """The same inside the windows: table rows 0, 13, 26 and an interior pair; the offset key may be a pad token."""
    case = A.shift_case(False, hd, d, e)
    got, ops = _run(ext, False, case), _window_ops(case)
    g, ref, model, S = _window_parts(case, ops, got, 0, 0)
    assert A.assert_shift_window(S, case["offset"]) > 0
    A.check(f"attn window shift hd{hd} d{d} e{e}", g, ref, model)


# ------------------------------------------------------------------- 4. - 6. the lazy-maximum rescale

@pytest.mark.parametrize("hd", [64, 80])
def test_global_rescale_coverage(ext, hd):
    """Staircase keys (attention_ref.GLOBAL_STAIRS) with non-zero tables: raises at tile 1 and 63, at tiles of all three
    residues mod 3, at consecutive tiles, three and four for one query, in both groups of four waves, at different tiles
    for two queries of one wave, forced from both halves of the key columns."""
    case = A.rescale_global_case(hd)
    got, ops = _run(ext, True, case), _global_ops(case)
    g, ref, model, S = _global_parts(case, ops, got, 0, 0)
    A.assert_rescale_global({t: S[t] for t in case["stairs"]}, case["stairs"])
    A.check(f"attn global rescale hd{hd}", g, ref, model)


@pytest.mark.parametrize("hd", [64, 80])
def test_global_no_raise_at_the_limit(ext, hd):
    """Planted keys 7 to 7.9 log2 units above the tile-0 maximum in 48 tiles: no raise is forced, P reaches 2^7.9.
    Reference on every fifth query."""
    case = A.no_raise_limit_case(hd)
    got, ops = _run(ext, True, case), _global_ops(case)
    g, ref, model, S = _global_parts(case, ops, got, 0, 0, np.arange(0, A.TOKENS, 5))
    A.assert_no_forced_raise(S, case["planted"])
    A.check(f"attn global no-raise hd{hd}", g, ref, model)


@pytest.mark.parametrize("hd", [64, 80])
def test_global_p_at_the_edge_of_f16(ext, hd):
    """The maximum in tile 0 and more than a quarter of the mass on keys 13 to 16 log2 units below it, P from 2^-13 down
    to 2^-16 around f16's smallest normal 2^-14.  The GPU keeps f16-subnormal P (as numpy's rounding does): flushed
    to zero, the 1.8 % of the mass that lies below 2^-14 would be an error of some 90 units (CPU model,
    test_attention_ref.py::test_check_rejects_flushed_subnormal_p); measured 1.000."""
    case = A.f16_edge_case(hd)
    got, ops = _run(ext, True, case), _global_ops(case)
    g, ref, model, S = _global_parts(case, ops, got, 0, 0, np.arange(0, A.TOKENS, 5))
    A.assert_f16_edge(S)
    A.check(f"attn global f16-edge hd{hd}", g, ref, model)


@pytest.mark.parametrize("hd", [64, 80])
def test_window_rescale_coverage(ext, hd):
    """Planted keys (attention_ref.WINDOW_STAIRS): a forced raise at each of key tiles 1 to 6, two and three for one query,
    one forced by a zero-padding key (the bias's k part aligned with a query of window (4, 0)) and one by the last real
    token of a window row, whose K row the two dummy slots behind it read."""
    case = A.rescale_window_case(hd)
    got, ops = _run(ext, False, case), _window_ops(case)
    g, ref, model, S = _window_parts(case, ops, got, 0, 0)
    A.assert_rescale_window(S, case)
    A.check(f"attn window rescale hd{hd}", g, ref, model)


@pytest.mark.parametrize("is_global", [True, False])
def test_row_sum_is_that_of_the_rounded_probabilities(ext, is_global):
    """The narrowest case of what the encoder chain's S2 found.  Diffuse attention over values with a common part: v = N(0, 1) + 4
    in every channel.  With numerator and denominator taken from the SAME f16-rounded probabilities, their rounding errors cancel in
    the common part; a row sum of the fp32 probabilities leaves an error of |output| x the relative error of the sum.  Behind
    the output's own f16 rounding (the reference rounded ONCE to f16, as S2 does) only the roundings in front of it remain:
    measured there, the kernel may need RMS_MARGIN / MAX_MARGIN times the rounding model's error and no more."""
    from conftest import within
    hd = 64
    case = A.diffuse_case(is_global, hd, seed=61)
    qkv = case["qkv"].copy()
    qkv[:, 2 * hd:] = (qkv[:, 2 * hd:].astype(np.float32) + 4).astype(np.float16)
    case["qkv"] = qkv
    got = A.head_columns(_run(ext, is_global, case), 1, 1, hd, 0, 0)
    if is_global:
        queries = np.arange(0, A.TOKENS, 8)
        r = A.global_reference(qkv, case["rel_h"], case["rel_w"], 1, 1, hd, 0, 0, queries)
        got = got[queries]
    else:
        r = A.window_reference(qkv, case["bias"], case["rel_h"], case["rel_w"], 1, 1, hd)
    once = A.round_f16(r["ref"])
    assert np.abs(r["ref"]).mean() > 3.5, "the common part is there"
    unit_rms, unit_max = A.rms(r["model"] - once), np.abs(r["model"] - once).max()
    assert unit_rms > 0
    name = f"attention {'global' if is_global else 'window'} common-part values behind the output rounding"
    try:
        within(name + " rms/model", A.rms(got - once) / unit_rms, np.nextafter(A.RMS_MARGIN, 2.0))
    finally:
        within(name + " max/model", np.abs(got - once).max() / unit_max, np.nextafter(A.MAX_MARGIN, 3.0))
