"""The measure of tests/test_gpu_row_kernels.py, shown to work before it judges a kernel (no GPU): on the hard inputs of the GPU
tests the fp32 yardsticks of tests/row_ref.py pass check / check_f16 against the float64 reference, a third correct evaluation
(another pairing of the partial sums, the scale and shift as one fused multiply-add) passes too, and every modified model -- each a
mistake a row LayerNorm could make that test_layernorm_parity's 2e-5 on N(1, 3) rows lets through -- needs at least 3 times the
allowance on the input that is there to expose it:

    modified model          exposed by     why the other input cannot see it
    one-pass variance       offset rows    near-eps rows have a mean of 0.01: E[x^2] - mean^2 loses nothing there
    eps = 1e-5              near-eps rows  offset rows have a variance of 1: eps changes rstd by 5e-6 relative, below the yardsticks' own
                                           error there (the mean of 1000 costs them 1e-4)
    unbiased variance       near-eps rows  (and offset rows at small D; at D = 1280 the change of 4e-4 is inside the yardsticks' error)
    tanh-form GELU          near-eps rows  offset rows: 4.7e-4 against yardsticks that are off by 1e-3

Every figure is printed.  Also: the conditions the inputs promise, the rounding cases of cast_values, and that place_map names
every place."""
import numpy as np
import pytest

import gemm_ref as G
import row_ref as R

f16, f32, f64 = np.float16, np.float32, np.float64

REJECT = 3.0                # a modified model counts as rejected at 3 times the allowance or more


def _adjacent_tree_sum(v32) -> np.ndarray:
    """64 partial sums of stride 64, then neighbours added first (lane 2 i with 2 i + 1, ...): another balanced tree."""
    v = np.asarray(v32, f32)
    rows, D = v.shape
    steps = -(-D // 64)
    padded = np.zeros((rows, steps * 64), f32)
    padded[:, :D] = v
    part = padded.reshape(rows, steps, 64).transpose(1, 0, 2)
    acc = np.zeros((rows, 64), f32)
    for p in part:
        acc = acc + p
    while acc.shape[1] > 1:
        acc = acc[:, 0::2] + acc[:, 1::2]
    return acc[:, 0]


def third_evaluation(x32, w, b, eps, act):
    """A correct fp32 LayerNorm that is neither yardstick: neighbour-first tree sums, (d * rstd) * w + b as one fused
    multiply-add (float64 product and sum, rounded once), the GELU as its formula."""
    v = np.asarray(x32, f32)
    D = v.shape[1]
    d = v - (_adjacent_tree_sum(v) / f32(D))[:, None]
    rstd = (f32(1) / np.sqrt(_adjacent_tree_sum(d * d) / f32(D) + f32(eps))).astype(f32)
    y = ((d * rstd[:, None]).astype(f64) * np.asarray(w, f32).astype(f64) + np.asarray(b, f32).astype(f64)).astype(f32)
    return R.gelu_steps_f32(y) if act else y


def _excess(name, got32, ref, yard, as_f16: bool) -> float:
    """How many times its allowance `got32` needs: the larger of rms and max over ALLOW * the larger yardstick (fp32 results), or
    the largest element-wise |got - ref| / f16_bound (f16 results)."""
    if as_f16:
        got = np.asarray(got32, f32).astype(f16).astype(f64)
        return float((np.abs(got - ref) / G.f16_bound(ref, yard)).max())
    model = R.round_f32(ref)
    g = G.ratios(got32, ref, model)
    bound = {k: max(G.ratios(y, ref, model)[k] for y in yard.values()) for k in g}
    return max(g[k] / (G.ALLOW * bound[k]) for k in g)


CASES = [(kind, D) for kind in ("offset", "near_eps") for D in (63, 256, 257, 1280)]


@pytest.mark.parametrize("kind,D", CASES)
def test_yardsticks_and_a_third_evaluation_pass(kind, D):
    w, b = R.affine(400 + D, D)
    x = R.rows_input(kind, 410 + D, 261, D)
    R.input_conditions(kind, x)
    for act in (0, 1):
        ref, yard = R.layernorm64(x, w, b, R.EPS, act), R.yardsticks(x, w, b, R.EPS, act)
        for name, y in yard.items():
            R.check_rows(f"row ref {kind} 261x{D} act{act} {name}", y, y.astype(f16), x, w, b, R.EPS, act, yard, ref)
        third = third_evaluation(x, w, b, R.EPS, act)
        R.check_rows(f"row ref {kind} 261x{D} act{act} third evaluation", third, third.astype(f16), x, w, b, R.EPS, act, yard, ref)


@pytest.mark.parametrize("rows,D", [(1, 63), (5, 1), (5, 63), (5, 65), (3, 256), (5, 1279), (261, 64), (261, 320)])
def test_third_evaluation_passes_on_the_small_gaussian_shapes(rows, D):
    """The smallest launches of the GPU test hold few elements, so the largest error is a noisy figure: a correct evaluation
    that is neither yardstick still stays inside the allowance on them."""
    w, b = R.affine(200 + D, D)
    x = R.rows_input("gaussian", 1000 * rows + D, rows, D)
    for act in (0, 1):
        if D == 1 and not act:
            assert np.array_equal(third_evaluation(x, w, b, R.EPS, act), np.broadcast_to(b, x.shape))
            continue
        third = third_evaluation(x, w, b, R.EPS, act)
        R.check_rows(f"row ref gaussian {rows}x{D} act{act} third evaluation", third, third.astype(f16), x, w, b, R.EPS, act)


# modified model -> (input that exposes it, act, builder of its fp32 result)
MODIFIED = {
    "one-pass variance": ("offset", 0, lambda x, w, b: R.layernorm_one_pass_f32(x, w, b, R.EPS)),
    "eps 1e-5": ("near_eps", 0, lambda x, w, b: R.layernorm64(x, w, b, 1e-5).astype(f32)),
    "unbiased variance": ("near_eps", 0, lambda x, w, b: R.layernorm64(x, w, b, R.EPS, unbiased=True).astype(f32)),
    "tanh-form GELU": ("near_eps", 1, lambda x, w, b: R.layernorm64(x, w, b, R.EPS, 1, gelu="tanh").astype(f32)),
}


@pytest.mark.parametrize("D", [64, 256, 1280])
@pytest.mark.parametrize("name", sorted(MODIFIED))
def test_modified_models_are_rejected(name, D):
    """Each modified model on both hard inputs, as an fp32 and as an f16 result: at least REJECT times the allowance on the input
    that exposes it, in both formats.  The figures of the other input are printed, not asserted (the module's docstring)."""
    exposing, act, build = MODIFIED[name]
    w, b = R.affine(400 + D, D)
    for kind in ("offset", "near_eps"):
        x = R.rows_input(kind, 410 + D, 261, D)
        ref, yard = R.layernorm64(x, w, b, R.EPS, act), R.yardsticks(x, w, b, R.EPS, act)
        bad = build(x, w, b)
        e32, e16 = _excess(name, bad, ref, yard, False), _excess(name, bad, ref, yard, True)
        print(f"row ref modified: {name} on {kind} 261x{D}: {e32:.3g} x the fp32 allowance, {e16:.3g} x the f16 allowance")
        if kind == exposing:
            assert e32 >= REJECT and e16 >= REJECT, (name, kind, D, e32, e16)


def test_inputs_keep_their_promises():
    for D in (63, 64, 256, 1280):
        for kind in ("offset", "near_eps", "constant"):
            R.input_conditions(kind, R.rows_input(kind, 1, 261, D))
    # constant rows: y = b exactly in float64 and in both yardsticks, whatever the order of the sums
    w, b = R.affine(2, 1279)
    x = R.rows_input("constant", 3, 5, 1279)
    assert np.array_equal(R.layernorm64(x, w, b), np.broadcast_to(b.astype(f64), x.shape))
    for y in R.yardsticks(x, w, b).values():
        assert np.array_equal(y, np.broadcast_to(b, x.shape))


def test_cast_values_hold_every_rounding_case():
    a = R.cast_values(255)
    with np.errstate(over="ignore"):
        h = a.astype(f16)
    def of(v):
        got = h[a == f32(v)]
        assert got.size >= 1 and (got.view(np.uint16) == got.view(np.uint16)[0]).all()
        return got[0]
    assert of(1 + 2.0 ** -11) == 1 and of(1 + 3 * 2.0 ** -11) == f16(1 + 2.0 ** -9)              # ties, to even on either side
    assert of(1 + 2.0 ** -11 + 2.0 ** -23) == f16(1 + 2.0 ** -10) and of(1 + 2.0 ** -11 - 2.0 ** -23) == 1
    assert of(2.0 ** -24) == f16(2.0 ** -24) and of(2.0 ** -25) == 0 and of(2.0 ** -25 * (1 + 2.0 ** -23)) == f16(2.0 ** -24)
    assert of(3 * 2.0 ** -25) == f16(2.0 ** -23)
    assert of(65504.0) == 65504 and of(65519.996) == 65504 and np.isinf(of(65520.0)) and np.isinf(of(-65520.0))
    assert np.signbit(h[(a == 0) & np.signbit(a)]).all() and ((a == 0) & np.signbit(a)).any()
    assert np.isnan(h).sum() == np.isnan(a).sum() == 2 and np.isinf(h[np.isinf(a)]).all()
    big = R.cast_values(2048 * 256 + 3)
    assert np.isnan(big[-1]) and np.isnan(big[32]), "the special values sit at both ends"
    assert R.same_bits(h, h.copy()) and not R.same_bits(h, np.where(np.isnan(h), f16(0), h))


def test_place_map_names_every_place():
    m = R.place_map(2, 256).astype(f64)
    assert (m > 0).all() and np.array_equal(m, m.astype(f16).astype(f64))
    # neighbours in every direction, and the two images, differ everywhere
    assert (m[:, 1:] != m[:, :-1]).all() and (m[:, :, 1:] != m[:, :, :-1]).all() and (m[..., 1:] != m[..., :-1]).all()
    assert (m[0] != m[1]).all()
