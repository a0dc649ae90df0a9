"""tests/gemm_ref.py on the CPU: the evidence that tests/test_gpu_gemm.py would fail on a subtly wrong kernel.  check() and the
element-wise f16 bound accept the two yardsticks themselves and REJECT each modified model below on the builders' own
inputs; the float64 reference agrees with the fp32 oracle product the older GEMM tests use; every builder meets its stated
conditions; and the fitted GELU's distance from the erf form is the number device_common.hpp states."""
import functools

import numpy as np
import pytest

import gemm_ref as R

f16, f32, f64 = np.float16, np.float32, np.float64
M, N, K, RESID_ROWS = 256, 256, 192, 128          # two 128-row tiles: the residual wraps once


def _rejected(name, got, ref, model, yardsticks):
    with pytest.raises(AssertionError):
        R.check(name, got, ref, model, yardsticks)


def _rejected_f16(name, got32, ref, yardsticks):
    """The modified model's fp32 result rounded to f16, as an f16-only launch would deliver it."""
    with pytest.raises(AssertionError):
        R.check_f16(name, np.asarray(got32, f32).astype(f16), ref, yardsticks)


@functools.lru_cache(maxsize=None)
def _plain_case(act: int):
    A, W, bias = R.gaussian_case(11 + act, M, N, K)
    resid = R.residual_rows(12, RESID_ROWS, N)
    ref = R.plain(A, W, bias, resid, act)
    acc = R.accumulate_chain(A, W)
    yard = {g: R.plain_yardsticks(A, W, bias, resid, act, gelu=g) for g in (("erf", "fitted") if act else ("erf",))}
    return A, W, bias, resid, ref, acc, yard


def test_builders_meet_their_conditions():
    A, W, bias, resid, ref, _, _ = _plain_case(0)
    R.gaussian_conditions(A, W)
    R.residual_conditions(resid)
    for kind in ("gaussian", "spike", "offset"):
        A1, W1, b1, r = R.stream_case(5, 256, 256, 64, kind)
        R.stream_conditions(R.plain(A1, W1, b1, r), kind)
    with pytest.raises(AssertionError):
        R.stream_conditions(R.plain(*R.stream_case(5, 256, 256, 64, "gaussian")), "offset")
    with pytest.raises(AssertionError):
        R.stream_conditions(R.plain(*R.stream_case(5, 256, 256, 64, "gaussian")), "spike")
    Ai, Wi = R.identity_case(256, 512)
    assert np.array_equal(R.plain(Ai, Wi), Wi.astype(f64).T) and not np.array_equal(Wi[:256, :256], Wi[:256, :256].T)
    assert np.array_equal(R.round_f16(R.plain(Ai, Wi)), R.plain(Ai, Wi)), "the identity case is not exact in f16"
    R.gelu_grid_conditions(R.gelu_grid()[3])


def test_ulp16():
    assert R.ulp16(1.0) == 2.0 ** -10 and R.ulp16(0.99) == 2.0 ** -11 and R.ulp16(2048.0) == 2.0
    assert R.ulp16(0.0) == 2.0 ** -24 and R.ulp16(1e-9) == 2.0 ** -24 and R.ulp16(-3.0) == 2.0 ** -9
    x = np.array([0.3, 7.7, 1000.3, 6.1e-5, 3e-6])
    assert np.array_equal(R.ulp16(x), np.spacing(x.astype(f16)).astype(f64))


def test_fitted_gelu_distance_from_the_erf_form():
    """float64 evaluation of the committed constants over [-12, 12]: 2.519e-5 at x = -0.5645 (device_common.hpp states it; the
    GPU test allows 2.6e-5, this number rounded up)."""
    x = np.linspace(-12.0, 12.0, 2400001)
    err = R.gelu_fitted(x) - R.gelu64(x)
    worst = int(np.abs(err).argmax())
    assert 2.5185e-5 < abs(err[worst]) < 2.5190e-5, err[worst]
    assert abs(x[worst] + 0.5645) < 1e-4, x[worst]
    big = np.array([-6e4, -1000.0, -100.0, -12.0, 12.0, 100.0, 1000.0, 6e4])
    # beyond the clamp at +-8 the sigmoid stays at 1.0e-12 instead of falling further: |x| 1.0e-12, 6.1e-8 at the f16 limit
    assert np.abs(R.gelu_fitted(big) - R.gelu64(big)).max() < 1e-7
    assert 4.6e-4 < np.abs(R.gelu_tanh(x) - R.gelu64(x)).max() < 4.8e-4


def test_yardsticks_reproduce_the_measured_table():
    """rms / max units of the two accumulation models on Gaussian operands, 256 x 256 outputs: K = 64 about 5 / 5, K = 768
    about 19 / 29 (chain) and 48 / 31 (trunc16).  Bands, not values: the max of 65536 errors moves with the seed."""
    for Kk, lo, hi in ((64, 3.0, 8.0), (768, 12.0, 70.0)):
        A, W, _ = R.gaussian_case(1, 256, 256, Kk)
        ref = R.plain(A, W)
        for name, acc in R.ACCUMULATIONS.items():
            r = R.ratios(acc(A, W), ref, R.output_model(ref))
            assert lo <= r["rms"] <= hi and lo <= r["max"] <= hi, (Kk, name, r)
    x = (np.random.default_rng(0).standard_normal((256, 256)) * 3 + 1).astype(f32)
    x[:, 5] += 60
    st, y = R.statistics(x, 256), R.statistics_yardstick(x, 256)
    for c, band in ((0, (5.0, 20.0)), (1, (7.0, 25.0))):
        r = R.ratios(y[..., c], st[..., c], R.round_f32(st[..., c]))
        assert band[0] <= r["rms"] <= band[1], (c, r)


@pytest.mark.parametrize("act", [0, 1])
def test_plain_accepts_the_yardsticks(act):
    A, W, bias, resid, ref, _, yard = _plain_case(act)
    for g, ys in yard.items():
        for name, y in ys.items():
            R.check(f"cpu plain act{act} {g}-yardsticks, {name} itself", y, ref, R.output_model(ref), ys)
            R.check_f16(f"cpu plain act{act} {g}-yardsticks, {name} itself as f16", y.astype(f16), ref, ys)
    if act:     # the fitted form is refused by erf-form yardsticks: that is the rounding they lack (gemm_ref's docstring)
        _rejected("cpu fitted GELU against erf yardsticks", yard["fitted"]["chain"], ref, R.output_model(ref), yard["erf"])


def test_plain_rejects_the_modified_models():
    A, W, bias, resid, ref, acc, yard = _plain_case(0)
    ys, model = yard["erf"], R.output_model(ref)
    good = R.plain_epilogue(acc, bias, resid)
    assert np.array_equal(good, ys["chain"])
    # the fp32 result taken through f16 (an f16 result IS that: the fp32 check only)
    _rejected("cpu through f16", good.astype(f16).astype(f32), ref, model, ys)
    candidates = {
        "k slice dropped": R.plain_epilogue(R.accumulate_chain(A, W, drop=(64, 128, 128, 256)), bias, resid),
        "bias as f16": R.plain_epilogue(acc, bias, resid, bias_f16=True),
        "residual dropped": R.plain_epilogue(acc, bias, None),
        "residual wrapped a tile late": R.plain_epilogue(acc, bias, resid, resid_shift=64),
    }
    for name, got in candidates.items():
        _rejected("cpu " + name, got, ref, model, ys)
        _rejected_f16("cpu " + name + " as f16", got, ref, ys)


@pytest.mark.parametrize("gelu", ["tanh", "skip_negative"])
def test_gelu_forms_are_rejected(gelu):
    A, W, bias, resid, ref, acc, yard = _plain_case(1)
    got = R.plain_epilogue(acc, bias, resid, act=1, gelu=gelu)
    for g, ys in yard.items():          # under the erf-form yardsticks and under the wider fitted-form ones
        _rejected(f"cpu {gelu} GELU, {g} yardsticks", got, ref, R.output_model(ref), ys)
        _rejected_f16(f"cpu {gelu} GELU as f16, {g} yardsticks", got, ref, ys)


@functools.lru_cache(maxsize=None)
def _stream(kind: str):
    A1, W1, b1, resid = R.stream_case(21, 256, 256, 64, kind)
    x = R.plain_epilogue(R.accumulate_chain(A1, W1), b1, resid)          # a delivered fp32 stream
    return x, x.astype(f16)


def _stats_outcome(name, got, x, bn, yardsticks=None):
    """[sums accepted, squares accepted]"""
    outcome = []
    for c in (0, 1):
        other = R.statistics(x, bn).astype(f32)          # the other component intact, so that each is judged alone
        other[..., c] = got[..., c]
        try:
            R.check_statistics(name, other, x, bn, yardsticks)
            outcome.append(True)
        except AssertionError:
            outcome.append(False)
    return outcome


@pytest.mark.parametrize("kind", ["gaussian", "spike", "offset"])
def test_statistics(kind):
    x, xh = _stream(kind)
    for bn in (64, 96, 256):
        xb, xhb = x[:, :bn * (256 // bn)], xh[:, :bn * (256 // bn)]
        for name, y in R.statistics_yardsticks(xb, bn).items():
            assert _stats_outcome(f"cpu stats {kind} bn{bn} {name} itself", y, xb, bn) == [True, True]
        # the statistics of the f16 copy in place of the fp32 result
        assert _stats_outcome(f"cpu stats {kind} bn{bn} of the f16 copy", R.statistics_yardstick(xhb.astype(f32), bn), xb, bn) == [False, False]
    if kind == "offset":
        # raw moments in fp32: the sum is the same, the squares cancel -- also under the merged models' wider allowance
        assert _stats_outcome("cpu stats offset raw moments", R.statistics_yardstick(x, 256, raw_moments=True), x, 256) == [True, False]
        # what the sequential yardstick lacks: on these rows it refuses the merged model, a correct algorithm
        merged = R.statistics_merged_yardstick(x, 256, 32)
        assert _stats_outcome("cpu stats offset merged32 against sequential alone", merged, x, 256,
                              {"sequential": R.statistics_yardstick(x, 256)}) == [True, False]


def test_statistics_squares_count_every_row_in_its_own_spacing():
    """A spike row's squares are hundreds to ten thousands of times the other rows': an error of 200 spacings in ONE ordinary
    row is refused all the same."""
    x, _ = _stream("spike")
    got = R.statistics(x, 64).astype(f32)
    R.check_statistics("cpu stats spike rounded reference", got, x, 64)
    got[1, 5, 1] += 200 * np.spacing(got[1, 5, 1])
    assert got[1, 5, 1] < 1e-2 * got[:, R.SPIKE_ROW, 1].max()
    with pytest.raises(AssertionError):
        R.check_statistics("cpu stats spike one ordinary row 200 spacings off", got, x, 64)


@functools.lru_cache(maxsize=None)
def _consumer_case(kind: str, act: int):
    x, xh = _stream(kind)
    W2, gamma, beta, b2 = R.consumer_weights(31, 256, 256)
    wg, colsum, bias = R.fold_layernorm(W2, gamma, beta, b2)
    ref = R.consumer(xh, wg, colsum, bias, x, R.EPS, act)
    yard = R.consumer_yardsticks(xh, wg, colsum, bias, x, R.EPS, act, gelu="fitted" if act else "erf")
    return x, xh, (W2, gamma, beta, b2), (wg, colsum, bias), ref, yard


@pytest.mark.parametrize("kind", ["gaussian", "spike", "offset"])
@pytest.mark.parametrize("act", [0, 1])
def test_consumer_accepts_the_yardsticks(kind, act):
    _, _, _, _, ref, yard = _consumer_case(kind, act)
    for name, y in yard.items():
        R.check(f"cpu consumer {kind} act{act} {name} itself", y, ref, R.output_model(ref), yard)
        R.check_f16(f"cpu consumer {kind} act{act} {name} itself as f16", y.astype(f16), ref, yard)


@pytest.mark.parametrize("act", [0, 1])
def test_consumer_rejects_the_modified_models(act):
    x, xh, (W2, gamma, beta, b2), (wg, colsum, bias), ref, yard = _consumer_case("offset", act)
    gelu = "fitted" if act else "erf"
    acc = R.accumulate_chain(xh, wg)
    mean, rstd = R.moments_yardstick(x)
    assert np.array_equal(R.consumer_epilogue(acc, colsum, bias, mean, rstd, act, gelu), yard["chain"])
    mean16, _ = R.moments_yardstick(xh.astype(f32))
    _, colsum_unrounded, _ = R.fold_layernorm(W2, gamma, beta, b2, round_weight=False)
    candidates = {
        "mean of the f16 copy": R.consumer_epilogue(acc, colsum, bias, mean16, rstd, act, gelu),
        "colsum of the un-rounded weight": R.consumer_epilogue(acc, colsum_unrounded, bias, mean, rstd, act, gelu),
    }
    for name, got in candidates.items():
        _rejected(f"cpu consumer act{act} {name}", got, ref, R.output_model(ref), yard)
        _rejected_f16(f"cpu consumer act{act} {name} as f16", got, ref, yard)


def test_f16_bound_is_element_wise():
    """One element off by one f16 spacing fails although every ratio over the array would not notice it."""
    A, W, bias, resid, ref, acc, yard = _plain_case(0)
    got = yard["erf"]["chain"].astype(f16)
    R.check_f16("cpu f16 intact", got, ref, yard["erf"])
    got = got.copy()
    got[200, 131] = np.nextafter(got[200, 131], f16(np.inf))
    got[200, 131] = np.nextafter(got[200, 131], f16(np.inf))
    with pytest.raises(AssertionError):
        R.check_f16("cpu f16 one element two spacings off", got, ref, yard["erf"])


@pytest.mark.parametrize("Mp,Np,Kp,act,with_bias,resid_rows", [
    (128, 128, 64, 0, False, 0), (256, 192, 256, 0, True, 0), (4096, 768, 768, 0, True, 4096), (4096, 2304, 768, 0, True, 0),
    (4096, 3072, 768, 1, True, 0), (4096, 768, 3072, 0, True, 4096), (8192, 768, 768, 0, True, 4096),
    (4096, 256, 2304, 0, False, 0), (16384, 128, 64, 1, True, 0), (4096, 320, 320, 0, True, 0)])
def test_reference_agrees_with_the_fp32_oracle_product(Mp, Np, Kp, act, with_bias, resid_rows):
    """test_gemm_parity's inputs (tests/test_gpu_kernels.py: same seeds, same draws), its fp32 reference against the float64
    one here, on the first 256 rows and the 256 rows behind the residual's wrap.  Allowance per element: the classical bound of
    an fp32 dot product in any order, (K + 8) 2^-24 (|A| |W|^T + |bias| + |resid|) -- the 8 for the epilogue's handful of
    fp32 operations and the oracle's fp32 erf."""
    from test_gpu_kernels import _gemm_ref
    rng = np.random.default_rng(Mp + Np + Kp)
    A = rng.standard_normal((Mp, Kp)).astype(f16)
    W = (rng.standard_normal((Np, Kp)) / np.sqrt(Kp)).astype(f16)
    bias = rng.standard_normal(Np).astype(f32) if with_bias else None
    resid = rng.standard_normal((resid_rows, Np)).astype(f32) if resid_rows else None
    rows = np.r_[0:256, resid_rows:resid_rows + 256] if 0 < resid_rows < Mp else np.r_[0:min(Mp, 256)]
    r = None if resid is None else resid[rows % resid_rows]
    want = R.plain(A[rows], W, bias, r, act)
    got = _gemm_ref(A[rows], W, bias, r, act)
    slack = np.abs(A[rows].astype(f64)) @ np.abs(W.astype(f64)).T
    slack = slack + (0 if bias is None else np.abs(bias.astype(f64))) + (0 if r is None else np.abs(r.astype(f64)))
    assert (np.abs(got - want) <= (Kp + 8) * 2.0 ** -24 * slack).all()
