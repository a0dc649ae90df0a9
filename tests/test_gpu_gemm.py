"""The GEMM family (kernels/gemm.hip, gemm_epilogue.inc, gemm_f16_tile.inc) against the float64 references of tests/gemm_ref.py,
in units of the result's own rounding: every tile configuration of k::kGemmTiles, the fp32 result and the f16-only result
the product's qkv / fc1 launches take, the LayerNorm-folded consumer in both, the row statistics a stream writer leaves, and
GELU as the epilogues apply it.  A kernel may need 1.25 times the units of the larger of two CPU yardsticks on the same
inputs (gemm_ref.py: `chain`, `trunc16`; how the numbers come about and what tests/test_gemm_ref.py shows they reject is
written there).  Shapes: two tiles each way (M = 2 bm, N = 2 bn, so m0 and n0 enter the addressing), K = 64 / 192 / 768
(one K step, fewer than the pipeline is deep, many), the residual wrapping once (resid_mod = bm).

MEASURED (MI355X, the run this file was committed with).  Columns: the kernels' rms / max in model units, the worst of the
cases of the line; that as a fraction of the larger yardstick's, the worst case (the assertion is <= 1.25); the yardsticks'
own largest rms / max.  Every single figure is in the margins log conftest.within appends to.

    fp32, bias only          K = 64     1.96 /  3.01    0.50 / 0.51    chain 3.96 / 7.79      trunc16 3.69 / 5.35
      (all 12 tiles; the    K = 192    2.87 /  4.67    0.31 / 0.51    chain 7.00 / 12.96     trunc16 9.44 / 9.33
      three kernel families K = 768    5.25 /  9.10    0.15 / 0.33    chain 14.01 / 24.32    trunc16 34.99 / 37.08
      within 4 %)           K = 3072   9.79 / 12.24    0.07 / 0.12    chain 27.42 / 42.38    trunc16 132.6 / 104.5
    fp32, bias + residual    K = 64     1.01 /  1.01    0.98 / 1.00    chain 1.04 / 1.05      trunc16 1.03 / 1.02
      (the residual, rms 20, K = 768    1.06 /  1.03    0.44 / 1.00    chain 1.40 / 1.04      trunc16 2.58 / 1.14
      sets the spacing)     K = 3072   1.19 /  1.00    0.14 / 0.62    chain 2.06 / 1.13      trunc16 8.76 / 1.62
    consumer fp32, act 0     gaussian   5.72 / 12.24    0.30 / 0.50    chain 16.3 / 29.4      trunc16 36.8 / 39.8
                             spike      6.78 / 13.94    0.29 / 0.50    chain 19.6 / 35.0      trunc16 47.0 / 52.0
                             offset      211 /   367    0.25 / 0.38    chain 703 / 1456       trunc16 1484 / 1495
    consumer fp32, GELU      gaussian    740 /   113    1.00 / 0.96    (the fitted form's 2.5e-5 in fp32 units, kernel and
                             offset      769 /   437    0.84 / 0.52     yardsticks alike: gemm_ref's docstring)
    statistics, sums         all rows   3.51 /  6.16    0.46 / 0.44    sequential 14.8 / 49.1   merged 7.3 / 24.3
    statistics, squares      gaussian   3.03 /  6.45    0.52 / 0.47    sequential 11.8 / 27.9   merged 5.2 / 12.2
                             spike      3.35 /  7.02    0.51 / 0.55    sequential 13.9 / 34.0   merged 6.1 / 15.8
                             offset    12.82 / 61.64    0.49 / 0.62    sequential 13.3 / 25.5   merged 29.5 / 140.9
    f16 results              309 launches, largest |got - ref| / element-wise bound 0.9989 (a result at a rounding tie)
    GELU, A = I              largest |out - gelu64(x)| over |x| <= 12: 2.551e-5 (fp32 result, tiles 2, 7 and 9 alike)

The hardware sits well below both yardsticks and nearer to `chain`: at K = 3072 it needs 9.8 units where `chain` needs 27 and
`trunc16` 133 -- what blocks of 16 or 32 products added with rounding to nearest give on the CPU (1.6 .. 9.8).  With the
sequential yardstick alone the squares of the offset rows failed on the ring tiles (up to 31.5 units against 1.25 x 6.7): what
that yardstick lacks is written at gemm_ref.statistics_merged_yardstick.
"""
import functools

import numpy as np
import pytest

import gemm_ref as R

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64
TILES = list(range(12))
PINGPONG = (9, 10, 11)
KS = (64, 192, 768)


@pytest.fixture(scope="module")
def ext():
    from dlimgedit_amd import api
    assert api.ext.device_count() >= 1, "no HIP device visible"
    return api.ext


@pytest.fixture(autouse=True)
def _product_tile_choice_after_each_test(ext):
    yield
    ext.force_gemm_tile(-1)


@functools.lru_cache(maxsize=None)
def _plain_inputs(M, N, K, resid_rows):
    A, W, bias = R.gaussian_case(1000 * M + N + K, M, N, K)
    resid = R.residual_rows(7 * M + N, resid_rows, N)
    acc = {name: fn(A, W) for name, fn in R.ACCUMULATIONS.items()}
    return A, W, bias, resid, acc


def _yardsticks(acc, bias, resid, act):
    """The accumulation models with the epilogue in fp32; a GELU launch's apply the fitted form (gemm_ref's docstring)."""
    return {name: R.plain_epilogue(a, bias, resid, act, gelu="fitted") for name, a in acc.items()}


# ------------------------------------------------------------------------------------------ 1. fp32 result

@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("tile", TILES)
def test_fp32_result(ext, tile, K):
    bm, bn = ext.gemm_tile_shape(tile)
    A, W, bias, resid, acc = _plain_inputs(2 * bm, 2 * bn, K, bm)
    ext.force_gemm_tile(tile)
    out = ext.test_gemm(A, W, bias, resid, 0)
    ref = R.plain(A, W, bias, resid)
    R.check(f"gemm fp32 tile{tile} K{K}", out, ref, R.output_model(ref), _yardsticks(acc, bias, resid, 0))
    # ... and with the bias alone: the residual (rms 20) sets the spacing of the sum and hides the accumulation under it
    out = ext.test_gemm(A, W, bias, None, 0)
    ref = R.plain(A, W, bias)
    R.check(f"gemm fp32 tile{tile} K{K} no residual", out, ref, R.output_model(ref), _yardsticks(acc, bias, None, 0))


@pytest.mark.parametrize("tile", [2, 9])
def test_fp32_result_long_k(ext, tile):
    A, W, bias, resid, acc = _plain_inputs(256, 256, 3072, 256)
    ext.force_gemm_tile(tile)
    out = ext.test_gemm(A, W, bias, resid, 0)
    ref = R.plain(A, W, bias, resid)
    R.check(f"gemm fp32 tile{tile} K3072", out, ref, R.output_model(ref), _yardsticks(acc, bias, resid, 0))
    out = ext.test_gemm(A, W, bias, None, 0)
    ref = R.plain(A, W, bias)
    R.check(f"gemm fp32 tile{tile} K3072 no residual", out, ref, R.output_model(ref), _yardsticks(acc, bias, None, 0))


# ------------------------------------------------------------------------------------------ 2. f16-only result

@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("tile", TILES)
def test_f16_only_result(ext, tile, K):
    """out_h alone: plain; bias + GELU; and bias + GELU + fp32 residual on the tiles that take one with this result (the ring
    tiles: the ping-pong tiles' f16-rows epilogue has no residual, test_pingpong_refuses_... below)."""
    bm, bn = ext.gemm_tile_shape(tile)
    A, W, bias, resid, acc = _plain_inputs(2 * bm, 2 * bn, K, bm)
    ext.force_gemm_tile(tile)
    flavours = [("plain", None, None, 0), ("bias", bias, None, 0), ("bias gelu", bias, None, 1)]
    if tile not in PINGPONG:
        flavours += [("bias resid", bias, resid, 0), ("bias gelu resid", bias, resid, 1)]
    for name, b, r, act in flavours:
        out16 = ext.test_gemm(A, W, b, r, act, want_f16=True, want_f32=False)
        assert out16.dtype == f16
        R.check_f16(f"gemm f16-only tile{tile} K{K} {name}", out16, R.plain(A, W, b, r, act), _yardsticks(acc, b, r, act))


@pytest.mark.parametrize("tile", TILES)
def test_f16_only_identity_layout(ext, tile):
    """A = I against an asymmetric integer W: a transposed, permuted or misplaced f16 row shows as a wrong integer."""
    bm, bn = ext.gemm_tile_shape(tile)
    A, W = R.identity_case(2 * bm, 2 * bn)
    ext.force_gemm_tile(tile)
    out16 = ext.test_gemm(A, W, want_f16=True, want_f32=False)
    assert np.array_equal(out16.astype(f32), W.astype(f32).T)


# ------------------------------------------------------------------------------------------ 3. LayerNorm-folded consumer

@pytest.mark.parametrize("kind", ["gaussian", "spike", "offset"])
@pytest.mark.parametrize("D", [256, 768])
@pytest.mark.parametrize("tile", TILES)
def test_consumer(ext, tile, D, kind):
    """The consumer on `tile` (the producer too where the tile fits it: D = 256 / 768 are 1 / 3 statistic groups of a ping-pong
    producer), fp32 result through check(), f16-only result -- the product's flavour -- element by element, act 0 and 1."""
    bm, bn = ext.gemm_tile_shape(tile)
    M, N = 2 * bm, 2 * bn
    A1, W1, b1, resid = R.stream_case(100 * tile + D, M, D, 64, kind)
    W2, gamma, beta, b2 = R.consumer_weights(tile + D, N, D)
    ext.force_gemm_tile(tile, consumer_tile=tile)
    acc = None
    for act in (0, 1):
        for fmt in ("f32", "f16"):
            x, xh, y, _, ops = ext.test_gemm_ln(A1, W1, b1, resid, W2, gamma, beta, b2, R.EPS, act, consumer_out=fmt, operands=True)
            if acc is None:          # the stream the producer delivered is the same in all four launches: one set of yardsticks
                x0 = x
                R.stream_conditions(x, kind)
                assert np.array_equal(xh, x.astype(f16))
                wg, colsum, bias = ops["wg"], ops["colsum"], ops["bias"]
                assert np.array_equal(wg, R.fold_layernorm(W2, gamma, beta, b2)[0])
                acc = {name: fn(xh, wg) for name, fn in R.ACCUMULATIONS.items()}
                mean, rstd = R.moments_yardstick(x)
            assert np.array_equal(x, x0)
            ref = R.consumer(xh, wg, colsum, bias, x, R.EPS, act)
            yard = {name: R.consumer_epilogue(a, colsum, bias, mean, rstd, act, gelu="fitted") for name, a in acc.items()}
            name = f"gemm consumer tile{tile} D{D} {kind} act{act} {fmt}"
            if fmt == "f32":
                R.check(name, y, ref, R.output_model(ref), yard)
            else:
                assert y.dtype == f16
                R.check_f16(name, y, ref, yard)


# ------------------------------------------------------------------------------------------ 4. row statistics

@pytest.mark.parametrize("kind", ["gaussian", "spike", "offset"])
@pytest.mark.parametrize("tile", TILES)
def test_row_statistics(ext, tile, kind):
    """What a stream writer (fp32 stream + f16 copy) on `tile` leaves in stats_out against the float64 statistics of the x it
    delivered, per block of bn columns.  (The f16-pair flavour writes the same bits: test_gpu_kernels.py,
    test_pair_stream_is_the_fp32_stream_split_in_two.)"""
    bm, bn = ext.gemm_tile_shape(tile)
    M, D = 2 * bm, 2 * bn
    A1, W1, b1, resid = R.stream_case(300 + tile, M, D, 64, kind)
    W2, gamma, beta, b2 = R.consumer_weights(tile, 64, D)
    ext.force_gemm_tile(tile)
    x, xh, _, stats = ext.test_gemm_ln(A1, W1, b1, resid, W2, gamma, beta, b2, R.EPS, 0, consumer_out="f16")
    assert stats.shape == (2, M, 2), (stats.shape, "the forced tile did not write the stream")
    R.stream_conditions(x, kind)
    x_ref = R.plain(A1, W1, b1, resid)
    x_yard = {name: R.plain_epilogue(fn(A1, W1), b1, resid) for name, fn in R.ACCUMULATIONS.items()}
    R.check(f"gemm stream tile{tile} {kind}", x, x_ref, R.output_model(x_ref), x_yard)
    assert np.array_equal(xh, x.astype(f16))
    R.check_statistics(f"gemm stats tile{tile} {kind}", stats, x, bn)


# ------------------------------------------------------------------------------------------ 5. GELU as the GEMM applies it

@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("tile", [2, 7, 9])
def test_gelu_as_the_gemm_applies_it(ext, tile, fmt):
    """A = I, so the accumulator is W exactly and x = W + bias is exact in fp32 (gemm_ref.gelu_grid: [-12, 12] at 3.9e-4, the
    fitted form's worst point -0.5645, the clamp at +-8, 0, +-100, +-1000, +-6e4).  |out - gelu64(x)| <= 2.6e-5 + 2^-18 |x|:
    the documented distance of the fitted form from the erf form (2.519e-5, test_gemm_ref.py) rounded up, plus its fp32
    evaluation -- v_exp_f32 and v_rcp_f32 one ulp each, the rounding of the exponent's argument amplified by at most about 6
    where the sigmoid is not saturated, one rounding of the product.  The f16-only result additionally half an f16 spacing.
    Largest measured |out - gelu64(x)| over |x| <= 12, fp32 result: 2.551e-5 on all three tiles."""
    A, W, bias, x = R.gelu_grid()
    ext.force_gemm_tile(tile)
    ref = R.gelu64(x)
    bound = 2.6e-5 + 2.0 ** -18 * np.abs(x)
    if fmt == "f32":
        out = ext.test_gemm(A, W, bias, None, 1).astype(f64)
    else:
        out = ext.test_gemm(A, W, bias, None, 1, want_f16=True, want_f32=False).astype(f64)
        bound = bound + R.ulp16(ref) / 2 * (1 + 2.0 ** -10)
    assert np.isfinite(out).all()
    err = np.abs(out - ref)
    from conftest import within
    within(f"gemm gelu tile{tile} {fmt} largest |out - gelu64| over |x| <= 12", err[np.abs(x) <= 12].max(), np.inf)
    within(f"gemm gelu tile{tile} {fmt} err/bound", (err / bound).max(), np.nextafter(1.0, np.inf))


# ------------------------------------------------------------------------------------------ the ping-pong tiles' f16-rows epilogue

@pytest.mark.parametrize("tile", PINGPONG)
def test_pingpong_refuses_a_residual_with_an_f16_only_result(ext, tile):
    """The f16-rows epilogue of tiles 9 / 10 / 11 reads no residual (and computes no row statistics): gemm_tile_fits refuses
    the combination, a forced tile is an error, and the planner's own choice -- a ring tile -- adds the residual."""
    from dlimgedit_amd import api
    bm, bn = ext.gemm_tile_shape(tile)
    A, W, bias, resid, acc = _plain_inputs(2 * bm, 2 * bn, 192, bm)
    ext.force_gemm_tile(tile)
    with pytest.raises(api.Error, match="takes no residual"):
        ext.test_gemm(A, W, bias, resid, 0, want_f16=True, want_f32=False)
    out32 = ext.test_gemm(A, W, bias, resid, 0)                  # the same tile with an fp32 result still runs
    ref = R.plain(A, W, bias, resid)
    R.check(f"gemm fp32 tile{tile} beside the refusal", out32, ref, R.output_model(ref), _yardsticks(acc, bias, resid, 0))
    ext.force_gemm_tile(-1)
    out16 = ext.test_gemm(A, W, bias, resid, 0, want_f16=True, want_f32=False)
    R.check_f16(f"gemm f16-only with residual, shape of tile{tile}, planner's tile", out16, ref, _yardsticks(acc, bias, resid, 0))
