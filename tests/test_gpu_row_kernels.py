"""The row kernels of kernels/elementwise.hip alone (kernels.hpp: k::layernorm, k::cast_f16, k::add_cast, k::im2col3x3), through
their hooks in lib/libdlimgedit_test.so: one launcher call on given operands, guard bytes around every device buffer.

k::layernorm is measured against the float64 reference of tests/row_ref.py in units of the rounding model; the allowance is
ALLOW = 1.25 times what the larger of the numpy fp32 yardsticks needs on the same inputs (sequential sums, sums in the order of a
wave reduction and, with GELU, the formula evaluated step by step); f16 results get half an f16 spacing on top (check_f16);
tests/test_row_ref.py shows what that measure rejects.  Every ratio goes to parity_margins.txt.  Covered: every extent at which the
launcher or the kernels take another path (four rows per workgroup; D below, at and above 64 and 256; the 16-byte kernel at 256,
768, 1280; the longest row), every combination of results the launcher has, the two launches of the SAM-HQ feature branch
exactly, rows whose mean dwarfs their spread, rows whose variance is near eps, constant rows, a misaligned x (the scalar kernel
at a D the 16-byte kernel would take), x aliasing out_f32, the non-finite report and its refusal.  The other three kernels only
move and round values: they are compared bit for bit.

Measured on MI355X (61 tests, 1.9 s; largest figure of each group, every single one is in parity_margins.txt; "allowed" is 1.25
times the larger yardstick on the same inputs, 1 for f16 results; the same table is in LABNOTES.md):

    k::layernorm alone                                                   kernel          allowed         where
    N(1, 3), all extents, fp32, rms / max units                          3.15 / 2.87     4.20 / 3.35     1 x 1280 / 5 x 255
    ... with GELU, fp32, rms / max units                                 3.64 / 7.09     4.35 / 8.87     1 x 1280 / 5 x 255
    ... f16, with and without GELU, error / bound                        0.998           1               261 x 64
    the two launches of the HQ branch, three inputs, error / bound       0.997           1               261 x 256 Gaussian
    offset rows, fp32, rms / max units                                   1223 / 525      5301 / 2669     261 x 63
    offset rows, f16 / f16 + GELU, error / bound                         0.753 / 0.709   1               261 x 63
    near-eps rows, fp32, rms / max units                                 20.6 / 7.87     121 / 34.6      261 x 257 / 261 x 63
    near-eps rows, f16 / f16 + GELU, error / bound                       0.991 / 0.989   1
    constant rows: b exactly; f16(gelu(b)), error / bound                0 / 0.998       0 / 1           5 x 256
    misaligned x (scalar kernel at D = 256, 1280), fp32 rms / max units  2.36 / 3.07     7.69 / 9.53     261 x 256
    misaligned x, f16, error / bound                                     0.996           1

Everything else is exact and passes: in-place = out-of-place, out_h == f16(out_f32), the non-finite report and its refusal,
the refusals, cast_f16, add_cast and im2col3x3 bit for bit.
"""
import numpy as np
import pytest

import neck_ref
import row_ref as R

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64

ROWS_FULL = (5, 261)                # the full cross product; four rows per workgroup: 2 and 66 workgroups, the last one part full
ROWS_FEW = (1, 3, 4)                # at a few widths only
WIDTHS = (1, 63, 64, 65, 255, 256, 257, 320, 768, 1216, 1279, 1280)
WIDTHS_FEW = (63, 256, 1280)
# (name, out_f32, out_f16, act): what the launcher can be asked for; "f16 gelu" is the only form the SAM-HQ branch launches
FLAVOURS = (("f32", True, False, 0), ("f16", False, True, 0), ("f16 gelu", False, True, 1), ("both", True, True, 0),
            ("both gelu", True, True, 1))


@pytest.fixture(scope="module")
def ext():
    from dlimgedit_amd import api
    assert api.ext.device_count() >= 1, "no HIP device visible"
    return api.ext


def _launch(ext, x, w, b, act, want32, want16, **kw):
    o32, o16, flag, ok = ext.test_layernorm_rows(x, w, b, R.EPS, act, want_f32=want32, want_f16=want16, **kw)
    assert ok, "a guard byte around a device buffer was overwritten"
    assert (o32 is not None) == want32 and (o16 is not None) == want16
    return o32, o16, flag


def _hold(name, ext, x, w, b, flavours=FLAVOURS, **kw):
    """Every flavour on one input against float64; the references and yardsticks are computed once per activation."""
    cache = {}
    for fname, want32, want16, act in flavours:
        if act not in cache:
            cache[act] = (R.layernorm64(x, w, b, R.EPS, act), R.yardsticks(x, w, b, R.EPS, act))
        ref, yard = cache[act]
        o32, o16, _ = _launch(ext, x, w, b, act, want32, want16, **kw)
        if x.shape[1] == 1 and not act:
            # one column: the deviation is zero and y = b exactly, so the rounding model has no error to measure in
            if want32:
                assert np.array_equal(o32, np.broadcast_to(b, o32.shape))
            if want16:
                assert np.array_equal(o16, np.broadcast_to(b.astype(f16), o16.shape))
            continue
        R.check_rows(f"{name} {fname}", o32, o16, x, w, b, R.EPS, act, yard, ref)


# ------------------------------------------------------------------------------------------ k::layernorm: extents and flavours

@pytest.mark.parametrize("D", WIDTHS)
def test_layernorm_extents_and_flavours(ext, D):
    """N(1, 3) rows, every width with 5 and 261 rows and every combination of results; 1, 3 and 4 rows at three widths."""
    w, b = R.affine(200 + D, D)
    for rows in ROWS_FULL + (ROWS_FEW if D in WIDTHS_FEW else ()):
        x = R.rows_input("gaussian", 1000 * rows + D, rows, D)
        _hold(f"row ln {rows}x{D}", ext, x, w, b)


@pytest.mark.parametrize("D", [256, 64], ids=["vit_256_vec_kernel", "emb_64_scalar_kernel"])
@pytest.mark.parametrize("kind", ["gaussian", "offset", "near_eps"])
def test_layernorm_product_shapes_of_the_hq_branch(ext, D, kind):
    """(261, 256, GELU, f16 only) and (261, 64, GELU, f16 only): the two launches of SamModel::hq_branch, on every input family."""
    w, b = R.affine(300 + D, D)
    x = R.rows_input(kind, 310 + D, 261, D)
    R.input_conditions(kind, x)
    _hold(f"row ln hq shape 261x{D} {kind}", ext, x, w, b, flavours=(("f16 gelu", False, True, 1),))


# ------------------------------------------------------------------------------------------ k::layernorm: inputs

@pytest.mark.parametrize("D", [63, 256, 257, 1280])
@pytest.mark.parametrize("kind", ["offset", "near_eps"])
def test_layernorm_hard_rows(ext, D, kind):
    """Rows whose mean is 1000 times their spread (a one-pass variance loses everything there) and rows whose variance lies
    within a factor 4 of eps (where eps, and which variance, decides the result), asserted on the input; fp32 and f16 + GELU."""
    w, b = R.affine(400 + D, D)
    x = R.rows_input(kind, 410 + D, 261, D)
    R.input_conditions(kind, x)
    _hold(f"row ln {kind} 261x{D}", ext, x, w, b, flavours=(("both", True, True, 0), ("f16 gelu", False, True, 1)))


@pytest.mark.parametrize("D", [1, 64, 65, 256, 1279, 1280])
def test_layernorm_constant_rows(ext, D):
    """Every row one value (a multiple of 1 / 8, so every partial sum is exact in any order): the mean is the value, every
    deviation is zero and the result is b exactly whatever eps divides by; with GELU, f16(gelu(b)) within the f16 bound."""
    w, b = R.affine(500 + D, D)
    x = R.rows_input("constant", 510 + D, 5, D)
    R.input_conditions("constant", x)
    o32, o16, _ = _launch(ext, x, w, b, 0, True, True)
    assert np.array_equal(o32, np.broadcast_to(b, o32.shape))
    assert np.array_equal(o16, np.broadcast_to(b.astype(f16), o16.shape))
    _, g16, _ = _launch(ext, x, w, b, 1, False, True)
    ref = np.broadcast_to(R.gelu64(b.astype(f64)), g16.shape)
    assert np.array_equal(R.layernorm64(x, w, b, R.EPS, 1), ref)
    R.check_f16(f"row ln constant 5x{D} f16 gelu", g16, ref, R.yardsticks(x, w, b, R.EPS, 1))


# ------------------------------------------------------------------------------------------ k::layernorm: paths

@pytest.mark.parametrize("D", [256, 1280])
def test_layernorm_misaligned_x_takes_the_scalar_kernel(ext, D):
    """x 4 bytes behind a 16-byte boundary at a width the 16-byte kernel would take: the launcher falls back to the scalar kernel.
    Held to the same bounds as every launch, not to the bits of the aligned call (another summation order)."""
    w, b = R.affine(600 + D, D)
    x = R.rows_input("gaussian", 610 + D, 261, D)
    _hold(f"row ln misaligned 261x{D}", ext, x, w, b, flavours=(("both", True, True, 0), ("f16 gelu", False, True, 1)),
          misalign_x=True)


@pytest.mark.parametrize("D", [64, 256, 257, 1280])
@pytest.mark.parametrize("act", [0, 1])
def test_layernorm_in_place_equals_out_of_place(ext, D, act):
    """kernels.hpp: x and out_f32 may alias.  The in-place call returns the bits of the out-of-place call, in both results, and
    no guard byte is touched."""
    w, b = R.affine(700 + D, D)
    x = R.rows_input("gaussian", 710 + D, 261, D)
    o32, o16, _ = _launch(ext, x, w, b, act, True, True)
    i32, i16, _ = _launch(ext, x, w, b, act, True, True, in_place=True)
    assert np.array_equal(i32.view(np.uint32), o32.view(np.uint32))
    assert np.array_equal(i16.view(np.uint16), o16.view(np.uint16))
    assert not np.array_equal(i32, x)


# ------------------------------------------------------------------------------------------ k::layernorm: the non-finite report

def test_layernorm_nonfinite_report(ext):
    """The encoder's overflow alarm on the unfused path: finite rows leave the int alone (0 stays 0, 1 stays 1), one infinity of
    either sign or one NaN in the first, a middle or the last of 261 rows sets it."""
    D = 256
    w, b = R.affine(800, D)
    rng = np.random.default_rng(801)
    x = (rng.standard_normal((261, D)) * 10.0 ** rng.uniform(-3, 29, (261, 1))).astype(f32)
    x[7, 3], x[8, 200] = 1e30, -1e30
    assert np.isfinite(x).all() and np.abs(x).max() == f32(1e30)
    assert _launch(ext, x, w, b, 0, True, False, nonfinite=0)[2] == 0
    assert _launch(ext, x, w, b, 0, True, False, nonfinite=1)[2] == 1
    x = R.rows_input("gaussian", 802, 261, D)
    for row in (0, 130, 260):
        for bad in (np.inf, -np.inf, np.nan):
            y = x.copy()
            y[row, 77] = bad
            assert _launch(ext, y, w, b, 0, False, True, nonfinite=0)[2] == 1, (row, bad)
    assert _launch(ext, x, w, b, 1, False, True, nonfinite=0)[2] == 0


def test_layernorm_nonfinite_report_refused_off_the_16_byte_path(ext):
    """Asked for at D = 257, or at D = 256 with a misaligned x, the report is refused with the launcher's message, the int is
    untouched, and the next good call works."""
    from dlimgedit_amd import api
    for D, kw in ((257, {}), (256, {"misalign_x": True})):
        w, b = R.affine(810 + D, D)
        x = R.rows_input("gaussian", 811 + D, 5, D)
        x[2, 1] = np.inf
        for start in (0, 1):
            with pytest.raises(api.Error, match="non-finite report needs rows that are a multiple of 256") as e:
                ext.test_layernorm_rows(x, w, b, R.EPS, 0, nonfinite=start, **kw)
            assert e.value.nonfinite == start
    w, b = R.affine(820, 256)
    x = R.rows_input("gaussian", 821, 5, 256)
    o32, _, flag = _launch(ext, x, w, b, 0, True, False, nonfinite=0)
    assert flag == 0
    R.check_rows("row ln after a refusal 5x256 f32", o32, None, x, w, b)


def test_layernorm_refusals(ext):
    """D = 0 and D = 1281 are refused; rows = 0 launches nothing and reports nothing."""
    from dlimgedit_amd import api
    one = np.ones((1, 1), f32)
    with pytest.raises(api.Error, match="row length must be in 1..1280"):
        ext.test_layernorm_rows(one, one[0], one[0], R.EPS, 0, rows=1, dim=0)
    x = R.rows_input("gaussian", 830, 2, 1281)
    with pytest.raises(api.Error, match="row length must be in 1..1280"):
        ext.test_layernorm_rows(x, np.ones(1281, f32), np.zeros(1281, f32), R.EPS, 0)
    x = R.rows_input("gaussian", 831, 1, 256)
    x[0, 0] = np.inf
    o32, o16, flag, ok = ext.test_layernorm_rows(x, np.ones(256, f32), np.zeros(256, f32), R.EPS, 0, want_f16=True, nonfinite=0, rows=0)
    assert ok and flag == 0 and o32.size == 0 and o16.size == 0
    w, b = R.affine(832, 1280)
    x = R.rows_input("gaussian", 833, 3, 1280)
    o32, _, _ = _launch(ext, x, w, b, 0, True, False)
    R.check_rows("row ln after the refusals 3x1280 f32", o32, None, x, w, b)


# ------------------------------------------------------------------------------------------ k::cast_f16

SWEEP = 2048 * 256                  # elements one pass of the capped grid covers


@pytest.mark.parametrize("n", [1, 255, SWEEP + 3])
def test_cast_f16_rounds_to_nearest_even(ext, n):
    """Every rounding case (row_ref.cast_values: ties to even on both sides, subnormals and the tie to zero, 65504, 65519.996,
    65520 to infinity, -0.0, infinities, NaN) at the front and, past one sweep of the grid, at the back: numpy's astype, bit for
    bit."""
    a = R.cast_values(n, seed=n)
    with np.errstate(over="ignore"):
        want = a.astype(f16)
    if n > 64:
        assert np.isinf(want[np.abs(a) == f32(65520.0)]).all() and (np.abs(want[np.abs(a) == f32(65519.996)]) == 65504).all()
        assert (want[np.abs(a) == f32(2.0 ** -25)] == 0).all() and np.signbit(want[(a == 0) & np.signbit(a)]).all()
        assert (np.abs(want[np.abs(a) == f32(1 + 2.0 ** -11)]) == 1).all() and np.isnan(want).sum() == np.isnan(a).sum() > 0
    _, got, ok = ext.test_elementwise("cast_f16", a)
    assert ok, "a guard byte around a device buffer was overwritten"
    assert R.same_bits(got, want), np.nonzero(got.view(np.uint16) != want.view(np.uint16))[0][:8]


# ------------------------------------------------------------------------------------------ k::add_cast

@pytest.mark.parametrize("n", [4, 1028, SWEEP * 4 + 4])
@pytest.mark.parametrize("addend", ["none", "whole", "wraps"])
def test_add_cast(ext, n, addend):
    """a + b[i % b_mod] in fp32 and its f16 rounding, bit for bit: without b, with b as long as a, with b_mod = 8 (4 for n = 4), which
    wraps; fp32 only, f16 only, both.  The last n is one 16-byte chunk past one sweep of the capped grid."""
    a = R.cast_values(n, seed=n + 1)
    b_mod = {"none": 0, "whole": n, "wraps": min(8, n)}[addend]
    b = None if addend == "none" else (np.random.default_rng(n).standard_normal(b_mod) * 100).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        want32 = R.add_cast_ref(a, b, b_mod)
        want16 = want32.astype(f16)
    for w32, w16 in ((True, False), (False, True), (True, True)):
        o32, o16, ok = ext.test_elementwise("add_cast", a, b, b_mod, want_f32=w32, want_f16=w16)
        assert ok, "a guard byte around a device buffer was overwritten"
        assert (o32 is not None) == w32 and (o16 is not None) == w16
        assert o32 is None or R.same_bits(o32, want32)
        assert o16 is None or R.same_bits(o16, want16)


def test_add_cast_refusals(ext):
    from dlimgedit_amd import api
    a = np.arange(8, dtype=f32)
    for n, b_mod in ((6, 4), (8, 6), (8, 0)):
        with pytest.raises(api.Error, match="add_cast: lengths must be multiples of 4"):
            ext.test_elementwise("add_cast", a, a, b_mod, n=n)
    o32, _, ok = ext.test_elementwise("add_cast", a, a, 4, want_f32=True)
    assert ok and np.array_equal(o32, a + np.tile(a[:4], 2))


# ------------------------------------------------------------------------------------------ k::im2col3x3

@pytest.mark.parametrize("B,C", [(1, 8), (2, 256)])
def test_im2col3x3_places(ext, B, C):
    """An integer map in which every element names its own place (no zero among them): the result is neck_ref.im2col3x3 bit for
    bit, the border taps are zero, and image 1 reads nothing of image 0."""
    fmap = R.place_map(B, C)
    _, got, ok = ext.test_elementwise("im2col3x3", fmap)
    assert ok, "a guard byte around a device buffer was overwritten"
    want = neck_ref.im2col3x3(fmap)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    cols = got.reshape(B, 64, 64, 9, C)
    assert not cols[:, 0, :, 0:3].any() and not cols[:, 63, :, 6:9].any()
    assert not cols[:, :, 0, 0::3].any() and not cols[:, :, 63, 2::3].any()
    assert (cols[:, 1:63, 1:63] != 0).all()
    if B > 1:
        alone = ext.test_elementwise("im2col3x3", fmap[1:])[1]
        assert np.array_equal(got[4096:].view(np.uint16), alone.view(np.uint16))


def test_im2col3x3_refuses_other_channel_counts(ext):
    from dlimgedit_amd import api
    with pytest.raises(api.Error, match="im2col3x3: channel count must be a positive multiple of 8"):
        ext.test_elementwise("im2col3x3", np.ones((1, 64, 64, 12), f16))
