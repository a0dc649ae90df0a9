"""k::lasso_derive alone on the GPU (kernels/mask_lasso.hip, through its hook in lib/libdlimgedit_test.so): upload,
k::mask_prior, the two derive launches and the host's fold behind plain host buffers.  The record -- inside cells, box, click,
squared distance -- must EQUAL tests/lasso_ref.py: the definition is integer arithmetic.  Extents: the identity, up-scaling
(footprints share source columns; sh = 171 with a 3-row last footprint), down-scaling, sw = 10, and an image smaller than one
wave's row.  Selections: what tests/lasso_cases.py lists.  The guard bytes around the mask's device copy, the plane, the column
distances and the row records stay intact in every call."""
import numpy as np
import pytest

import lasso_cases as LC
import lasso_ref
import prior_ref


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


@pytest.mark.gpu
@pytest.mark.parametrize("extent", LC.EXTENTS, ids=LC.EXTENT_IDS)
def test_records_equal_the_reference(api, extent):
    w, h = extent
    pre_w, pre_h = prior_ref.pre_extent(w, h)
    if (w, h) == (600, 400):
        assert (pre_h + 3) // 4 == 171 and pre_h - 4 * 170 == 3       # the last low-res row stands for 3 rows of the encoded image
    if (w, h) == (37, 1024):
        assert (pre_w + 3) // 4 == 10
    for name, mask in LC.kernel_masks(w, h).items():
        want = lasso_ref.derive(mask, pre_w, pre_h)
        got, guards_ok = api.ext.test_lasso_derive(mask, pre_w, pre_h)
        print(f"lasso.kernel.{w}x{h}.{name}: {got.tolist()}")
        assert guards_ok, f"{w}x{h} {name}: guard bytes were written"
        assert got.dtype == np.int32 and got.shape == (8,)
        assert np.array_equal(got, want), f"{w}x{h} {name}: {got.tolist()} for {want.tolist()}"
        if name in ("zeros", "uniform_127"):
            assert not got.any()
        if name in ("full", "uniform_128"):
            assert got[0] == ((pre_w + 3) // 4) * ((pre_h + 3) // 4) and tuple(got[1:5]) == (0, 0, w, h)


@pytest.mark.gpu
def test_launcher_refusals(api):
    mask = np.full((3, 5), 255, np.uint8)
    for pre_w, pre_h in ((0, 614), (1024, 1025), (1028, 614)):
        with pytest.raises(api.Error, match="mask_prior|lasso_derive"):
            api.ext.test_lasso_derive(mask, pre_w, pre_h)
    got, ok = api.ext.test_lasso_derive(mask, 1024, 614)
    assert ok and np.array_equal(got, lasso_ref.derive(mask, 1024, 614))
