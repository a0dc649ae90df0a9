"""The stroke derivation alone (k::stroke_derive through ext.test_stroke_derive) against tests/stroke_ref.py: the ballots and the
record BYTE FOR BYTE, with guard bytes around the map, the ballots and the record intact.

Maps are the smallest that take each path: an upscaled image (a footprint below one pixel, a pixel shared by many cells), a
partial last cell row and column, a downscaled odd extent, widths that are and are not a multiple of 16 (16-byte loads or byte
loads), more than 4096 columns (a second column tile), ON cells at the borders of a ballot word and of the grid."""
import numpy as np
import pytest

import stroke_ref as SR
from test_stroke_ref import DIAGONALS, diagonal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


def _check(api, m, clicks, what, pre=None):
    h, w = m.shape
    pre_w, pre_h = pre or SR.pre_extent(w, h)
    on = SR.cells(m, pre_w, pre_h)
    record, bits, ok = api.ext.test_stroke_derive(m, pre_w, pre_h, clicks)
    assert ok, f"{what}: guard bytes overwritten"
    want = SR.ballots(on)
    assert bits.tobytes() == want.tobytes(), f"{what}: {int((bits != want).sum())} ballot words differ, first at {tuple(np.argwhere(bits != want)[0])}"
    assert record.tobytes() == SR.record(on, clicks).tobytes(), f"{what}: record {record.tolist()} for {SR.record(on, clicks).tolist()}"
    return record


@pytest.mark.parametrize("extent,pre,on_cells,first,pixels", DIAGONALS, ids=[f"{d[0][0]}x{d[0][1]}" for d in DIAGONALS])
def test_pinned_diagonals(api, extent, pre, on_cells, first, pixels):
    record = _check(api, diagonal(*extent), 4, f"diagonal {extent}", pre)
    assert record[0] == on_cells and [tuple(record[2 + 2 * i:4 + 2 * i]) for i in range(4)] == first


def test_pinned_small_maps(api):
    m = np.zeros((512, 512), np.uint8)
    m[100, 100], m[300, 400] = 200, 128
    assert _check(api, m, 4, "two pixels").tolist()[:10] == [2, 4, 50, 50, 200, 150, 50, 50, 50, 50]
    m = np.zeros((1024, 1024), np.uint8)
    m[:4, :4] = m[-4:, -4:] = 255
    assert _check(api, m, 3, "centroid tie").tolist()[:8] == [2, 3, 0, 0, 255, 255, 0, 0]
    assert _check(api, np.full((64, 64), 255, np.uint8), 5, "full map").tolist()[:12] == [65536, 5, 127, 127, 255, 255, 255, 0, 0, 255, 0, 0]


@pytest.mark.parametrize("w,h", [(301, 203), (37, 23), (1040, 517)], ids=["301x203", "37x23", "1040x517"])
def test_a_single_pixel_at_each_corner(api, w, h):
    for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 128
        assert _check(api, m, 3, f"{w}x{h} corner ({x}, {y})")[0] > 0


def test_127_and_128_side_by_side(api):
    for w, h in ((1024, 1024), (1000, 333)):
        m = np.zeros((h, w), np.uint8)
        m[h // 2, 400:404] = 127
        m[h // 2, 404] = 128
        m[h // 3, 16:32] = 127                       # a whole 16-byte load of bytes just below
        record = _check(api, m, 2, f"{w}x{h} 127 | 128")
        assert record[0] in (1, 2)                   # the one pixel at 128, which a cell row or two may share


@pytest.mark.parametrize("cells", [[(63, 10)], [(64, 10)], [(63, 10), (64, 10)], [(5, 255)], [(63, 255), (64, 255), (255, 255), (0, 255)],
                                   [(127, 0), (128, 0), (191, 63), (192, 64)]], ids=["x63", "x64", "x63-x64", "y255", "row255", "words"])
def test_cells_at_word_and_wave_boundaries(api, cells):
    m = np.zeros((1024, 1024), np.uint8)             # encoded as it is: cell (x, y) is pixels 4x .. 4x + 3, 4y .. 4y + 3
    for x, y in cells:
        m[4 * y + 3, 4 * x] = 255
    record = _check(api, m, 8, f"cells {cells}")
    assert record[0] == len(cells)


def test_an_empty_stroke_is_an_all_zero_record(api):
    for w, h in ((37, 23), (1040, 517)):
        m = np.full((h, w), 127, np.uint8)
        record = _check(api, m, 3, f"{w}x{h} empty")
        assert not record.any()


@pytest.mark.parametrize("clicks", [1, 8])
def test_one_click_and_eight(api, clicks):
    rng = np.random.default_rng(clicks)
    m = np.where(rng.random((517, 1030)) < 0.0005, 255, 0).astype(np.uint8)        # a downscaled odd extent, scattered cells
    record = _check(api, m, clicks, f"{clicks} clicks")
    assert record[1] == clicks and not record[2 + 2 * clicks:].any()
    # fewer ON cells than clicks: a cell is chosen again
    m = np.zeros((203, 301), np.uint8)
    m[100, 150] = 255
    record = _check(api, m, clicks, f"{clicks} clicks of one pixel")
    assert len({tuple(record[2 + 2 * i:4 + 2 * i]) for i in range(clicks)}) <= record[0]


@pytest.mark.parametrize("w,h", [(4112, 5), (4100, 3), (8200, 8), (16, 1), (1, 1), (3, 4000)], ids=lambda v: str(v))
def test_column_tiles_and_load_paths(api, w, h):
    rng = np.random.default_rng(w + h)
    m = np.where(rng.random((h, w)) < 0.01, 200, 100).astype(np.uint8)
    m[h - 1, w - 1] = 255                            # the last byte of the map, behind the first tile where there are two
    _check(api, m, 3, f"{w}x{h}")


def test_launcher_refusals(api):
    m = np.zeros((8, 8), np.uint8)
    for pre_w, pre_h, clicks in ((1024, 1024, 0), (1024, 1024, 9), (1028, 1024, 3), (0, 1024, 3)):
        with pytest.raises(api.Error):
            api.ext.test_stroke_derive(m, pre_w, pre_h, clicks)
