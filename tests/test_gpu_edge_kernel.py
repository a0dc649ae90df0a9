"""The edge kernels alone (k::mask_edge through ext.test_edge) against tests/edge_ref.py: BYTE FOR BYTE, with guard bytes around
the mask and the workspace intact -- with the one-polarity shortcut and without it.

Extents are the smallest at which the kernel can go wrong.  Its constants (kernels/mask_edge.hip): a strip is 256 columns in
both passes, whatever R; a band is 128 rows in the column pass and 16 in the row pass; a cell of the shortcut is 64 x 64; the
largest reach is R = 129, with (64, 32, 32).  So: every window clipped on all four sides (1 x 1, 3 x 2); one row and one column
(300 x 1, 1 x 300: two strips, three column bands); an image narrower and lower than the reach (97 x 131: two column bands);
one column less than, exactly, and one more than one strip and two strips (255, 256, 257, 511, 512, 513 columns by 3 rows),
where the halo of R = 129 columns crosses into the neighbouring strip or past the image; one row more than a band of the row
pass (5 x 17) and of the column pass (5 x 129); and several strips, bands and ragged cells (600 x 150: three strips, two column
bands, ten row bands, 10 x 3 cells)."""
import numpy as np
import pytest

import edge_ref as ER
from test_edge_ref import PARAMS, blobs, masks

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 2), (300, 1), (1, 300), (97, 131), (255, 3), (256, 3), (257, 3), (511, 3), (512, 3), (513, 3), (5, 17), (5, 129),
         (600, 150)]


@pytest.fixture(scope="module")
def api():
    from dlimgedit_amd import api
    return api


def wanted(mask, params):
    """params -> the reference's bytes; the squared distances of one reach are computed once"""
    d2, out = {}, {}
    for p in params:
        R = ER.reach(*p)
        if R not in d2:
            d2[R] = ER.squared_distance_separable(mask, R)
        out[p] = ER.level(d2[R], mask >= 128, *p)
    return out


def _check(api, mask, p, want, what):
    for shortcut in (True, False):
        got, ok = api.ext.test_edge(mask, p, shortcut=shortcut)
        diff = got != want
        assert ok, f"{what}: guard bytes overwritten (shortcut {shortcut})"
        assert not diff.any(), (f"{what} (shortcut {shortcut}): {int(diff.sum())} of {diff.size} bytes differ, first at "
                                f"{tuple(np.argwhere(diff)[0])}: {got[diff][0]} for {want[diff][0]}")


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_every_mask_and_parameter_set(api, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    for name, m in masks(w, h, rng).items():
        want = wanted(m, PARAMS)
        for p in PARAMS:
            _check(api, m, p, want[p], f"{w}x{h} {name} {p}")


def test_bytes_from_128_on_are_foreground(api):
    rng = np.random.default_rng(4)
    m = blobs(130, 70, rng)
    soft = np.where(m > 0, rng.integers(128, 256, m.shape), rng.integers(0, 128, m.shape)).astype(np.uint8)
    for p in ((2, 0, 0), (0, 3, 0), (-1, 1, 1)):
        _check(api, soft, p, ER.edge(m, *p), f"any byte {p}")


@pytest.mark.parametrize("lone", [255, 0], ids=["foreground", "background"])
def test_a_single_pixel_visits_every_distance_up_to_the_reach(api, lone):
    p = (64, 32, 32)
    m = np.full((261, 261), 255 - lone, np.uint8)
    m[130, 130] = lone
    yy, xx = np.mgrid[0:261, 0:261]
    d2 = (yy - 130) ** 2 + (xx - 130) ** 2
    d2[130, 130] = 1
    R = ER.reach(*p)
    assert R == 129 and {int(v) for v in np.unique(d2) if v < R * R} == {a * a + b * b for a in range(R) for b in range(R)
                                                                        if 0 < a * a + b * b < R * R}
    want = ER.level(d2, m >= 128, *p)
    assert np.array_equal(want, ER.edge(m, *p))
    _check(api, m, p, want, f"a single pixel of {lone}")
    _check(api, m, (-64, 32, 32), ER.level(d2, m >= 128, -64, 32, 32), f"a single pixel of {lone}, shrunk")


def test_one_opposite_pixel_just_inside_at_and_past_the_reach(api):
    # the lone pixel in one corner, the pixel that looks at it in the other: horizontally, vertically and diagonally; 100 =
    # 6^2 + 8^2 is R^2 of (3, 2, 4), 2 * 91^2 < 129^2 < 2 * 92^2
    cases = [((3, 2, 4), [(9, 0), (10, 0), (11, 0), (0, 9), (0, 10), (0, 11), (5, 8), (6, 8), (6, 9), (7, 7), (8, 7)]),
             ((64, 32, 32), [(128, 0), (129, 0), (130, 0), (0, 128), (0, 129), (0, 130), (91, 91), (92, 91), (92, 92)]),
             ((-64, 32, 32), [(128, 0), (0, 129), (91, 91), (92, 92)])]
    for p, offsets in cases:
        for dx, dy in offsets:
            for lone in (255, 0):
                m = np.full((dy + 1, dx + 1), 255 - lone, np.uint8)
                m[0, 0] = lone
                want = ER.edge(m, *p, separable=True)
                _check(api, m, p, want, f"{p} lone {lone} at ({dx}, {dy})")


def test_the_shortcut_takes_whole_blocks_and_changes_nothing(api):
    # a disc in the middle of a field and a foreground slab on the right: with R = 4 most blocks are of one polarity
    w, h = 900, 300
    yy, xx = np.mgrid[0:h, 0:w]
    m = (255 * (np.hypot(xx - 350, yy - 150) < 60)).astype(np.uint8)
    m[:, 760:] = 255
    for p in ((2, 1, 0), (-2, 0, 1), (0, 0, 3)):
        want = ER.edge(m, *p)
        _check(api, m, p, want, f"disc in a field {p}")
        assert (want[:, :200] == 0).all() and (want[:, 800:] == (0 if p[2] else 255)).all()


def test_sixteen_jobs_of_mixed_sizes_and_one_more_than_a_group_holds(api):
    rng = np.random.default_rng(33)
    shapes = [(1, 1), (3, 2), (97, 260), (300, 40), (257, 5), (7, 129), (64, 64), (65, 65), (5, 3), (200, 131), (31, 17), (256, 2), (2, 256),
              (129, 129), (50, 40), (513, 3)]
    ms = [list(masks(w, h, rng).values())[k % 4] if k % 4 else blobs(w, h, rng) for k, (w, h) in enumerate(shapes)]
    ps = [PARAMS[k % len(PARAMS)] for k in range(16)]
    want = [ER.edge(m, *p) for m, p in zip(ms, ps)]
    for shortcut in (True, False):
        outs, ok, launches = api.ext.test_edge(ms, ps, shortcut=shortcut)
        assert ok and launches == 3                 # (what the launcher makes WITH the shortcut: cells, columns, rows)
        for k in range(16):
            assert np.array_equal(outs[k], want[k]), (k, shapes[k], ps[k], shortcut)
    # the seventeenth job starts the next group of launches
    outs, ok, launches = api.ext.test_edge(ms + ms[2:3], ps + ps[2:3])
    assert ok and launches == 6
    assert all(np.array_equal(o, q) for o, q in zip(outs, want + want[2:3]))


def test_launcher_refusals_then_one_good_call(api):
    m = np.zeros((8, 9), np.uint8)
    for mask, p, why in ((m, (0, 0, 0), "all 0"), (m, (65, 0, 0), "offset"), (m, (-65, 0, 0), "offset"), (m, (0, 33, 0), "feather"),
                         (m, (0, -1, 0), "feather"), (m, (0, 0, 33), "border"), (m, (1, 0, -1), "border"),
                         (None, (1, 0, 0, 9, 8), "null mask"), (np.zeros((0, 9), np.uint8), (1, 0, 0), "extent"),
                         (None, (1, 0, 0, 0, 5), "extent"), (None, (1, 0, 0, 5, -1), "extent"),
                         (None, (1, 0, 0, 65536, 32768), "does not fit an int")):
        with pytest.raises(api.Error, match=f"mask_edge: .*{why}"):
            api.ext.test_edge(mask, p)
    m[2:5, 3:7] = 255
    got, ok = api.ext.test_edge(m, (1, 1, 0))
    assert ok and np.array_equal(got, ER.edge(m, 1, 1, 0))
