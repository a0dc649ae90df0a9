"""The mask clean-up kernels alone (csrc/kernels/mask_cleanup.hip) through their hook, ext.test_mask_cleanup (lib/libdlimgedit_test.so),
against the numpy reference (tests/cleanup_ref.py) on the named cases of tests/cleanup_cases.py.  The result is an integer problem: every
comparison is np.array_equal.  That the cases are not vacuous (the reference changes pixels) is asserted on the CPU
(tests/test_cleanup_oracle.py).
"""
import numpy as np
import pytest

import cleanup_cases as CC
from dlimgedit_amd import api

pytestmark = pytest.mark.gpu

PATTERNS = sorted({CC.pattern_of(c) for c in CC.cases()})


def _check(case, got):
    want = CC.expected(case)
    assert got.shape == want.shape and got.dtype == np.uint8
    if not np.array_equal(got, want):
        ys, xs = np.nonzero(got != want)
        raise AssertionError(f"{case[0]}: {len(ys)} pixels differ, the first at (x={xs[0]}, y={ys[0]}): "
                             f"got {got[ys[0], xs[0]]}, want {want[ys[0], xs[0]]}")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_pattern_matches_reference(pattern):
    mine = [c for c in CC.cases() if CC.pattern_of(c) == pattern]
    assert mine
    for case in mine:
        _, mask, hole, island = case
        before = mask.copy()
        got = api.ext.test_mask_cleanup([mask], hole, island)[0]
        assert np.array_equal(mask, before)              # the hook works on a copy
        _check(case, got)


def test_three_jobs_of_different_sizes_in_one_call():
    jobs = CC.multi_job_call()
    assert len({c[1].shape for c in jobs}) == 3 and len({(c[2], c[3]) for c in jobs}) == 3
    got = api.ext.test_mask_cleanup([c[1] for c in jobs], [c[2] for c in jobs], [c[3] for c in jobs])
    for case, g in zip(jobs, got):
        _check(case, g)
    # ... and in another order: nothing depends on the place of a job in the call
    got = api.ext.test_mask_cleanup([c[1] for c in jobs[::-1]], [c[2] for c in jobs[::-1]], [c[3] for c in jobs[::-1]])
    for case, g in zip(jobs[::-1], got):
        _check(case, g)


def test_more_jobs_than_one_launch_holds():
    """17 jobs: the launcher packs 16 per launch."""
    case = next(c for c in CC.cases() if c[0].startswith("noise5-91x37-h8-i8"))
    got = api.ext.test_mask_cleanup([case[1]] * 17, case[2], case[3])
    for g in got:
        _check(case, g)


def test_result_is_the_same_every_time():
    case = next(c for c in CC.cases() if c[0].startswith("noise5-257x130-h8-i8"))
    first = api.ext.test_mask_cleanup([case[1]], case[2], case[3])[0]
    for _ in range(3):
        assert np.array_equal(api.ext.test_mask_cleanup([case[1]], case[2], case[3])[0], first)


def test_launcher_refusals_leave_the_next_call_working():
    good = next(c for c in CC.cases() if c[0].startswith("equal_threshold-65x63"))
    mask = good[1]

    def still_works():
        _check(good, api.ext.test_mask_cleanup([mask], good[2], good[3])[0])

    still_works()
    with pytest.raises(api.Error, match="both thresholds are 0"):
        api.ext.test_mask_cleanup([mask], 0, 0)
    still_works()
    with pytest.raises(api.Error, match="null mask"):
        api.ext.test_mask_cleanup([None], 3, 3, shapes=[(4, 4)])
    still_works()
    with pytest.raises(api.Error, match="does not fit an int"):
        api.ext.test_mask_cleanup([mask], 3, 3, shapes=[(65536, 65536)])
    still_works()
    with pytest.raises(api.Error, match="negative threshold"):
        api.ext.test_mask_cleanup([mask], -1, 3)
    with pytest.raises(api.Error, match="invalid extent"):
        api.ext.test_mask_cleanup([mask], 3, 3, shapes=[(0, 5)])
    # one bad job among good ones refuses the whole call before anything is launched
    with pytest.raises(api.Error, match="both thresholds are 0"):
        api.ext.test_mask_cleanup([mask, mask], [3, 0], [3, 0])
    still_works()
