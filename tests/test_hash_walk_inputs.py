"""CPU: the inputs of test_gpu_hash_walk.py do what they are for -- asserted on the oracle alone, for every forest and
matcher the GPU cases use, so that no case there can be degenerate (or fail for its input) on the device."""
import pytest

import hash_walk_util as hw
import test_gpu_hash_walk as t


@pytest.fixture(scope="module")
def fast():
    from oracle.pyoracle import Oracle
    return Oracle(fast=True)


@pytest.mark.parametrize("W,H", hw.SHAPES, ids=t.SHAPE_IDS)
def test_inputs_meet_their_conditions(fast, forest_paths, W, H):
    for kind in hw.KINDS:
        for fkey in ("zero", "tau"):
            for naive in (False, True):
                c = t.walk_case(fast, forest_paths, W, H, kind, fkey, naive)   # (asserts hw.conditions)
                assert c.B == 2 and (c.W, c.H) == (W, H)
        t.group_wants(fast, forest_paths, W, H, kind)
        # the frames [L, R, L] of pair 0: both consecutive pairs have correspondences
        for fkey in ("zero", "tau"):
            want, ncand = t.walk_case(fast, forest_paths, W, H, kind, fkey).want_corr(fast, 0, True, False)
            assert len(want[0]) > 0 and len(want[1]) > 0 and min(ncand) > 0
        if H == 155:   # the device-wide matchers behind tpw 3
            c = t.walk_case(fast, forest_paths, W, H, kind, "tau")
            for epi, ht in ((False, False), (True, True)):
                assert all(len(w[0]) > 0 for w in c.want(fast, epi, ht)), (kind, epi, ht)


def test_input_b_ends_and_input_c_starts_where_the_walk_needs_them(fast, forest_paths):
    """b: the last candidate row lies inside the first 32-row tile but not in its first rows; c: the first candidate row lies
    below the first 40-row tile, and at H = 155 the single-row tile H - 14 holds candidates of both images"""
    for W, H in hw.SHAPES:
        b, c = (t.walk_case(fast, forest_paths, W, H, k, "tau") for k in "bc")
        for i in range(2):
            assert all(13 + 16 <= r.max() < 13 + 32 for r in hw.cand_rows(b, i))
            assert all(r.min() >= 13 + 40 and r.max() == H - 14 for r in hw.cand_rows(c, i))


def test_plan_arithmetic():
    assert [hw.split(5, k) for k in hw.TPWS] == [[1] * 5, [2, 2, 1], [3, 2], [4, 1], [5], [5]]
    assert hw.plan(272, 155, 4, 32, 2, 256) == (32, 2, 3, 0) and hw.plan(96, 91, 4, 40, 64, 256) == (40, 2, 1, 0)
    assert hw.plan(48, 155, 208, 32, 2, 256) == (32, 2, 3, 112)
