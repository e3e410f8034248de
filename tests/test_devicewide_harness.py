"""The comparison step of devicewide_util.run / run_corr, fed arrays a wrong writer would leave (no device needed).

A writer whose capacity guard is off by one (`pos <= cap` for `pos < cap`) puts record `cap` of pair i into slot `cap` of
pair i's slots, which is slot 0 of pair i + 1 -- or, for the last pair, slot 0 of the spare pair's worth of slots that the
harness allocates behind the batch.  `expected` holds the fill there, so `compare` names that slot."""
import numpy as np
import pytest

from devicewide_util import FILL32, compare, corr_words, expected, supp_words


def records(n, words, seed):
    return np.random.default_rng(seed).integers(0, 500, (n, words)).astype(np.uint32)


@pytest.mark.parametrize("words", [3, 4])
def test_expected_slots(words):
    wants = [records(7, words, 1), records(5, words, 2), records(9, words, 3)]
    for cap in (1, 4, 5, 6, 8, 9, 12):
        exp = expected(wants, cap)
        assert exp.shape == (4, cap, words)
        for i, w in enumerate(wants):
            k = min(len(w), cap)
            assert np.array_equal(exp[i, :k], w[:k]) and (exp[i, k:] == FILL32).all()
        assert (exp[3] == FILL32).all()
        compare(exp.copy(), exp, wants, "as expected")   # (and a faithful result passes)


@pytest.mark.parametrize("words", [3, 4])
@pytest.mark.parametrize("cap", [1, 8])
def test_a_record_behind_the_last_pairs_capacity_is_flagged(words, cap):
    """the off-by-one at cap = 1 (every pair cut) and at n_max - 1 (the last and largest pair cut by one record): record
    `cap` of the last pair lands in slot 0 of the spare pair"""
    wants = [records(7, words, 1), records(5, words, 2), records(9, words, 3)]
    exp = expected(wants, cap)
    got = exp.copy()
    got.reshape(-1, words)[2 * cap + cap] = wants[2][cap]
    with pytest.raises(AssertionError, match=r"pair 3 of 3: slot 0 of %d holds" % cap):
        compare(got, exp, wants, "spilt")


def test_a_record_in_the_next_pairs_slots_is_flagged():
    """pair 0 (7 records) at cap = 6 spills record 6 into pair 1's slot 0; where pair 1's own record 0 was written first, the
    spilt one stays and differs.  (Where pair 1's record comes last the spill is overwritten: the capacities that cut the
    LAST pair are the ones that always show it.)"""
    wants = [records(7, 3, 1), records(5, 3, 2), records(9, 3, 3)]
    exp = expected(wants, 6)
    got = exp.copy()
    got[1, 0] = wants[0][6]
    with pytest.raises(AssertionError, match="pair 1 of 3: slot 0 of 6 holds"):
        compare(got, exp, wants, "spilt")


def test_a_record_short_and_a_wrong_word_are_flagged():
    wants = [records(7, 4, 1), records(5, 4, 2)]
    exp = expected(wants, 6)
    got = exp.copy()
    got[0, 5] = FILL32                     # `pos < cap - 1`: the last slot below the capacity left alone
    with pytest.raises(AssertionError, match="pair 0 of 2: slot 5 of 6"):
        compare(got, exp, wants, "short")
    got = exp.copy()
    got[1, 5, 3] ^= 1                      # one bit behind pair 1's five records
    with pytest.raises(AssertionError, match="pair 1 of 2: slot 5 of 6"):
        compare(got, exp, wants, "behind the count")


def test_record_words():
    s = np.zeros(2, np.dtype([("x", "<i4"), ("y", "<i4"), ("d", "<f4")]))
    s["x"], s["y"], s["d"] = (3, 4), (5, 6), (1.0, -2.0)
    assert supp_words(s).tolist() == [[3, 5, 0x3F800000], [4, 6, 0xC0000000]]
    c = np.zeros(1, np.dtype([("sx", "<i4"), ("sy", "<i4"), ("tx", "<i4"), ("ty", "<i4")]))
    c["sx"], c["sy"], c["tx"], c["ty"] = 1, 2, 3, 4
    assert corr_words(c).tolist() == [[1, 2, 3, 4]]
