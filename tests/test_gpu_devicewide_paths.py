"""Every host path of the two device-wide matchers (non-epipolar sort-matcher, hash table) against the CPU oracle, at small shapes.

The host side of these matchers reads four plan words back and chooses launches by them: the 4096-record join alone, an
8192-record launch beside it with the planner's work list as its grid, the radix-sort fallback (k_partition.h / k_global.h);
k_ht_join<4, 1024>, <4, 512> alone or beside a <4, 1024> launch over the list of larger bins, <8, 1024>, a second planning
round with fewer buckets per bin, or the fallback (k_htjoin.h / k_hashtable.h).  Which of them a call took is recorded in
kernel_launch_names()["k_global_match"].  Every case here
  * chooses its input on the CPU: the codes come from the oracle, are binned as gp_bin (k_partition.h) bins them, and the
    largest bin is asserted to lie where the case needs it BEFORE anything runs on the device;
  * runs on outputs filled with 0xA5 and compares every byte with oracle.match_pair per pair (counts, candidate counts,
    records; everything behind a pair's count, and a spare pair's worth of array behind the batch, still holds the fill);
  * asserts the recorded path, so that no case passes by taking another path than it claims.
A band of striped rows (every row alike) puts thousands of equal codes into one bin; with the row in the state (epipolar
hash table) they spread over the rows' buckets again, so the paths for over-large bins are reached without the row only."""
import numpy as np
import pytest

from devicewide_util import HJ, HM_BUCKETS, VJ4, VJ8, Case, banded, load_forest, make_ctx, path, run, shared, textured

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fast():
    from oracle.pyoracle import Oracle
    return Oracle(fast=True)


def tex272(fast, fp):
    return shared("tex272", lambda: Case(fast, fp["tau"], [textured(272, 61, 4, 9)]))


def tex528(fast, fp):
    return shared("tex528", lambda: Case(fast, fp["tau"], [textured(528, 90, 20 + i, 4 + 2 * i) for i in range(2)]))


def band_of_three(fast, fp, H, band):
    """textured, banded, textured: only the middle pair has an over-large bin (528 x H, zero forest)"""
    return shared(("three", H, band), lambda: Case(fast, fp["zero"], [textured(528, H, 20, 4), banded(528, H, 22, 5, band), textured(528, H, 21, 6)]))


def one_banded(fast, fp, H, band):
    return shared(("banded", H, band), lambda: Case(fast, fp["zero"], [banded(528, H, 22, 5, band)]))


# ------------------------------------------------------------------------------------------------- the code-range matcher
def test_code_ranges_one_launch(fast, forest_paths):
    """every partition holds at most 4096 records a side: k_row_join<4, 1024> alone, twice on one context"""
    c = tex272(fast, forest_paths)
    assert c.code_range_bins(0) <= 4096
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        for rep in range(2):
            run(ctx, fast, c, False, False, VJ4, "one launch, call %d" % rep)
    finally:
        ctx.close()


def test_code_ranges_side_launch_over_the_work_list(fast, forest_paths):
    """The middle pair of three has bins of 4097 .. 8192 records a side: the 8192-record launch with the planner's work list
    as its grid beside the 4096-record one.  The plan words are maxima over the batch: the other pairs' workgroups of the
    side launch find empty lists.  Then the middle pair's correspondences (mode 1) through the same path."""
    import opengpc_amd as g
    c = band_of_three(fast, forest_paths, 150, 90)
    sides = [c.code_range_bins(i) for i in range(3)]
    assert sides[0] <= 4096 and 4096 < sides[1] <= 8192 and sides[2] <= 4096, sides
    name = VJ8 + "[list] + " + VJ4
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        run(ctx, fast, c, False, False, name, "side launch, three pairs")
        pl, pr = fast.preprocess(c.L[1], 5), fast.preprocess(c.R[1], 5)
        want = fast.find_correspondences(fast.descriptors(fast.hash(pl[0], pl[1], c.f), pl[2], c.W, False), pl[2],
                                         fast.descriptors(fast.hash(pr[0], pr[1], c.f), pr[2], c.W, False), pr[2], c.W)
        got, n, st = ctx.stereo_match(pl, pr, g.Settings(5, 128, 1, False, False, 1))
        assert st == 0 and n == len(want) > 0 and path(ctx) == name
        for a, b in (("src_x", "sx"), ("src_y", "sy"), ("tar_x", "tx"), ("tar_y", "ty")):
            assert np.array_equal(got[a], want[b]), "correspondences: %s differs" % a
    finally:
        ctx.close()


def test_code_ranges_fall_back_to_the_sort(fast, forest_paths):
    """a bin beyond 8192 records a side: the plan is abandoned with nothing written, gpc::k_g_match produces the result"""
    c = one_banded(fast, forest_paths, 190, 130)
    assert c.code_range_bins(0) > 8192
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        run(ctx, fast, c, False, False, "gpc::k_g_match", "fallback")
    finally:
        ctx.close()


def mostly_true_forest_text(tau):
    """32 tests that hold for most pixels under the SSE=OFF predicate (as tests/test_naive_mode.py builds it)"""
    rng = np.random.default_rng(1234)
    lines = ["4"]
    for fern in range(4):
        lines.append("%d l 8" % fern)
        for t in range(8):
            ix, iy, jx, jy = rng.integers(-13, 14, 4)
            lines.append("%d %d %d %d %d %d" % (t, ix, iy, jx, jy, tau))
    return "\n".join(lines)


def test_code_ranges_wide_codes(fast):
    """SSE=OFF arithmetic with 32 tests: codes use bit 31 and 0xFFFFFFFF is a code; the one-launch path, WIDE"""
    c = Case(fast, None, [textured(272, 61, 4, 9)], naive=True, forest_text=mostly_true_forest_text(60))
    assert c.bits == 32 and c.code_range_bins(0) <= 4096
    assert all((cd >> np.uint64(31)).any() for cd, _ in c.recs[0])
    ctx = make_ctx(naive=True)
    try:
        load_forest(ctx, c)
        run(ctx, fast, c, False, False, "gpc::k_row_join<4, 1024, true, true>", "wide codes")
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------- the hash table
EPI = pytest.mark.parametrize("epi", [True, False])


@EPI
def test_hash_table_default_plan(fast, forest_paths, epi):
    c = tex272(fast, forest_paths)
    assert c.bucket_bins(0, 10, epi) <= 4096
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        run(ctx, fast, c, epi, True, HJ % (4, 1024), "default plan")
    finally:
        ctx.close()


@EPI
@pytest.mark.parametrize("no_half", [False, True])
def test_hash_table_bins_of_512_buckets(fast, forest_paths, epi, no_half):
    """GPC_HIP_HT_LBITS=9 and no bin beyond 2048 records: the 512-thread join alone; with GPC_HIP_HT_NO_HALF the 1024-thread one"""
    c = tex528(fast, forest_paths)
    assert max(c.bucket_bins(i, 9, epi) for i in range(c.B)) <= 2048
    env = {"GPC_HIP_HT_LBITS": 9}
    if no_half:
        env["GPC_HIP_HT_NO_HALF"] = 1
    ctx = make_ctx(env)
    try:
        load_forest(ctx, c)
        run(ctx, fast, c, epi, True, HJ % (4, 1024 if no_half else 512), "512 buckets per bin")
    finally:
        ctx.close()


def test_hash_table_larger_bins_beside_the_512_thread_join(fast, forest_paths):
    """GPC_HIP_HT_LBITS=9, the middle pair of three has a bin of 2049 .. 4096 records: a 1024-thread launch over the list of
    such bins beside the 512-thread launch; the other pairs' lists are empty.  (State without the row: see the module's text.)"""
    c = band_of_three(fast, forest_paths, 120, 60)
    bins = [c.bucket_bins(i, 9, False) for i in range(3)]
    assert bins[0] <= 2048 and 2048 < bins[1] <= 4096 and bins[2] <= 2048, bins
    ctx = make_ctx({"GPC_HIP_HT_LBITS": 9})
    try:
        load_forest(ctx, c)
        run(ctx, fast, c, False, True, (HJ % (4, 1024)) + "[list] + " + (HJ % (4, 512)), "larger bins beside")
    finally:
        ctx.close()


def test_hash_table_8192_record_bins(fast, forest_paths):
    """few states, a bin of 4097 .. 8192 records however few buckets a bin has: the planner halves until 128, then k_ht_join<8, 1024>"""
    c = one_banded(fast, forest_paths, 150, 90)
    assert all(4096 < c.bucket_bins(0, lbits, False) <= 8192 for lbits in (10, 9, 8, 7))
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        run(ctx, fast, c, False, True, HJ % (8, 1024), "8192-record bins")
    finally:
        ctx.close()


def test_hash_table_falls_back_to_the_sort(fast, forest_paths):
    """a bin beyond 8192 records at every bin width: nothing written by the abandoned attempts, gpc::k_ht_pairs produces the result"""
    c = one_banded(fast, forest_paths, 190, 130)
    assert all(c.bucket_bins(0, lbits, False) > 8192 for lbits in (10, 9, 8, 7))
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        run(ctx, fast, c, False, True, "gpc::k_ht_pairs", "fallback")
    finally:
        ctx.close()


@pytest.mark.parametrize("epi,H", [(False, 400), (True, 520)])
def test_hash_table_second_planning_round(fast, forest_paths, epi, H):
    """A textured 1024 x H pair whose largest bin of 1024 buckets exceeds 4096 records while the estimate still plans for 1024
    and whose bins of 512 buckets fit (heights 380 .. 540 were tried in steps of ten on the CPU: 400 without the row in the
    state, 520 with it, are the smallest that do both): the first round overflows, the second takes 512 buckets per bin.  A
    second call at the same size starts from the remembered width (ht_hint_*) and reproduces the result and the path."""
    c = shared(("second", H), lambda: Case(fast, forest_paths["zero"], [textured(1024, H, 3, 21)]))
    assert 2 * c.cap * 0.7 / ((HM_BUCKETS >> 10) + 1) <= 3500.0, "the estimate no longer starts at 1024 buckets per bin"
    assert c.bucket_bins(0, 10, epi) > 4096 >= c.bucket_bins(0, 9, epi)
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        first = run(ctx, fast, c, epi, True, None, "second round, first call")
        # (bins of 1024 buckets never take the 512-thread join: its name says that the plan ended at 512 buckets or fewer)
        assert first.startswith("gpc::k_ht_join<") and first.endswith(HJ % (4, 512)), first
        run(ctx, fast, c, epi, True, first, "second round, the remembered width")
    finally:
        ctx.close()


@EPI
def test_hash_table_large_then_small_on_one_context(fast, forest_paths, epi):
    """528x90 then 272x61 then 528x90: the carve-up of the workspace is made anew for every call, not reused"""
    big, small = tex528(fast, forest_paths), tex272(fast, forest_paths)
    ctx = make_ctx()
    try:
        for c in (big, small, big):
            load_forest(ctx, c)
            run(ctx, fast, c, epi, True, HJ % (4, 1024), "%dx%d after another shape" % (c.W, c.H))
    finally:
        ctx.close()
