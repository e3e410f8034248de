"""Short output capacities on every launch path of the two device-wide matchers (non-epipolar sort-matcher, hash table).

The C ABI promises for every output: with more records than cap_per_pair the count is the true count, the first cap records
are valid, and nothing else is written -- not the next pair's slots, not the memory behind the last pair's.  Every writer
keeps that with a branch of its own (k_gp_gather, k_g_match, k_ht_pairs, k_ht_gather, k_group_union), and a capacity no pair
reaches (test_gpu_devicewide_paths.py) never takes those branches.  Here every named path of that file runs again, on the
same cases (devicewide_util.shared) under the same knobs, with the CPU-side bin sizes that select the path asserted first,
  * in supports mode (gpc_hip_match_batch_device, 12-byte records: devicewide_util.run) and
  * in correspondences mode (gpc_hip_match_sequence_device over [L, R, L], 16-byte records: devicewide_util.run_corr),
at capacities computed on the CPU from the oracle's counts (n_min, n_max: the smallest and largest pair of the call):
  * 1: every pair is cut to one record;
  * n_max - 1: only the largest pair is cut, by exactly one record (pos < cap against pos <= cap);
  * n_max: nothing is cut, and there is no slack behind the largest pair;
  * n_min // 2 + 3: every pair is cut mid-stream;
  * three pairs of unequal counts: a capacity strictly between n_min and n_max, so one launch cuts some pairs and not others;
  * the paths of two launches: a capacity that ends among the records of the launch over the larger bins.
The arrays hold one pair's worth of slots more than the call may touch, all filled with 0xA5: a record written past a
pair's capacity shows as a wrong word in the next pair's slots or in the spare ones, never as an access out of bounds.  The
launch path must not depend on the capacity: its recorded name at every short capacity equals the name at full capacity.
Both device forms return GPC_OK whatever the counts (the Context methods raise on any other status)."""
import ctypes as C

import numpy as np
import pytest

from devicewide_util import (FILL32, HJ, HM_BUCKETS, VJ4, VJ8, Case, compare, expected, filled, load_forest, make_ctx, path, run,
                             run_corr, shared, supp_words, textured)
from test_gpu_devicewide_paths import band_of_three, mostly_true_forest_text, one_banded, tex272, tex528   # the same Case objects

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fast():
    from oracle.pyoracle import Oracle
    return Oracle(fast=True)


def capacities(lens, between=False):
    """[(what, cap)] for one call whose pairs have `lens` records, preconditions asserted"""
    n_min, n_max = min(lens), max(lens)
    mid = n_min // 2 + 3
    assert 0 < mid < n_min and n_max >= 2, lens
    caps = [("one record", 1), ("the largest pair cut by one", n_max - 1), ("nothing cut", n_max), ("every pair cut", mid)]
    if between:
        assert n_min < n_max - 1, "the pairs' counts do not differ: %s" % (lens,)
        cap = (n_min + n_max) // 2
        assert n_min < cap < n_max and any(n <= cap for n in lens) and any(n > cap for n in lens)
        caps.append(("some pairs cut, some not", cap))
    return caps


def sweep(ctx, fast, c, epi, ht, name, what, corr_pair=0, between=False, more=((), ())):
    """full capacity (the path by `name`), then every short capacity on the same path: supports of the case's batch, then
    correspondences of [L, R, L] of pair corr_pair.  more: further (what, cap) for supports, for correspondences.  Returns
    the path name and the capacities used per mode."""
    full = run(ctx, fast, c, epi, ht, name, what + ", supports, full capacity")
    scaps = capacities([len(w[0]) for w in c.want(fast, epi, ht)], between) + list(more[0])
    for label, cap in scaps:
        run(ctx, fast, c, epi, ht, full, "%s, supports, cap %d (%s)" % (what, cap, label), cap=cap)
    cfull = run_corr(ctx, fast, c, corr_pair, epi, ht, name, what + ", correspondences, full capacity")
    ccaps = capacities([len(w) for w in c.want_corr(fast, corr_pair, epi, ht)[0]]) + list(more[1])
    for label, cap in ccaps:
        run_corr(ctx, fast, c, corr_pair, epi, ht, cfull, "%s, correspondences, cap %d (%s)" % (what, cap, label), cap=cap)
    assert cfull == full, (full, cfull)
    return full, [cap for _, cap in scaps], [cap for _, cap in ccaps]


def inside_the_larger_bins(big):
    """big[k]: record k of a pair's output comes from the launch over the larger bins.  A capacity that ends among them."""
    at = np.flatnonzero(big)
    assert len(at) >= 2 and not big.all(), "the pair's records come from one launch"
    cap = int(at[len(at) // 2]) + 1
    assert 0 < cap < len(big) and big[:cap].any() and not big[:cap].all() and big[cap:].any()
    return ("ends among the larger bins' records", cap)


def both_and_one_launch(big, caps, what):
    """Among the capacities that cut the pair, one leaves records of both launches in its slots and one leaves records of a
    single launch."""
    kinds = [set(big[:cap].tolist()) for cap in caps if cap < len(big)]
    assert any(len(k) == 2 for k in kinds) and any(len(k) == 1 for k in kinds), "%s: %s at capacities %s" % (what, kinds, caps)


# ------------------------------------------------------------------------------------------------- the code-range matcher
def test_code_ranges_one_launch(fast, forest_paths):
    """k_row_join<4, 1024, false, true> alone: k_gp_gather's `pos >= cap` for one pair (supports) and two (correspondences)"""
    c = tex272(fast, forest_paths)
    assert c.code_range_bins(0) <= 4096
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        sweep(ctx, fast, c, False, False, VJ4, "one launch")
    finally:
        ctx.close()


def test_code_ranges_side_launch_over_the_work_list(fast, forest_paths):
    """<8, 1024>[list] + <4, 1024>: three pairs of unequal counts, the middle one with bins of 4097 .. 8192 records a side;
    its frames [L, R, L] in correspondences mode.  A record belongs to the 8192-record launch when its code's bin holds more
    than 4096 records of a side (Case.code_range_hist): asserted on the CPU that some capacity keeps records of both launches
    in the middle pair's slots and another keeps records of one launch only."""
    c = band_of_three(fast, forest_paths, 150, 90)
    sides = [c.code_range_bins(i) for i in range(3)]
    assert sides[0] <= 4096 and 4096 < sides[1] <= 8192 and sides[2] <= 4096, sides
    hist = c.code_range_hist(1)
    large = (hist[0] > 4096) | (hist[1] > 4096)
    codes = c.hashed[1][0][0].reshape(c.H, c.W)   # (the middle pair's left image: the source of its records in both modes)
    w = c.want(fast, False, False)[1][0]
    sbig = large[c.code_range_of(codes[w["y"], w["x"]])]
    w = c.want_corr(fast, 1, False, False)[0][0]
    cbig = large[c.code_range_of(codes[w["sy"], w["sx"]])]
    more = ([inside_the_larger_bins(sbig)], [inside_the_larger_bins(cbig)])
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        took, scaps, ccaps = sweep(ctx, fast, c, False, False, VJ8 + "[list] + " + VJ4, "side launch", corr_pair=1, between=True,
                                   more=more)
        both_and_one_launch(sbig, scaps, "supports")
        both_and_one_launch(cbig, ccaps, "correspondences")
    finally:
        ctx.close()


def test_code_ranges_fall_back_to_the_sort(fast, forest_paths):
    """gpc::k_g_match: the plan is abandoned "with nothing written".  At a short capacity the abandoned plan must have left
    the fill intact as well -- in the slots behind `cap` and in the spare pair -- which is part of the byte comparison; then
    k_g_match's own `pos < cap`."""
    c = one_banded(fast, forest_paths, 190, 130)
    assert c.code_range_bins(0) > 8192
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        sweep(ctx, fast, c, False, False, "gpc::k_g_match", "fallback")
    finally:
        ctx.close()


def test_code_ranges_wide_codes(fast):
    """k_row_join<4, 1024, true, true>: 32-bit codes (SSE=OFF arithmetic, 32 tests)"""
    c = shared("wide272", lambda: Case(fast, None, [textured(272, 61, 4, 9)], naive=True, forest_text=mostly_true_forest_text(60)))
    assert c.bits == 32 and c.code_range_bins(0) <= 4096
    ctx = make_ctx(naive=True)
    try:
        load_forest(ctx, c)
        sweep(ctx, fast, c, False, False, "gpc::k_row_join<4, 1024, true, true>", "wide codes")
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------- the hash table
EPI = pytest.mark.parametrize("epi", [True, False])


@EPI
def test_hash_table_default_plan(fast, forest_paths, epi):
    """k_ht_join<4, 1024>: k_ht_gather's `pos >= cap`"""
    c = tex272(fast, forest_paths)
    assert c.bucket_bins(0, 10, epi) <= 4096
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        sweep(ctx, fast, c, epi, True, HJ % (4, 1024), "default plan")
    finally:
        ctx.close()


@EPI
@pytest.mark.parametrize("no_half", [False, True])
def test_hash_table_bins_of_512_buckets(fast, forest_paths, epi, no_half):
    """k_ht_join<4, 512> alone (GPC_HIP_HT_LBITS=9), and <4, 1024> over the same bins without halving (GPC_HIP_HT_NO_HALF): two
    pairs of unequal counts"""
    c = tex528(fast, forest_paths)
    assert max(c.bucket_bins(i, 9, epi) for i in range(c.B)) <= 2048
    env = {"GPC_HIP_HT_LBITS": 9}
    if no_half:
        env["GPC_HIP_HT_NO_HALF"] = 1
    ctx = make_ctx(env)
    try:
        load_forest(ctx, c)
        sweep(ctx, fast, c, epi, True, HJ % (4, 1024 if no_half else 512), "512 buckets per bin")
    finally:
        ctx.close()


def test_hash_table_larger_bins_beside_the_512_thread_join(fast, forest_paths):
    """<4, 1024>[list] + <4, 512>: three pairs of unequal counts, the middle one with a bin of 2049 .. 4096 records.  A record
    belongs to the 1024-thread launch when its bucket's bin holds more than 2048 records, left and right (Case.bucket_hist):
    asserted on the CPU that some capacity keeps records of both launches in the middle pair's slots and another keeps
    records of one launch only."""
    c = band_of_three(fast, forest_paths, 120, 60)
    bins = [c.bucket_bins(i, 9, False) for i in range(3)]
    assert bins[0] <= 2048 and 2048 < bins[1] <= 4096 and bins[2] <= 2048, bins
    large = c.bucket_hist(1, 9, False) > 2048
    codes = c.hashed[1][0][0].reshape(c.H, c.W)   # (the middle pair's left image: the source of its records in both modes)
    w = c.want(fast, False, True)[1][0]
    sbig = large[c.bucket_bin_of(codes[w["y"], w["x"]], w["y"], 9, False)]
    w = c.want_corr(fast, 1, False, True)[0][0]
    cbig = large[c.bucket_bin_of(codes[w["sy"], w["sx"]], w["sy"], 9, False)]
    more = ([inside_the_larger_bins(sbig)], [inside_the_larger_bins(cbig)])
    ctx = make_ctx({"GPC_HIP_HT_LBITS": 9})
    try:
        load_forest(ctx, c)
        name = (HJ % (4, 1024)) + "[list] + " + (HJ % (4, 512))
        took, scaps, ccaps = sweep(ctx, fast, c, False, True, name, "larger bins beside", corr_pair=1, between=True, more=more)
        both_and_one_launch(sbig, scaps, "supports")
        both_and_one_launch(cbig, ccaps, "correspondences")
    finally:
        ctx.close()


def test_hash_table_8192_record_bins(fast, forest_paths):
    """k_ht_join<8, 1024> after the planner has halved down to 128 buckets per bin: the earlier rounds wrote nothing"""
    c = one_banded(fast, forest_paths, 150, 90)
    assert all(4096 < c.bucket_bins(0, lbits, False) <= 8192 for lbits in (10, 9, 8, 7))
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        sweep(ctx, fast, c, False, True, HJ % (8, 1024), "8192-record bins")
    finally:
        ctx.close()


def test_hash_table_falls_back_to_the_sort(fast, forest_paths):
    """gpc::k_ht_pairs: every planning attempt is abandoned "with nothing written".  At a short capacity the abandoned
    attempts must have left the fill intact as well -- in the slots behind `cap` and in the spare pair -- which is part of
    the byte comparison; then k_ht_pairs' own `pos < cap`."""
    c = one_banded(fast, forest_paths, 190, 130)
    assert all(c.bucket_bins(0, lbits, False) > 8192 for lbits in (10, 9, 8, 7))
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        sweep(ctx, fast, c, False, True, "gpc::k_ht_pairs", "fallback")
    finally:
        ctx.close()


@pytest.mark.parametrize("epi,H", [(False, 400), (True, 520)])
def test_hash_table_second_planning_round(fast, forest_paths, epi, H):
    """The 1024 x H pair of test_gpu_devicewide_paths.py whose first round (1024 buckets per bin) overflows.  A context
    remembers the width a size ended at, so only a context's FIRST call at a size plans twice: the sweep's first call does
    so at full capacity, and a fresh context's first call does so at a short one, in either record mode -- the round that was
    abandoned wrote nothing, the second round's join cut at `cap`."""
    c = shared(("second", H), lambda: Case(fast, forest_paths["zero"], [textured(1024, H, 3, 21)]))
    assert 2 * c.cap * 0.7 / ((HM_BUCKETS >> 10) + 1) <= 3500.0, "the estimate no longer starts at 1024 buckets per bin"
    assert c.bucket_bins(0, 10, epi) > 4096 >= c.bucket_bins(0, 9, epi)
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        first, scaps, ccaps = sweep(ctx, fast, c, epi, True, None, "second round")
        assert first.startswith("gpc::k_ht_join<") and first.endswith(HJ % (4, 512)), first
    finally:
        ctx.close()
    for corr in (False, True):
        ctx = make_ctx()
        try:
            load_forest(ctx, c)
            if corr:
                run_corr(ctx, fast, c, 0, epi, True, first, "second round at a short capacity, correspondences", cap=ccaps[1])
            else:
                run(ctx, fast, c, epi, True, first, "second round at a short capacity, supports", cap=scaps[1])
        finally:
            ctx.close()


# -------------------------------------------------------------------------------------------------------------- group mode
def test_group_union_of_unequal_groups(oracle):
    """Group mode, sort matcher, non-epipolar: the forest of 32 / 26 / 16 tests of test_gpu_forest_shapes.py at 176x67 (the
    narrow groups take the 8192-record join over the work list) on a batch of two pairs, the pair and its mirror.  The
    groups' joins write a workspace at full capacity; k_group_union places the kept records and is what `cap` cuts
    (`keep && at < cap`): n_max - 1 and 1, every word against the oracle's union, fill elsewhere."""
    import torch
    import opengpc_amd as g
    from forest_groups_util import forest_text, group_texts
    from test_gpu_forest_groups import gsettings, oracle_union_pair
    W, H = 176, 67
    text = forest_text([32, 5, 1, 20, 7, 9], seed=6, scales="sml")
    texts = group_texts(text)
    st, groups = g.parse_forest_groups(text, W, H)
    assert st == 0 and [x.num_tests for x in groups] == [32, 26, 16]
    L, R = oracle.synth_pair(W, H, 3, 9)
    pairs = [(L, R), (R, L)]
    want = [oracle_union_pair(oracle, texts, a, b, False) for a, b in pairs]
    words = [supp_words(w) for w, _ in want]
    n_min, n_max = min(len(w) for w in words), max(len(w) for w in words)
    assert n_min >= 2
    dev = torch.device("cuda", 0)
    d_L = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
    d_R = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    ctx = make_ctx()
    try:
        ctx.set_forest_groups(groups)
        names = []
        for cap in (3 * (W - 26) * (H - 26), n_max - 1, 1):
            d_out, d_cnt, d_nc = filled(3 * cap * 12, dev), filled(3 * 4, dev), filled(3 * 8, dev)
            torch.cuda.synchronize(dev)
            ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, 2, gsettings(False), d_out.data_ptr(), cap, d_cnt.data_ptr(),
                                   d_nc.data_ptr())
            ctx.synchronize()
            names.append(path(ctx))
            cnt, nc = d_cnt.cpu().numpy().view(np.int32), d_nc.cpu().numpy().view(np.int32).reshape(3, 2)
            for p in range(2):
                assert cnt[p] == len(words[p]), "cap %d, pair %d: count %d, the oracle's union %d" % (cap, p, cnt[p], len(words[p]))
                assert tuple(nc[p]) == tuple(want[p][1]), (cap, p)
            assert cnt[2:].view(np.uint32) == FILL32 and (nc[2:].view(np.uint32) == FILL32).all()
            compare(d_out.cpu().numpy().view(np.uint32).reshape(3, cap, 3), expected(words, cap), words, "group union, cap %d" % cap)
        assert names[0] == VJ8 + "[list] + " + VJ4 and names[1] == names[2] == names[0], names
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- fetch again after a short fetch
@pytest.mark.parametrize("epi,ht", [(True, False), (False, False), (True, True), (False, True)])
def test_fetch_again_after_a_short_fetch(fast, forest_paths, epi, ht):
    """gpc_hip_match_fetch: "the results stay until the next call on the context".  A fetch with half the room returns
    GPC_E_CAPACITY, the true count and the first cap records, and leaves the caller's array behind them alone; a second
    fetch with room for all returns GPC_OK and every record.  (tests/test_resident.py::test_two_step_forms fetches twice
    through Context.match_async, which compares the two fetches with each other over the first cap records; here both are
    compared with the oracle, and the array behind the short fetch with its fill.)"""
    import opengpc_amd as g
    from oracle.pyoracle import sparsematch_settings
    W, H = 176, 67
    L, R = (np.ascontiguousarray(a, np.uint8) for a in textured(W, H, 5, 9))
    rc, f = fast.read_forest(forest_paths["tau"], W, H)
    assert rc == 0
    want, nl, nr = fast.match_pair(L, R, f, sparsematch_settings(5, 128, 1, epi, ht, False))
    words = supp_words(want)
    n = len(words)
    cap = n // 2
    assert 0 < cap < n
    ctx = make_ctx()
    try:
        ctx.load_forest(forest_paths["tau"], W, H)
        gs = g.Settings(5, 128, 1, epi, ht, 1)
        assert ctx.L.gpc_hip_match_pair_begin(ctx.h, L.ctypes.data, R.ctypes.data, W, H, C.byref(gs)) == 0
        got = np.full((n + 8, 3), FILL32, np.uint32)
        k, cl, cr = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        st = ctx.L.gpc_hip_match_fetch(ctx.h, got.ctypes.data, cap, C.byref(k), C.byref(cl), C.byref(cr))
        assert st == g.capi.E_CAPACITY and k.value == n and (cl.value, cr.value) == (nl, nr)
        assert np.array_equal(got[:cap], words[:cap]), "the first cap records"
        assert (got[cap:] == FILL32).all(), "written behind the capacity"
        got = np.full((n + 8, 3), FILL32, np.uint32)
        k, cl, cr = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        st = ctx.L.gpc_hip_match_fetch(ctx.h, got.ctypes.data, n, C.byref(k), C.byref(cl), C.byref(cr))
        assert st == 0 and k.value == n and (cl.value, cr.value) == (nl, nr)
        assert np.array_equal(got[:n], words) and (got[n:] == FILL32).all()
    finally:
        ctx.close()
