"""The fused join's scheduling space against the CPU oracle, at shapes small enough that a failure names a pair and a row.

k_row_join_fused (opengpc_amd/csrc/k_rowjoin_fused.h) hands rows out from ticket counters sharded over the pairs, turns a
ticket into (pair, row) with a host-made multiply-high, finds each row's place in the output by a look-back between
workgroups and writes a row's records one row late.  A mistake in any of these puts right records in a wrong place or skips
a row, and nothing returns a status.  Every case here runs a batch of banded synthetic pairs through one setting of the
knobs that shape that schedule (GPC_HIP_FUSE_ALWAYS / _WGS / _SHARDS, GPC_HIP_JOIN_NT, two lanes) and compares EVERY BYTE of
the outputs with the oracle's match_pair per pair: outputs start filled with 0xA5, records below min(count, cap) equal the
oracle's, everything behind them -- a spare pair's worth of array behind the last pair included -- still holds the fill.

The rule of this module: no case asks for more workgroups than the device holds resident, and contexts are created, used
and closed one after the other (the knobs are read when a context is created)."""
import os

import numpy as np
import pytest

from oracle.pyoracle import sparsematch_settings

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FILL = 0xA5
FILL32 = np.uint32(0xA5A5A5A5)
R = 13  # patch radius: rows 13 .. H - 14 hold candidates


# ---------------------------------------------------------------------------------------------------------------- inputs
def seeds_for(n, first=0):
    """synth_batch's pair i has disparity 8 + i % 64.  Seeds whose disparity is 9, 10, 11, 13, 14 or 15: 96-pixel rows keep
    most of their overlap, and no pair has twice the supports of another (disparities 8 and 12 sit on the texture's 4-pixel
    grid and give 525 and 261 supports at 96x40 where the others give 300 .. 380)."""
    offs = (1, 2, 3, 5, 6, 7)
    return [64 * ((first + j) // 6) + offs[(first + j) % 6] for j in range(n)]


def band_of(H):
    """the constant rows of a banded pair: a quarter of the candidate rows (five at least), a third of the way down"""
    n = max(5, (H - 2 * R) // 4)
    return R + (H - 2 * R) // 3, n


def banded_batch(W, H, seeds, every=2, band=None):
    """synth_batch with a band of constant rows in BOTH images of pairs 1, 3, 5, ... (every = 1: of every pair): the rows
    inside the band have no candidates, so rows in the middle of a pair publish a count of 0."""
    from opengpc_amd.synth import synth_batch
    L, Rr = synth_batch(W, H, seeds)
    y0, n = band or band_of(H)
    for j in range(every - 1, len(seeds), every):
        L[j, y0:y0 + n] = 77
        Rr[j, y0:y0 + n] = 77
    return L, Rr


class Case:
    """A batch, the oracle's answer per pair, and the conditions that keep a degenerate input from passing silently --
    asserted on the oracle's result alone, before anything runs on the device."""

    def __init__(self, fast, forest, W, H, seeds, every=2, band=None, naive=False, forest_text=None):
        self.W, self.H, self.B = W, H, len(seeds)
        self.L, self.R = banded_batch(W, H, seeds, every, band)
        if forest_text is not None:
            rc, f = fast.parse_forest_text(forest_text, W, H)
        else:
            rc, f = fast.read_forest(forest, W, H)
        assert rc == 0
        self.forest, self.forest_text, self.oracle_forest = forest, forest_text, f
        st = sparsematch_settings(5, 128, 0, True, False, naive)
        self.want = [fast.match_pair(self.L[i], self.R[i], f, st) for i in range(self.B)]
        self.rows = [np.bincount(w["y"], minlength=H)[:H] for w, _, _ in self.want]
        self.banded = [every == 1 or i % every == every - 1 for i in range(self.B)]
        self.cap_full = (W - 2 * R) * (H - 2 * R)
        # a capacity that cuts pair 0 in the middle of a row
        self.cap_short = len(self.want[0][0]) // 2 + 3
        self.check_inputs()

    def sub(self, B):
        """the first B pairs of this case (the oracle ran once per pair, not once per batch size)"""
        c = object.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.B, c.L, c.R = B, self.L[:B], self.R[:B]
        c.want, c.rows, c.banded = self.want[:B], self.rows[:B], self.banded[:B]
        return c

    def check_inputs(self):
        H = self.H
        for i in range(self.B):
            r = self.rows[i][R:H - R]
            assert r.sum() == len(self.want[i][0]) and self.rows[i][:R].sum() == 0 and self.rows[i][H - R:].sum() == 0
            assert 2 * np.count_nonzero(r) >= len(r), ("pair %d: supports in fewer than half of its rows" % i, r)
            if self.banded[i]:
                assert any(r[:z].any() and r[z + 1:].any() for z in np.flatnonzero(r == 0)), \
                    ("pair %d: no empty row between rows with supports" % i, r)
            assert len(self.want[i][0]) > self.cap_short, ("pair %d: its total does not exceed the short capacity" % i)
        ends = np.cumsum(self.rows[0])
        assert 0 < self.cap_short < ends[-1] and self.cap_short not in ends, "the short capacity falls on a row boundary"


def fast_oracle():
    from oracle.pyoracle import Oracle
    return Oracle(fast=True)


@pytest.fixture(scope="module")
def fast():
    return fast_oracle()


_cases = {}


def case(fast, forest, W, H, B, first=0, every=2, band=None):
    """cases are computed once and shared, unchanged, among the tests that need them"""
    key = (forest, W, H, first, every, band)
    have = _cases.get(key)
    if have is None or have.B < B:
        have = _cases[key] = Case(fast, forest, W, H, seeds_for(B, first), every, band)
    return have if have.B == B else have.sub(B)


# --------------------------------------------------------------------------------------------------------------- harness
def make_ctx(env, naive=False):
    """the knobs are read in gpc_hip_create: set, create, delete"""
    import opengpc_amd as g
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        c = g.Context(0)
    finally:
        for k in env:
            del os.environ[k]
    if naive:
        c.set_arithmetic(True)
    return c


def load_forest(ctx, c):
    import opengpc_amd as g
    if c.forest_text is not None:
        st, fm = g.parse_forest(c.forest_text, c.W, c.H)
        assert st == 0
        ctx.set_forest(fm)
    else:
        ctx.load_forest(c.forest, c.W, c.H)


def filled(nbytes, dev):
    """nbytes of device memory holding the fill (the library's streams do not wait for torch's: settle() before a launch)"""
    import torch
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev)


def settle(dev):
    import torch
    torch.cuda.synchronize(dev)


def upload(c, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(c.L)).to(dev), torch.from_numpy(np.ascontiguousarray(c.R)).to(dev)


def first_difference(got, exp, c, i, cap, what):
    """which pair, which record, which row: the message of a failed comparison"""
    bad = np.flatnonzero((got != exp).reshape(len(got), -1).any(axis=1))
    j = int(bad[0])
    w = c.want[i][0] if i < c.B else []
    where = "record %d of %d (row %d)" % (j, len(w), w["y"][j]) if j < min(len(w), cap) else \
        "slot %d, behind the %d records the pair may hold at capacity %d" % (j, min(len(w), cap), cap)
    return "%s: %dx%d, %d pairs, pair %d%s: %s holds %s, expected %s; %d slots differ, the last is %d" % (
        what, c.W, c.H, c.B, i, " (the spare array behind the last pair)" if i >= c.B else "", where, got[j], exp[j], len(bad), int(bad[-1]))


def check_counts(c, cnt, nc, what):
    for i in range(c.B):
        w, nl, nr = c.want[i]
        assert cnt[i] == len(w), "%s: pair %d of %d counts %d supports, the oracle %d" % (what, i, c.B, cnt[i], len(w))
        assert tuple(nc[i]) == (nl, nr), "%s: pair %d of %d: candidates %s, the oracle's %s" % (what, i, c.B, tuple(nc[i]), (nl, nr))
    # the spare entries behind the batch's
    assert (cnt[c.B:].view(np.uint32) == FILL32).all() and (nc[c.B:].view(np.uint32) == FILL32).all(), what + ": a count behind the batch's was written"


def run_records(ctx, c, d_L, d_R, cap, dev, what):
    """12-byte records (gpc_hip_match_batch_device), whole arrays compared"""
    import opengpc_amd as g
    B = c.B
    d_out, d_cnt, d_nc = filled((B + 1) * cap * 12, dev), filled((B + 1) * 4, dev), filled((B + 1) * 8, dev)
    settle(dev)
    ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), c.W, c.H, B, g.Settings.sparsematch(), d_out.data_ptr(), cap,
                           d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    verify_records(c, cap, d_out, d_cnt, d_nc, what)


def verify_records(c, cap, d_out, d_cnt, d_nc, what):
    B = c.B
    out = d_out.cpu().numpy().view(np.uint32).reshape(B + 1, cap, 3)
    check_counts(c, d_cnt.cpu().numpy().view(np.int32), d_nc.cpu().numpy().view(np.int32).reshape(B + 1, 2), what)
    for i in range(B + 1):
        exp = np.full((cap, 3), FILL32, np.uint32)
        if i < B:
            w = c.want[i][0]
            k = min(cap, len(w))
            exp[:k, 0], exp[:k, 1] = w["x"][:k], w["y"][:k]
            exp[:k, 2] = np.ascontiguousarray(w["d"][:k], np.float32).view(np.uint32)
        if not np.array_equal(out[i], exp):
            raise AssertionError(first_difference(out[i], exp, c, i, cap, what))


def run_packed(ctx, c, d_L, d_R, cap, dev, what):
    """packed words + per-row counts (gpc_hip_match_batch_device_packed): the words behind a pair's count and the rows outside
    13 .. H - 14 (include/gpc_hip.h: "not written") keep the fill; expanded, the words are the oracle's records"""
    import opengpc_amd as g
    B, H = c.B, c.H
    d_pk, d_rows = filled((B + 1) * cap * 4, dev), filled((B + 1) * H * 4, dev)
    d_cnt, d_nc = filled((B + 1) * 4, dev), filled((B + 1) * 8, dev)
    settle(dev)
    ctx.match_batch_device_packed(d_L.data_ptr(), d_R.data_ptr(), c.W, H, B, g.Settings.sparsematch(), d_pk.data_ptr(), cap,
                                  d_rows.data_ptr(), d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    pk = d_pk.cpu().numpy().view(np.uint32).reshape(B + 1, cap, 1)
    rows = d_rows.cpu().numpy().view(np.int32).reshape(B + 1, H)
    check_counts(c, d_cnt.cpu().numpy().view(np.int32), d_nc.cpu().numpy().view(np.int32).reshape(B + 1, 2), what)
    for i in range(B + 1):
        exp = np.full((cap, 1), FILL32, np.uint32)
        exp_rows = np.full(H, FILL32, np.uint32).view(np.int32)
        if i < B:
            w = c.want[i][0]
            k = min(cap, len(w))
            xr = w["x"][:k] - w["d"][:k].astype(np.int32)
            exp[:k, 0] = w["x"][:k].astype(np.uint32) | (xr.astype(np.uint32) << 16)
            exp_rows[R:H - R] = c.rows[i][R:H - R]
        if not np.array_equal(pk[i], exp):
            raise AssertionError(first_difference(pk[i], exp, c, i, cap, what))
        assert np.array_equal(rows[i], exp_rows), "%s: pair %d of %d: row counts %s, expected %s" % (what, i, B, rows[i], exp_rows)
        if i < B and cap >= len(c.want[i][0]):
            clean = np.zeros(H, np.int32)
            clean[R:H - R] = rows[i, R:H - R]
            got = g.capi.expand_packed(pk[i, :, 0], clean, len(w))
            assert np.array_equal(got, w.astype(got.dtype)), "%s: pair %d of %d: the expanded records differ" % (what, i, B)


def run_case(ctx, c, dev, what, packed=False):
    """a case at the full capacity and at one that cuts pair 0 in the middle of a row (the count stays the full count)"""
    load_forest(ctx, c)
    d_L, d_R = upload(c, dev)
    for cap in (c.cap_full, c.cap_short):
        run_records(ctx, c, d_L, d_R, cap, dev, "%s, capacity %d" % (what, cap))
        if packed:
            run_packed(ctx, c, d_L, d_R, cap, dev, "%s, packed, capacity %d" % (what, cap))


def device():
    import torch
    return torch.device("cuda", 0)


def join_name(ctx):
    return ctx.kernel_launch_names()["k_row_join"]


# ----------------------------------------------------------------------------------------------------------------- cases
BATCH_SIZES = list(range(1, 41)) + [41, 44, 47, 50, 53, 56, 59, 62, 63, 64, 65, 67, 70]


def test_every_split_of_pairs_over_shards(fast, forest_paths):
    """96x40 (14 rows, <1, 256>), every batch size 1 .. 40 and 41 .. 70 in steps (63, 64, 65, 70 among them), launch after
    launch on ONE context with the default shards and grid: every ps, n_hi and divisor join_shards makes for these sizes,
    with counters and epochs carried over between launches of different geometry."""
    dev = device()
    all70 = case(fast, forest_paths["tau"], 96, 40, 70)
    ctx = make_ctx({"GPC_HIP_FUSE_ALWAYS": 1})
    try:
        for B in BATCH_SIZES:
            run_case(ctx, all70.sub(B), dev, "%d pairs" % B)
            assert join_name(ctx) == "gpc::k_row_join_fused<1, 256, false>"
    finally:
        ctx.close()


@pytest.mark.parametrize("shards", [1, 2, 8, 16, 23, 64])
def test_forced_shard_counts(fast, forest_paths, shards):
    """GPC_HIP_FUSE_SHARDS (clamped to the pairs and to RJ_SHARDS by the library), 23 pairs of 96x40"""
    c = case(fast, forest_paths["tau"], 96, 40, 70).sub(23)
    ctx = make_ctx({"GPC_HIP_FUSE_ALWAYS": 1, "GPC_HIP_FUSE_SHARDS": shards})
    try:
        for rep in range(2):
            run_case(ctx, c, device(), "%d shards forced, launch %d" % (shards, rep))
        assert join_name(ctx).startswith("gpc::k_row_join_fused<")
    finally:
        ctx.close()


FEW_SHAPES = [(96, 40), (528, 56), (1040, 44)]
FEW_NAMES = {96: "gpc::k_row_join_fused<1, 256, false>", 528: "gpc::k_row_join_fused<4, 256, false>",
             1040: "gpc::k_row_join_fused<4, 512, false>"}


@pytest.mark.parametrize("wgs", [1, 2, 3, 5, 16, 61])
def test_few_workgroups_many_rows_each(fast, forest_paths, wgs):
    """GPC_HIP_FUSE_WGS: a grid far below what the device holds, so every workgroup takes many rows and the pending row
    whose records leave one row late belongs to ANOTHER pair than the row being joined at every pair boundary.  One workgroup:
    the host clamps the shards to one and a single workgroup walks every row of every pair; 2 or 3: shards unequal in pairs;
    5 or 61: shards unequal in workgroups (the draw that resets a shard's counter, f_last).  1, 7 and 10 pairs of 96x40,
    528x56 and 1040x44, in the order big, small, big, small, twice over on one context: the granule array is used again at
    another pairs x rows layout with stale epochs lying in it."""
    dev = device()
    cases = [case(fast, forest_paths["tau"], W, H, 10).sub(B) for (W, H) in FEW_SHAPES for B in (1, 7, 10)]
    cases.sort(key=lambda c: -c.B * (c.H - 2 * R))
    order = []
    while cases:
        order.append(cases.pop(0))
        if cases:
            order.append(cases.pop())
    ctx = make_ctx({"GPC_HIP_FUSE_ALWAYS": 1, "GPC_HIP_FUSE_WGS": wgs})
    try:
        for rep in range(2):
            for c in order:
                run_case(ctx, c, dev, "%d workgroups, round %d" % (wgs, rep))
                assert join_name(ctx) == FEW_NAMES[c.W]
    finally:
        ctx.close()


@pytest.mark.parametrize("B,wgs", [(1, None), (2, None), (1, 1)])
def test_long_look_back(fast, forest_paths, B, wgs):
    """Pairs of 96x426 (400 rows each) with the default grid: all rows of a pair are in flight together, so the nearest
    published prefix can lie further back than the first window of 64 rows and than the four windows of a round; every pair
    carries a band of 100 constant rows, so whole windows of zero counts occur.  The same pair with one workgroup, where
    every look-back finds its prefix in the row before.  (Which window path a run took cannot be asserted from here: the shape
    makes those paths reachable, it does not prove them taken.)"""
    c = case(fast, forest_paths["tau"], 96, 426, 2, every=1, band=(150, 100)).sub(B)
    env = {"GPC_HIP_FUSE_ALWAYS": 1}
    if wgs:
        env["GPC_HIP_FUSE_WGS"] = wgs
    ctx = make_ctx(env)
    try:
        for rep in range(2):
            run_case(ctx, c, device(), "400 rows, %s workgroups, launch %d" % (wgs or "default", rep), packed=True)
        assert join_name(ctx) == "gpc::k_row_join_fused<1, 256, false>"
    finally:
        ctx.close()


PLANS = [(None, 96, "<1, 256, false>"), (None, 272, "<2, 256, false>"), (None, 528, "<4, 256, false>"),
         (None, 1040, "<4, 512, false>"), (None, 2064, "<4, 1024, false>"),
         (512, 96, "<1, 512, false>"), (512, 528, "<2, 512, false>"), (1024, 96, "<1, 1024, false>"), (1024, 1040, "<2, 1024, false>")]


@pytest.mark.parametrize("nt,W,inst", PLANS)
def test_every_instantiation(fast, forest_paths, nt, W, inst):
    """The natural plans and the four that only GPC_HIP_JOIN_NT reaches, three pairs of W x 44 on four workgroups (several
    rows each); the launch's name says that the intended instantiation ran."""
    c = case(fast, forest_paths["tau"], W, 44, 3)
    env = {"GPC_HIP_FUSE_ALWAYS": 1, "GPC_HIP_FUSE_WGS": 4}
    if nt:
        env["GPC_HIP_JOIN_NT"] = nt
    ctx = make_ctx(env)
    try:
        for rep in range(2):
            run_case(ctx, c, device(), "k_row_join_fused%s, launch %d" % (inst, rep), packed=True)
            assert join_name(ctx) == "gpc::k_row_join_fused" + inst
    finally:
        ctx.close()


def mostly_true_forest_text(tau):
    """32 tests that hold for most pixels under the SSE=OFF predicate (as tests/test_naive_mode.py builds it): many
    candidates then carry the all-ones code"""
    rng = np.random.default_rng(1234)
    lines = ["4"]
    for fern in range(4):
        lines.append("%d l 8" % fern)
        for t in range(8):
            ix, iy, jx, jy = rng.integers(-13, 14, 4)
            lines.append("%d %d %d %d %d %d" % (t, ix, iy, jx, jy, tau))
    return "\n".join(lines)


@pytest.mark.parametrize("W,inst", [(96, "<1, 256, true>"), (528, "<4, 256, true>")])
def test_wide_instantiations(fast, W, inst):
    """SSE=OFF arithmetic with a 32-test forest (codes use bit 31, 0xFFFFFFFF is a code that has no key in the join's table)
    against the oracle's naive path, three pairs on four workgroups.  The inputs produce the all-ones code on both sides."""
    text = mostly_true_forest_text(60)
    c = Case(fast, None, W, 44, seeds_for(3), naive=True, forest_text=text)
    for side in (c.L, c.R):
        ones = bit31 = 0
        for img in side:
            sm, gr, m = fast.preprocess_naive(img, 5)
            codes = fast.hash_naive(sm, m, c.oracle_forest).reshape(-1)[m]
            ones += int((codes == 0xFFFFFFFF).sum())
            bit31 += int((codes >> 31).sum())
        assert ones > 0 and bit31 > 0
    ctx = make_ctx({"GPC_HIP_FUSE_ALWAYS": 1, "GPC_HIP_FUSE_WGS": 4}, naive=True)
    try:
        for rep in range(2):
            run_case(ctx, c, device(), "k_row_join_fused%s, launch %d" % (inst, rep), packed=True)
            assert join_name(ctx) == "gpc::k_row_join_fused" + inst
    finally:
        ctx.close()


def test_three_output_modes_on_three_workgroups(fast, forest_paths):
    """GPC_HIP_FUSE_WGS=3, five pairs of 272x61: 12-byte records, packed words + row counts, and stereoMatch's
    correspondences of one pair on the same context against the oracle's"""
    import opengpc_amd as g
    c = case(fast, forest_paths["tau"], 272, 61, 5)
    ctx = make_ctx({"GPC_HIP_FUSE_ALWAYS": 1, "GPC_HIP_FUSE_WGS": 3})
    try:
        run_case(ctx, c, device(), "three workgroups", packed=True)
        W, H, f = c.W, c.H, c.oracle_forest
        for i in (1, 0):
            pl, pr = fast.preprocess(c.L[i], 5), fast.preprocess(c.R[i], 5)
            want = fast.find_correspondences(fast.descriptors(fast.hash(pl[0], pl[1], f), pl[2], W, True), pl[2],
                                             fast.descriptors(fast.hash(pr[0], pr[1], f), pr[2], W, True), pr[2], W)
            got, n, st = ctx.stereo_match(pl, pr, g.Settings(5, 128, 0, True, False, 1))
            assert st == 0 and n == len(want) and n >= len(c.want[i][0]) > 0
            assert join_name(ctx) == "gpc::k_row_join_fused<2, 256, false>"
            for a, b in (("src_x", "sx"), ("src_y", "sy"), ("tar_x", "tx"), ("tar_y", "ty")):
                assert np.array_equal(got[a], want[b]), "stereo_match, pair %d: %s differs" % (i, a)
        run_case(ctx, c, device(), "three workgroups, after the correspondences", packed=True)
    finally:
        ctx.close()


def test_two_lanes_small(fast, forest_paths):
    """gpc_hip_set_pipeline(2) with the default grid: six batches of nine pairs of 272x61, different pairs in each, queued
    back to back three times over -- every batch against the oracle, byte for byte"""
    import opengpc_amd as g
    dev = device()
    NB, B = 6, 9
    batches = [case(fast, forest_paths["tau"], 272, 61, B, first=B * k) for k in range(NB)]
    ctx = make_ctx({"GPC_HIP_FUSE_ALWAYS": 1})
    try:
        load_forest(ctx, batches[0])
        ctx.set_pipeline(2)
        ins = [upload(c, dev) for c in batches]
        for cap_of in (lambda c: c.cap_full, lambda c: c.cap_short):
            outs = [(filled((B + 1) * cap_of(c) * 12, dev), filled((B + 1) * 4, dev), filled((B + 1) * 8, dev)) for c in batches]
            settle(dev)
            for rep in range(3):  # (the lanes' first calls allocate: later rounds run with everything in place)
                for c, (d_L, d_R), (o, n, nc) in zip(batches, ins, outs):
                    ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), c.W, c.H, B, g.Settings.sparsematch(), o.data_ptr(), cap_of(c),
                                           n.data_ptr(), nc.data_ptr())
            ctx.synchronize()
            assert join_name(ctx) == "gpc::k_row_join_fused<2, 256, false>"
            for k, (c, (o, n, nc)) in enumerate(zip(batches, outs)):
                verify_records(c, cap_of(c), o, n, nc, "two lanes, batch %d, capacity %d" % (k, cap_of(c)))
    finally:
        ctx.close()
