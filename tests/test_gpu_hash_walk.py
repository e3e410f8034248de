"""k_hash's walk over several tiles per workgroup against the CPU oracle, at shapes small enough that a failure names a tile.

On the benchmark's launches a workgroup of k_hash (opengpc_amd/csrc/k_hash_body.h) walks `tpw` vertically adjacent tiles:
it prefetches the next tile's window while the current one is tested, restages LDS behind a barrier, carries the candidate
count, the last candidate row and the OR of the codes across the tiles, caps its waves' priorities by the tiles it has left
in the launch's last round, and stops early where a column's last workgroup has fewer tiles.  run_hash (gpc_hip.hip) gives a
workgroup more than one tile only from about a thousand tiles on, so every small launch of the suite runs tpw = 1.  Here
GPC_HIP_HASH_TPW forces 1, 2, 3, 4, 5 and 64 tiles (clamped to the column's) at 96 and 272 pixels by 91, 122 and 155 rows:
two to five tiles of 32 or 40 rows (GPC_HIP_HASH_TALL) with a ragged last one, down to the single row H - 14.  Every case
first asserts gpc_hip_hash_plan against the plan restated from the shape (a knob that did not take effect fails there), then
compares every byte of the outputs -- filled with 0xA5 before the call -- with the oracle, and last the results of the
different tpw with each other.  The inputs and what the oracle must show for them: hash_walk_util.py.

Contexts are created under the knobs, used and closed one after the other."""
import numpy as np
import pytest

import hash_walk_util as hw
from devicewide_util import Case, load_forest, make_ctx, run, run_corr, shared
from forest_groups_util import forest_text, group_texts
from test_gpu_forest_groups import STRESS, oracle_union_pair

pytestmark = pytest.mark.gpu

# 32 tests: the last byte plane of the SSE codes is full (7 tests), the SSE=OFF codes use bit 31 (WIDE joins)
TEXT32 = {"zero": forest_text([16, 16], seed=7, tau=False), "tau": forest_text([16, 16], seed=8, tau=True)}
SHAPE_IDS = ["%dx%d" % s for s in hw.SHAPES]


@pytest.fixture(scope="module")
def fast():
    from oracle.pyoracle import Oracle
    return Oracle(fast=True)


@pytest.fixture(scope="module")
def cus():
    return hw.device_cus()


def settings(epi=True, ht=False, vtol=1):
    import opengpc_amd as g
    return g.Settings(hw.THR, 128, vtol, epi, ht, 1)


def walk_case(fast, forest_paths, W, H, kind, fkey, naive=False):
    """the two pairs of input `kind` with the oracle's answer under one forest ("zero" / "tau": the default forests, SSE;
    naive: the 32-test texts); the input's conditions are asserted when the case is made"""
    def make():
        c = Case(fast, None if naive else forest_paths[fkey], hw.walk_pairs(W, H, kind, naive), naive=naive,
                 forest_text=TEXT32[fkey] if naive else None, thr=hw.THR)
        hw.conditions(c, kind, [w[0] for w in c.want(fast, True, False)], "%dx%d input %s, %s%s" % (W, H, kind, "naive " if naive else "", fkey))
        return c
    return shared(("walk", W, H, kind, fkey, naive), make)


def hash_name(ctx):
    return ctx.kernel_launch_names()["k_hash"]


class Report:
    """failed comparisons of one test, gathered so that "differs between tpw" is reported beside "differs from the oracle" """

    def __init__(self):
        self.errors = []

    def check(self, fn, *args):
        try:
            fn(*args)
        except AssertionError as e:
            self.errors.append(str(e))

    def done(self):
        assert not self.errors, "%d comparisons failed:\n%s" % (len(self.errors), "\n".join(self.errors[:12]))


def batch_walk(fast, forest_paths, cus, W, H, env, tpws, ty, fkeys, naive, gbits):
    """the B = 2 batch of every input under every forest at every tpw: plan, launch name, every byte, then tpw against tpw"""
    rep, results = Report(), {}
    for tpw in tpws:
        ctx = make_ctx(dict(env, GPC_HIP_HASH_TPW=tpw), naive=naive)
        try:
            for fkey in fkeys:
                for kind in hw.KINDS:
                    c = walk_case(fast, forest_paths, W, H, kind, fkey, naive)
                    what = "%dx%d, input %s, %s, %d-row tiles, tpw %d" % (W, H, kind, fkey, ty, tpw)
                    load_forest(ctx, c)
                    got = hw.launch_batch(ctx, c, settings(), c.cap)
                    assert ctx.hash_plan() == hw.plan(W, H, 2 * c.B, ty, tpw, cus), (what, ctx.hash_plan())
                    assert hash_name(ctx) == "gpc::k_hash<%s, false, %s, %s, %d>" % (
                        "true" if c.f.type else "false", "true" if naive else "false", "true" if gbits else "false", ty), (what, hash_name(ctx))
                    rep.check(hw.check_batch, got, c.want(fast, True, False), what)
                    results.setdefault((fkey, kind), {})[tpw] = got
        finally:
            ctx.close()
    for (fkey, kind), r in results.items():
        rep.check(hw.same_across, r, "%dx%d, input %s, %s, %d-row tiles" % (W, H, kind, fkey, ty))
    rep.done()


# ------------------------------------------------------------------------------------------------------------------ plan
def test_plan_before_any_launch_and_the_split_of_five_tiles():
    """gpc_hip_hash_plan refuses before the context's first k_hash launch; the table of the five-tile column restated"""
    import opengpc_amd as g
    ctx = make_ctx()
    try:
        with pytest.raises(g.GpcError) as e:
            ctx.hash_plan()
        assert e.value.status == g.capi.E_INVALID
    finally:
        ctx.close()
    assert [hw.split(5, t) for t in (1, 2, 3, 4, 5, 64)] == [[1] * 5, [2, 2, 1], [3, 2], [4, 1], [5], [5]]
    assert [b - a for a, b in hw.tile_rows(91, 32)] == [32, 32, 1] and [b - a for a, b in hw.tile_rows(91, 40)] == [40, 25]
    assert [b - a for a, b in hw.tile_rows(122, 32)] == [32] * 3 and [b - a for a, b in hw.tile_rows(122, 40)] == [40, 40, 16]
    assert [b - a for a, b in hw.tile_rows(155, 32)] == [32] * 4 + [1] and [b - a for a, b in hw.tile_rows(155, 40)] == [40] * 3 + [9]


# ----------------------------------------------------------------------------------------------------- 1. dense code image
@pytest.mark.parametrize("W,H", hw.SHAPES, ids=SHAPE_IDS)
def test_hash_codes_every_tpw(fast, cus, W, H):
    """Context.hash_codes (dense, byte gradient image, 32-row tiles): SSE and SSE=OFF codes of 32-test forests without and
    with taus, the whole code image of every input against oracle.hash / hash_naive"""
    import opengpc_amd as g
    rep, results = Report(), {}
    for tpw in hw.TPWS:
        ctx = make_ctx({"GPC_HIP_HASH_TPW": tpw})
        try:
            for fkey, text in TEXT32.items():
                rc, f = fast.parse_forest_text(text, W, H)
                st, fm = g.parse_forest(text, W, H)
                assert (rc, st) == (0, 0) and fm.num_tests == f.num_tests == 32
                ctx.set_forest(fm)
                for naive in (False, True):
                    ctx.set_arithmetic(naive)
                    for kind in hw.KINDS:
                        def planes():
                            sm, gr, mk = (fast.preprocess_naive if naive else fast.preprocess)(hw.walk_pairs(W, H, kind, naive)[0][0], hw.THR)
                            want = fast.hash_naive(sm, mk, f) if naive else fast.hash(sm, gr, f)
                            assert want.any()
                            return sm, gr, want
                        sm, gr, want = shared(("walk codes", W, H, kind, fkey, naive), planes)
                        what = "%dx%d, input %s, %s %s, tpw %d" % (W, H, kind, "naive" if naive else "SSE", fkey, tpw)
                        got = ctx.hash_codes(sm, gr)
                        assert ctx.hash_plan() == hw.plan(W, H, 1, 32, tpw, cus), (what, ctx.hash_plan())
                        assert hash_name(ctx) == "gpc::k_hash<%s, true, %s, false, 32>" % ("true" if f.type else "false", "true" if naive else "false")
                        bad = np.argwhere(got != want)
                        if len(bad):
                            rep.errors.append("%s: %d codes differ from the oracle's, the first at row %d (tile %d of the column), x %d" % (
                                what, len(bad), bad[0][0], (bad[0][0] - 13) // 32, bad[0][1]))
                        results.setdefault((fkey, naive, kind), {})[tpw] = (got,)
        finally:
            ctx.close()
    for (fkey, naive, kind), r in results.items():
        rep.check(hw.same_across, r, "%dx%d, input %s, %s %s" % (W, H, kind, "naive" if naive else "SSE", fkey))
    rep.done()


# ----------------------------------------------------------------------------------------- 2. the batch, bit gradient image
@pytest.mark.parametrize("W,H", hw.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("ty", [32, 40])
def test_batch_every_tpw(fast, forest_paths, cus, W, H, ty):
    """match_batch_device, two pairs, the bit gradient image (k_hash<TAU, false, false, true, TY>), 32-row tiles and the
    40-row ones: supports, counts and candidate counts -- the candidate count is the walk's `cnt`, a support in the last
    candidate row needs its `last`, the rank buckets of the join its OR of the codes"""
    batch_walk(fast, forest_paths, cus, W, H, {"GPC_HIP_HASH_TALL": 1 if ty == 40 else 0}, hw.TPWS, ty, ("zero", "tau"), False, True)


@pytest.mark.parametrize("epi,ht", [(False, False), (True, True)], ids=["whole image", "hash table"])
@pytest.mark.parametrize("W", [96, 272])
def test_device_wide_matchers_behind_a_walk(fast, forest_paths, cus, W, epi, ht):
    """tpw 3 at H = 155 (3 + 2 tiles, the last one row) in front of the non-epipolar and the hash-table matcher"""
    ctx = make_ctx({"GPC_HIP_HASH_TPW": 3, "GPC_HIP_HASH_TALL": 0})
    try:
        for kind in hw.KINDS:
            c = walk_case(fast, forest_paths, W, 155, kind, "tau")
            load_forest(ctx, c)
            run(ctx, fast, c, epi, ht, None, "%dx155, input %s, epipolar %s, hash table %s, tpw 3" % (W, kind, epi, ht))
            assert ctx.hash_plan() == hw.plan(W, 155, 4, 32, 3, cus)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------- 3. the batch, byte gradient image kept
@pytest.mark.parametrize("W,H", hw.SHAPES, ids=SHAPE_IDS)
def test_batch_byte_gradient_image(fast, forest_paths, cus, W, H):
    """GPC_HIP_NO_GRAD_BITS: the batched pipelines keep the byte image, k_hash<TAU, false, false, false, 32>"""
    batch_walk(fast, forest_paths, cus, W, H, {"GPC_HIP_NO_GRAD_BITS": 1}, (1, 3, 64), 32, ("zero", "tau"), False, False)


# --------------------------------------------------------------------------------------------------------- 4. SSE=OFF batch
@pytest.mark.parametrize("W,H", hw.SHAPES, ids=SHAPE_IDS)
def test_batch_naive_wide(fast, forest_paths, cus, W, H):
    """SSE=OFF arithmetic with 32-test forests: row H - 14 is hashed, the codes use bit 31"""
    batch_walk(fast, forest_paths, cus, W, H, {}, (1, 3), 32, ("zero", "tau"), True, False)


# ------------------------------------------------------------------------------------------------------------ 5. group mode
def group_wants(fast, forest_paths, W, H, kind):
    """the oracle's union over the stress forest's 16 groups per pair of the input, shared among tile heights and tpw"""
    def make():
        c = walk_case(fast, forest_paths, W, H, kind, "tau")   # (the images and their candidate rows)
        texts = group_texts(open(STRESS).read())
        wants = []
        for i in range(c.B):
            u, (nl, nr) = oracle_union_pair(fast, texts, c.L[i], c.R[i], True)
            wants.append((u, nl, nr))
        hw.conditions(c, kind, [w[0] for w in wants], "%dx%d input %s, the groups' union" % (W, H, kind))
        return c, wants
    return shared(("walk groups", W, H, kind), make)


@pytest.mark.parametrize("W,H", hw.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("ty", [32, 40])
def test_group_batch(fast, forest_paths, cus, W, H, ty):
    """set_forest_groups(stress16x20Forest), match_batch_device against the oracle's union: k_hash_groups carries one OR of
    the codes per group and the candidate statistics of group 0 across the walk"""
    import opengpc_amd as g
    rep, results = Report(), {}
    for tpw in (1, 2, 5):
        ctx = make_ctx({"GPC_HIP_HASH_TPW": tpw, "GPC_HIP_HASH_TALL": 1 if ty == 40 else 0})
        try:
            st, groups = g.read_forest_groups(STRESS, W, H)
            assert st == 0 and len(groups) == 16
            ctx.set_forest_groups(groups)
            for kind in hw.KINDS:
                c, wants = group_wants(fast, forest_paths, W, H, kind)
                what = "%dx%d, input %s, 16 groups, %d-row tiles, tpw %d" % (W, H, kind, ty, tpw)
                got = hw.launch_batch(ctx, c, settings(vtol=0), max(len(w[0]) for w in wants) + 5)
                assert ctx.hash_plan() == hw.plan(W, H, 2 * c.B, ty, tpw, cus), (what, ctx.hash_plan())
                assert hash_name(ctx) == "gpc::k_hash_groups<true, false, false, true, %d>" % ty, (what, hash_name(ctx))
                rep.check(hw.check_batch, got, wants, what)
                results.setdefault(kind, {})[tpw] = got
        finally:
            ctx.close()
    for kind, r in results.items():
        rep.check(hw.same_across, r, "%dx%d, input %s, 16 groups, %d-row tiles" % (W, H, kind, ty))
    rep.done()


@pytest.mark.parametrize("W,H", hw.SHAPES, ids=SHAPE_IDS)
def test_group_codes(fast, forest_paths, cus, W, H):
    """hash_codes_groups: the dense code image of every group against the oracle's under the group's own forest text"""
    import opengpc_amd as g
    rep, results = Report(), {}
    texts = group_texts(open(STRESS).read())
    for tpw in (1, 2, 5):
        ctx = make_ctx({"GPC_HIP_HASH_TPW": tpw})
        try:
            st, groups = g.read_forest_groups(STRESS, W, H)
            assert st == 0
            ctx.set_forest_groups(groups)
            for kind in hw.KINDS:
                def planes():
                    sm, gr, _ = fast.preprocess(hw.walk_pairs(W, H, kind)[0][0], hw.THR)
                    want = np.stack([fast.hash(sm, gr, fast.parse_forest_text(t, W, H)[1]) for t in texts])
                    assert all(w.any() for w in want)
                    return sm, gr, want
                sm, gr, want = shared(("walk group codes", W, H, kind), planes)
                what = "%dx%d, input %s, tpw %d" % (W, H, kind, tpw)
                got = ctx.hash_codes_groups(sm, gr)
                assert ctx.hash_plan() == hw.plan(W, H, 1, 32, tpw, cus), (what, ctx.hash_plan())
                assert hash_name(ctx) == "gpc::k_hash_groups<true, true, false, false, 32>", (what, hash_name(ctx))
                for k in range(len(texts)):
                    bad = np.argwhere(got[k] != want[k])
                    if len(bad):
                        rep.errors.append("%s: group %d: %d codes differ from the oracle's, the first at row %d, x %d" % (
                            what, k, len(bad), bad[0][0], bad[0][1]))
                results.setdefault(kind, {})[tpw] = (got,)
        finally:
            ctx.close()
    for kind, r in results.items():
        rep.check(hw.same_across, r, "%dx%d, input %s, the groups' codes" % (W, H, kind))
    rep.done()


# ------------------------------------------------------------------------------------------------------- 6. frame sequences
@pytest.mark.parametrize("W,H", hw.SHAPES, ids=SHAPE_IDS)
def test_sequence_of_three_frames(fast, forest_paths, cus, W, H):
    """match_sequence_device over the frames [L, R, L]: one k_hash launch over an odd number of images"""
    for tpw in (1, 4):
        ctx = make_ctx({"GPC_HIP_HASH_TPW": tpw, "GPC_HIP_HASH_TALL": 0})
        try:
            for fkey in ("zero", "tau"):
                for kind in hw.KINDS:
                    c = walk_case(fast, forest_paths, W, H, kind, fkey)
                    load_forest(ctx, c)
                    run_corr(ctx, fast, c, 0, True, False, None, "%dx%d, input %s, %s, three frames, tpw %d" % (W, H, kind, fkey, tpw))
                    assert ctx.hash_plan() == hw.plan(W, H, 3, 32, tpw, cus), ctx.hash_plan()
        finally:
            ctx.close()


# ------------------------------------------------------------------------------------------------- 7. the planner's choice
def test_planner_walks_by_itself_and_caps_the_last_round(fast, forest_paths, cus):
    """No knob: pairs of 48x155 (one tile column of five tiles per image), as many as give run_hash the 2 x 2 x CUs tiles
    from which it lets a workgroup walk.  The launch then has more workgroups than the device holds (last_from > 0): both
    values of last_round occur in it.  Beside it a single 96x155 pair, which keeps one tile per workgroup -- why the other
    cases force the walk."""
    W, H = 48, 155
    B = -(-4 * cus // 10) + 1
    c = shared(("walk planner", B), lambda: Case(fast, forest_paths["tau"], [hw.walk_pair(W, H, "a", 100 + i, 3 + i % 4) for i in range(B)], thr=hw.THR))
    assert 1 * hw.tiles(H, 32) * 2 * B >= 2 * 2 * cus and sum(len(w[0]) for w in c.want(fast, True, False)) > B
    ctx = make_ctx()
    try:
        load_forest(ctx, c)
        got = hw.launch_batch(ctx, c, settings(), c.cap)
        ty, tpw, per_col, last_from = ctx.hash_plan()
        assert ty == 32 and tpw >= 2 and last_from > 0, ctx.hash_plan()
        assert (per_col, last_from) == (-(-5 // tpw), per_col * 2 * B - 2 * cus), ctx.hash_plan()
        hw.check_batch(got, c.want(fast, True, False), "%d pairs of 48x155, the planner's tpw %d" % (B, tpw))
        one = shared(("walk one pair",), lambda: Case(fast, forest_paths["tau"], hw.walk_pairs(96, 155, "a")[:1], thr=hw.THR))
        load_forest(ctx, one)   # (a forest is laid out for one image width)
        hw.check_batch(hw.launch_batch(ctx, one, settings(), one.cap), one.want(fast, True, False), "one pair of 96x155, no knob")
        ty, tpw, per_col, last_from = ctx.hash_plan()
        assert (tpw, per_col, last_from) == (1, hw.tiles(155, ty), 0), ctx.hash_plan()
    finally:
        ctx.close()
