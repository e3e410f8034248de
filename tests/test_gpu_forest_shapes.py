"""Forest shape on the GPU: every test count, tau placement and group mix against the CPU oracle, bit for bit.

k_hash (k_hash_body.h) lays the tests out in byte planes gated by T > 0, > 8, > 9, > 17 and > 25; test 8 is a plane of its
own OR-ed into bit 0 by the pixel's x; the last plane holds n3 = min(T, 32) - 25 tests and is read through a mask and a shift
that depend on n3; a plane's first test takes another form of the compare than the others, and either form again by whether
the test's tau is 0.  The width of the codes (code_bits, gpc_hip.hip: T up to 8 tests, T - 1 beyond) sizes the joins' rank
buckets and the device-wide matchers' bins.  The rest of the GPU suite runs forests of 20, 30 and 32 tests only; here the
test count runs over 0 .. 33, the taus are placed by rule (forest_groups_util.forest_text), and groups of unequal size are
matched together.  Expected values come from the oracle alone and every comparison is exact.

What the two ends of the range do, library and oracle alike (the header: gpc_filter_mask keeps the first GPC_MAX_TESTS = 32
tests and counts the rest in `discarded`): a forest without tests parses (status 0, num_tests 0, type 0), is accepted by
set_forest and gives the code 0 at every pixel; with every state alike the oracle emits no match in any mode, and neither
does the library (asserted below, candidate counts included); a forest of 33 tests is cut to its first 32 with
discarded = 1, and the tau of the discarded test still counts towards the forest's type.  Neither refuses where the other
accepts."""
import numpy as np
import pytest

from devicewide_util import HJ, SLOT, VJ4, VJ8, Case, load_forest, make_ctx, run, shared, textured
from forest_groups_util import TAU_RULES, fern_split, forest_text, group_texts, union
from test_gpu_forest_groups import SUPP_KEY, oracle_union_corr, oracle_union_pair, same_corr, same_supports

pytestmark = pytest.mark.gpu

FERNS = (1, 2, "each")
SCALES = "sml"
SHAPES = ((160, 100), (176, 67))
RULE_COUNTS = (1, 8, 9, 10, 17, 18, 25, 26, 30, 32)
MATCH_COUNTS = (0, 1, 2, 3, 4, 7, 8, 9, 10, 16, 17, 18, 24, 25, 26, 31, 32)
NAIVE_COUNTS = (1, 8, 9, 25, 31, 32)
MATCHERS = ((True, False), (True, True), (False, False), (False, True))   # (epipolar, hash table)
DOT_THRESHOLD, DOT_DENSITY = 40, 0.03


@pytest.fixture(scope="module")
def fast():
    from oracle.pyoracle import Oracle
    return Oracle(fast=True)


@pytest.fixture(scope="module")
def ctxs():
    """One context per way of running: as it comes, the fused join wherever it can run (as test_gpu_fuzz.py's fused_ctx), and
    the 40-row hash tile wherever it exists.  The knobs are read at creation and removed again straight after."""
    made = {"plain": make_ctx(), "fused": make_ctx({"GPC_HIP_FUSE_ALWAYS": 1}), "tall": make_ctx({"GPC_HIP_HASH_TALL": 1})}
    yield made
    for c in made.values():
        c.close()


def shape_text(T, tau, m128_last=False, split=0):
    """T tests over 1, 2 or T ferns (by T + split), the ferns' scales cycling through s, m, l; the taps depend on T only"""
    return forest_text(fern_split(T, FERNS[(T + split) % 3]), seed=T, tau=tau, scales=SCALES, m128_last=m128_last)


def code_bits(T, naive):
    T = min(T, 32)
    return T if naive or T <= 8 else T - 1


# ------------------------------------------------------------------------------------------------------------ hash codes
def inside(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    return (xx >= 13) & (xx < W - 13) & (yy >= 13) & (yy < H - 13)


def planes(fast, W, H):
    """[(name, smooth plane, gradient plane, candidates)] per arithmetic, computed once per shape: a noise and a blocky image
    preprocessed, each image itself as the smooth plane (every byte value beside every other), and the noise under a
    gradient plane with every third 16-pixel group empty, the empty group moving by one per row -- the SSE arithmetic
    skips such a group, so skipped and hashed groups meet test 8's two cases (x % 8 == 0 or not) in every column."""
    def make():
        rng = np.random.default_rng(W * 1000 + H)
        noise = rng.integers(0, 256, (H, W), dtype=np.uint8)
        blocky = (rng.integers(0, 256, (H // 5 + 1, W // 5 + 1)).repeat(5, 0).repeat(5, 1)[:H, :W] * 3 // 4
                  + rng.integers(0, 64, (H, W))).astype(np.uint8)
        yy, xx = np.mgrid[0:H, 0:W]
        holes = np.where((xx // 16 + yy) % 3 == 0, 0, 9).astype(np.uint8)
        out = {}
        for naive in (False, True):
            pre = fast.preprocess_naive if naive else fast.preprocess
            lst = []
            for name, img in (("noise", noise), ("blocky", blocky)):
                sm, gr, mk = pre(img, 5)
                lst += [(name, sm, gr, mk), (name + " raw", img, gr, mk)]
            lst.append(("holes", noise, holes, np.flatnonzero((holes != 0) & inside(W, H)).astype(np.int32)))
            out[naive] = lst
        return out
    return shared(("planes", W, H), make)


def slot8_true(sm, f):
    """test 8's decision per pixel in numpy, from its two taps in linear addressing (filter.hpp:647-652: with taus the second
    tap takes a saturating signed subtract, the compare is unsigned): valid where both taps lie inside the image"""
    flat = sm.reshape(-1).astype(np.int64)
    k = np.arange(flat.size)
    ia, ib = k + f.offs[16], k + f.offs[17]
    ok = (ia >= 0) & (ia < flat.size) & (ib >= 0) & (ib < flat.size)
    a, b = flat[np.clip(ia, 0, flat.size - 1)], flat[np.clip(ib, 0, flat.size - 1)]
    if f.type:
        s8 = lambda v: ((v + 128) & 0xFF) - 128
        b = np.clip(s8(b) - s8(np.int64(f.tau[8])), -128, 127) & 0xFF
    return ((a > b) & ok).reshape(sm.shape)


def check_codes(ctxs, fast, text, T, what, vacuity=True):
    """SSE and naive codes of one forest over every plane of both shapes; the oracle's codes must use the highest bit and,
    from 9 tests on, show test 8 true on both sides of the x % 8 == 0 carry"""
    import opengpc_amd as g
    ctx = ctxs["plain"]
    top = {False: False, True: False}
    at0 = rest = False
    for W, H in SHAPES:
        rc, f = fast.parse_forest_text(text, W, H)
        st, fm = g.parse_forest(text, W, H)
        assert (rc, st) == (0, 0) and fm.num_tests == f.num_tests == min(T, 32), what
        assert (fm.type, fm.discarded) == (f.type, f.discarded) == (fm.type, max(T - 32, 0)), what
        ctx.set_forest(fm)
        for naive in (False, True):
            ctx.set_arithmetic(naive)
            try:
                for name, sm, gr, mk in planes(fast, W, H)[naive]:
                    want = fast.hash_naive(sm, mk, f) if naive else fast.hash(sm, gr, f)
                    got = ctx.hash_codes(sm, gr)
                    assert np.array_equal(got, want), "%s, %dx%d %s, %s: %d codes differ" % (
                        what, W, H, name, "naive" if naive else "SSE", int((got != want).sum()))
                    if T >= 1:
                        top[naive] |= bool(((want >> (code_bits(T, naive) - 1)) & 1).any())
                    if code_bits(T, naive) < 32:
                        assert not (want >> code_bits(T, naive)).any(), what + ": the oracle's codes are wider than code_bits"
                    if T >= 9 and not naive:
                        yy, xx = np.mgrid[0:H, 0:W]
                        hashed = (yy >= 13) & (yy < H - 15) & (np.repeat(gr.reshape(H, W // 16, 16).max(axis=2), 16, axis=1) != 0)
                        t8 = slot8_true(sm, f) & hashed
                        at0 |= bool(t8[:, 0::8].any())
                        rest |= bool((t8 & (xx % 8 != 0)).any())
            finally:
                ctx.set_arithmetic(False)
    if vacuity and T >= 1:
        assert top[False] and top[True], what + ": no code of the oracle's has the highest bit set"
    if vacuity and T >= 9:
        assert at0 and rest, what + ": test 8 is not true on both sides of x % 8 == 0"


@pytest.mark.parametrize("T", list(range(34)))
def test_hash_codes_at_every_test_count(ctxs, fast, T):
    """0 .. 32 tests and 33 (cut to 32): a forest without taus and one with, SSE codes (hash_codes, DENSE) and naive codes,
    160x100 and 176x67.  0 tests: every code is 0; 33: see the module's text."""
    for tau in (False, True):
        check_codes(ctxs, fast, shape_text(T, tau), T, "T = %d, %s" % (T, "tau" if tau else "zero"))


@pytest.mark.parametrize("T", RULE_COUNTS)
def test_hash_codes_tau_placement(ctxs, fast, T):
    """Zero and non-zero taus placed by rule, so that a plane's first test and its other tests meet both forms of the
    compare; the non-zero taus cycle through -127, -20, -1, 1, 20, 127; and one forest whose last test alone has a tau of
    -128 (tau_m128: the every-tau form of the subtract).  The highest bit's non-vacuity is asserted in the sweep above: a
    tau of -127 or 127 on the last test may leave it always true or never.  The sweep gives each count one split over ferns;
    here the two other splits run as well, so every count of this list is seen as 1 fern, 2 ferns and T ferns."""
    for rule in TAU_RULES:
        check_codes(ctxs, fast, shape_text(T, rule), T, "T = %d, taus %s" % (T, rule), vacuity=False)
    for split in (1, 2):   # the same tests split over ferns in the two other ways (1, 2 or T ferns: all three at these counts)
        check_codes(ctxs, fast, shape_text(T, "alternating", split=split), T, "T = %d, %s fern(s)" % (T, FERNS[(T + split) % 3]),
                    vacuity=False)
        check_codes(ctxs, fast, shape_text(T, True, split=split), T, "T = %d, random taus, %s fern(s)" % (T, FERNS[(T + split) % 3]))
    text = shape_text(T, "alternating", m128_last=True)
    import opengpc_amd as g
    assert g.parse_forest(text, 160, 100)[1].tau[T - 1] == -128
    check_codes(ctxs, fast, text, T, "T = %d, -128 on the last test" % T, vacuity=False)


# --------------------------------------------------------------------------------------------------------- whole matches
def dots_pair(W, H, seed, d):
    """a flat background with sparse dots (kind 3 of draw_pair in test_gpu_fuzz.py), the right image shifted by d"""
    rng = np.random.default_rng(seed)
    base = np.full((H, W + 64), 60, np.uint8)
    m = rng.random((H, W + 64)) < DOT_DENSITY
    base[m] = rng.integers(0, 256, int(m.sum()), dtype=np.uint8)
    return np.ascontiguousarray(base[:, 32:32 + W]), np.ascontiguousarray(base[:, 32 + d:32 + d + W])


def match_case(fast, T, tau, naive, dots):
    def make():
        if dots:
            a, b = dots_pair(176, 67, 7, 9), dots_pair(176, 67, 8, 4)
        else:
            a, b = textured(176, 67, 3, 9), textured(176, 67, 4, 5)
        return Case(fast, None, [a, (a[1], a[0]), b], naive=naive, forest_text=shape_text(T, tau),
                    thr=DOT_THRESHOLD if dots else 5)
    return shared(("shape", T, tau, naive, dots), make)


def oracle_has_empty(fast, c, epi, ht):
    """the harness refuses a pair without supports unless the oracle itself has none for one of the case's pairs"""
    return not all(len(w[0]) for w in c.want(fast, epi, ht))


def check_matches(ctx, fast, c, what, batch=True, tall=False):
    """match_pair on the first pair and one three-pair match_batch_device (filled outputs, every byte) per matcher; returns
    the first pair's four counts.  From 8 tests on every pair has supports in the epipolar modes, from 16 on in all four."""
    import opengpc_amd as g
    counts = []
    load_forest(ctx, c)
    for epi, ht in MATCHERS:
        w, nl, nr = c.want(fast, epi, ht)[0]
        tag = "%s, %s %s" % (what, "epipolar" if epi else "global", "hash table" if ht else "sort")
        got, n, nc, st = ctx.match_pair(c.L[0], c.R[0], g.Settings(c.thr, 128, 1, epi, ht, 1))
        assert st == 0, tag
        assert tuple(nc) == (nl, nr), "%s: candidates %s, the oracle's %s" % (tag, tuple(nc), (nl, nr))
        assert n == len(w), "%s: %d supports, the oracle %d" % (tag, n, len(w))
        assert np.array_equal(got, w.astype(got.dtype)), tag + ": records differ"
        if tall:
            assert ctx.kernel_launch_names()["k_hash"].endswith(", true, 40>"), ctx.kernel_launch_names()["k_hash"]
        if batch:
            run(ctx, fast, c, epi, ht, None, tag + ", batch of three", may_be_empty=oracle_has_empty(fast, c, epi, ht))
            if tall:
                assert ctx.kernel_launch_names()["k_hash"].endswith(", true, 40>"), ctx.kernel_launch_names()["k_hash"]
        if c.f.num_tests >= (8 if epi else 16):
            assert not oracle_has_empty(fast, c, epi, ht), tag + ": the oracle has no support for one of the pairs"
        counts.append(len(w))
    return counts


@pytest.mark.parametrize("T", MATCH_COUNTS)
def test_matches_at_every_boundary_count(ctxs, fast, T):
    """All four matchers on 176x67 synth_pair(3, 9) -- match_pair, and three pairs (the pair, its mirror, another) through
    match_batch_device on a context with the fused join: status, both candidate counts, the count and every record.
    Up to 3 tests the synthetic pair gives the oracle nothing to emit (0 supports in every mode; in the non-epipolar modes up
    to 7 tests), which is kept as a check of the empty result; a second image stands beside it for those counts: sparse dots
    on a flat background (density 0.03, seed 7, shift 9) at a gradient threshold of 40, where the oracle alone returns, in
    epipolar mode (sort / hash table), 1 / 1 supports with 1 test and no taus and 7 / 7 with taus, 3 / 2 and 2 / 1 with 2
    tests, 7 / 6 and 1 / 1 with 3 tests.  (Thresholds 5, 20, 40 and densities 0.002 .. 0.03 were tried on the CPU: at 5 and
    20 the forest of one test without taus matched nothing at any density.)"""
    for tau in (False, True):
        c = match_case(fast, T, tau, False, False)
        what = "T = %d, %s" % (T, "tau" if tau else "zero")
        counts = check_matches(ctxs["plain"], fast, c, what, batch=False)
        check_matches(ctxs["fused"], fast, c, what + ", fused join")
        print("T = %2d %s: supports %s (epipolar sort, epipolar hash table, global sort, global hash table)" % (
            T, "tau " if tau else "zero", counts))
        if T >= 4:
            assert counts[0] > 0 and counts[1] > 0, what
        if T >= 8 and (tau or T >= 9):
            assert counts[2] > 0 or counts[3] > 0, what
        if T == 32:
            assert min(counts) > 2500, what
        if 1 <= T <= 3:
            d = match_case(fast, T, tau, False, True)
            assert all(len(d.want(fast, True, ht)[0][0]) > 0 for ht in (False, True)), what + ": the dots give the oracle nothing"
            dc = check_matches(ctxs["plain"], fast, d, what + ", dots", batch=False)
            check_matches(ctxs["fused"], fast, d, what + ", dots, fused join")
            print("T = %2d %s: supports %s on the dots" % (T, "tau " if tau else "zero", dc))


@pytest.mark.parametrize("T", NAIVE_COUNTS)
def test_matches_naive_arithmetic(ctxs, fast, T):
    """the same under the SSE=OFF arithmetic: T code bits, test t on bit T - 1 - t, 32 tests with WIDE codes"""
    for tau in (False, True):
        c = match_case(fast, T, tau, True, False)
        for name in ("plain", "fused"):
            ctxs[name].set_arithmetic(True)
            try:
                counts = check_matches(ctxs[name], fast, c, "naive, T = %d, %s, %s" % (T, "tau" if tau else "zero", name))
            finally:
                ctxs[name].set_arithmetic(False)
        print("T = %2d %s naive: supports %s" % (T, "tau " if tau else "zero", counts))
        if T >= 8:
            assert counts[0] > 0 and counts[1] > 0


@pytest.mark.parametrize("T", MATCH_COUNTS)
def test_matches_with_the_tall_hash_tile(ctxs, fast, T):
    """The SSE cases once more on a context created under GPC_HIP_HASH_TALL=1: run_hash (gpc_hip.hip) then takes the 40-row
    tile, whose taps have LDS offsets of their own (GpcForestDev ft), for every launch that hashes from the bit image of the
    gradients, whatever the image size -- match_pair and match_batch_device both do, 176x67 included (two tiles of 40 rows
    over its 41 candidate rows); the launch's recorded name says so."""
    for tau in (False, True):
        check_matches(ctxs["tall"], fast, match_case(fast, T, tau, False, False), "tall tile, T = %d, %s" % (T, "tau" if tau else "zero"),
                      tall=True)


# -------------------------------------------------------------------------------- the device-wide paths under narrow codes
def narrow_case(fast, T, W, H, n):
    return shared(("narrow", T, W, H), lambda: Case(fast, None, [textured(W, H, 20 + i, 4 + 2 * i) for i in range(n)] if n > 1
                                                   else [textured(W, H, 4, 9)], forest_text=shape_text(T, True)))


@pytest.mark.parametrize("T", [1, 4, 8, 9, 12])
def test_code_ranges_under_narrow_codes(fast, T):
    """The non-epipolar sort matcher at 272x61 (where test_gpu_devicewide_paths.py reaches the one-launch path) with codes of
    1 .. 11 bits: fewer bins than 256 (run_partition_match: never more bin bits than code bits), each of them large.  The
    path is the one the planner documents for the largest bin of a side, binned here on the CPU first: up to 4096 records
    the 4096-record join alone, up to 8192 the 8192-record launch over the work list beside it, beyond that the radix sort;
    with GPC_HIP_NO_PARTITION the radix sort always.  (Without the row in the state the oracle has no support here up to 9
    tests -- the empty result and both candidate counts are what is compared -- and 276 with 12.)"""
    c = narrow_case(fast, T, 272, 61, 1)
    assert oracle_has_empty(fast, c, False, False) == (T < 12)
    side = c.code_range_bins(0)
    name = VJ4 if side <= 4096 else VJ8 + "[list] + " + VJ4 if side <= 8192 else "gpc::k_g_match"
    print("T = %2d: largest bin of a side %d records -> %s" % (T, side, name))
    for env, want in (({}, name), ({"GPC_HIP_NO_PARTITION": 1}, "gpc::k_g_match")):
        ctx = make_ctx(env)
        try:
            load_forest(ctx, c)
            run(ctx, fast, c, False, False, want, "T = %d, %s" % (T, "no partition" if env else "partition"),
                may_be_empty=oracle_has_empty(fast, c, False, False))
        finally:
            ctx.close()


@pytest.mark.parametrize("T", [1, 4, 8, 9, 12])
@pytest.mark.parametrize("epi", [True, False])
def test_hash_table_under_narrow_codes(fast, T, epi):
    """The hash-table matcher under GPC_HIP_HT_LBITS=7 (the smallest value the library accepts: 128 buckets per bin) on the
    two 528x90 pairs of the 512-bucket tests there.  A few states put thousands of records into one bucket; a forced width
    is not planned again, so the path follows from the largest bin (left + right records, binned on the CPU first): up to
    2048 the 512-thread join alone, up to 4096 a 1024-thread launch over the list of larger bins beside it, up to 8192
    k_ht_join<8, 1024>, beyond that the sort.  (The oracle has supports for both pairs from 8 tests on with the row in the
    state, and with 12 tests without it; the other cases compare the empty result and the candidate counts.)"""
    c = narrow_case(fast, T, 528, 90, 2)
    assert oracle_has_empty(fast, c, epi, True) == (T < (8 if epi else 12))
    big = max(c.bucket_bins(i, 7, epi) for i in range(c.B))
    name = (HJ % (4, 512) if big <= 2048 else (HJ % (4, 1024)) + "[list] + " + (HJ % (4, 512)) if big <= 4096
            else HJ % (8, 1024) if big <= 8192 else "gpc::k_ht_pairs")
    print("T = %2d, epipolar %d: largest bin %d records -> %s" % (T, epi, big, name))
    ctx = make_ctx({"GPC_HIP_HT_LBITS": 7})
    try:
        load_forest(ctx, c)
        run(ctx, fast, c, epi, True, name, "T = %d, 128 buckets per bin" % T, may_be_empty=oracle_has_empty(fast, c, epi, True))
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------- groups of unequal size
SORT = "gpc::k_g_match"
SIDE = VJ8 + "[list] + " + VJ4


def group_side_bins(oracle, texts, imgs, W, H):
    """per group the largest bin of a side as run_partition_match bins a group-mode call: every group by the top 8 of the
    LARGEST group's code bits (code_bits: one planner width for every group), so a smaller group fills the low bins"""
    forests = [oracle.parse_forest_text(t, W, H)[1] for t in texts]
    bits = code_bits(max(f.num_tests for f in forests), False)
    out = []
    for f in forests:
        big = 0
        for img in imgs:
            sm, gr, mk = oracle.preprocess(img, 5)
            codes = oracle.hash(sm, gr, f).reshape(-1)[mk].astype(np.int64)
            assert not (codes >> code_bits(f.num_tests, False)).any()
            big = max(big, int(np.bincount(codes >> (bits - min(8, bits)), minlength=1).max()))
        out.append(big)
    return out


@pytest.mark.parametrize("sizes,packed,W,H,D,name", [
    ([32, 5, 1, 20, 7, 9], [32, 26, 16], 256, 96, 11, SORT),
    ([40, 3], [32, 8, 3], 256, 96, 11, SORT),
    ([32, 5, 1, 20, 7, 9], [32, 26, 16], 176, 67, 9, SIDE),
    ([40, 3], [32, 8, 3], 176, 67, 9, SIDE),
    ([12, 25, 10, 20], [12, 25, 30], 176, 67, 9, SIDE),
    ([30, 24], [30, 24], 256, 96, 11, VJ4),
])
def test_groups_of_unequal_size(ctxs, oracle, sizes, packed, W, H, D, name):
    """code_bits takes the largest group's width for every group ("a smaller group's codes then fill the low bins").  The
    groups are virtual pairs of one plan, so the non-epipolar path follows from the largest bin of a side over all groups,
    binned here on the CPU first and asserted by the launch's recorded name:
      * 32 / 26 / 16 and 32 / 8 / 3 tests at 256x96: the groups of 16, 8 and 3 tests put every record of a side (11174) into
        bin 0, beyond the 8192 a workgroup takes -- the plan is abandoned and the radix sort produces the union;
      * the same forests, and 12 / 25 / 30 (the narrow group first), at 176x67: bin 0 holds 4319 records of a side, so the
        narrow groups go to the 8192-record join over the work list beside the 4096-record join of the others;
      * 30 / 24 tests at 256x96: the smaller group spreads over the four lowest bins (3826 records at most): the
        4096-record join alone.
    Per group the codes; match_pair's supports and stereo_match's correspondences in epipolar and global mode against the union
    of the oracle's per-group results; and, for the first two cases, a batch of three pairs whose capacity ends inside the
    second group's share of the union: the first `cap` records and the true count."""
    import torch
    import opengpc_amd as g
    from test_gpu_forest_groups import gsettings
    text = forest_text(sizes, seed=len(sizes), scales=SCALES)
    texts = group_texts(text)
    st, groups = g.parse_forest_groups(text, W, H)
    assert st == 0 and [x.num_tests for x in groups] == packed
    for t, n in zip(texts, packed):   # the packing restated on the text agrees, group by group
        rc, f = oracle.parse_forest_text(t, W, H)
        assert rc == 0 and f.num_tests == n
    L, R = oracle.synth_pair(W, H, 3, D)
    sides = group_side_bins(oracle, texts, (L, R), W, H)
    print("groups %s at %dx%d: largest bin of a side per group %s -> %s" % (packed, W, H, sides, name))
    assert name == (VJ4 if max(sides) <= 4096 else SIDE if max(sides) <= 8192 else SORT), sides
    assert min(sides) <= 4096, sides   # (a group of the batch that the 4096-record join takes)
    ctx = ctxs["plain"]
    try:
        ctx.set_forest_groups(groups)
        pl, pr = oracle.preprocess(L, 5), oracle.preprocess(R, 5)
        codes = ctx.hash_codes_groups(pl[0], pl[1])
        for k, t in enumerate(texts):
            rc, f = oracle.parse_forest_text(t, W, H)
            assert np.array_equal(codes[k], oracle.hash(pl[0], pl[1], f)), "group %d" % k
        for epi in (True, False):
            want, nc = oracle_union_pair(oracle, texts, L, R, epi)
            got, n, ncg, st = ctx.match_pair(L, R, gsettings(epi))
            assert st == 0 and ncg == nc and len(want) > 0
            assert epi or ctx.kernel_launch_names()[SLOT] == name, ctx.kernel_launch_names()[SLOT]
            same_supports(got, want)
            got, n, st = ctx.stereo_match(pl, pr, gsettings(epi))
            assert st == 0
            assert epi or ctx.kernel_launch_names()[SLOT] == name, ctx.kernel_launch_names()[SLOT]
            same_corr(got, oracle_union_corr(oracle, texts, pl, pr, epi))
        if name != SORT:
            return
        # three pairs (the pair, its mirror, the pair): one capacity that ends inside the second group's records of each union
        pairs = [(L, R), (R, L), (L, R)]
        from oracle.pyoracle import sparsematch_settings
        wants, cuts = [], []
        for a, b in pairs:
            per = []
            for t in texts:
                rc, f = oracle.parse_forest_text(t, W, H)
                per.append(oracle.match_pair(a, b, f, sparsematch_settings(5, 128, 0, True))[0])
            u = union(per, SUPP_KEY)
            wants.append(u)
            cuts.append((len(per[0]), len(union(per[:2], SUPP_KEY)), len(u)))
        cap = (max(c[0] for c in cuts) + min(c[1] for c in cuts)) // 2
        assert all(c[0] < cap < c[1] <= c[2] for c in cuts), cuts
        dev = torch.device("cuda", 0)
        d_L = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
        d_R = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
        d_out = torch.full((4, cap, 3), -1, dtype=torch.int32, device=dev)
        d_cnt = torch.zeros(3, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, 3, gsettings(True), d_out.data_ptr(), cap, d_cnt.data_ptr(), 0)
        ctx.synchronize()
        out, cnt = d_out.cpu().numpy(), d_cnt.cpu().numpy()
        assert (out[3] == -1).all(), "written behind the batch's records"
        for p in range(3):
            assert cnt[p] == len(wants[p]), "pair %d: count %d, the oracle's union %d" % (p, cnt[p], len(wants[p]))
            rec = out[p].copy().view(np.dtype([("x", "<i4"), ("y", "<i4"), ("d", "<f4")])).reshape(-1)
            same_supports(rec, wants[p][:cap])
    finally:
        ctx.set_forest(g.parse_forest(shape_text(4, False), W, H)[1])   # leaves group mode
