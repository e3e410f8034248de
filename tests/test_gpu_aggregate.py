"""The scanline aggregation on the GPU (gpc_hip_aggregate_*): every byte of out, cost, choice, stats and agg EQUALS the
restatement of the rule (tests/aggregate_util.py, which takes the minimum over all pairs of labels and knows nothing of the
kernels' shift form) -- every output starts out filled with a sentinel, and every element must be written.  Both channel
counts, radii 1, 2 and 4, ranges 0, 1 and 2, with and without the parabola, every single bit of paths and 3, 12, 15, penalties
with p1 = p2 and p2 = 32767; shapes where a direction never has a predecessor (1 x 1, 1 x N, N x 1), 2 x 2, search_util.SIZES,
and one below, at and one above every extent of the kernels: the 64 chains of a workgroup in either axis, the 8, 16 or 32
columns a horizontal path stages, the 32 x 8 tile of the cost kernel; search_util's three kinds of field and a stepped prior
with holes, targets outside the image and the extremes of int32.  A crafted scene with hand-written winners; the two
identities against search_fields_device; the single cases of the search's tests; more than one workspace group; the host
form; the match forms; the refusals."""
import ctypes as C

import numpy as np
import pytest

import aggregate_util as au
import search_util as su
import track_util as tu
from aggregate_util import AGGREGATE_WINNERS, SEARCH_WINNERS

pytestmark = pytest.mark.gpu

FILL = 0xA5
N = su.NONE
NAMES = ("out", "cost", "choice", "stats", "agg")
PATHS = (1, 2, 4, 8, 3, 12, 15)
PENALTIES = ((8, 32), (5, 5), (0, 32767), (20, 100), (32767, 32767))
# (W, H, P): a direction without a predecessor; 2 x 2; around 8, 16, 32 and 64 columns; around 8 and 64 rows; more than one
# workgroup in both axes with more than one pair
SHAPES = [(1, 1, 1), (1, 9, 1), (9, 1, 1), (2, 2, 1), (7, 3, 1), (8, 9, 1), (15, 2, 1), (16, 7, 1), (17, 8, 1), (31, 5, 1), (32, 3, 1),
          (33, 9, 2), (63, 4, 1), (64, 2, 1), (65, 66, 1), (5, 63, 1), (3, 64, 1), (9, 65, 2), (130, 19, 1), (97, 67, 3)]


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def A_(prm):
    import opengpc_amd as g
    return g.Aggregate(*prm)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))       # (a copy: the shared cases are read-only)


def filled(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def aggregate_device(ctx, d_field, d_L, d_R, shape, prm, flags=(True,) * 4, in_place=False):
    """the device form over arrays already on the device: the outputs read back from sentinel-filled arrays"""
    import torch
    P, Cn, H, W = shape
    d_out = d_field if in_place else filled(P, Cn, H, W, 4)
    d = [filled(P, H, W, 2), filled(P, H, W), filled(P, 4, 4), filled(P, H, W, 4)]
    torch.cuda.synchronize()
    ctx.aggregate_fields_device(d_field.data_ptr(), d_L.data_ptr(), d_R.data_ptr(), Cn, W, H, P, A_(prm), d_out.data_ptr(),
                                *[t.data_ptr() if f else 0 for t, f in zip(d, flags)])
    ctx.synchronize()
    return (d_out.cpu().numpy().view(np.int32).reshape(P, Cn, H, W), d[0].cpu().numpy().view(np.uint16).reshape(P, H, W),
            d[1].cpu().numpy().reshape(P, H, W), d[2].cpu().numpy().view(np.int32).reshape(P, 4),
            d[3].cpu().numpy().view(np.uint32).reshape(P, H, W))


def same(got, want, what, names=NAMES):
    for n, g_, w in zip(names, got, want):
        assert g_.dtype == w.dtype and g_.shape == w.shape, (what, n)
        if not np.array_equal(g_, w):
            bad = np.argwhere(g_ != w)
            raise AssertionError("%s: %s differs at %d of %d elements, the first at %s: %s, expected %s" % (
                what, n, len(bad), w.size, bad[0].tolist(), g_[tuple(bad[0])], w[tuple(bad[0])]))


def check(ctx, field, L, R, prm, what):
    got = aggregate_device(ctx, dev(field), dev(L), dev(R), field.shape, prm)
    same(got, au.aggregate(field, L, R, prm), what)
    return got


@pytest.mark.parametrize("R", [0, 1, 2])
@pytest.mark.parametrize("radius", [1, 2, 4])
@pytest.mark.parametrize("Cn", [1, 2])
def test_every_byte_equals_the_rule(ctx, Cn, radius, R):
    """the stepped prior at every shape, the paths, penalties and the parabola taking turns; then search_util's kinds"""
    turn = 3 * Cn + radius + R
    for i, (W, H, P) in enumerate(SHAPES):
        field, L, Rr = au.stepped_case(W, H, P, Cn, R)
        d = dev(field), dev(L), dev(Rr)
        for j in range(2):
            t = turn + 2 * i + j
            prm = (radius, R, t % 2, 0xFFFF) + PENALTIES[t % len(PENALTIES)] + (PATHS[t % len(PATHS)],)
            same(aggregate_device(ctx, *d, field.shape, prm), au.expected_stepped(W, H, P, Cn, prm), ("stepped", W, H, P, Cn, prm))
    for kind in su.KINDS:
        for W, H, P in su.SIZES:
            field, L, Rr = su.case(kind, W, H, P, Cn)
            prm = (radius, R, 1, 0xFFFF, 8, 32, 15)
            same(aggregate_device(ctx, dev(field), dev(L), dev(Rr), field.shape, prm), au.expected_search_case(kind, W, H, P, Cn, prm),
                 (kind, W, H, P, Cn, prm))


@pytest.mark.parametrize("paths", PATHS)
@pytest.mark.parametrize("Cn", [1, 2])
def test_every_path_with_every_penalty(ctx, Cn, paths):
    """each single bit of paths, 3, 12 and 15, with every pair of penalties, at the ranges that have more than one label"""
    W, H, P = 97, 67, 3
    for R in (1, 2):
        field, L, Rr = au.stepped_case(W, H, P, Cn, R)
        d = dev(field), dev(L), dev(Rr)
        for p1, p2 in PENALTIES:
            prm = (2, R, 1, 0xFFFF, p1, p2, paths)
            got = aggregate_device(ctx, *d, field.shape, prm)
            same(got, au.expected_stepped(W, H, P, Cn, prm), ("paths", Cn, prm))
            assert (got[3][:, :3] > 0).all()                                   # kept, holes and unmatched pixels, all there


def test_the_crafted_scene(ctx):
    """the winners are written out by hand (tests/test_aggregate.py has the arithmetic, and checks the scene on the CPU): in
    the band without texture the search keeps the prior, the aggregated choice follows its neighbours"""
    import opengpc_amd as g
    field, L, R = au.scene()
    d_f, d_L, d_R = dev(field), dev(L), dev(R)
    prm = au.SCENE_PRM
    got = aggregate_device(ctx, d_f, d_L, d_R, field.shape, prm)
    d_choice, d_tmp = filled(1, au.SCENE_H, au.SCENE_W), filled(1, 1, au.SCENE_H, au.SCENE_W, 4)
    ctx.search_fields_device(d_f.data_ptr(), d_L.data_ptr(), d_R.data_ptr(), 1, au.SCENE_W, au.SCENE_H, 1, g.Search(*prm[:4]),
                             d_tmp.data_ptr(), 0, d_choice.data_ptr())
    ctx.synchronize()
    for y in range(au.SCENE_H):
        assert d_choice.cpu().numpy()[0, y].tolist() == SEARCH_WINNERS, y
        assert got[2][0, y].tolist() == AGGREGATE_WINNERS, y
        assert got[0][0, 0, y, 2:].tolist() == [256] * 18 and got[0][0, 0, y, :2].tolist() == [-256, -256], y
    assert SEARCH_WINNERS[7:12] == [1] * 5 and AGGREGATE_WINNERS[7:12] == [0] * 5


@pytest.mark.parametrize("Cn", [1, 2])
def test_identities_on_the_device(ctx, Cn):
    """paths = 0 (any p1, p2) and p1 = p2 = 0 (any paths): out, cost, choice and stats are search_fields_device's"""
    import opengpc_amd as g
    W, H, P = su.SIZES[-1]
    for field, L, R in (su.case("random", W, H, P, Cn), au.stepped_case(W, H, P, Cn, 2)):
        d_f, d_L, d_R = dev(field), dev(L), dev(R)
        for sp in ((2, 1, 1, 0xFFFF), (1, 2, 0, 2500), (4, 2, 1, 0xFFFF)):
            d_out, d_cost, d_choice, d_stats = filled(P, Cn, H, W, 4), filled(P, H, W, 2), filled(P, H, W), filled(P, 4, 4)
            ctx.search_fields_device(d_f.data_ptr(), d_L.data_ptr(), d_R.data_ptr(), Cn, W, H, P, g.Search(*sp), d_out.data_ptr(),
                                     d_cost.data_ptr(), d_choice.data_ptr(), d_stats.data_ptr())
            ctx.synchronize()
            want = (d_out.cpu().numpy().view(np.int32).reshape(P, Cn, H, W), d_cost.cpu().numpy().view(np.uint16).reshape(P, H, W),
                    d_choice.cpu().numpy().reshape(P, H, W), d_stats.cpu().numpy().view(np.int32).reshape(P, 4))
            for p1, p2, paths in ((8, 32, 0), (0, 32767, 0), (0, 0, 15), (0, 0, 2), (0, 0, 12)):
                got = aggregate_device(ctx, d_f, d_L, d_R, field.shape, sp + (p1, p2, paths))
                same(got[:4], want, ("identity", Cn, sp, p1, p2, paths))
                matched = want[1] != 0xFFFF
                assert np.array_equal(got[4][matched], (bin(paths).count("1") or 1) * want[1][matched].astype(np.uint32))
                assert (got[4][~matched] == au.NO_AGG).all()


@pytest.mark.parametrize("Cn", [1, 2])
def test_ceiling_and_documented_defaults(ctx, Cn):
    import opengpc_amd as g
    W, H, P = su.SIZES[-1]
    field, L, R = su.case("random", W, H, P, Cn)
    for max_cost in (3000, 0):
        got = check(ctx, field, L, R, (2, 1, 1, max_cost, 8, 32, 15), ("ceiling", Cn, max_cost))
        assert got[3][:, 3].sum() > 0 and ((got[1] != 0xFFFF) & (got[0][:, 0] == N)).any()      # rejected pixels keep their cost
        assert ((got[4] != au.NO_AGG) & (got[0][:, 0] == N)).any()                              # and their sum
    d = g.Aggregate()
    assert (d.radius, d.range, d.subpixel, d.max_cost, d.p1, d.p2, d.paths) == au.DEFAULTS
    got = check(ctx, field, L, R, au.DEFAULTS, ("defaults", Cn))
    assert (got[3][:, 3] == 0).all() and (got[3][:, :3] > 0).all()


@pytest.mark.parametrize("Cn", [1, 2])
def test_aliasing_optional_outputs_and_inputs(ctx, Cn):
    W, H, P = su.SIZES[-1]
    field, L, R = au.stepped_case(W, H, P, Cn, 2)
    prm = (2, 2, 1, 4000, 6, 50, 15)
    want = au.aggregate(field, L, R, prm)
    d_f, d_L, d_R = dev(field), dev(L), dev(R)
    same(aggregate_device(ctx, d_f, d_L, d_R, field.shape, prm), want, "plain")
    for d, a in ((d_f, field), (d_L, L), (d_R, R)):                            # the inputs are as they were
        assert np.array_equal(d.cpu().numpy(), a)
    for k in range(4):                                                          # each optional output left out: the others unchanged, it untouched
        flags = [True] * 4
        flags[k] = False
        got = aggregate_device(ctx, d_f, d_L, d_R, field.shape, prm, flags)
        keep = [i for i in range(5) if i != k + 1]
        same([got[i] for i in keep], [want[i] for i in keep], ("without", NAMES[k + 1]), [NAMES[i] for i in keep])
        assert (got[k + 1].view(np.uint8) == FILL).all()
    same(aggregate_device(ctx, d_f, d_L, d_R, field.shape, prm, in_place=True), want, "out == field")


def test_no_leak_between_pairs(ctx):
    """pair t of a batch equals pair t alone, whatever stands beside it"""
    W, H, P = su.SIZES[-1]
    for Cn in (1, 2):
        field, L, R = au.stepped_case(W, H, P, Cn, 1)
        prm = (2, 1, 1, 3000, 8, 32, 15)
        whole = check(ctx, field, L, R, prm, ("batch", Cn))
        for t in range(P):
            one = check(ctx, field[t:t + 1], L[t:t + 1], R[t:t + 1], prm, ("alone", Cn, t))
            for a, b in zip(whole, one):
                assert np.array_equal(a[t:t + 1], b)


@pytest.mark.parametrize("Cn", [1, 2])
def test_extremes(ctx, Cn):
    """INT32_MAX, INT32_MIN + 1 and (C = 2) a GPC_DENSE_NONE in channel 1 of a valued pixel: their targets lie far outside the
    image, so the pixels are unmatched and every path through them starts anew -- beside pixels that are matched"""
    W, H = 37, 19
    rng = np.random.default_rng(11)
    L, R = su.images("random", W, H, 1, Cn, seed=5)
    field = np.zeros((1, Cn, H, W), np.int32)
    field[0, 0] = rng.choice(np.array([su.IMAX, su.IMIN1, 0, 256, -512], np.int64), (H, W)).astype(np.int32)
    if Cn == 2:
        field[0, 1] = rng.choice(np.array([su.IMAX, su.IMIN1, N, 0, 300], np.int64), (H, W)).astype(np.int32)
    for prm in ((1, 0, 1, 0xFFFF, 8, 32, 15), (4, 2, 1, 0xFFFF, 3, 32767, 15)):
        got = check(ctx, field, L, R, prm, ("extremes", Cn, prm))
        assert got[3][0, 0] > 0 and got[3][0, 2] > 0 and got[3][0, 1] == 0


@pytest.mark.parametrize("Cn", [1, 2])
def test_a_path_starts_anew_behind_a_pixel_that_is_not_live(ctx, Cn):
    """The directed case of DESIGN.md 4.20's mutation record for `live` (mutant (c), which no test fails because it changes
    no value): a hole and a pixel whose targets all lie outside the image stand in the middle of a row and of a column of
    random images; the expectation is aggregate_plain's, pixel by pixel, and behind either pixel every path that comes
    through it holds the raw cost again -- one direction at a time, so that the sum is the path's own value."""
    W, H = 11, 7
    L, R = su.images("random", W, H, 1, Cn, seed=9)
    field = np.zeros((1, Cn, H, W), np.int32)
    field[0, 0, 3, 4] = N                                                     # a hole
    field[0, 0, 3, 7] = 256 * (W + 5) * (1 if Cn == 2 else -1)                # every target right of the image
    field[0, 0, 1, 5] = N
    for paths in (1, 2, 4, 8, 15):
        prm = (1, 1, 1, 0xFFFF, 7, 40, paths)
        got = aggregate_device(ctx, dev(field), dev(L), dev(R), field.shape, prm)
        out, cost, choice, state, agg = au.aggregate_plain(field[0], L[0], R[0], prm)
        same(got, (out[None], cost[None], choice[None], np.bincount(state.ravel(), minlength=4)[None, :4].astype(np.int32), agg[None]),
             ("not live", Cn, paths))
        assert state[3, 4] == 1 and state[3, 7] == 2 and got[3][0, 1] == 2 and got[3][0, 2] == 1
        if paths < 15:                                                        # the pixel behind, in the path's direction: S is the raw cost
            dx, dy = {1: (1, 0), 2: (-1, 0), 4: (0, 1), 8: (0, -1)}[paths]
            for x, y in ((4 + dx, 3 + dy), (7 + dx, 3 + dy), (5 + dx, 1 + dy)):
                assert state[y, x] in (0, 3) and got[4][0, y, x] == got[1][0, y, x], (paths, x, y)


def test_more_than_one_workspace_group(monkeypatch):
    """GPC_HIP_AGG_GROUP_BYTES (read when a context is made) shrinks the budget of a group of pairs: 5 pairs in groups of 1, of
    2 and in one go give the same bytes, in place too"""
    import opengpc_amd as g
    W, H, P = 41, 23, 5
    for Cn in (1, 2):
        field, L, R = au.stepped_case(W, H, P, Cn, 1)
        prm = (2, 1, 1, 3000, 8, 32, 15)
        want = au.aggregate(field, L, R, prm)
        per_pair = 2 * ((3 if Cn == 1 else 9) * 4 + (5 if Cn == 1 else 25)) * W * H      # the header: 10 + 6 d, 50 + 18 d bytes a pixel
        for budget in (1, 2 * per_pair + 5, None):
            if budget is None:
                monkeypatch.delenv("GPC_HIP_AGG_GROUP_BYTES", raising=False)
            else:
                monkeypatch.setenv("GPC_HIP_AGG_GROUP_BYTES", str(budget))
            c = g.Context(0)
            try:
                same(aggregate_device(c, dev(field), dev(L), dev(R), field.shape, prm), want, ("groups", Cn, budget))
                same(aggregate_device(c, dev(field), dev(L), dev(R), field.shape, prm, in_place=True), want, ("groups in place", Cn, budget))
            finally:
                c.close()


def test_host_form(ctx):
    """gpc_hip_aggregate_fields: 35 pairs go up in chunks of 16, 16 and 3; what comes back equals the device form"""
    W, H, P = 33, 9, 35
    for Cn in (1, 2):
        field, (L, R) = au.stepped_fields(W, H, Cn, P, 1, seed=77 + Cn), su.images("random", W, H, P, Cn, seed=3)
        prm = (2, 1, 1, 3000, 8, 32, 15)
        want = aggregate_device(ctx, dev(field), dev(L), dev(R), field.shape, prm)
        same(ctx.aggregate_fields(field, L, R, A_(prm)), want, ("host", Cn))
        same(want, au.aggregate(field, L, R, prm), ("host: the device form", Cn))
        res = ctx.aggregate_fields(field, L, R, A_(prm), want_cost=False, want_choice=False, want_stats=False, want_agg=False)
        assert np.array_equal(res[0], want[0]) and all(r is None for r in res[1:])


def settings(epipolar):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epipolar, False, 1)


def match_forms(c, batch, images, W, H, P, Cn, s, radius, ag, prm, what):
    """aggregate_batch_device / aggregate_sequence_device against the chain of calls they are made of: match, refine, fill,
    aggregate, flip, fill, aggregate with the images exchanged, clean -- every output"""
    import opengpc_amd as g
    import torch
    fill = g.Densify()
    corr = not batch
    cap = (W - 26) * (H - 26) + 1
    rec_bytes = 16 if corr else 12
    iL, iR = (images[0], images[1]) if batch else (images[0], images[0] + W * H)
    check_on = prm.check_tol_q8 >= 0

    def buffers():
        return dict(out=filled(P, Cn, H, W, 4), state=filled(P, H, W), label=filled(P, H, W, 4), stats=filled(P, 4, 4),
                    fwd=filled(P, Cn, H, W, 4), level=filled(P, H, W), cnt=filled(P, 4), nc=filled(*((P, 2, 4) if batch else (P + 1, 4))),
                    cost=filled(P, H, W, 2))

    a, b = buffers(), buffers()
    rec, ref, bwd = filled(P, cap, rec_bytes), filled(P, cap, 8), filled(P, Cn, H, W, 4)
    p = lambda d, n: d[n].data_ptr()
    torch.cuda.synchronize()
    if batch:
        c.match_batch_device(iL, iR, W, H, P, s, rec.data_ptr(), cap, p(a, "cnt"), p(a, "nc"))
    else:
        c.match_sequence_device(iL, W, H, P + 1, s, rec.data_ptr(), cap, p(a, "cnt"), p(a, "nc"))
    d_ref = 0
    if radius >= 1:
        d_ref = ref.data_ptr()
        c.refine_records_device(rec.data_ptr(), corr, cap, p(a, "cnt"), iL, iR, W, H, P, radius, d_ref)
    c.densify_records_device(rec.data_ptr(), corr, cap, p(a, "cnt"), W, H, P, fill, p(a, "fwd"), p(a, "level"), d_ref)
    c.aggregate_fields_device(p(a, "fwd"), iL, iR, Cn, W, H, P, ag, p(a, "fwd"), p(a, "cost"))
    if check_on:
        c.flip_records_device(rec.data_ptr(), corr, cap, p(a, "cnt"), P, rec.data_ptr(), d_ref, d_ref)
        c.densify_records_device(rec.data_ptr(), corr, cap, p(a, "cnt"), W, H, P, fill, bwd.data_ptr(), 0, d_ref)
        c.aggregate_fields_device(bwd.data_ptr(), iR, iL, Cn, W, H, P, ag, bwd.data_ptr())
    c.clean_fields_device(p(a, "fwd"), Cn, W, H, P, prm, p(a, "out"), bwd.data_ptr() if check_on else 0, p(a, "state"), p(a, "label"),
                          p(a, "stats"))
    args = (s, fill, ag, prm, p(b, "out"), p(b, "state"), p(b, "label"), p(b, "stats"), p(b, "fwd"), p(b, "level"), radius, p(b, "cnt"),
            p(b, "nc"), p(b, "cost"))
    if batch:
        c.aggregate_batch_device(iL, iR, W, H, P, *args)
    else:
        c.aggregate_sequence_device(iL, W, H, P + 1, *args)
    c.synchronize()
    A, B = ({n: d.cpu().numpy() for n, d in x.items()} for x in (a, b))
    for n in A:
        assert np.array_equal(A[n], B[n]), (what, n)
        assert not (A[n] == FILL).all(), (what, n)
    stats = A["stats"].view(np.int32).reshape(P, 4)
    cost = A["cost"].view(np.uint16).reshape(P, H, W)
    print("clean stats", what, stats.tolist(), "pixels with a cost", (cost != 0xFFFF).sum((1, 2)).tolist())
    assert (stats[:, 0] > 0).all() and ((cost != 0xFFFF).sum((1, 2)) > 0).all(), what
    d_only = filled(P, Cn, H, W, 4)                                            # the optional outputs left out
    torch.cuda.synchronize()
    if batch:
        c.aggregate_batch_device(iL, iR, W, H, P, s, fill, ag, prm, d_only.data_ptr(), refine_radius=radius)
    else:
        c.aggregate_sequence_device(iL, W, H, P + 1, s, fill, ag, prm, d_only.data_ptr(), refine_radius=radius)
    c.synchronize()
    assert np.array_equal(d_only.cpu().numpy(), A["out"]), what


@pytest.mark.parametrize("check_tol", [256, -1])
def test_match_fill_aggregate_and_clean_batch(oracle, forest_paths, check_tol):
    """the synthetic pairs of tests/test_gpu_dense.py (96 x 64, D = 5), the zero forest"""
    import opengpc_amd as g
    W, H, B, D = 96, 64, 2, 5
    c = g.Context(0)
    try:
        c.load_forest(forest_paths["zero"], W, H)
        pairs = [oracle.synth_pair(W, H, i, D) for i in range(B)]
        d_L, d_R = (dev(np.stack([q[k] for q in pairs])) for k in (0, 1))
        for radius in (0, 3):
            match_forms(c, True, (d_L.data_ptr(), d_R.data_ptr()), W, H, B, 1, settings(True), radius, g.Aggregate(),
                        g.Clean(check_tol), ("batch", check_tol, radius))
    finally:
        c.close()


@pytest.mark.parametrize("check_tol", [256, -1])
def test_match_fill_aggregate_and_clean_sequence(ctx, forest_paths, check_tol):
    """three frames of 96 x 64 (the sequence of tests/test_gpu_clean.py): the images of pair t are frames t and t + 1"""
    import opengpc_amd as g
    W, H, F = 96, 64, 3
    d_f = dev(tu.frames_of(W, H, F, 1, 0))
    ctx.load_forest(forest_paths["zero"], W, H)
    for radius in (0, 3):
        match_forms(ctx, False, (d_f.data_ptr(),), W, H, F - 1, 2, settings(True), radius, g.Aggregate(2, 2, 1, 0xFFFF, 10, 40, 15),
                    g.Clean(check_tol), ("sequence", check_tol, radius))


def test_refusals(forest_paths):
    """every refusal of the group, and the outputs afterwards: not a byte written"""
    import opengpc_amd as g
    import torch
    W, H = 96, 64
    E, U = g.capi.E_INVALID, g.capi.E_UNSUPPORTED
    c = g.Context(0)
    try:
        L = c.L
        d_f, d_l, d_r = filled(2, 2, H, W, 4), filled(2, H, W), filled(2, H, W)
        d_out, d_cost, d_choice, d_stats, d_agg = filled(2, 2, H, W, 4), filled(2, H, W, 2), filled(2, H, W), filled(2, 4, 4), filled(2, H, W, 4)
        good = g.Aggregate()
        torch.cuda.synchronize()

        def fields(fn=L.gpc_hip_aggregate_fields_device, field=d_f.data_ptr(), l=d_l.data_ptr(), r=d_r.data_ptr(), ch=2, w=W, h=H,
                   npairs=2, prm=good, out=d_out.data_ptr()):
            return fn(c.h, field, l, r, ch, w, h, npairs, C.byref(prm) if prm is not None else None, out, d_cost.data_ptr(),
                      d_choice.data_ptr(), d_stats.data_ptr(), d_agg.data_ptr())

        A = g.Aggregate
        for bad in (A(0), A(5), A(2, -1), A(2, 3), A(2, 1, -1), A(2, 1, 2), A(2, 1, 1, -1), A(2, 1, 1, 0x10000),      # the search's
                    A(p1=-1), A(p1=513, p2=512), A(p1=0, p2=32768), A(p1=32768, p2=32768), A(p2=-1, p1=-2), A(paths=-1), A(paths=16)):
            assert fields(prm=bad) == E, (bad.radius, bad.range, bad.subpixel, bad.max_cost, bad.p1, bad.p2, bad.paths)
        assert fields(prm=None) == E and fields(field=None) == E and fields(out=None) == E and fields(l=None) == E and fields(r=None) == E
        assert fields(ch=0) == E and fields(ch=3) == E and fields(npairs=0) == E and fields(w=0) == E and fields(h=-1) == E
        assert fields(out=d_f.data_ptr() + 4 * W * H) == E and fields(out=d_f.data_ptr() - 16) == E      # any overlap but the field itself
        assert fields(out=d_l.data_ptr(), ch=1, npairs=1, w=8, h=8) == E                                  # out over an image
        assert fields(out=d_r.data_ptr() + 2 * W * H - 4, ch=1) == E
        assert fields(w=32769, h=1, npairs=1) == U and fields(w=1, h=32769, npairs=1) == U and fields(w=32768, h=32769, npairs=1) == U
        assert fields(npairs=65536, w=1, h=1) == U
        c.synchronize()
        for d in (d_out, d_cost, d_choice, d_stats, d_agg, d_f, d_l, d_r):
            assert bool((d == FILL).all())
        # the host form: the same checks on host arrays
        hf, hl, hr = np.zeros((2, 1, H, W), np.int32), np.zeros((2, H, W), np.uint8), np.zeros((2, H, W), np.uint8)
        ho = np.full((2, 1, H, W, 4), FILL, np.uint8)
        host = lambda prm=good, l=hl.ctypes.data, npairs=2, out=ho.ctypes.data, w=W: L.gpc_hip_aggregate_fields(
            c.h, hf.ctypes.data, l, hr.ctypes.data, 1, w, H, npairs, C.byref(prm), out, None, None, None, None)
        assert host(prm=A(0)) == E and host(prm=A(paths=16)) == E and host(prm=A(p1=9, p2=8)) == E
        assert host(l=None) == E and host(npairs=0) == E and host(out=None) == E
        assert host(out=hf.ctypes.data + 4) == E and host(out=hl.ctypes.data) == E and host(npairs=65536) == U and host(w=40000) == U
        assert (ho == FILL).all()
        # the match forms: their own refusals and those of the calls they wrap
        s, fill, cl = settings(True), g.Densify(), g.Clean()
        d_fr = dev(tu.frames_of(W, H, 3, 1))
        iL, iR = d_fr.data_ptr(), d_fr.data_ptr() + W * H
        seq = lambda nframes=3, radius=0, fl=fill, prm=cl, ag=good, out=d_out.data_ptr(), w=W, fwd=None: \
            L.gpc_hip_aggregate_sequence_device(c.h, iL, w, H, nframes, C.byref(s), radius, C.byref(fl), C.byref(ag) if ag is not None else None,
                                                C.byref(prm), out, None, None, None, fwd, None, None, None, None)
        bat = lambda npairs=2, radius=0, fl=fill, prm=cl, ag=good, out=d_out.data_ptr(), w=W, fwd=None: \
            L.gpc_hip_aggregate_batch_device(c.h, iL, iR, w, H, npairs, C.byref(s), radius, C.byref(fl), C.byref(ag) if ag is not None else None,
                                             C.byref(prm), out, None, None, None, fwd, None, None, None, None)
        assert seq() == g.capi.E_NO_FOREST and bat() == g.capi.E_NO_FOREST
        c.load_forest(forest_paths["zero"], W, H)
        for call in (seq, bat):
            assert call(radius=-1) == E and call(radius=7) == E and call(out=None) == E and call(w=W + 1) == E
            assert call(fl=g.Densify(15, 1, 3)) == E and call(prm=g.Clean(256, 256, 64, 3)) == E
            assert call(ag=None) == E and call(ag=A(5)) == E and call(ag=A(2, 3)) == E and call(ag=A(paths=16)) == E and call(ag=A(p1=600)) == E
            assert call(fwd=d_out.data_ptr()) == E
        assert seq(nframes=1) == E and bat(npairs=0) == E
        c.synchronize()
        assert bool((d_out == FILL).all())
    finally:
        c.close()
