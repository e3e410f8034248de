"""The local dense search on the GPU (gpc_hip_search_*): every byte of out, cost, choice and stats EQUALS the restatement of
the rule (tests/search_util.py) -- every output starts out filled with a sentinel, and every element must be written -- at
sizes below, at and across the 32 x 8 tile with more than one pair, both channel counts, radii 1, 2 and 4, ranges 0, 1 and 2,
with and without the parabola, on three kinds of image pair; single cases for a ceiling that rejects, the documented
defaults, aliasing, the optional outputs, leaks between pairs, untouched inputs and the extremes of int32; the host form
equals the device form; the match forms equal the chain of the calls they are made of; the refusals; the timing slot."""
import ctypes as C

import numpy as np
import pytest

import search_util as su
import track_util as tu

pytestmark = pytest.mark.gpu

FILL = 0xA5
N = su.NONE
NAMES = ("out", "cost", "choice", "stats")


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def S_(prm):
    import opengpc_amd as g
    return g.Search(*prm)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))       # (a copy: the shared cases are read-only)


def filled(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def search_device(ctx, d_field, d_L, d_R, shape, prm, with_cost=True, with_choice=True, with_stats=True, in_place=False):
    """the device form over arrays already on the device: the outputs read back from sentinel-filled arrays"""
    import torch
    P, Cn, H, W = shape
    d_out = d_field if in_place else filled(P, Cn, H, W, 4)
    d_cost, d_choice, d_stats = filled(P, H, W, 2), filled(P, H, W), filled(P, 4, 4)
    torch.cuda.synchronize()
    ctx.search_fields_device(d_field.data_ptr(), d_L.data_ptr(), d_R.data_ptr(), Cn, W, H, P, S_(prm), d_out.data_ptr(),
                             d_cost.data_ptr() if with_cost else 0, d_choice.data_ptr() if with_choice else 0,
                             d_stats.data_ptr() if with_stats else 0)
    ctx.synchronize()
    return (d_out.cpu().numpy().view(np.int32).reshape(P, Cn, H, W), d_cost.cpu().numpy().view(np.uint16).reshape(P, H, W),
            d_choice.cpu().numpy().reshape(P, H, W), d_stats.cpu().numpy().view(np.int32).reshape(P, 4))


def same(got, want, what, names=NAMES):
    for n, g_, w in zip(names, got, want):
        if n in NAMES and w is not None:
            assert g_.dtype == w.dtype and g_.shape == w.shape, (what, n)
            if not np.array_equal(g_, w):
                bad = np.argwhere(g_ != w)
                raise AssertionError("%s: %s differs at %d of %d elements, the first at %s: %s, expected %s" % (
                    what, n, len(bad), w.size, bad[0].tolist(), g_[tuple(bad[0])], w[tuple(bad[0])]))


def check(ctx, field, L, R, prm, what):
    got = search_device(ctx, dev(field), dev(L), dev(R), field.shape, prm)
    same(got, su.search(field, L, R, prm), what)
    return got


@pytest.mark.parametrize("R", [0, 1, 2])
@pytest.mark.parametrize("radius", [1, 2, 4])
@pytest.mark.parametrize("Cn", [1, 2])
def test_every_byte_equals_the_rule(ctx, Cn, radius, R):
    for kind in su.KINDS:
        for W, H, P in su.SIZES:
            field, L, Rr = su.case(kind, W, H, P, Cn)
            d = dev(field), dev(L), dev(Rr)
            for subpixel in (0, 1):
                prm = (radius, R, subpixel, 0xFFFF)
                same(search_device(ctx, *d, field.shape, prm), su.expected(kind, W, H, P, Cn, prm), (kind, W, H, P, Cn, prm))


@pytest.mark.parametrize("Cn", [1, 2])
def test_ceiling_and_documented_defaults(ctx, Cn):
    import opengpc_amd as g
    W, H, P = su.SIZES[-1]
    field, L, R = su.case("random", W, H, P, Cn)
    for max_cost in (3000, 0):
        got = check(ctx, field, L, R, (2, 1, 1, max_cost), ("ceiling", Cn, max_cost))
        assert got[3][:, 3].sum() > 0 and ((got[1] != 0xFFFF) & (got[0][:, 0] == N)).any()      # rejected pixels keep their cost
    d = g.Search()
    assert (d.radius, d.range, d.subpixel, d.max_cost) == su.DEFAULTS
    got = check(ctx, field, L, R, su.DEFAULTS, ("defaults", Cn))
    assert (got[3][:, 3] == 0).all() and (got[3][:, :3] > 0).all()


@pytest.mark.parametrize("Cn", [1, 2])
def test_aliasing_optional_outputs_and_inputs(ctx, Cn):
    W, H, P = su.SIZES[-1]
    field, L, R = su.case("random", W, H, P, Cn)
    prm = (2, 2, 1, 4000)
    want = su.search(field, L, R, prm)
    d_f, d_L, d_R = dev(field), dev(L), dev(R)
    same(search_device(ctx, d_f, d_L, d_R, field.shape, prm), want, "plain")
    for d, a in ((d_f, field), (d_L, L), (d_R, R)):                            # the inputs are as they were
        assert np.array_equal(d.cpu().numpy(), a)
    for k in range(3):                                                          # each optional output left out: the others unchanged, it untouched
        flags = [True] * 3
        flags[k] = False
        got = search_device(ctx, d_f, d_L, d_R, field.shape, prm, *flags)
        same([g_ for i, g_ in enumerate(got) if i != k + 1], [w for i, w in enumerate(want) if i != k + 1], ("without", NAMES[k + 1]),
             [n for i, n in enumerate(NAMES) if i != k + 1])
        assert (got[k + 1].view(np.uint8) == FILL).all()
    same(search_device(ctx, d_f, d_L, d_R, field.shape, prm, in_place=True), want, "out == field")


def test_no_leak_between_pairs(ctx):
    """pair t of a batch equals pair t alone, whatever stands beside it"""
    W, H, P = su.SIZES[-1]
    for Cn in (1, 2):
        field, L, R = su.case("random", W, H, P, Cn)
        whole = check(ctx, field, L, R, (2, 1, 1, 3000), ("batch", Cn))
        for t in range(P):
            one = check(ctx, field[t:t + 1], L[t:t + 1], R[t:t + 1], (2, 1, 1, 3000), ("alone", Cn, t))
            for a, b in zip(whole, one):
                assert np.array_equal(a[t:t + 1], b)


@pytest.mark.parametrize("Cn", [1, 2])
def test_extremes(ctx, Cn):
    """INT32_MAX, INT32_MIN + 1 and (C = 2) a GPC_DENSE_NONE in channel 1 of a valued pixel are values like any other: their
    targets lie far outside the image, so the pixels are unmatched -- beside pixels that are matched"""
    W, H = 37, 19
    rng = np.random.default_rng(11)
    L, R = su.images("random", W, H, 1, Cn, seed=5)
    field = np.zeros((1, Cn, H, W), np.int32)
    field[0, 0] = rng.choice(np.array([su.IMAX, su.IMIN1, 0, 256, -512], np.int64), (H, W)).astype(np.int32)
    if Cn == 2:
        field[0, 1] = rng.choice(np.array([su.IMAX, su.IMIN1, N, 0, 300], np.int64), (H, W)).astype(np.int32)
    for prm in ((1, 0, 1, 0xFFFF), (4, 2, 1, 0xFFFF)):
        got = check(ctx, field, L, R, prm, ("extremes", Cn, prm))
        assert got[3][0, 0] > 0 and got[3][0, 2] > 0 and got[3][0, 1] == 0


def test_host_form(ctx):
    """gpc_hip_search_fields: 35 pairs go up in chunks of 16, 16 and 3; what comes back equals the device form"""
    W, H, P = 33, 9, 35
    for Cn in (1, 2):
        field, (L, R) = su.random_fields(W, H, Cn, P, seed=77 + Cn), su.images("random", W, H, P, Cn, seed=3)
        prm = (2, 1, 1, 3000)
        want = search_device(ctx, dev(field), dev(L), dev(R), field.shape, prm)
        same(ctx.search_fields(field, L, R, S_(prm)), want, ("host", Cn))
        same(want, su.search(field, L, R, prm), ("host: the device form", Cn))
        out, cost, choice, stats = ctx.search_fields(field, L, R, S_(prm), want_cost=False, want_choice=False, want_stats=False)
        assert np.array_equal(out, want[0]) and cost is None and choice is None and stats is None


def settings(epipolar):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epipolar, False, 1)


def match_forms(c, batch, images, W, H, P, Cn, s, radius, sr, prm, what):
    """search_batch_device / search_sequence_device against the chain of calls they are made of: match, refine, fill, search,
    flip, fill, search with the images exchanged, clean -- every output"""
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
    c.search_fields_device(p(a, "fwd"), iL, iR, Cn, W, H, P, sr, p(a, "fwd"), p(a, "cost"))
    if check_on:
        c.flip_records_device(rec.data_ptr(), corr, cap, p(a, "cnt"), P, rec.data_ptr(), d_ref, d_ref)
        c.densify_records_device(rec.data_ptr(), corr, cap, p(a, "cnt"), W, H, P, fill, bwd.data_ptr(), 0, d_ref)
        c.search_fields_device(bwd.data_ptr(), iR, iL, Cn, W, H, P, sr, bwd.data_ptr())
    c.clean_fields_device(p(a, "fwd"), Cn, W, H, P, prm, p(a, "out"), bwd.data_ptr() if check_on else 0, p(a, "state"), p(a, "label"),
                          p(a, "stats"))
    args = (s, fill, sr, prm, p(b, "out"), p(b, "state"), p(b, "label"), p(b, "stats"), p(b, "fwd"), p(b, "level"), radius, p(b, "cnt"),
            p(b, "nc"), p(b, "cost"))
    if batch:
        c.search_batch_device(iL, iR, W, H, P, *args)
    else:
        c.search_sequence_device(iL, W, H, P + 1, *args)
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
        c.search_batch_device(iL, iR, W, H, P, s, fill, sr, prm, d_only.data_ptr(), refine_radius=radius)
    else:
        c.search_sequence_device(iL, W, H, P + 1, s, fill, sr, prm, d_only.data_ptr(), refine_radius=radius)
    c.synchronize()
    assert np.array_equal(d_only.cpu().numpy(), A["out"]), what


@pytest.mark.parametrize("check_tol", [256, -1])
def test_match_fill_search_and_clean_batch(oracle, forest_paths, check_tol):
    """the synthetic pairs of tests/test_gpu_dense.py (96 x 64, D = 5), the zero forest"""
    import opengpc_amd as g
    W, H, B, D = 96, 64, 2, 5
    c = g.Context(0)
    try:
        c.load_forest(forest_paths["zero"], W, H)
        pairs = [oracle.synth_pair(W, H, i, D) for i in range(B)]
        d_L, d_R = (dev(np.stack([q[k] for q in pairs])) for k in (0, 1))
        for radius in (0, 3):
            match_forms(c, True, (d_L.data_ptr(), d_R.data_ptr()), W, H, B, 1, settings(True), radius, g.Search(),
                        g.Clean(check_tol), ("batch", check_tol, radius))
    finally:
        c.close()


@pytest.mark.parametrize("check_tol", [256, -1])
def test_match_fill_search_and_clean_sequence(ctx, forest_paths, check_tol):
    """three frames of 96 x 64 (the sequence of tests/test_gpu_clean.py): the images of pair t are frames t and t + 1"""
    import opengpc_amd as g
    W, H, F = 96, 64, 3
    d_f = dev(tu.frames_of(W, H, F, 1, 0))
    ctx.load_forest(forest_paths["zero"], W, H)
    for radius in (0, 3):
        match_forms(ctx, False, (d_f.data_ptr(),), W, H, F - 1, 2, settings(True), radius, g.Search(2, 2, 1, 0xFFFF), g.Clean(check_tol),
                    ("sequence", check_tol, radius))


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
        d_out, d_cost, d_choice, d_stats = filled(2, 2, H, W, 4), filled(2, H, W, 2), filled(2, H, W), filled(2, 4, 4)
        good = g.Search()
        torch.cuda.synchronize()

        def fields(fn=L.gpc_hip_search_fields_device, field=d_f.data_ptr(), l=d_l.data_ptr(), r=d_r.data_ptr(), ch=2, w=W, h=H, npairs=2,
                   prm=good, out=d_out.data_ptr()):
            return fn(c.h, field, l, r, ch, w, h, npairs, C.byref(prm) if prm is not None else None, out, d_cost.data_ptr(),
                      d_choice.data_ptr(), d_stats.data_ptr())

        for bad in (g.Search(0), g.Search(5), g.Search(2, -1), g.Search(2, 3), g.Search(2, 1, -1), g.Search(2, 1, 2), g.Search(2, 1, 1, -1),
                    g.Search(2, 1, 1, 0x10000)):
            assert fields(prm=bad) == E, (bad.radius, bad.range, bad.subpixel, bad.max_cost)
        assert fields(prm=None) == E and fields(field=None) == E and fields(out=None) == E and fields(l=None) == E and fields(r=None) == E
        assert fields(ch=0) == E and fields(ch=3) == E and fields(npairs=0) == E and fields(w=0) == E and fields(h=-1) == E
        assert fields(out=d_f.data_ptr() + 4 * W * H) == E and fields(out=d_f.data_ptr() - 16) == E      # any overlap but the field itself
        assert fields(out=d_l.data_ptr(), ch=1, npairs=1, w=8, h=8) == E                                  # out over an image
        assert fields(out=d_r.data_ptr() + 2 * W * H - 4, ch=1) == E
        assert fields(w=32769, h=1, npairs=1) == U and fields(w=1, h=32769, npairs=1) == U and fields(w=32768, h=32769, npairs=1) == U
        assert fields(npairs=65536, w=1, h=1) == U
        c.synchronize()
        for d in (d_out, d_cost, d_choice, d_stats, d_f, d_l, d_r):
            assert bool((d == FILL).all())
        # the host form: the same checks on host arrays
        hf, hl, hr = np.zeros((2, 1, H, W), np.int32), np.zeros((2, H, W), np.uint8), np.zeros((2, H, W), np.uint8)
        ho = np.full((2, 1, H, W, 4), FILL, np.uint8)
        host = lambda prm=good, l=hl.ctypes.data, npairs=2, out=ho.ctypes.data, w=W: L.gpc_hip_search_fields(
            c.h, hf.ctypes.data, l, hr.ctypes.data, 1, w, H, npairs, C.byref(prm), out, None, None, None)
        assert host(prm=g.Search(0)) == E and host(l=None) == E and host(npairs=0) == E and host(out=None) == E
        assert host(out=hf.ctypes.data + 4) == E and host(out=hl.ctypes.data) == E and host(npairs=65536) == U and host(w=40000) == U
        assert (ho == FILL).all()
        # the match forms: their own refusals and those of the calls they wrap
        s, fill, cl = settings(True), g.Densify(), g.Clean()
        d_fr = dev(tu.frames_of(W, H, 3, 1))
        iL, iR = d_fr.data_ptr(), d_fr.data_ptr() + W * H
        seq = lambda nframes=3, radius=0, fl=fill, prm=cl, sr=good, out=d_out.data_ptr(), w=W, fwd=None: \
            L.gpc_hip_search_sequence_device(c.h, iL, w, H, nframes, C.byref(s), radius, C.byref(fl), C.byref(sr) if sr is not None else None,
                                             C.byref(prm), out, None, None, None, fwd, None, None, None, None)
        bat = lambda npairs=2, radius=0, fl=fill, prm=cl, sr=good, out=d_out.data_ptr(), w=W, fwd=None: \
            L.gpc_hip_search_batch_device(c.h, iL, iR, w, H, npairs, C.byref(s), radius, C.byref(fl), C.byref(sr) if sr is not None else None,
                                          C.byref(prm), out, None, None, None, fwd, None, None, None, None)
        assert seq() == g.capi.E_NO_FOREST and bat() == g.capi.E_NO_FOREST
        c.load_forest(forest_paths["zero"], W, H)
        for call in (seq, bat):
            assert call(radius=-1) == E and call(radius=7) == E and call(out=None) == E and call(w=W + 1) == E
            assert call(fl=g.Densify(15, 1, 3)) == E and call(prm=g.Clean(256, 256, 64, 3)) == E
            assert call(sr=None) == E and call(sr=g.Search(5)) == E and call(sr=g.Search(2, 3)) == E
            assert call(fwd=d_out.data_ptr()) == E
        assert seq(nframes=1) == E and bat(npairs=0) == E
        c.synchronize()
        assert bool((d_out == FILL).all())
    finally:
        c.close()


def test_kernel_time_is_reported(ctx):
    """the timing slot before k_refine counts one launch per search and carries the instantiation's name"""
    W, H, P = su.SIZES[-1]
    names = [ctx.L.gpc_hip_kernel_name(i).decode() for i in range(ctx.L.gpc_hip_kernel_slots())]
    at = names.index("k_search")
    ctx.L.gpc_hip_enable_kernel_timing(ctx.h, 1)
    try:
        for Cn, prm in ((1, (2, 1, 1, 0xFFFF)), (2, (4, 2, 0, 0xFFFF))):
            field, L, R = su.case("random", W, H, P, Cn)
            ctx.L.gpc_hip_reset_kernel_timing(ctx.h)
            for k in range(3):
                search_device(ctx, dev(field), dev(L), dev(R), field.shape, prm)
            ms, n = C.c_float(0), C.c_int(0)
            assert ctx.L.gpc_hip_kernel_time(ctx.h, at, C.byref(ms), C.byref(n)) == 0
            assert n.value == 3 and ms.value > 0, (ms.value, n.value)
            assert ctx.L.gpc_hip_kernel_launch_name(ctx.h, at).decode() == "gpc::k_search<%d, %d, %d>" % (Cn, prm[0], prm[1])
    finally:
        ctx.L.gpc_hip_enable_kernel_timing(ctx.h, 0)
