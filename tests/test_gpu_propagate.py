"""The propagation of field values between neighbours on the GPU (gpc_hip_propagate_*): every byte of out, cost, choice and
stats EQUALS the restatement of the rule (tests/propagate_util.py) -- every output starts out filled with a sentinel, and
every element must be written -- at sizes below, at and across the 32 x 8 tile with more than one pair, both channel counts,
radii 1, 2 and 4, spans 1, 4 and 64 (larger than every image), 1, 2 and 3 iterations (both parities of the ping-pong), 4 and
8 neighbours, on the image kinds of the search plus "edge"; single cases for out == field, the optional outputs, untouched
inputs, leaks between pairs, the extremes of int32, a field of holes, a workspace that grows, the host form, the refusals,
and the composition with the search."""
import ctypes as C

import numpy as np
import pytest

import propagate_util as pu
import search_util as su

pytestmark = pytest.mark.gpu

FILL = 0xA5
N = pu.NONE
NAMES = ("out", "cost", "choice", "stats")


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def P_(prm):
    import opengpc_amd as g
    return g.Propagate(*prm)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))       # (a copy: the shared cases are read-only)


def filled(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def propagate_device(ctx, d_field, d_L, d_R, shape, prm, with_cost=True, with_choice=True, with_stats=True, in_place=False):
    """the device form over arrays already on the device: the outputs read back from sentinel-filled arrays"""
    import torch
    P, Cn, H, W = shape
    it = prm[2]
    d_out = d_field if in_place else filled(P, Cn, H, W, 4)
    d_cost, d_choice, d_stats = filled(P, H, W, 2), filled(P, H, W), filled(P, it, 4, 4)
    torch.cuda.synchronize()
    ctx.propagate_fields_device(d_field.data_ptr(), d_L.data_ptr(), d_R.data_ptr(), Cn, W, H, P, P_(prm), d_out.data_ptr(),
                                d_cost.data_ptr() if with_cost else 0, d_choice.data_ptr() if with_choice else 0,
                                d_stats.data_ptr() if with_stats else 0)
    ctx.synchronize()
    return (d_out.cpu().numpy().view(np.int32).reshape(P, Cn, H, W), d_cost.cpu().numpy().view(np.uint16).reshape(P, H, W),
            d_choice.cpu().numpy().reshape(P, H, W), d_stats.cpu().numpy().view(np.int32).reshape(P, it, 4))


def same(got, want, what, names=NAMES):
    for n, g_, w in zip(names, got, want):
        assert g_.dtype == w.dtype and g_.shape == w.shape, (what, n)
        if not np.array_equal(g_, w):
            bad = np.argwhere(g_ != w)
            raise AssertionError("%s: %s differs at %d of %d elements, the first at %s: %s, expected %s" % (
                what, n, len(bad), w.size, bad[0].tolist(), g_[tuple(bad[0])], w[tuple(bad[0])]))


def check(ctx, field, L, R, prm, what, **kw):
    got = propagate_device(ctx, dev(field), dev(L), dev(R), field.shape, prm, **kw)
    same(got, pu.propagate(field, L, R, prm), what)
    return got


@pytest.mark.parametrize("nb", [4, 8])
@pytest.mark.parametrize("radius", [1, 2, 4])
@pytest.mark.parametrize("Cn", [1, 2])
def test_every_byte_equals_the_rule(ctx, Cn, radius, nb):
    for kind in pu.KINDS:
        for W, H, P in pu.SIZES:
            field, L, Rr = pu.case(kind, W, H, P, Cn)
            d = dev(field), dev(L), dev(Rr)
            for span in pu.SPANS:
                for it in (1, 2, 3):
                    prm = (radius, span, it, nb)
                    same(propagate_device(ctx, *d, field.shape, prm), pu.expected(kind, W, H, P, Cn, prm), (kind, W, H, P, Cn, prm))


@pytest.mark.parametrize("Cn", [1, 2])
def test_documented_defaults(ctx, Cn):
    import opengpc_amd as g
    W, H, P = pu.SIZES[-1]
    d = g.Propagate()
    assert (d.radius, d.span, d.iterations, d.neighbours) == pu.DEFAULTS
    for kind in ("random", "edge"):
        field, L, R = pu.case(kind, W, H, P, Cn)
        got = check(ctx, field, L, R, pu.DEFAULTS, ("defaults", kind, Cn))
        assert (got[3][:, :, 3].sum(1) > 0).all()                                # every pair moved pixels


@pytest.mark.parametrize("Cn", [1, 2])
def test_aliasing_optional_outputs_and_inputs(ctx, Cn):
    W, H, P = pu.SIZES[-1]
    field, L, R = pu.case("random", W, H, P, Cn)
    for it in (3, 2, 1, 4):                                                     # odd and even N: both ends of the ping-pong
        prm = (2, 4, it, 8)
        want = pu.propagate(field, L, R, prm)
        d_f, d_L, d_R = dev(field), dev(L), dev(R)
        same(propagate_device(ctx, d_f, d_L, d_R, field.shape, prm), want, ("plain", it))
        for d, a in ((d_f, field), (d_L, L), (d_R, R)):                        # the inputs are as they were
            assert np.array_equal(d.cpu().numpy(), a)
        if it == 3:
            for k in range(3):                                                  # each optional output left out: the others unchanged, it untouched
                flags = [True] * 3
                flags[k] = False
                got = propagate_device(ctx, d_f, d_L, d_R, field.shape, prm, *flags)
                same([g_ for i, g_ in enumerate(got) if i != k + 1], [w for i, w in enumerate(want) if i != k + 1],
                     ("without", NAMES[k + 1]), [n for i, n in enumerate(NAMES) if i != k + 1])
                assert (got[k + 1].view(np.uint8) == FILL).all()
            got = propagate_device(ctx, d_f, d_L, d_R, field.shape, prm, False, False, False)      # none of them: no own cost is taken
            assert np.array_equal(got[0], want[0]) and all((g_.view(np.uint8) == FILL).all() for g_ in got[1:])
        same(propagate_device(ctx, d_f, d_L, d_R, field.shape, prm, in_place=True), want, ("out == field", it))
        assert np.array_equal(d_L.cpu().numpy(), L) and np.array_equal(d_R.cpu().numpy(), R)


def test_no_leak_between_pairs(ctx):
    """pair t of a batch equals pair t alone, whatever stands beside it"""
    W, H, P = pu.SIZES[-1]
    for Cn in (1, 2):
        field, L, R = pu.case("random", W, H, P, Cn)
        whole = check(ctx, field, L, R, (2, 4, 3, 8), ("batch", Cn))
        for t in range(P):
            one = check(ctx, field[t:t + 1], L[t:t + 1], R[t:t + 1], (2, 4, 3, 8), ("alone", Cn, t))
            for a, b in zip(whole, one):
                assert np.array_equal(a[t:t + 1], b)


@pytest.mark.parametrize("Cn", [1, 2])
def test_extremes(ctx, Cn):
    """INT32_MAX, INT32_MIN + 1 and (C = 2) a GPC_DENSE_NONE in channel 1 of a valued pixel are values like any other: their
    targets lie far outside the image, so where no neighbour helps the pixels are unmatched and copied unchanged -- beside
    pixels that are matched"""
    W, H = 37, 19
    rng = np.random.default_rng(11)
    L, R = su.images("random", W, H, 1, Cn, seed=5)
    field = np.zeros((1, Cn, H, W), np.int32)
    field[0, 0] = rng.choice(np.array([su.IMAX, su.IMIN1, 0, 256, -512], np.int64), (H, W)).astype(np.int32)
    field[0, 0, :, :12] = rng.choice(np.array([su.IMAX, su.IMIN1], np.int64), (H, 12)).astype(np.int32)   # further than 4 + 2 + 1 from help
    if Cn == 2:
        field[0, 1] = rng.choice(np.array([su.IMAX, su.IMIN1, N, 0, 300], np.int64), (H, W)).astype(np.int32)
    for prm in ((1, 1, 1, 4), (4, 4, 3, 8)):
        got = check(ctx, field, L, R, prm, ("extremes", Cn, prm))
        st = got[3][0, -1]
        assert st[0] > 0 and st[2] > 0 and st[1] == 0, st
        un = got[2][0] == 255
        assert np.array_equal(got[0][0][:, un], field[0][:, un]) and np.isin(field[0, 0][un], [su.IMAX, su.IMIN1]).any()
        if Cn == 2:
            assert (field[0, 1][un] == N).any()


@pytest.mark.parametrize("Cn", [1, 2])
def test_a_field_of_holes_only(ctx, Cn):
    W, H, P = 33, 9, 2
    L, R = su.images("random", W, H, P, Cn, seed=2)
    field = np.full((P, Cn, H, W), N, np.int32)
    if Cn == 2:
        field[:, 1] = 777                                                       # a hole's other channel is copied as it is
    got = check(ctx, field, L, R, (2, 4, 2, 8), ("holes", Cn))
    assert np.array_equal(got[0], field) and (got[1] == 0xFFFF).all() and (got[2] == 255).all()
    assert (got[3] == np.array([0, W * H, 0, 0])).all()


def test_the_workspace_grows():
    """a second call with a larger shape on the same context, then the small one again"""
    import opengpc_amd as g
    c = g.Context(0)
    try:
        for W, H, P in ((7, 5, 1), (70, 45, 3), (7, 5, 1)):
            field, L, R = pu.case("random", W, H, P, 2)
            check(c, field, L, R, (2, 4, 3, 8), ("grow", W, H, P))
            check(c, field, L, R, (2, 4, 3, 8), ("grow, in place", W, H, P), in_place=True)
    finally:
        c.close()


def test_host_form(ctx):
    """gpc_hip_propagate_fields: 35 pairs go up in chunks of 16, 16 and 3; what comes back equals the device form"""
    W, H, P = 33, 9, 35
    for Cn in (1, 2):
        field, (L, R) = su.random_fields(W, H, Cn, P, seed=77 + Cn), su.images("random", W, H, P, Cn, seed=3)
        prm = (2, 4, 3, 8)
        want = propagate_device(ctx, dev(field), dev(L), dev(R), field.shape, prm)
        same(ctx.propagate_fields(field, L, R, P_(prm)), want, ("host", Cn))
        same(want, pu.propagate(field, L, R, prm), ("host: the device form", Cn))
        out, cost, choice, stats = ctx.propagate_fields(field, L, R, P_(prm), want_cost=False, want_choice=False, want_stats=False)
        assert np.array_equal(out, want[0]) and cost is None and choice is None and stats is None


@pytest.mark.parametrize("Cn", [1, 2])
def test_propagate_then_search_equals_the_models_composed(ctx, Cn):
    import opengpc_amd as g
    W, H, P = pu.SIZES[-1]
    for kind in ("edge", "random"):
        field, L, R = pu.case(kind, W, H, P, Cn)
        mid = pu.propagate(field, L, R, (2, 4, 3, 8))[0]
        want = su.search(mid, L, R, su.DEFAULTS)
        d_f, d_L, d_R = dev(field), dev(L), dev(R)
        d_cost, d_choice, d_stats = filled(P, H, W, 2), filled(P, H, W), filled(P, 4, 4)
        ctx.propagate_fields_device(d_f.data_ptr(), d_L.data_ptr(), d_R.data_ptr(), Cn, W, H, P, P_((2, 4, 3, 8)), d_f.data_ptr())
        ctx.search_fields_device(d_f.data_ptr(), d_L.data_ptr(), d_R.data_ptr(), Cn, W, H, P, g.Search(*su.DEFAULTS), d_f.data_ptr(),
                                 d_cost.data_ptr(), d_choice.data_ptr(), d_stats.data_ptr())
        ctx.synchronize()
        got = (d_f.cpu().numpy(), d_cost.cpu().numpy().view(np.uint16).reshape(P, H, W), d_choice.cpu().numpy(),
               d_stats.cpu().numpy().view(np.int32).reshape(P, 4))
        same(got, want, ("composed", kind, Cn))


def test_refusals():
    """every refusal, and the outputs afterwards: not a byte written"""
    import opengpc_amd as g
    import torch
    W, H = 96, 64
    E, U = g.capi.E_INVALID, g.capi.E_UNSUPPORTED
    c = g.Context(0)
    try:
        L = c.L
        d_f, d_l, d_r = filled(2, 2, H, W, 4), filled(2, H, W), filled(2, H, W)
        d_out, d_cost, d_choice, d_stats = filled(2, 2, H, W, 4), filled(2, H, W, 2), filled(2, H, W), filled(2, 16, 4, 4)
        good = g.Propagate()
        torch.cuda.synchronize()

        def fields(fn=L.gpc_hip_propagate_fields_device, field=d_f.data_ptr(), l=d_l.data_ptr(), r=d_r.data_ptr(), ch=2, w=W, h=H, npairs=2,
                   prm=good, out=d_out.data_ptr()):
            return fn(c.h, field, l, r, ch, w, h, npairs, C.byref(prm) if prm is not None else None, out, d_cost.data_ptr(),
                      d_choice.data_ptr(), d_stats.data_ptr())

        for bad in (g.Propagate(0), g.Propagate(5), g.Propagate(2, 0), g.Propagate(2, 65), g.Propagate(2, 4, 0), g.Propagate(2, 4, 17),
                    g.Propagate(2, 4, 3, 0), g.Propagate(2, 4, 3, 5), g.Propagate(2, 4, 3, 9), g.Propagate(2, -4), g.Propagate(2, 4, -1),
                    g.Propagate(-2)):
            assert fields(prm=bad) == E, (bad.radius, bad.span, bad.iterations, bad.neighbours)
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
        host = lambda prm=good, l=hl.ctypes.data, npairs=2, out=ho.ctypes.data, w=W: L.gpc_hip_propagate_fields(
            c.h, hf.ctypes.data, l, hr.ctypes.data, 1, w, H, npairs, C.byref(prm), out, None, None, None)
        assert host(prm=g.Propagate(0)) == E and host(prm=g.Propagate(2, 4, 3, 6)) == E and host(l=None) == E and host(npairs=0) == E
        assert host(out=None) == E and host(out=hf.ctypes.data + 4) == E and host(out=hl.ctypes.data) == E
        assert host(npairs=65536) == U and host(w=40000) == U
        assert (ho == FILL).all()
    finally:
        c.close()
