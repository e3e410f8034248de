"""The scanline hole closing on the GPU (gpc_hip_gapfill_*): every byte of out, how and stats EQUALS the restatement of the
rule (tests/gapfill_util.py) -- every output starts out filled with a sentinel, and every element must be written -- at widths
below, at and across the 64-pixel chunk of the row scan, heights below and across a band of the column scan (64 rows, and 100
with max_gap = 100), one and three pairs, both channel counts, on the three random kinds and the crafted situations of
gapfill_util; single cases for the optional outputs, out == field, a workspace that grows, the host form across its chunks of
16 pairs, the refusals, and the composition with the real cleaner's output."""
import ctypes as C

import numpy as np
import pytest

import gapfill_util as gu

pytestmark = pytest.mark.gpu

FILL = 0xA5
NAMES = ("out", "how", "stats")


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def G_(prm):
    import opengpc_amd as g
    return g.Gapfill(*prm)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))       # (a copy: the shared cases are read-only)


def filled(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def gapfill_device(ctx, d_field, d_guide, shape, prm, with_how=True, with_stats=True, in_place=False):
    """the device form over arrays already on the device: the outputs read back from sentinel-filled arrays"""
    import torch
    P, Cn, H, W = shape
    d_out = d_field if in_place else filled(P, Cn, H, W, 4)
    d_how, d_stats = filled(P, H, W), filled(P, 4, 4)
    torch.cuda.synchronize()
    ctx.gapfill_fields_device(d_field.data_ptr(), d_guide.data_ptr() if d_guide is not None else 0, Cn, W, H, P, G_(prm), d_out.data_ptr(),
                              d_how.data_ptr() if with_how else 0, d_stats.data_ptr() if with_stats else 0)
    ctx.synchronize()
    return (d_out.cpu().numpy().view(np.int32).reshape(P, Cn, H, W), d_how.cpu().numpy().reshape(P, H, W),
            d_stats.cpu().numpy().view(np.int32).reshape(P, 4))


def same(got, want, what, names=NAMES):
    for n, g_, w in zip(names, got, want):
        assert g_.dtype == w.dtype and g_.shape == w.shape, (what, n)
        if not np.array_equal(g_, w):
            bad = np.argwhere(g_ != w)
            raise AssertionError("%s: %s differs at %d of %d elements, the first at %s: %s, expected %s" % (
                what, n, len(bad), w.size, bad[0].tolist(), g_[tuple(bad[0])], w[tuple(bad[0])]))


def check(ctx, field, guide, prm, what, **kw):
    got = gapfill_device(ctx, dev(field), dev(guide) if guide is not None else None, field.shape, prm, **kw)
    same(got, gu.gapfill(field, guide, prm), what)
    return got


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("Cn", [1, 2])
def test_every_byte_equals_the_rule(ctx, Cn, P):
    for kind, W, H in gu.sweep():
        field, guide = gu.case(kind, W, H, P, Cn)
        d_f, d_g = dev(field), dev(guide)
        for prm in gu.PRMS:
            same(gapfill_device(ctx, d_f, d_g, field.shape, prm), gu.gapfill(field, guide, prm), (kind, W, H, P, Cn, prm))
        assert np.array_equal(d_f.cpu().numpy(), field) and np.array_equal(d_g.cpu().numpy(), guide)   # the inputs are as they were


def test_crafted_situations(ctx):
    for name, field, guide, prm in gu.crafted():
        check(ctx, field, guide, prm, name)
        check(ctx, field, guide, prm, name + ", in place", in_place=True)
        if prm[2] == 0:
            check(ctx, field, None, prm, name + ", no guide")


@pytest.mark.parametrize("Cn", [1, 2])
def test_documented_defaults(ctx, Cn):
    import opengpc_amd as g
    d = g.Gapfill()
    assert (d.max_gap, d.discon_q8, d.select, d.border) == gu.DEFAULTS
    for kind in gu.KINDS:
        field, guide = gu.case(kind, 130, 67, 3, Cn)
        got = check(ctx, field, guide, gu.DEFAULTS, ("defaults", kind, Cn))
        assert (got[2][:, :3].sum(1) > 0).all()                                 # every pair closed holes


@pytest.mark.parametrize("Cn", [1, 2])
def test_optional_outputs_and_in_place(ctx, Cn):
    W, H, P = 130, 67, 3
    field, guide = gu.case("runs", W, H, P, Cn)
    for prm in ((8, 255, 1, 0), (100, 256, 0, 1)):
        want = gu.gapfill(field, guide, prm)
        d_f, d_g = dev(field), dev(guide)
        for k in range(2):                                                      # each optional output left out: the other unchanged, it untouched
            flags = [True] * 2
            flags[k] = False
            got = gapfill_device(ctx, d_f, d_g, field.shape, prm, *flags)
            same([g_ for i, g_ in enumerate(got) if i != k + 1], [w for i, w in enumerate(want) if i != k + 1], ("without", NAMES[k + 1]),
                 [n for i, n in enumerate(NAMES) if i != k + 1])
            assert (got[k + 1].view(np.uint8) == FILL).all()
        got = gapfill_device(ctx, d_f, d_g, field.shape, prm, False, False)
        assert np.array_equal(got[0], want[0]) and all((g_.view(np.uint8) == FILL).all() for g_ in got[1:])
        assert np.array_equal(d_f.cpu().numpy(), field)
        same(gapfill_device(ctx, d_f, d_g, field.shape, prm, in_place=True), want, ("out == field", prm))
        assert np.array_equal(d_g.cpu().numpy(), guide)


def test_nothing_outside_an_output_is_written(ctx):
    """the outputs in the middle of sentinel-filled blocks: the bytes before and behind them stay"""
    import torch
    W, H, P, Cn = 65, 9, 3, 2
    field, guide = gu.case("random", W, H, P, Cn)
    prm = (8, 255, 1, 1)
    want = gu.gapfill(field, guide, prm)
    pad = 256
    sizes = (P * Cn * H * W * 4, P * H * W, P * 16)
    blocks = [filled(pad + s + pad) for s in sizes]
    d_f, d_g = dev(field), dev(guide)
    torch.cuda.synchronize()
    ctx.gapfill_fields_device(d_f.data_ptr(), d_g.data_ptr(), Cn, W, H, P, G_(prm), *[b.data_ptr() + pad for b in blocks])
    ctx.synchronize()
    for b, s, w in zip(blocks, sizes, want):
        raw = b.cpu().numpy()
        assert (raw[:pad] == FILL).all() and (raw[pad + s:] == FILL).all()
        assert np.array_equal(raw[pad:pad + s].view(w.dtype).reshape(w.shape), w)


def test_the_workspace_grows():
    """a second call with a larger shape on the same context, then the small one again"""
    import opengpc_amd as g
    c = g.Context(0)
    try:
        for W, H, P in ((7, 5, 1), (130, 67, 3), (7, 5, 1)):
            field, guide = gu.case("random", W, H, P, 2)
            check(c, field, guide, (8, 255, 1, 1), ("grow", W, H, P))
            check(c, field, guide, (8, 255, 1, 1), ("grow, in place", W, H, P), in_place=True)
    finally:
        c.close()


def test_host_form(ctx):
    """gpc_hip_gapfill_fields: 17 pairs go up in chunks of 16 and 1; what comes back equals the device form"""
    P = 17
    for W, H in ((1, 1), (65, 9)):
        for Cn in (1, 2):
            field, guide = gu.case("random", W, H, P, Cn)
            for prm in ((8, 255, 1, 1), (3, 256, 0, 1)):
                want = gapfill_device(ctx, dev(field), dev(guide), field.shape, prm)
                same(ctx.gapfill_fields(field, guide, G_(prm)), want, ("host", W, H, Cn, prm))
                same(want, gu.gapfill(field, guide, prm), ("host: the device form", W, H, Cn, prm))
            same(ctx.gapfill_fields(field, None, G_((3, 256, 0, 1))), want, ("host, no guide", W, H, Cn))
            out, how, stats = ctx.gapfill_fields(field, guide, G_((3, 256, 0, 1)), want_how=False, want_stats=False)
            assert np.array_equal(out, want[0]) and how is None and stats is None


@pytest.mark.parametrize("Cn", [1, 2])
def test_composed_with_the_cleaner(ctx, Cn):
    """the real cleaner's output of the dense chain at 96 x 64, guided by the chain's left image"""
    import dense_chain_util as dc
    res, sc = dc.chain_cpu(Cn, 96, 64), dc.scene(Cn, 96, 64, dc.SEEDS[(Cn, 96, 64)])
    field, guide = res["clean_out"], sc["imgL"]
    assert (field[:, 0] == gu.NONE).any() and (field[:, 0] != gu.NONE).any()
    for prm in (gu.DEFAULTS, (8, 256, 1, 0)):
        got = check(ctx, field, guide, prm, ("cleaner", Cn, prm))
        assert (got[2][:, :2].sum(1) > 0).all()


def test_refusals():
    """every refusal, and the outputs afterwards: not a byte written"""
    import opengpc_amd as g
    import torch
    W, H = 96, 64
    E, U = g.capi.E_INVALID, g.capi.E_UNSUPPORTED
    c = g.Context(0)
    try:
        L = c.L
        d_f, d_g = filled(2, 2, H, W, 4), filled(2, H, W)
        d_out, d_how, d_stats = filled(2, 2, H, W, 4), filled(2, H, W), filled(2, 4, 4)
        good = g.Gapfill()
        torch.cuda.synchronize()

        def fields(fn=L.gpc_hip_gapfill_fields_device, field=d_f.data_ptr(), guide=d_g.data_ptr(), ch=2, w=W, h=H, npairs=2, prm=good,
                   out=d_out.data_ptr()):
            return fn(c.h, field, guide, ch, w, h, npairs, C.byref(prm) if prm is not None else None, out, d_how.data_ptr(), d_stats.data_ptr())

        for bad in (g.Gapfill(0), g.Gapfill(32768), g.Gapfill(-1), g.Gapfill(16, -1), g.Gapfill(16, (1 << 24) + 1), g.Gapfill(16, 256, 2),
                    g.Gapfill(16, 256, -1), g.Gapfill(16, 256, 0, 2), g.Gapfill(16, 256, 0, -1)):
            assert fields(prm=bad) == E, (bad.max_gap, bad.discon_q8, bad.select, bad.border)
        assert fields(prm=None) == E and fields(field=None) == E and fields(out=None) == E
        assert fields(guide=None, prm=g.Gapfill(16, 256, 1, 1)) == E                                      # select = 1 without a guide
        assert fields(ch=0) == E and fields(ch=3) == E and fields(npairs=0) == E and fields(w=0) == E and fields(h=-1) == E
        assert fields(out=d_f.data_ptr() + 4 * W * H) == E and fields(out=d_f.data_ptr() - 16) == E      # any overlap but the field itself
        assert fields(out=d_g.data_ptr(), ch=1, npairs=1, w=8, h=8) == E                                  # out over the guide
        assert fields(out=d_g.data_ptr() + 2 * W * H - 4, ch=1) == E
        assert fields(w=32769, h=1, npairs=1) == U and fields(w=1, h=32769, npairs=1) == U and fields(w=32768, h=32769, npairs=1) == U
        assert fields(npairs=65536, w=1, h=1) == U
        c.synchronize()
        for d in (d_out, d_how, d_stats, d_f, d_g):
            assert bool((d == FILL).all())
        # the host form: the same checks on host arrays
        hf, hg = np.zeros((2, 1, H, W), np.int32), np.zeros((2, H, W), np.uint8)
        ho = np.full((2, 1, H, W, 4), FILL, np.uint8)
        host = lambda prm=good, guide=hg.ctypes.data, npairs=2, out=ho.ctypes.data, w=W: L.gpc_hip_gapfill_fields(
            c.h, hf.ctypes.data, guide, 1, w, H, npairs, C.byref(prm), out, None, None)
        assert host(prm=g.Gapfill(0)) == E and host(prm=g.Gapfill(16, 256, 1, 1), guide=None) == E and host(npairs=0) == E
        assert host(out=None) == E and host(out=hf.ctypes.data + 4) == E and host(out=hg.ctypes.data) == E
        assert host(npairs=65536) == U and host(w=40000) == U
        assert (ho == FILL).all()
    finally:
        c.close()
