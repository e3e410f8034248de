"""Completing cleaned dense fields on the GPU (gpc_hip_inpaint_*): every byte of out, pass and stats EQUALS the restatement
of the rule (tests/inpaint_util.py) -- every output starts out filled with a sentinel, and every element must be written --
for random fields at sizes below, at and across a 32-pixel tile, both channel counts, radii 1, 3 and 8, guided and unguided,
few and many holes, three kinds of guide; single cases for what a pass may read, the rounding, the threshold, the extremes
of int32, stopping, aliasing and the optional outputs; the host form equals the device form; the match forms equal the chain
of the calls they are made of; the refusals; the timing slots."""
import ctypes as C

import numpy as np
import pytest

import inpaint_util as iu
import track_util as tu

pytestmark = pytest.mark.gpu

FILL = 0xA5
N = iu.NONE
NAMES = ("out", "pass", "stats")


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def I_(prm):
    import opengpc_amd as g
    return g.Inpaint(*prm)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def filled(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def read(d_out, d_pass, d_stats, P, Cn, H, W):
    return (d_out.cpu().numpy().view(np.int32).reshape(P, Cn, H, W), d_pass.cpu().numpy().reshape(P, H, W),
            d_stats.cpu().numpy().view(np.int32).reshape(P, 2))


def inpaint_device(ctx, field, guide, prm, with_pass=True, with_stats=True, in_place=False):
    """the device form over a host field [P, C, H, W] and guide [P, H, W]: the outputs read back from sentinel-filled arrays"""
    import torch
    P, Cn, H, W = field.shape
    d_field, d_guide = dev(field), dev(guide)
    d_out = d_field if in_place else filled(P, Cn, H, W, 4)
    d_pass, d_stats = filled(P, H, W), filled(P, 2, 4)
    torch.cuda.synchronize()
    ctx.inpaint_fields_device(d_field.data_ptr(), d_guide.data_ptr(), Cn, W, H, P, I_(prm), d_out.data_ptr(),
                              d_pass.data_ptr() if with_pass else 0, d_stats.data_ptr() if with_stats else 0)
    ctx.synchronize()
    assert np.array_equal(d_guide.cpu().numpy(), guide) and (in_place or np.array_equal(d_field.cpu().numpy(), field))
    return read(d_out, d_pass, d_stats, P, Cn, H, W)


def same(got, want, what, names=NAMES):
    for k, name in enumerate(NAMES):
        if name in names and not np.array_equal(got[k], want[k]):
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError((what, name, len(bad), bad[:4].tolist(), [got[k][tuple(b)] for b in bad[:4]],
                                  [want[k][tuple(b)] for b in bad[:4]]))


def check(ctx, field, guide, prm, what=None):
    field, guide = np.ascontiguousarray(field, np.int32), np.ascontiguousarray(guide, np.uint8)
    want = iu.inpaint(field, guide, prm)
    same(inpaint_device(ctx, field, guide, prm), want, (what, field.shape, prm))
    return want


def one(rows, Cn=1):
    """a field [1, Cn, H, W] from nested rows [H][W]; channel 1, where there is one, holds the value + 1000 (none stays none)"""
    f = np.array(rows, np.int64)[None, None]
    if Cn == 2:
        f = np.concatenate([f, np.where(f == N, N, f + 1000)], 1)
    return f.astype(np.int32)


@pytest.mark.parametrize("holes", [0.1, 0.5, 0.95])
@pytest.mark.parametrize("Cn", [1, 2])
@pytest.mark.parametrize("W,H,P", iu.SIZES)
def test_random_fields_every_parameter(ctx, W, H, P, Cn, holes):
    """a random guide at radius 1, 3, 8 x range_shift 0, 3, 8; a constant and a step-edge guide at three of those nine; four
    passes, so that pixels filled in one pass feed the next; min_weight at two neighbours' full weight"""
    field = iu.random_fields(W, H, Cn, P, holes)
    for kind, combos in (("random", [(r, shift) for r in (1, 3, 8) for shift in (0, 3, 8)]), ("constant", [(1, 3), (3, 0), (8, 3)]),
                         ("step", [(1, 0), (3, 3), (8, 3)])):
        guide = iu.guides(kind, W, H, P)
        for r, shift in combos:
            out, pz, stats = check(ctx, field, guide, (r, shift, 512, 4), kind)
            assert (stats.sum(1) == (field[:, 0] == N).sum((1, 2))).all()


@pytest.mark.parametrize("Cn", [1, 2])
def test_documented_defaults(ctx, Cn):
    field = iu.random_fields(70, 45, Cn, 3, 0.95, seed=3)
    out, pz, stats = check(ctx, field, iu.guides("random", 70, 45, 3, seed=3), iu.DEFAULTS, "defaults")
    assert pz.max() > 1 and (stats[:, 0] > 0).all()


def test_no_leak_between_pairs(ctx):
    """pair 1 has no value anywhere: it stays all holes, whatever pairs 0 and 2 hold around it in memory"""
    W, H = 70, 45
    field = iu.random_fields(W, H, 2, 3, 0.0, seed=9)
    field[1] = N
    out, pz, stats = check(ctx, field, iu.guides("random", W, H, 3), iu.DEFAULTS, "pairs")
    assert (out[1] == N).all() and (pz[1] == 255).all() and stats.tolist() == [[0, 0], [0, W * H], [0, 0]]
    assert np.array_equal(out[0], field[0]) and np.array_equal(out[2], field[2])


@pytest.mark.parametrize("Cn", [1, 2])
def test_passes_read_the_previous_pass_only(ctx, Cn):
    """a strip valued at one pixel, r = 1, three passes, min_weight 1: exactly three pixels follow it, one per pass -- along x,
    along y, and across a tile edge (the valued pixel at x = 30 of 70, and at y = 30 of 70)"""
    prm = (1, 8, 1, 3)
    strip = [9] + [N] * 39
    out, pz, stats = check(ctx, one([strip], Cn), np.zeros((1, 1, 40)), prm, "strip x")
    assert pz[0, 0].tolist() == [0, 1, 2, 3] + [255] * 36 and out[0, 0, 0].tolist() == [9] * 4 + [N] * 36 and stats.tolist() == [[3, 36]]
    out, pz, stats = check(ctx, one([[v] for v in strip], Cn), np.zeros((1, 40, 1)), prm, "strip y")
    assert pz[0, :, 0].tolist() == [0, 1, 2, 3] + [255] * 36 and out[0, 0, :, 0].tolist() == [9] * 4 + [N] * 36
    edge = [N] * 70
    edge[30] = 9
    want = [255] * 27 + [3, 2, 1, 0, 1, 2, 3] + [255] * 36
    out, pz, stats = check(ctx, one([edge], Cn), np.zeros((1, 1, 70)), prm, "tile edge x")
    assert pz[0, 0].tolist() == want and stats.tolist() == [[6, 63]]
    out, pz, stats = check(ctx, one([[v] for v in edge], Cn), np.zeros((1, 70, 1)), prm, "tile edge y")
    assert pz[0, :, 0].tolist() == want
    # two dimensions: a valued pixel in the corner of four tiles grows a square per pass
    f = np.full((64, 64), N, np.int64)
    f[31, 31] = -7
    out, pz, stats = check(ctx, one(f, Cn), np.zeros((1, 64, 64)), prm, "corner of four tiles")
    ys, xs = np.mgrid[0:64, 0:64]
    ring = np.maximum(abs(ys - 31), abs(xs - 31))
    assert np.array_equal(pz[0], np.where(ring <= 3, ring, 255))


def test_rounding(ctx):
    g = np.zeros((1, 1, 3))
    assert check(ctx, one([[-1, N, -2]]), g, (1, 8, 1, 1))[0][0, 0, 0].tolist() == [-1, -2, -2]
    assert check(ctx, one([[1, N, 2]]), g, (1, 8, 1, 1))[0][0, 0, 0].tolist() == [1, 2, 2]
    g = np.zeros((1, 2, 3))
    assert check(ctx, one([[1, 2, 5], [N, N, N]]), g, (1, 8, 1, 1))[0][0, 0, 1].tolist() == [2, 3, 4]
    assert check(ctx, one([[-1, -2, -4], [N, N, N]]), g, (1, 8, 1, 1))[0][0, 0, 1].tolist() == [-2, -2, -3]
    # guided: the weights 256 and 1 of test_inpaint.py's case
    out, _, _ = check(ctx, one([[0, 0, N, 1000, 1000]]), np.array([[[0, 0, 200, 200, 200]]]), (2, 0, 1, 1))
    assert out[0, 0, 0, 2] == 996


@pytest.mark.parametrize("n", [1, 3, 8])
def test_threshold_is_inclusive(ctx, n):
    """a constant guide, so every neighbour weighs 256: n valued neighbours fill the hole at min_weight 256 n, not at 256 n + 1"""
    f = np.full((5, 5), N, np.int64)
    for k in [k for k in range(9) if k != 4][:n]:
        f[k // 3, k % 3] = 10 + k
    g = np.full((1, 5, 5), 200)
    _, pz, _ = check(ctx, one(f), g, (1, 3, 256 * n, 1))
    assert pz[0, 1, 1] == 1
    _, pz, _ = check(ctx, one(f), g, (1, 3, 256 * n + 1, 1))
    assert pz[0, 1, 1] == 255


@pytest.mark.parametrize("Cn", [1, 2])
def test_extremes(ctx, Cn):
    """every neighbour INT32_MAX, then every neighbour INT32_MIN + 1, r = 8, unguided: 288 x 256 x the value in the sum, and
    the value itself comes back; mixed extremes against the model; a hole whose channel 1 holds a value"""
    for v in (iu.IMAX, iu.IMIN1):
        f = np.full((1, Cn, 40, 40), v, np.int32)
        f[:, :, 20, 20] = N
        f[:, :, 8, 33] = N                                                  # (across a tile edge)
        out, pz, stats = check(ctx, f, np.zeros((1, 40, 40)), (8, 8, 1, 1), "extreme")
        assert (out == v).all() and stats.tolist() == [[2, 0]]
    rng = np.random.default_rng(12)
    f = rng.choice(np.array([iu.IMAX, iu.IMIN1, N, N, 0, -1], np.int64), (2, Cn, 37, 41)).astype(np.int32)
    if Cn == 2:
        f[:, 1][f[:, 1] == N] = iu.IMAX                                     # channel 1 of the holes holds values, of the valued both ends
        f[0, 1, 0, :8] = N                                                  # INT32_MIN is a value in channel 1
        f[0, 0, 0, :8] = 5
    for prm in ((8, 8, 1, 3), (8, 0, 300, 3), (2, 3, 1, 2)):
        out, pz, stats = check(ctx, f, iu.guides("random", 41, 37, 2), prm, "mixed extremes")
        assert (out[np.broadcast_to((pz == 255)[:, None], out.shape)] == N).all() and 0 < stats[:, 0].min()
    if Cn == 2:
        h = np.array([[[[N, 3]], [[44, 7]]]], np.int32)
        out, pz, stats = check(ctx, h, np.zeros((1, 1, 2)), (1, 8, 512, 5), "channel 1 of a hole")
        assert out.tolist() == [[[[N, 3]], [[N, 7]]]] and pz.tolist() == [[[255, 0]]] and stats.tolist() == [[0, 1]]


@pytest.mark.parametrize("Cn", [1, 2])
def test_stopping_is_not_observable(ctx, Cn):
    # complete after three passes: every hole within three pixels of a value (70 x 35, values every seventh pixel), r = 1
    W, H = 70, 35
    f = np.full((H, W), N, np.int64)
    f[3::7, 3::7] = np.arange(50).reshape(5, 10) * 37 - 900
    g = iu.guides("step", W, H, 1)
    a = check(ctx, one(f, Cn), g, (1, 3, 1, 3), "three passes")
    assert a[1].max() == 3 and a[2].tolist() == [[W * H - 50, 0]]
    same(check(ctx, one(f, Cn), g, (1, 3, 1, 254), "254 passes"), a, "254 passes equal 3")
    # islands that can never reach min_weight (pair 0: two lone values, each hole sees one at most), while in pair 1 a block
    # grows by two pixels a pass until nothing is left: the passes that pair 1 needs change nothing in pair 0
    W, H = 70, 45
    f = np.full((2, H, W), N, np.int64)
    f[0, 40, 60], f[0, 5, 5] = 5, 100
    f[1, :6, :6] = 100
    f = np.stack([one(f[0], Cn)[0], one(f[1], Cn)[0]])
    out, pz, stats = check(ctx, f, iu.guides("random", W, H, 2), (2, 8, 257, 254), "island")
    assert stats.tolist() == [[0, W * H - 2], [W * H - 36, 0]] and np.array_equal(out[0], f[0]) and pz[1].max() > 30
    # no hole at all; nothing but holes
    full = iu.random_fields(W, H, Cn, 2, 0.0)
    out, pz, stats = check(ctx, full, iu.guides("random", W, H, 2), iu.DEFAULTS, "no hole")
    assert np.array_equal(out, full) and (pz == 0).all() and stats.tolist() == [[0, 0]] * 2
    out, pz, stats = check(ctx, np.full((2, Cn, H, W), N, np.int32), iu.guides("random", W, H, 2), iu.DEFAULTS, "all holes")
    assert (out == N).all() and (pz == 255).all() and stats.tolist() == [[0, W * H]] * 2


@pytest.mark.parametrize("Cn", [1, 2])
def test_aliasing_and_optional_outputs(ctx, Cn):
    W, H, P = 70, 45, 3
    field, guide = iu.random_fields(W, H, Cn, P, 0.5, seed=21), iu.guides("random", W, H, P, seed=21)
    want = iu.inpaint(field, guide, iu.DEFAULTS)
    same(inpaint_device(ctx, field, guide, iu.DEFAULTS, in_place=True), want, "in place")
    for flags in ((False, True), (True, False), (False, False)):
        for in_place in (False, True):
            got = inpaint_device(ctx, field, guide, iu.DEFAULTS, *flags, in_place=in_place)
            same(got, want, (flags, in_place), [NAMES[0]] + [n for n, f in zip(NAMES[1:], flags) if f])
            for k, f in enumerate(flags):
                assert f or (got[k + 1].view(np.uint8) == FILL).all(), (flags, k)


def test_host_form(ctx):
    """17 pairs (two chunks: 16 and 1) of 7 x 5, and 3 pairs of 70 x 45: the host form, from pageable and from page-locked
    arrays, with and without the optional outputs, in place too, leaves the bytes the device form leaves"""
    for W, H, P in ((7, 5, 17), (70, 45, 3)):
        for Cn in (1, 2):
            field, guide = iu.random_fields(W, H, Cn, P, 0.5, seed=30), iu.guides("random", W, H, P, seed=30)
            for prm in (iu.DEFAULTS, (1, 0, 256, 2)):
                want = inpaint_device(ctx, field, guide, prm)
                same(want, iu.inpaint(field, guide, prm), ("device", Cn, prm))
                for what, alloc in (("pageable", np.empty), ("page-locked", ctx.pinned_empty)):
                    hf, hg = alloc(field.shape, field.dtype), alloc(guide.shape, guide.dtype)
                    hf[...], hg[...] = field, guide
                    same(ctx.inpaint_fields(hf, hg, I_(prm)), want, (what, Cn, prm))
                out, pz, stats = ctx.inpaint_fields(field, guide, I_(prm), False, False)
                assert pz is None and stats is None and np.array_equal(out, want[0])
                hf = field.copy()
                st = ctx.L.gpc_hip_inpaint_fields(ctx.h, hf.ctypes.data, guide.ctypes.data, Cn, W, H, P, C.byref(I_(prm)), hf.ctypes.data,
                                                  None, None)
                assert st == 0 and np.array_equal(hf, want[0])


def settings(epipolar):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epipolar, False, 1)


def match_forms(c, batch, images, W, H, P, Cn, s, radius, prm, ip, what):
    """inpaint_batch_device / inpaint_sequence_device against clean_*_device followed by inpaint_fields_device: every output"""
    import opengpc_amd as g
    import torch
    fill = g.Densify()
    nc_shape = (P, 2, 4) if batch else (P + 1, 4)

    def buffers():
        return dict(out=filled(P, Cn, H, W, 4), state=filled(P, H, W), label=filled(P, H, W, 4), stats=filled(P, 4, 4),
                    fwd=filled(P, Cn, H, W, 4), level=filled(P, H, W), cnt=filled(P, 4), nc=filled(*nc_shape))

    a, b = buffers(), buffers()
    a.update(done=filled(P, Cn, H, W, 4), pz=filled(P, H, W), fstats=filled(P, 2, 4))
    b.update(done=filled(P, Cn, H, W, 4), pz=filled(P, H, W), fstats=filled(P, 2, 4))
    p = lambda d, n: d[n].data_ptr()
    torch.cuda.synchronize()
    if batch:
        c.clean_batch_device(images[0], images[1], W, H, P, s, fill, prm, p(a, "out"), p(a, "state"), p(a, "label"), p(a, "stats"), p(a, "fwd"),
                             p(a, "level"), radius, p(a, "cnt"), p(a, "nc"))
        c.inpaint_fields_device(p(a, "out"), images[0], Cn, W, H, P, ip, p(a, "done"), p(a, "pz"), p(a, "fstats"))
        c.inpaint_batch_device(images[0], images[1], W, H, P, s, fill, prm, ip, p(b, "done"), p(b, "pz"), p(b, "fstats"), p(b, "out"),
                               p(b, "state"), p(b, "label"), p(b, "stats"), p(b, "fwd"), p(b, "level"), radius, p(b, "cnt"), p(b, "nc"))
    else:
        c.clean_sequence_device(images[0], W, H, P + 1, s, fill, prm, p(a, "out"), p(a, "state"), p(a, "label"), p(a, "stats"), p(a, "fwd"),
                                p(a, "level"), radius, p(a, "cnt"), p(a, "nc"))
        c.inpaint_fields_device(p(a, "out"), images[0], Cn, W, H, P, ip, p(a, "done"), p(a, "pz"), p(a, "fstats"))
        c.inpaint_sequence_device(images[0], W, H, P + 1, s, fill, prm, ip, p(b, "done"), p(b, "pz"), p(b, "fstats"), p(b, "out"),
                                  p(b, "state"), p(b, "label"), p(b, "stats"), p(b, "fwd"), p(b, "level"), radius, p(b, "cnt"), p(b, "nc"))
    c.synchronize()
    A, B = ({n: d.cpu().numpy() for n, d in x.items()} for x in (a, b))
    for n in A:
        assert np.array_equal(A[n], B[n]), (what, n)
        assert not (A[n] == FILL).all(), (what, n)
    cleaned = A["out"].view(np.int32).reshape(P, Cn, H, W)
    fstats = A["fstats"].view(np.int32).reshape(P, 2)
    print("holes of the cleaned field", what, (cleaned[:, 0] == N).sum((1, 2)).tolist(), "fill stats", fstats.tolist())
    assert ((cleaned[:, 0] == N).sum((1, 2)) > 0).all() and (fstats[:, 0] > 0).all(), (what, fstats.tolist())
    # the optional outputs left out: the cleaner writes d_out, the completion runs in place
    d_only = filled(P, Cn, H, W, 4)
    torch.cuda.synchronize()
    if batch:
        c.inpaint_batch_device(images[0], images[1], W, H, P, s, fill, prm, ip, d_only.data_ptr(), refine_radius=radius)
    else:
        c.inpaint_sequence_device(images[0], W, H, P + 1, s, fill, prm, ip, d_only.data_ptr(), refine_radius=radius)
    c.synchronize()
    assert np.array_equal(d_only.cpu().numpy(), A["done"]), what
    return A


@pytest.mark.parametrize("lanes", [1, 2])
def test_match_fill_clean_and_complete_batch(oracle, forest_paths, lanes):
    """the synthetic pairs of tests/test_gpu_dense.py (96 x 64, D = 5), the zero forest, the documented defaults of every
    stage: the cleaned field has holes (the columns whose target lies left of the image fail the check) and they are filled"""
    import opengpc_amd as g
    W, H, B, D = 96, 64, 2, 5
    c = g.Context(0)
    try:
        c.load_forest(forest_paths["zero"], W, H)
        c.set_pipeline(lanes)
        pairs = [oracle.synth_pair(W, H, i, D) for i in range(B)]
        d_L, d_R = (dev(np.stack([q[k] for q in pairs])) for k in (0, 1))
        for radius in (0, 3):
            match_forms(c, True, (d_L.data_ptr(), d_R.data_ptr()), W, H, B, 1, settings(True), radius, g.Clean(), g.Inpaint(),
                        ("batch", lanes, radius))
    finally:
        c.close()


def test_match_fill_clean_and_complete_sequence(ctx, forest_paths):
    """three frames of 96 x 64 (the sequence of tests/test_gpu_clean.py), the documented defaults: guided by frame t"""
    import opengpc_amd as g
    W, H, F = 96, 64, 3
    d_f = dev(tu.frames_of(W, H, F, 1, 0))
    ctx.load_forest(forest_paths["zero"], W, H)
    for radius in (0, 3):
        match_forms(ctx, False, (d_f.data_ptr(),), W, H, F - 1, 2, settings(True), radius, g.Clean(), g.Inpaint(), ("sequence", radius))


def test_refusals(forest_paths):
    """every refusal of the group, and the outputs afterwards: not a byte written"""
    import opengpc_amd as g
    import torch
    W, H = 96, 64
    E, U = g.capi.E_INVALID, g.capi.E_UNSUPPORTED
    c = g.Context(0)
    try:
        L = c.L
        d_f, d_g = filled(2, 2, H, W, 4), filled(2, H, W)
        d_out, d_pass, d_stats = filled(2, 2, H, W, 4), filled(2, H, W), filled(2, 2, 4)
        good = g.Inpaint()
        torch.cuda.synchronize()

        def fields(fn=L.gpc_hip_inpaint_fields_device, field=d_f.data_ptr(), guide=d_g.data_ptr(), ch=2, w=W, h=H, npairs=2, prm=good,
                   out=d_out.data_ptr()):
            return fn(c.h, field, guide, ch, w, h, npairs, C.byref(prm) if prm is not None else None, out, d_pass.data_ptr(),
                      d_stats.data_ptr())

        for bad in (g.Inpaint(0), g.Inpaint(9), g.Inpaint(4, -1), g.Inpaint(4, 9), g.Inpaint(4, 3, 0), g.Inpaint(4, 3, (1 << 24) + 1),
                    g.Inpaint(4, 3, 512, 0), g.Inpaint(4, 3, 512, 255)):
            assert fields(prm=bad) == E, (bad.radius, bad.range_shift, bad.min_weight, bad.passes)
        assert fields(prm=None) == E and fields(field=None) == E and fields(out=None) == E and fields(guide=None) == E
        assert fields(ch=0) == E and fields(ch=3) == E and fields(npairs=0) == E and fields(w=0) == E and fields(h=-1) == E
        assert fields(out=d_f.data_ptr() + 4 * W * H) == E and fields(out=d_f.data_ptr() - 16) == E      # any overlap but the field itself
        assert fields(w=32769, h=1, npairs=1) == U and fields(w=1, h=32769, npairs=1) == U and fields(w=32768, h=32769, npairs=1) == U
        assert fields(npairs=65536, w=1, h=1) == U
        c.synchronize()
        for d in (d_out, d_pass, d_stats, d_f, d_g):
            assert bool((d == FILL).all())
        # the host form: the same checks on host arrays
        hf, hg = np.zeros((2, 1, H, W), np.int32), np.zeros((2, H, W), np.uint8)
        ho = np.full((2, 1, H, W, 4), FILL, np.uint8)
        host = lambda prm=good, guide=hg.ctypes.data, npairs=2, out=ho.ctypes.data, w=W: L.gpc_hip_inpaint_fields(
            c.h, hf.ctypes.data, guide, 1, w, H, npairs, C.byref(prm), out, None, None)
        assert host(prm=g.Inpaint(0)) == E and host(guide=None) == E and host(npairs=0) == E and host(out=None) == E
        assert host(out=hf.ctypes.data + 4) == E and host(npairs=65536) == U and host(w=40000) == U
        assert (ho == FILL).all()
        # the match forms: their own refusals and those of the calls they wrap
        s, fill, cl = settings(True), g.Densify(), g.Clean()
        d_fr = dev(tu.frames_of(W, H, 3, 1))
        iL, iR = d_fr.data_ptr(), d_fr.data_ptr() + W * H
        d_cl = filled(2, 2, H, W, 4)
        seq = lambda nframes=3, radius=0, fl=fill, prm=cl, ip=good, out=d_out.data_ptr(), w=W, fwd=None, cleaned=None: \
            L.gpc_hip_inpaint_sequence_device(c.h, iL, w, H, nframes, C.byref(s), radius, C.byref(fl), C.byref(prm),
                                              C.byref(ip) if ip is not None else None, out, None, None, cleaned, None, None, None, fwd, None,
                                              None, None)
        bat = lambda npairs=2, radius=0, fl=fill, prm=cl, ip=good, out=d_out.data_ptr(), w=W, fwd=None, cleaned=None: \
            L.gpc_hip_inpaint_batch_device(c.h, iL, iR, w, H, npairs, C.byref(s), radius, C.byref(fl), C.byref(prm),
                                           C.byref(ip) if ip is not None else None, out, None, None, cleaned, None, None, None, fwd, None,
                                           None, None)
        assert seq() == g.capi.E_NO_FOREST and bat() == g.capi.E_NO_FOREST
        c.load_forest(forest_paths["zero"], W, H)
        for call in (seq, bat):
            assert call(radius=-1) == E and call(radius=7) == E and call(out=None) == E and call(w=W + 1) == E
            assert call(fl=g.Densify(15, 1, 3)) == E and call(prm=g.Clean(256, 256, 64, 3)) == E
            assert call(ip=None) == E and call(ip=g.Inpaint(9)) == E and call(ip=g.Inpaint(4, 3, 512, 255)) == E
            assert call(fwd=d_out.data_ptr()) == E and call(cleaned=d_out.data_ptr() + 8) == E
            assert call(cleaned=d_cl.data_ptr(), fwd=d_cl.data_ptr()) == E and call(cleaned=d_cl.data_ptr(), fwd=d_out.data_ptr()) == E
        assert seq(nframes=1) == E and bat(npairs=0) == E
        c.synchronize()
        for d in (d_out, d_cl):
            assert bool((d == FILL).all())
    finally:
        c.close()


def test_kernel_times_are_reported(ctx):
    """the two timing slots between k_tf_commit and k_quad_sides take time when timing is on: one begin, one launch per pass"""
    field, guide = iu.random_fields(70, 45, 1, 3, 0.5), iu.guides("random", 70, 45, 3)
    names = [ctx.L.gpc_hip_kernel_name(i).decode() for i in range(ctx.L.gpc_hip_kernel_slots())]
    ctx.L.gpc_hip_enable_kernel_timing(ctx.h, 1)
    ctx.L.gpc_hip_reset_kernel_timing(ctx.h)
    try:
        inpaint_device(ctx, field, guide, (4, 3, 512, 5))
        for k, launches in (("k_inpaint_begin", 1), ("k_inpaint_pass", 5)):
            ms, n = C.c_float(0), C.c_int(0)
            assert ctx.L.gpc_hip_kernel_time(ctx.h, names.index(k), C.byref(ms), C.byref(n)) == 0
            assert n.value == launches >= 1 and ms.value > 0, (k, ms.value, n.value)
            assert ctx.L.gpc_hip_kernel_launch_name(ctx.h, names.index(k)).decode().startswith("gpc::" + k)
    finally:
        ctx.L.gpc_hip_enable_kernel_timing(ctx.h, 0)
