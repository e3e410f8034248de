"""Cleaning dense fields on the GPU (gpc_hip_clean_*): every byte of out, state, label and stats EQUALS the restatement of
the rule (tests/clean_util.py) -- every output starts out filled with a sentinel, and every element must be written -- for
random fields at sizes below, across and well above a 32-pixel tile, both channel counts, every parameter; constructed
fields that label wrongly when the union across tiles is wrong; the reversed records; the match-fill-and-clean forms equal
the chain of the calls they are made of; the host form equals the device form; the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import clean_util as cu
import dense_util as du
import track_util as tu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
NAMES = ("out", "state", "label", "stats")


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def K_(prm):
    import opengpc_amd as g
    return g.Clean(*prm)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def filled(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def read(d_out, d_state, d_label, d_stats, P, Cn, H, W):
    return (d_out.cpu().numpy().view(np.int32).reshape(P, Cn, H, W), d_state.cpu().numpy().reshape(P, H, W),
            d_label.cpu().numpy().view(np.int32).reshape(P, H, W), d_stats.cpu().numpy().view(np.int32).reshape(P, 4))


def clean_device(ctx, fwd, bwd, prm, with_state=True, with_label=True, with_stats=True):
    """the device form over host fields [P, C, H, W]: the four outputs read back from sentinel-filled arrays"""
    import torch
    P, Cn, H, W = fwd.shape
    d_fwd, d_bwd = dev(fwd), (dev(bwd) if bwd is not None else None)
    d_out, d_state, d_label, d_stats = filled(P, Cn, H, W, 4), filled(P, H, W), filled(P, H, W, 4), filled(P, 4, 4)
    torch.cuda.synchronize()
    ctx.clean_fields_device(d_fwd.data_ptr(), Cn, W, H, P, K_(prm), d_out.data_ptr(), d_bwd.data_ptr() if d_bwd is not None else 0,
                            d_state.data_ptr() if with_state else 0, d_label.data_ptr() if with_label else 0,
                            d_stats.data_ptr() if with_stats else 0)
    ctx.synchronize()
    assert np.array_equal(d_fwd.cpu().numpy(), fwd) and (bwd is None or np.array_equal(d_bwd.cpu().numpy(), bwd))
    return read(d_out, d_state, d_label, d_stats, P, Cn, H, W)


def same(got, want, what, names=NAMES):
    for k, name in enumerate(NAMES):
        if name in names and not np.array_equal(got[k], want[k]):
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError((what, name, len(bad), bad[:4].tolist(), [got[k][tuple(b)] for b in bad[:4]],
                                  [want[k][tuple(b)] for b in bad[:4]]))


def check(ctx, fwd, bwd, prm, what=None):
    want = cu.clean(fwd, bwd if prm[0] >= 0 else None, prm)
    same(clean_device(ctx, fwd, bwd if prm[0] >= 0 else None, prm), want, (what, fwd.shape, prm))
    return want


PARAMS = [cu.DEFAULTS, (-1, 256, 64, 1), (256, 256, 64, 0), (256, 256, 64, 2), (0, 100, 0, 1), (300, 0, 2, 2), (-1, 1 << 24, 1, 0),
          (1 << 24, 256, 5, 1)]


@pytest.mark.parametrize("Cn", [1, 2])
@pytest.mark.parametrize("W,H", cu.SIZES)
def test_random_fields_every_parameter(ctx, W, H, Cn):
    """three pairs (the middle one without a value anywhere): the check on and off, every median radius, speckle_min 0, 1, 2,
    5 and 64, tolerances and differences at their ends"""
    fwd, bwd = cu.random_fields(W, H, Cn)
    for prm in PARAMS:
        out, state, label, stats = check(ctx, fwd, bwd, prm, "random")
        assert stats[1].tolist() == [0, W * H, 0, 0] and (out[1] == cu.NONE).all() and (label[1] == -1).all()


@pytest.mark.parametrize("Cn", [1, 2])
def test_optional_outputs(ctx, Cn):
    """state, label and stats left out, one at a time and all together: the others do not change, what is left out is not
    touched; without label and with speckle_min <= 1 no labelling runs at all"""
    fwd, bwd = cu.random_fields(130, 67, Cn)
    for prm in (cu.DEFAULTS, (256, 256, 1, 1)):
        want = cu.clean(fwd, bwd, prm)
        for flags in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            got = clean_device(ctx, fwd, bwd, prm, *flags)
            same(got, want, (prm, flags), [NAMES[0]] + [n for n, f in zip(NAMES[1:], flags) if f])
            for k, f in enumerate(flags):
                assert f or (got[k + 1].view(np.uint8) == FILL).all(), (prm, flags, k)


@pytest.mark.parametrize("Cn", [1, 2])
def test_constructed_fields(ctx, Cn):
    """200 x 90 (7 x 3 tiles): one component over the whole plane, a checkerboard, a serpentine through every row, a spiral,
    a comb whose teeth meet in the last row, a U over two tile columns, two blocks that touch diagonally, two halves one unit
    further apart than speckle_diff_q8 (and exactly that far).  speckle_min at the largest component's size and one above."""
    W, H = 200, 90
    made = cu.constructed(W, H, 256)
    names = sorted(made)
    fwd = np.stack([np.stack([made[n][0]] + [np.where(made[n][0] == cu.NONE, 77, 3)] * (Cn - 1)) for n in names]).astype(np.int32)
    out, state, label, stats = check(ctx, fwd, None, (-1, 256, 0, 1), "constructed")
    for t, n in enumerate(names):
        roots, sizes = np.unique(label[t][label[t] >= 0], return_counts=True)
        assert len(roots) == made[n][1], (n, len(roots))
        assert roots[0] == np.flatnonzero(fwd[t, 0].ravel() != cu.NONE)[0]
    for n in ("whole", "serpentine", "spiral", "comb", "u", "diagonal", "step"):
        t = names.index(n)
        s = int(np.unique(label[t][label[t] >= 0], return_counts=True)[1].max())
        _, st_at, _, _ = check(ctx, fwd[t:t + 1], None, (-1, 256, s, 0), (n, "at its size"))
        _, st_over, _, _ = check(ctx, fwd[t:t + 1], None, (-1, 256, s + 1, 0), (n, "one above"))
        assert (st_at == 0).sum() >= s and (st_over == 0).sum() == 0 and (st_over == 3).sum() == (fwd[t, 0] != cu.NONE).sum()
    # the second channel alone splits a plane that the first one joins
    if Cn == 2:
        f = np.zeros((1, 2, H, W), np.int32)
        f[0, 1, :, 100:] = 257
        _, _, lab, _ = check(ctx, f, None, (-1, 256, 0, 0), "channel 1 splits")
        assert np.unique(lab).tolist() == [0, 100]


def test_large_plane_many_pairs(ctx):
    """1024 x 436, the size the timing tool runs at: a serpentine and a random field, labels through 32 x 14 tiles"""
    W, H = 1024, 436
    ys, xs = np.mgrid[0:H, 0:W]
    snake = (ys % 2 == 0) | ((ys % 4 == 1) & (xs == W - 1)) | ((ys % 4 == 3) & (xs == 0))
    fwd = np.stack([np.where(snake, 5, cu.NONE)[None], cu.random_fields(W, H, 1, 1, seed=5)[0][0]]).astype(np.int32)
    _, _, label, stats = check(ctx, fwd, None, (-1, 256, 64, 1), "large")
    assert np.unique(label[0]).tolist() == [-1, 0] and stats[0].tolist() == [int(snake.sum()), int((~snake).sum()), 0, 0]


def flip_device(ctx, rec, counts, ref=None, in_place=False):
    import torch
    P, cap = rec.shape
    corr = rec.dtype == du.CORR
    d_rec = dev(rec.view(np.uint8).reshape(P, cap, rec.dtype.itemsize))
    d_cnt = dev(np.asarray(counts, np.int32))
    d_ref = dev(ref.view(np.uint8).reshape(P, cap, 8)) if ref is not None else None
    d_out = d_rec if in_place else filled(P, cap, rec.dtype.itemsize)
    d_fout = (d_ref if in_place else filled(P, cap, 8)) if ref is not None else None
    torch.cuda.synchronize()
    ctx.flip_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), P, d_out.data_ptr(),
                            d_ref.data_ptr() if ref is not None else 0, d_fout.data_ptr() if ref is not None else 0)
    ctx.synchronize()
    out = d_out.cpu().numpy().reshape(P, -1).view(rec.dtype).reshape(P, cap)
    return out, (d_fout.cpu().numpy().reshape(P, -1).view(du.REFINEMENT).reshape(P, cap) if ref is not None else None)


@pytest.mark.parametrize("corr", [False, True])
def test_flip(ctx, corr):
    """the reversed records equal the restatement byte for byte (supports with a d that is no whole number, NaN, the
    infinities, 2^24 and 3e38 among them; counts negative, zero and above the slots; slots beyond the count untouched), with
    and without refinements, in place too; the reverse of the reverse is the input wherever the record was valid"""
    rng = np.random.default_rng(31 + corr)
    W, H, P, cap = 130, 67, 4, 700
    rec = np.stack([du.random_records(rng, W, H, 640, corr, cap, hole=False) for _ in range(P)])
    if not corr:
        rec["d"][:, 7] = 3e38
        rec["d"][:, 8] = -0.0
    ref = np.stack([du.random_refinements(rng, cap) for _ in range(P)])
    ref["dx_q8"][:, 3] = -32768
    counts = [640, -3, cap + 9, 0]
    blank = np.full((P, cap), FILL, np.uint8)
    pre = np.frombuffer(np.full(P * cap * rec.dtype.itemsize, FILL, np.uint8).tobytes(), rec.dtype).reshape(P, cap)
    pre_ref = np.frombuffer(np.full(P * cap * 8, FILL, np.uint8).tobytes(), du.REFINEMENT).reshape(P, cap)
    want, want_ref = cu.flip(rec, counts, ref, pre, pre_ref)
    got, got_ref = flip_device(ctx, rec, counts, ref)
    assert got.tobytes() == want.tobytes() and got_ref.tobytes() == want_ref.tobytes() and blank.shape == (P, cap)
    got, got_ref = flip_device(ctx, rec, counts)
    assert got.tobytes() == want.tobytes() and got_ref is None
    want_in, want_ref_in = cu.flip(rec, counts, ref, rec, ref)
    got, got_ref = flip_device(ctx, rec, counts, ref, in_place=True)
    assert got.tobytes() == want_in.tobytes() and got_ref.tobytes() == want_ref_in.tobytes()
    back, back_ref = flip_device(ctx, got, counts, got_ref)
    for t in (0, 2):
        m = du.valid(counts[t], cap)
        ok = np.ones(m, bool)
        if not corr:
            d = rec["d"][t, :m].astype(np.float64)
            with np.errstate(invalid="ignore"):
                ok = np.isfinite(d) & (d == np.trunc(d)) & (np.abs(d) < 2.0 ** 24)
            assert 0 < ok.sum() < m
        assert back[t, :m][ok].tobytes() == rec[t, :m][ok].tobytes()
        assert back_ref[t, :m].tobytes() == ref[t, :m].tobytes()


def test_host_form(ctx):
    """17 pairs (two chunks: 16 and 1) of 33 x 17: the host form, from pageable and from page-locked arrays, with and without
    bwd and the optional outputs, leaves the bytes the device form leaves"""
    W, H, P = 33, 17, 17
    for Cn in (1, 2):
        parts = [cu.random_fields(W, H, Cn, 3, seed=400 + 10 * k + Cn) for k in range(6)]
        fwd, bwd = (np.concatenate([p[k] for p in parts])[:P] for k in (0, 1))
        for prm in (cu.DEFAULTS, (-1, 100, 3, 2)):
            use_bwd = prm[0] >= 0
            want = clean_device(ctx, fwd, bwd if use_bwd else None, prm)
            same(want, cu.clean(fwd, bwd if use_bwd else None, prm), ("device", Cn, prm))
            for what, alloc in (("pageable", np.empty), ("page-locked", ctx.pinned_empty)):
                hf, hb = alloc(fwd.shape, fwd.dtype), alloc(bwd.shape, bwd.dtype)
                hf[...], hb[...] = fwd, bwd
                same(ctx.clean_fields(hf, hb if use_bwd else None, K_(prm)), want, (what, Cn, prm))
            out, state, label, stats = ctx.clean_fields(fwd, bwd if use_bwd else None, K_(prm), False, False, False)
            assert state is None and label is None and stats is None and np.array_equal(out, want[0])


def settings(epipolar):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epipolar, False, 1)


def chain(c, corr, d_rec, cap, d_cnt, d_ref, W, H, P, fill, prm):
    """the records form, flip, the records form again, clean: (fwd, level, cleaned outputs) from sentinel-filled arrays"""
    import torch
    Cn = 2 if corr else 1
    d_fwd, d_lev, d_bwd = filled(P, Cn, H, W, 4), filled(P, H, W), filled(P, Cn, H, W, 4)
    d_rrec, d_rref = filled(P, cap, 16 if corr else 12), (filled(P, cap, 8) if d_ref is not None else None)
    d_out, d_state, d_label, d_stats = filled(P, Cn, H, W, 4), filled(P, H, W), filled(P, H, W, 4), filled(P, 4, 4)
    torch.cuda.synchronize()
    ref, rref = (d_ref.data_ptr() if d_ref is not None else 0), (d_rref.data_ptr() if d_ref is not None else 0)
    c.densify_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, fill, d_fwd.data_ptr(), d_lev.data_ptr(), ref)
    c.flip_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), P, d_rrec.data_ptr(), ref, rref)
    c.densify_records_device(d_rrec.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, fill, d_bwd.data_ptr(), 0, rref)
    c.clean_fields_device(d_fwd.data_ptr(), Cn, W, H, P, prm, d_out.data_ptr(), d_bwd.data_ptr(), d_state.data_ptr(),
                          d_label.data_ptr(), d_stats.data_ptr())
    c.synchronize()
    return d_fwd.cpu().numpy(), d_lev.cpu().numpy(), read(d_out, d_state, d_label, d_stats, P, Cn, H, W)


@pytest.mark.parametrize("epipolar", [True, False])
@pytest.mark.parametrize("lanes", [1, 2])
def test_match_fill_and_clean_batch(oracle, forest_paths, epipolar, lanes):
    """the synthetic pairs of tests/test_gpu_dense.py (96 x 64, D = 5): clean_batch_device == match_batch_device (then
    refine_batch_device), the records form, flip, the records form, clean_fields_device; all outputs of both stages.  With
    the default parameters the pair's stats show kept pixels (5824 of 6144) and pixels that fail the check (320: the five
    columns whose target lies left of the image) but no speckle: every support has d = 5, the field is one value and one
    component.  Speckles (> 0 asserted, 3638 .. 3726 measured) show at STATE3_AT: with the sub-pixel refinement the values
    differ by a few 1/256 pixel, and speckle_diff_q8 = 0 then cuts the plane into segments of equal value."""
    import opengpc_amd as g
    import torch
    W, H, B, D = 96, 64, 2, 5
    c = g.Context(0)
    try:
        c.load_forest(forest_paths["zero"], W, H)
        c.set_pipeline(lanes)
        pairs = [oracle.synth_pair(W, H, i, D) for i in range(B)]
        d_L, d_R = (dev(np.stack([q[k] for q in pairs])) for k in (0, 1))
        cap = (W - 26) * (H - 26) + 1
        s, fill = settings(epipolar), g.Densify()
        for radius, prm in ((0, g.Clean()), (3, g.Clean()), (3, g.Clean(256, 0, 64, 1)), (0, g.Clean(-1, 256, 64, 2))):
            d_sup, d_cnt, d_nc, d_ref = filled(B, cap, 12), filled(B, 4), filled(B, 2, 4), None
            torch.cuda.synchronize()
            if radius:
                d_ref = filled(B, cap, 8)
                c.refine_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, radius, d_sup.data_ptr(), cap, d_cnt.data_ptr(),
                                      d_nc.data_ptr(), d_ref.data_ptr())
            else:
                c.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, d_sup.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
            c.synchronize()
            fwd, lev, want = chain(c, False, d_sup, cap, d_cnt, d_ref, W, H, B, fill, prm)
            d_out, d_state, d_label, d_stats = filled(B, 1, H, W, 4), filled(B, H, W), filled(B, H, W, 4), filled(B, 4, 4)
            d_fwd, d_lev, d_cnt2, d_nc2 = filled(B, 1, H, W, 4), filled(B, H, W), filled(B, 4), filled(B, 2, 4)
            torch.cuda.synchronize()
            c.clean_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, fill, prm, d_out.data_ptr(), d_state.data_ptr(),
                                 d_label.data_ptr(), d_stats.data_ptr(), d_fwd.data_ptr(), d_lev.data_ptr(), radius, d_cnt2.data_ptr(),
                                 d_nc2.data_ptr())
            c.synchronize()
            what = (epipolar, lanes, radius, prm.check_tol_q8, prm.speckle_diff_q8)
            assert np.array_equal(d_cnt2.cpu().numpy(), d_cnt.cpu().numpy()) and np.array_equal(d_nc2.cpu().numpy(), d_nc.cpu().numpy())
            assert np.array_equal(d_fwd.cpu().numpy(), fwd) and np.array_equal(d_lev.cpu().numpy(), lev), what
            got = read(d_out, d_state, d_label, d_stats, B, 1, H, W)
            same(got, want, what)
            f = fwd.view(np.int32).reshape(B, 1, H, W)
            assert (f != cu.NONE).all()
            print("stats", what, got[3].tolist())
            if prm.check_tol_q8 >= 0:
                assert (got[3][:, 0] > 0).all() and (got[3][:, 2] > 0).all(), (what, got[3].tolist())
            if (radius, prm.speckle_diff_q8) == STATE3_AT:
                assert (got[3][:, 3] > 0).all(), (what, got[3].tolist())
            # the optional outputs left out: out alone
            d_out2 = filled(B, 1, H, W, 4)
            torch.cuda.synchronize()
            c.clean_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, fill, prm, d_out2.data_ptr(), refine_radius=radius)
            c.synchronize()
            assert np.array_equal(d_out2.cpu().numpy().view(np.int32).reshape(B, 1, H, W), want[0]), what
    finally:
        c.close()


# (refine_radius, speckle_diff_q8) at which the synthetic pair shows speckles (the test above says why not at the defaults)
STATE3_AT = (3, 0)


@pytest.mark.parametrize("epipolar", [True, False])
def test_match_fill_and_clean_sequence(ctx, forest_paths, epipolar):
    """three frames of 96 x 64: clean_sequence_device == match_sequence_device (then refine), the records form, flip, the
    records form, clean_fields_device"""
    import torch
    import opengpc_amd as g
    W, H, N = 96, 64, 3
    frames = tu.frames_of(W, H, N, 1, 0 if epipolar else 3)
    ctx.load_forest(forest_paths["zero"], W, H)
    s, fill = settings(epipolar), g.Densify()
    cap = (W - 26) * (H - 26) + 1
    d_f = dev(frames)
    d_corr, d_cnt, d_nc = filled(N - 1, cap, 16), filled(N - 1, 4), filled(N, 4)
    torch.cuda.synchronize()
    ctx.match_sequence_device(d_f.data_ptr(), W, H, N, s, d_corr.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    for radius, prm in ((0, g.Clean()), (3, g.Clean(300, 100, 10, 2))):
        d_ref = None
        if radius:
            d_ref = filled(N - 1, cap, 8)
            torch.cuda.synchronize()
            ctx.refine_records_device(d_corr.data_ptr(), True, cap, d_cnt.data_ptr(), d_f.data_ptr(), d_f.data_ptr() + W * H, W, H, N - 1,
                                      radius, d_ref.data_ptr())
            ctx.synchronize()
        fwd, lev, want = chain(ctx, True, d_corr, cap, d_cnt, d_ref, W, H, N - 1, fill, prm)
        d_out, d_state, d_label, d_stats = filled(N - 1, 2, H, W, 4), filled(N - 1, H, W), filled(N - 1, H, W, 4), filled(N - 1, 4, 4)
        d_fwd, d_lev, d_cnt2, d_nc2 = filled(N - 1, 2, H, W, 4), filled(N - 1, H, W), filled(N - 1, 4), filled(N, 4)
        torch.cuda.synchronize()
        ctx.clean_sequence_device(d_f.data_ptr(), W, H, N, s, fill, prm, d_out.data_ptr(), d_state.data_ptr(), d_label.data_ptr(),
                                  d_stats.data_ptr(), d_fwd.data_ptr(), d_lev.data_ptr(), radius, d_cnt2.data_ptr(), d_nc2.data_ptr())
        ctx.synchronize()
        assert np.array_equal(d_cnt2.cpu().numpy(), d_cnt.cpu().numpy()) and np.array_equal(d_nc2.cpu().numpy(), d_nc.cpu().numpy())
        assert np.array_equal(d_fwd.cpu().numpy(), fwd) and np.array_equal(d_lev.cpu().numpy(), lev)
        got = read(d_out, d_state, d_label, d_stats, N - 1, 2, H, W)
        same(got, want, ("sequence", epipolar, radius))
        print("stats", epipolar, radius, got[3].tolist())
        assert (got[3][:, 0] > 0).all()


def test_refusals(forest_paths):
    """every refusal of the group, and the outputs afterwards: not a byte written"""
    import opengpc_amd as g
    import torch
    W, H = 96, 64
    E, U = g.capi.E_INVALID, g.capi.E_UNSUPPORTED
    c = g.Context(0)
    try:
        L = c.L
        d_f, d_b = filled(2, 2, H, W, 4), filled(2, 2, H, W, 4)
        d_out, d_state, d_label, d_stats = filled(2, 2, H, W, 4), filled(2, H, W), filled(2, H, W, 4), filled(2, 4, 4)
        good = g.Clean()
        torch.cuda.synchronize()

        def fields(fn=L.gpc_hip_clean_fields_device, fwd=d_f.data_ptr(), bwd=d_b.data_ptr(), ch=2, w=W, h=H, npairs=2, prm=good,
                   out=d_out.data_ptr()):
            return fn(c.h, fwd, bwd, ch, w, h, npairs, C.byref(prm) if prm is not None else None, out, d_state.data_ptr(),
                      d_label.data_ptr(), d_stats.data_ptr())

        for bad in (g.Clean(-2), g.Clean((1 << 24) + 1), g.Clean(256, -1), g.Clean(256, (1 << 24) + 1), g.Clean(256, 256, -1),
                    g.Clean(256, 256, (1 << 30) + 1), g.Clean(256, 256, 64, -1), g.Clean(256, 256, 64, 3)):
            assert fields(prm=bad) == E, (bad.check_tol_q8, bad.speckle_diff_q8, bad.speckle_min, bad.median_radius)
        assert fields(prm=None) == E and fields(fwd=None) == E and fields(out=None) == E and fields(bwd=None) == E   # the check needs bwd
        assert fields(ch=0) == E and fields(ch=3) == E and fields(npairs=0) == E and fields(w=0) == E and fields(h=-1) == E
        assert fields(out=d_f.data_ptr()) == E and fields(out=d_b.data_ptr() + 4 * W * H) == E and fields(out=d_f.data_ptr() - 16) == E
        assert fields(w=32769, h=1, npairs=1) == U and fields(w=1, h=32769, npairs=1) == U and fields(w=32768, h=32769, npairs=1) == U
        assert fields(npairs=65536, w=1, h=1) == U
        flip = lambda fn, rec=d_f.data_ptr(), ref=None, cap=64, cnt=d_stats.data_ptr(), npairs=2, out=d_out.data_ptr(), fout=None: fn(
            c.h, rec, ref, cap, cnt, npairs, out, fout)
        for fn in (L.gpc_hip_flip_supports_device, L.gpc_hip_flip_correspondences_device):
            assert flip(fn, rec=None) == E and flip(fn, cnt=None) == E and flip(fn, out=None) == E
            assert flip(fn, ref=d_b.data_ptr()) == E and flip(fn, fout=d_b.data_ptr()) == E            # ref and ref_out go together
            assert flip(fn, cap=0) == E and flip(fn, npairs=0) == E
            assert flip(fn, npairs=65536, cap=1) == U and flip(fn, cap=1 << 20, npairs=2048) == U
        c.synchronize()
        for d in (d_out, d_state, d_label, d_stats, d_f, d_b):
            assert bool((d == FILL).all())
        # the host form: the same checks on host arrays
        hf = np.zeros((2, 1, H, W), np.int32)
        ho = np.full((2, 1, H, W, 4), FILL, np.uint8)
        host = lambda prm=good, bwd=hf.ctypes.data, npairs=2, out=ho.ctypes.data, w=W: L.gpc_hip_clean_fields(
            c.h, hf.ctypes.data, bwd, 1, w, H, npairs, C.byref(prm), out, None, None, None)
        assert host(prm=g.Clean(-2)) == E and host(bwd=None) == E and host(npairs=0) == E and host(out=None) == E
        assert host(out=hf.ctypes.data) == E and host(npairs=65536) == U and host(w=40000) == U
        assert (ho == FILL).all()
        # match-fill-and-clean: their own refusals and those of the calls they wrap
        s, fill = settings(True), g.Densify()
        d_fr = dev(tu.frames_of(W, H, 3, 1))
        iL, iR = d_fr.data_ptr(), d_fr.data_ptr() + W * H
        seq = lambda nframes=3, radius=0, fl=fill, prm=good, out=d_out.data_ptr(), w=W, fwd=None: L.gpc_hip_clean_sequence_device(
            c.h, iL, w, H, nframes, C.byref(s), radius, C.byref(fl), C.byref(prm), out, None, None, None, fwd, None, None, None)
        bat = lambda npairs=2, radius=0, fl=fill, prm=good, out=d_out.data_ptr(), w=W, fwd=None: L.gpc_hip_clean_batch_device(
            c.h, iL, iR, w, H, npairs, C.byref(s), radius, C.byref(fl), C.byref(prm), out, None, None, None, fwd, None, None, None)
        assert seq() == g.capi.E_NO_FOREST and bat() == g.capi.E_NO_FOREST
        c.load_forest(forest_paths["zero"], W, H)
        for call in (seq, bat):
            assert call(radius=-1) == E and call(radius=7) == E and call(out=None) == E and call(w=W + 1) == E
            assert call(fl=g.Densify(15, 1, 3)) == E and call(fl=g.Densify(15, 1, 1, 500)) == E and call(prm=g.Clean(256, 256, 64, 3)) == E
            assert call(fwd=d_out.data_ptr()) == E
        assert seq(nframes=1) == E and bat(npairs=0) == E
        c.synchronize()
        st, groups = g.read_forest_groups(os.path.join(ROOT, "forests", "stress16x20Forest.txt"), W, H)
        c.set_forest_groups(groups)
        assert seq() == U                                            # group-mode sequences, as the sequence itself
        c.synchronize()
        assert bool((d_out == FILL).all())
        # group mode: the batch form cleans the union's field, and equals the chain over the union's records
        cap = 16 * (W - 26) * (H - 26) + 1
        d_sup, d_cnt, d_nc = filled(2, cap, 12), filled(2, 4), filled(2, 2, 4)
        torch.cuda.synchronize()
        c.match_batch_device(iL, iR, W, H, 2, s, d_sup.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
        c.synchronize()
        _, _, want = chain(c, False, d_sup, cap, d_cnt, None, W, H, 2, fill, good)
        d_o, d_s, d_l, d_t = filled(2, 1, H, W, 4), filled(2, H, W), filled(2, H, W, 4), filled(2, 4, 4)
        torch.cuda.synchronize()
        c.clean_batch_device(iL, iR, W, H, 2, s, fill, good, d_o.data_ptr(), d_s.data_ptr(), d_l.data_ptr(), d_t.data_ptr())
        c.synchronize()
        same(read(d_o, d_s, d_l, d_t, 2, 1, H, W), want, "group batch")
    finally:
        c.close()


def test_kernel_times_are_reported(ctx):
    """the seven timing slots behind k_quad_write take time when timing is on"""
    fwd, bwd = cu.random_fields(200, 90, 1)
    names = [ctx.L.gpc_hip_kernel_name(i).decode() for i in range(ctx.L.gpc_hip_kernel_slots())]
    ctx.L.gpc_hip_enable_kernel_timing(ctx.h, 1)
    ctx.L.gpc_hip_reset_kernel_timing(ctx.h)
    try:
        clean_device(ctx, fwd, bwd, cu.DEFAULTS)
        for k in ("k_clean_check", "k_clean_tile", "k_clean_border", "k_clean_flatten", "k_clean_sizes", "k_clean_apply"):
            ms, n = C.c_float(0), C.c_int(0)
            assert ctx.L.gpc_hip_kernel_time(ctx.h, names.index(k), C.byref(ms), C.byref(n)) == 0
            assert n.value == 1 and ms.value > 0, (k, ms.value, n.value)
            assert ctx.L.gpc_hip_kernel_launch_name(ctx.h, names.index(k)).decode().startswith("gpc::" + k)
    finally:
        ctx.L.gpc_hip_enable_kernel_timing(ctx.h, 0)
