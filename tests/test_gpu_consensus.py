"""Grid motion consensus on the GPU (gpc_hip_consensus_*): keep masks, kept records, their indices and the counts EQUAL the
plain restatement of the rule (tests/consensus_util.py) byte for byte -- every output starts out filled with a sentinel, so
the entries a call must leave alone are compared too -- for constructed records, thin grids, a neighbourhood larger than any
table, short outputs, and the records of the four matchers; the host forms equal the device forms; the filtered lists
compose with the track and score calls; refusals; the context's state afterwards."""
import ctypes as C

import numpy as np
import pytest

import consensus_util as cu
import score_util as su
import track_util as tu

pytestmark = pytest.mark.gpu

MATCHERS = [(True, False), (False, False), (True, True), (False, True)]   # (epipolar_mode, use_hashtable)
FILL = 0xA5


def P_(cell=16, shifts=4, num=6, den=1):
    import opengpc_amd as g
    return g.Consensus(cell, shifts, num, den), cu.Params(cell, shifts, num, den)


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def settings(epipolar, hashtable):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epipolar, hashtable, 1)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def filled(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def records_device(ctx, rec, counts, W, H, prm, cap_out, keep=True, index=True):
    """the records form over host records [P, cap]: (keep, out, index, out_counts) read back from sentinel-filled outputs"""
    import torch
    P, cap = rec.shape
    esz = rec.dtype.itemsize
    d_rec = dev(rec.view(np.uint8).reshape(P, cap, esz))
    d_cnt = dev(np.asarray(counts, np.int32))
    d_keep, d_out, d_idx, d_n = filled(P, cap), filled(P, cap_out, esz), filled(P, cap_out, 4), filled(P, 4)
    torch.cuda.synchronize()
    ctx.consensus_records_device(d_rec.data_ptr(), rec.dtype == cu.CORR, cap, d_cnt.data_ptr(), W, H, P, prm, d_keep.data_ptr() if keep else 0,
                                 d_out.data_ptr(), cap_out, d_idx.data_ptr() if index else 0, d_n.data_ptr())
    ctx.synchronize()
    return (d_keep.cpu().numpy(), d_out.cpu().numpy().view(rec.dtype).reshape(P, cap_out),
            d_idx.cpu().numpy().view(np.int32).reshape(P, cap_out), d_n.cpu().numpy().view(np.int32).reshape(P))


def same(got, want, what, skip=()):
    for k, name in enumerate(("keep", "out", "index", "out_counts")):
        if name not in skip:
            assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (what, name)


def check_records(ctx, rec, counts, W, H, cell, shifts, num, den, cap_out, what):
    prm, p = P_(cell, shifts, num, den)
    want = cu.expected_arrays(rec, counts, W, H, p, cap_out, FILL)
    same(records_device(ctx, rec, counts, W, H, prm, cap_out), want, what)
    return want


def constructed(W, H, P, per_pair, slots, seed, corr, special=True):
    """records [P, slots] and counts.  Half of a pair's records move by (+16, +8) (supports: d = -16), a sixth by (+9, -5)
    (d = 5), the rest anywhere; sources and targets repeat; some records lie outside the image; supports get a d that is
    no whole number, NaN and both infinities; every slot beyond a pair's count holds a copy of one of its valid records.
    special: pair 2 has count 0, pair 3 a count above the slots, pair 4 a negative one."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((P, slots), cu.CORR if corr else cu.SUPPORT)
    counts = np.zeros(P, np.int32)
    for t in range(P):
        m = int(per_pair * rng.uniform(0.8, 1.0))
        sx, sy = rng.integers(0, W, m), rng.integers(0, H, m)
        how = rng.random(m)
        dx = np.where(how < 0.5, 16, np.where(how < 0.67, 9, rng.integers(-W, W, m)))
        dy = np.where(how < 0.5, 8, np.where(how < 0.67, -5, rng.integers(-H, H, m)))
        d = rng.integers(0, m, m // 10)                      # duplicate sources
        sx[d], sy[d] = sx[d[::-1]], sy[d[::-1]]
        tx, ty = sx + dx, sy + dy
        d = rng.integers(0, m, m // 10)                      # shared targets
        tx[d], ty[d] = tx[d[::-1]], ty[d[::-1]]
        r = np.zeros(m, rec.dtype)
        if corr:
            r["src_x"], r["src_y"], r["tar_x"], r["tar_y"] = sx, sy, tx, ty
            for col, val in (("src_x", -1), ("src_y", H), ("tar_x", W), ("tar_y", -3), ("src_x", W + 5)):
                r[col][rng.integers(0, m, 3)] = val
        else:
            r["x"], r["y"], r["d"] = sx, sy, (sx - tx).astype(np.float32)
            for col, val in (("x", -1), ("y", H), ("x", W + 5), ("y", -2)):
                r[col][rng.integers(0, m, 3)] = val
            r["d"][rng.integers(0, m, 8)] = (0.5, -16.25, np.nan, np.inf, -np.inf, 2.0 ** 24, -2.0 ** 24, 3e38)
        rec[t, :m] = r
        rec[t, m:] = r[rng.integers(0, m, slots - m)]
        counts[t] = m
    if special:
        counts[2], counts[3], counts[4] = 0, slots + 7, -3
    return rec, counts


@pytest.mark.parametrize("corr", [True, False])
@pytest.mark.parametrize("shifts", [1, 4])
def test_constructed_records_72x50(ctx, corr, shifts):
    """Cells of 8 pixels: ragged at both edges (72 = 9 * 8, 50 = 6 * 8 + 2), the shifted grids one cell larger.  5 pairs."""
    W, H = 72, 50
    rec, counts = constructed(W, H, 5, 340, 400, 17 + corr, corr)
    for num, den in ((6, 1), (3, 2), (0, 1)):
        keep, out, index, n = check_records(ctx, rec, counts, W, H, 8, shifts, num, den, 400, (corr, shifts, num, den))
        assert n[2] == 0 and n[4] == 0 and (keep[2] == FILL).all() and (keep[4] == FILL).all()
        assert (keep[3] != FILL).all()                           # a count above the slots reads every slot
        if num == 6:
            assert 0 < n[0] < counts[0] and 0 < n[1] < counts[1]  # some kept, some dropped
    # no keep mask and no index wanted: the rest is the same
    prm, p = P_(8, shifts, 6, 1)
    want = cu.expected_arrays(rec, counts, W, H, p, 400, FILL)
    got = records_device(ctx, rec, counts, W, H, prm, 400, keep=False, index=False)
    same(got, want, "no keep, no index", skip=("keep", "index"))
    assert (got[0] == FILL).all() and (got[2].view(np.uint8) == FILL).all()


@pytest.mark.parametrize("W,H", [(16, 16), (40, 16)])
def test_thin_grids(ctx, W, H):
    """16x16 with cells of 16: one cell (k = 1), 2x2 under the shifts (k = 4); 40x16: a single row of cells"""
    for corr in (True, False):
        rec, counts = constructed(W, H, 2, 60, 64, 5 + corr, corr, special=False)
        for shifts in (1, 4):
            for num, den in ((6, 1), (1, 1), (5, 2)):
                check_records(ctx, rec, counts, W, H, 16, shifts, num, den, 64, (W, H, corr, shifts, num, den))


def test_over_full_neighbourhood_at_the_grid_limit(ctx):
    """8192 x 8192 with cells of 4 is the grid limit exactly (2^22 cells).  Pair 0: 40 000 records whose sources lie in one
    cell and whose targets are drawn over the whole image -- tens of thousands of distinct classes in one neighbourhood,
    more than any table in LDS holds; with alpha 1/64 a record passes iff another one shares its class (S = 1:
    9 * 4096 < 40 000; S = 2 passes).  Pair 1: 40 000 records of one class.  8196 wide is refused."""
    import opengpc_amd as g
    W = H = 8192
    n = 40000
    rng = np.random.default_rng(4)
    rec = np.zeros((2, n), cu.CORR)
    rec["src_x"], rec["src_y"] = 4000 + rng.integers(0, 4, (2, n)), 4000 + rng.integers(0, 4, (2, n))
    rec["tar_x"][0], rec["tar_y"][0] = rng.integers(0, W, n), rng.integers(0, H, n)
    rec["tar_x"][1], rec["tar_y"][1] = 6000 + rng.integers(0, 2, n), 120 + rng.integers(0, 2, n)
    counts = np.array([n, n], np.int32)
    keep, out, index, kept = check_records(ctx, rec, counts, W, H, 4, 4, 1, 64, n, "over-full")
    assert 0 < kept[0] < n // 4 and kept[1] == n
    classes = len(set(zip((rec["tar_x"][0] // 4 - 1000).tolist(), (rec["tar_y"][0] // 4 - 1000).tolist())))
    assert classes > 30000
    prm, p = P_(4, 4, 1, 64)
    import torch
    d = filled(2, 16, 16)
    for w, status in ((8192, 0), (8196, g.capi.E_UNSUPPORTED)):
        st = ctx.L.gpc_hip_consensus_correspondences_device(ctx.h, d.data_ptr(), 8, dev(np.zeros(2, np.int32)).data_ptr(), w, H, 2,
                                                            C.byref(prm), None, filled(2, 8, 16).data_ptr(), 8, None,
                                                            filled(2, 4).data_ptr())
        assert st == status, (w, st)
    ctx.synchronize()


def test_capacity_and_host_forms(ctx):
    """cap_out below the kept count: the device form writes the true count and the first cap_out records; the host form
    returns GPC_E_CAPACITY with the same bytes.  Pageable and page-locked arrays; more than one chunk of 16 pairs."""
    import opengpc_amd as g
    W, H = 72, 50
    for corr in (True, False):
        rec, counts = constructed(W, H, 19, 120, 140, 31 + corr, corr)
        prm, p = P_(8, 4, 3, 1)
        full = cu.expected_arrays(rec, counts, W, H, p, 140, FILL)[3]
        assert full.max() > 20
        for cap_out, status in ((140, 0), (int(full.max()), 0), (int(full.max()) - 1, g.capi.E_CAPACITY), (5, g.capi.E_CAPACITY)):
            want = cu.expected_arrays(rec, counts, W, H, p, cap_out, FILL)
            same(records_device(ctx, rec, counts, W, H, prm, cap_out), want, ("device", corr, cap_out))
            for what, alloc in (("pageable", np.empty), ("page-locked", ctx.pinned_empty)):
                hrec = alloc(rec.shape, rec.dtype)
                hrec[...] = rec
                keep, out, index = alloc(rec.shape, np.uint8), alloc((19, cap_out), rec.dtype), alloc((19, cap_out), np.int32)
                for a in (keep, out, index):
                    a.view(np.uint8)[...] = FILL
                k, o, i, n, st = ctx.consensus_records(hrec, counts, W, H, prm, cap_out, keep, out, index)
                assert st == status, (what, corr, cap_out, st)
                same((k, o, i, n), want, (what, corr, cap_out))


def sequence_device(ctx, frames, s, cap):
    import torch
    N, H, W = frames.shape
    d_f = dev(frames)
    d_out, d_cnt, d_nc = filled(N - 1, cap, 16), filled(N - 1, 4), filled(N, 4)
    torch.cuda.synchronize()
    ctx.match_sequence_device(d_f.data_ptr(), W, H, N, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    return (d_out.cpu().numpy().view(cu.CORR).reshape(N - 1, cap), d_cnt.cpu().numpy().view(np.int32).reshape(-1),
            d_nc.cpu().numpy().view(np.int32).reshape(-1))


def consensus_sequence(ctx, frames, s, prm, cap_out):
    import torch
    N, H, W = frames.shape
    d_f = dev(frames)
    d_out, d_n, d_raw, d_nc = filled(N - 1, cap_out, 16), filled(N - 1, 4), filled(N - 1, 4), filled(N, 4)
    torch.cuda.synchronize()
    ctx.consensus_sequence_device(d_f.data_ptr(), W, H, N, s, prm, d_out.data_ptr(), cap_out, d_n.data_ptr(), d_raw.data_ptr(),
                                  d_nc.data_ptr())
    ctx.synchronize()
    i32 = lambda d: d.cpu().numpy().view(np.int32).reshape(-1)
    return d_out.cpu().numpy().view(cu.CORR).reshape(N - 1, cap_out), i32(d_n), i32(d_raw), i32(d_nc), (d_out, d_n)


@pytest.mark.parametrize("W,H", [(160, 101), (1040, 77)])
@pytest.mark.parametrize("epipolar,hashtable", MATCHERS)
def test_match_and_filter_sequence(ctx, forest_paths, W, H, epipolar, hashtable):
    """the frame sets of tests/track_util.py, zero forest: consensus_sequence_device == the restatement over
    match_sequence_device's own records, d_raw_counts == its counts; a short output too"""
    frames = tu.frames_of(W, H, 8, 1, 0 if epipolar else 12)
    ctx.load_forest(forest_paths["zero"], W, H)
    s = settings(epipolar, hashtable)
    cap = (W - 26) * (H - 26)
    rec, cnt, nc = sequence_device(ctx, frames, s, cap)
    prm, p = P_()
    want = cu.expected_arrays(rec, cnt, W, H, p, cap, FILL)
    out, n, raw, nc2, _ = consensus_sequence(ctx, frames, s, prm, cap)
    print("kept / raw per pair", list(zip(want[3].tolist(), cnt.tolist())))
    assert np.array_equal(raw, cnt) and np.array_equal(nc2, nc)
    same((None, out, None, n), want, (W, H, epipolar, hashtable), skip=("keep", "index"))
    if not epipolar:     # the crops that move in y: the matchers without the epipolar constraint emit some lone collisions
        assert 0 < want[3].sum() < cnt.sum(), (want[3].tolist(), cnt.tolist())
    small = max(int(want[3].max()) // 2, 1)
    out, n, raw, nc2, _ = consensus_sequence(ctx, frames, s, prm, small)
    same((None, out, None, n), cu.expected_arrays(rec, cnt, W, H, p, small, FILL), "short", skip=("keep", "index"))


@pytest.mark.parametrize("lanes", [1, 2])
def test_match_and_filter_batch_then_plain_batch(oracle, forest_paths, lanes):
    """3 synthetic pairs of 256x64: consensus_batch_device == the restatement over match_batch_device's records, with one
    lane and with two (the same bytes); a plain match_batch_device on the same context afterwards still equals the oracle"""
    import opengpc_amd as g
    import torch
    from oracle.pyoracle import sparsematch_settings
    W, H, B = 256, 64, 3
    c = g.Context(0)
    try:
        c.load_forest(forest_paths["zero"], W, H)
        c.set_pipeline(lanes)
        rc, f = oracle.read_forest(forest_paths["zero"], W, H)
        pairs = [oracle.synth_pair(W, H, i, 9 + i) for i in range(B)]
        Lh, Rh = (np.ascontiguousarray(np.stack([q[k] for q in pairs])) for k in (0, 1))
        d_L, d_R = dev(Lh), dev(Rh)
        cap = (W - 26) * (H - 26)
        prm, p = P_(16, 4, 2, 1)

        def plain(s):
            d_out, d_cnt, d_nc = filled(B, cap, 12), filled(B, 4), filled(B, 2, 4)
            torch.cuda.synchronize()
            c.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
            c.synchronize()
            return (d_out.cpu().numpy().view(cu.SUPPORT).reshape(B, cap), d_cnt.cpu().numpy().view(np.int32).reshape(-1),
                    d_nc.cpu().numpy().view(np.int32).reshape(B, 2))

        for epipolar, hashtable in MATCHERS:
            s = settings(epipolar, hashtable)
            rec, cnt, nc = plain(s)
            d_out, d_n, d_raw, d_nc = filled(B, cap, 12), filled(B, 4), filled(B, 4), filled(B, 2, 4)
            torch.cuda.synchronize()
            c.consensus_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, prm, d_out.data_ptr(), cap, d_n.data_ptr(),
                                     d_raw.data_ptr(), d_nc.data_ptr())
            c.synchronize()
            i32 = lambda d: d.cpu().numpy().view(np.int32)
            want = cu.expected_arrays(rec, cnt, W, H, p, cap, FILL)
            print("kept / raw per pair", list(zip(want[3].tolist(), cnt.tolist())))
            assert np.array_equal(i32(d_raw).reshape(-1), cnt) and np.array_equal(i32(d_nc).reshape(B, 2), nc)
            same((None, d_out.cpu().numpy().view(cu.SUPPORT).reshape(B, cap), None, i32(d_n).reshape(-1)), want,
                 (lanes, epipolar, hashtable), skip=("keep", "index"))
        for epipolar in (True, False):
            rec, cnt, nc = plain(settings(epipolar, False))
            for q in range(B):
                want, nl, nr = oracle.match_pair(Lh[q], Rh[q], f, sparsematch_settings(5, 128, 0, epipolar))
                assert tuple(nc[q]) == (nl, nr) and cnt[q] == len(want), (epipolar, q)
                assert np.array_equal(rec[q, :cnt[q]], want.astype(cu.SUPPORT)), (epipolar, q)
    finally:
        c.close()


def test_filtered_records_compose_with_tracks_and_scores(ctx, forest_paths):
    """the correspondences consensus_sequence_device leaves on the device go to gpc_hip_track_records_device and
    gpc_hip_score_correspondences_device as they are: the results equal track_util / score_util over the restatement's
    kept list"""
    import opengpc_amd as g
    import torch
    W, H, N = 160, 101, 8
    frames = tu.frames_of(W, H, N, 1, 12)
    ctx.load_forest(forest_paths["zero"], W, H)
    s = settings(False, False)
    cap = (W - 26) * (H - 26)
    rec, cnt, nc = sequence_device(ctx, frames, s, cap)
    prm, p = P_()
    klist, kn = cu.kept_list(rec, cnt, W, H, p)
    out, n, raw, nc2, (d_out, d_n) = consensus_sequence(ctx, frames, s, prm, cap)
    assert np.array_equal(n, kn)
    # tracks
    P = N - 1
    track_cap = int(kn.sum()) + 1
    d_next, d_id = filled(P, cap, 4), filled(P, cap, 4)
    d_tab, d_nt = filled(track_cap, 16), filled(4)
    torch.cuda.synchronize()
    ctx.track_records_device(d_out.data_ptr(), cap, d_n.data_ptr(), W, H, P, d_next.data_ptr(), d_id.data_ptr(), d_tab.data_ptr(),
                             track_cap, d_nt.data_ptr())
    ctx.synchronize()
    fill32 = int(np.array([FILL] * 4, np.uint8).view(np.int32)[0])
    wn, wi, wt, wnum = tu.expected_arrays(klist.view(tu.CORR).reshape(P, cap), kn, W, H, fill32, track_cap)
    i32 = lambda d, *shape: d.cpu().numpy().view(np.int32).reshape(*shape)
    assert int(i32(d_nt, -1)[0]) == wnum
    assert np.array_equal(i32(d_next, P, cap), wn) and np.array_equal(i32(d_id, P, cap), wi)
    assert np.array_equal(i32(d_tab, track_cap, 4), wt.view(np.int32).reshape(track_cap, 4))
    # scores
    rng = np.random.default_rng(2)
    u = rng.integers(-8, 9, (P, H, W)).astype(np.float32)
    v = rng.integers(-13, 14, (P, H, W)).astype(np.float32)
    d_sc = torch.full((P, 15), -3, dtype=torch.int64, device=torch.device("cuda", 0))
    d_u, d_v = dev(u), dev(v)
    torch.cuda.synchronize()
    thr = [1.0, 3.0]
    ctx.score_correspondences_device(d_out.data_ptr(), cap, d_n.data_ptr(), W, H, P, d_u.data_ptr(), d_v.data_ptr(), 0, thr,
                                     d_sc.data_ptr())
    ctx.synchronize()
    got = d_sc.cpu().numpy().copy().view(g.SCORE_DTYPE).reshape(-1)
    for t in range(P):
        want = su.score_records(klist[t], kn[t], cap, u[t], v[t], None, thr)
        have = su.as_dict(got[t])
        for k in su.SCORE_FIELDS:
            assert have[k] == want[k], (t, k)


def test_refusals(forest_paths):
    import opengpc_amd as g
    import torch
    W, H = 96, 64
    E, U = g.capi.E_INVALID, g.capi.E_UNSUPPORTED
    c = g.Context(0)
    try:
        L = c.L
        d_rec, d_out = filled(2, 64, 16), filled(2, 64, 16)
        d_cnt, d_n = dev(np.array([10, 20], np.int32)), filled(2, 4)
        d_keep, d_idx = filled(2, 64), filled(2, 64, 4)
        good = g.Consensus()
        torch.cuda.synchronize()

        def recs(fn=L.gpc_hip_consensus_correspondences_device, rec=d_rec.data_ptr(), cap=64, cnt=d_cnt.data_ptr(), w=W, h=H, npairs=2,
                 prm=good, out=d_out.data_ptr(), cap_out=64, n=d_n.data_ptr()):
            return fn(c.h, rec, cap, cnt, w, h, npairs, C.byref(prm) if prm is not None else None, d_keep.data_ptr(), out, cap_out,
                      d_idx.data_ptr(), n)

        for fn in (L.gpc_hip_consensus_correspondences_device, L.gpc_hip_consensus_supports_device):
            assert recs(fn) == 0                                     # (the records forms need no forest)
            for bad in (g.Consensus(2), g.Consensus(258), g.Consensus(15), g.Consensus(16, 2), g.Consensus(16, 0),
                        g.Consensus(16, 4, -1), g.Consensus(16, 4, 1025), g.Consensus(16, 4, 6, 0), g.Consensus(16, 4, 6, 65)):
                assert recs(fn, prm=bad) == E, (bad.cell, bad.shifts, bad.alpha_num, bad.alpha_den)
            assert recs(fn, prm=g.Consensus(256, 1, 1024, 64)) == 0 and recs(fn, prm=g.Consensus(4, 4, 0, 1)) == 0
            assert recs(fn, prm=None) == E and recs(fn, rec=None) == E and recs(fn, cnt=None) == E and recs(fn, out=None) == E
            assert recs(fn, n=None) == E and recs(fn, npairs=0) == E and recs(fn, cap=0) == E and recs(fn, cap_out=0) == E
            assert recs(fn, w=0) == E and recs(fn, h=-1) == E
            assert recs(fn, out=d_rec.data_ptr()) == E and recs(fn, out=d_rec.data_ptr() + 48 * 20) == E   # out inside the records
            assert recs(fn, cap=(1 << 23) + 1, npairs=1) == U and recs(fn, npairs=65536, cap=1) == U
            assert recs(fn, cap=1 << 20, npairs=2048) == U            # npairs * cap_per_pair = 2^31
            assert recs(fn, w=8196, h=8192, prm=g.Consensus(4)) == U
        c.synchronize()
        # host forms: the same checks on host arrays
        hrec, hcnt = np.zeros((2, 64), g.CORR_DTYPE), np.array([3, 4], np.int32)
        hkeep, hout, hidx, hn = np.zeros((2, 64), np.uint8), np.zeros((2, 64), g.CORR_DTYPE), np.zeros((2, 64), np.int32), np.zeros(2, np.int32)
        host = lambda prm=good, out=hout.ctypes.data, npairs=2: L.gpc_hip_consensus_correspondences(
            c.h, hrec.ctypes.data, 64, hcnt.ctypes.data, W, H, npairs, C.byref(prm), hkeep.ctypes.data, out, 64, hidx.ctypes.data,
            hn.ctypes.data)
        assert host() == 0 and host(prm=g.Consensus(6, 3)) == E and host(out=hrec.ctypes.data) == E and host(npairs=0) == E
        # match-and-filter forms: the refusals of the match they wrap
        frames = tu.frames_of(W, H, 3, 1)
        d_f = dev(frames)
        s = settings(True, False)
        seq = lambda nframes=3, prm=good, out=d_out.data_ptr(), cap_out=64: L.gpc_hip_consensus_sequence_device(
            c.h, d_f.data_ptr(), W, H, nframes, C.byref(s), C.byref(prm), out, cap_out, d_n.data_ptr(), None, None)
        bat = lambda npairs=1, prm=good, out=d_out.data_ptr(), cap_out=64: L.gpc_hip_consensus_batch_device(
            c.h, d_f.data_ptr(), d_f.data_ptr() + W * H, W, H, npairs, C.byref(s), C.byref(prm), out, cap_out, d_n.data_ptr(), None, None)
        assert seq() == g.capi.E_NO_FOREST and bat() == g.capi.E_NO_FOREST
        c.load_forest(forest_paths["zero"], W, H)
        assert seq() == 0 and bat() == 0
        c.synchronize()
        for call in (seq, bat):
            assert call(prm=g.Consensus(5)) == E and call(out=None) == E and call(cap_out=0) == E
        assert seq(nframes=1) == E and bat(npairs=0) == E
        import os
        st, groups = g.read_forest_groups(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "forests",
                                                       "stress16x20Forest.txt"), W, H)
        assert st == 0 and len(groups) == 16
        c.set_forest_groups(groups)
        assert seq() == U                                            # group-mode sequences, as the sequence itself
        assert recs() == 0
        c.synchronize()
    finally:
        c.close()
