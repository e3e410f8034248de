"""Point tracks on the GPU (gpc_hip_track_*): links, track ids, the track table and the number of tracks EQUAL the plain
restatement of the rule (tests/track_util.py), byte for byte, for constructed records and for the records of
match_sequence_device; the host forms equal the device forms; refusals; the context's state afterwards."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import track_util as tu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCHERS = [(True, False), (False, False), (True, True), (False, True)]   # (epipolar_mode, use_hashtable)
FILL = -7
SEED = {(160, 101): 1, (1040, 77): 1}   # frames_of seeds chosen on the CPU: see test_match_and_track


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def settings(epipolar, hashtable):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epipolar, hashtable, 1)


def outputs(P, cap, track_cap):
    import torch
    dev = torch.device("cuda", 0)
    return (torch.full((P, cap), FILL, dtype=torch.int32, device=dev), torch.full((P, cap), FILL, dtype=torch.int32, device=dev),
            torch.full((max(track_cap, 1), 4), FILL, dtype=torch.int32, device=dev), torch.full((1,), FILL, dtype=torch.int32, device=dev))


def fetch(d_next, d_id, d_tab, d_n, track_cap):
    return (d_next.cpu().numpy(), d_id.cpu().numpy(), d_tab.cpu().numpy()[:track_cap].copy().view(tu.TRACK).reshape(-1),
            int(d_n.cpu().numpy()[0]))


def records_device(ctx, rec, counts, W, H, track_cap):
    """gpc_hip_track_records_device over host records [P, cap]: outputs that held FILL everywhere, read back"""
    import torch
    P, cap = rec.shape
    dev = torch.device("cuda", 0)
    d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(P, cap, 4)).to(dev)
    d_cnt = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).to(dev)
    d_next, d_id, d_tab, d_n = outputs(P, cap, track_cap)
    torch.cuda.synchronize(dev)
    ctx.track_records_device(d_rec.data_ptr(), cap, d_cnt.data_ptr(), W, H, P, d_next.data_ptr(), d_id.data_ptr(),
                             d_tab.data_ptr() if track_cap else 0, track_cap, d_n.data_ptr())
    ctx.synchronize()
    return fetch(d_next, d_id, d_tab, d_n, track_cap)


def same(got, want, what):
    for k, name in enumerate(("next", "track_id", "table")):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, name)
    assert got[3] == want[3], (what, "n_tracks", got[3], want[3])


def constructed(W, H, P, per_pair, slots, seed, empty=None):
    """records [P, slots] and counts: the targets of pair t are drawn partly from the sources of pair t + 1, sources and
    targets repeat, some records lie outside the image, pair `empty` has count 0, and every slot beyond a pair's count
    holds a copy of one of the pair's valid records (which would link if it were read)"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((P, slots, 4), np.int32)
    counts = np.zeros(P, np.int32)
    for t in range(P - 1, -1, -1):
        m = int(per_pair * rng.uniform(0.8, 1.0))
        r = np.stack([rng.integers(0, W, m), rng.integers(0, H, m), rng.integers(0, W, m), rng.integers(0, H, m)], 1)
        if t + 1 < P:                                        # chains: targets that are sources of pair t + 1
            k = rng.random(m) < 0.6
            r[k, 2:] = rec[t + 1, rng.integers(0, slots, int(k.sum())), :2]
        d = rng.integers(0, m, m // 10)                      # duplicate sources
        r[d, :2] = r[rng.integers(0, m, len(d)), :2]
        d = rng.integers(0, m, m // 10)                      # shared targets
        r[d, 2:] = r[rng.integers(0, m, len(d)), 2:]
        for col, val in ((0, -1), (1, H), (2, W), (3, -3), (0, W + 5)):   # outside the image
            r[rng.integers(0, m, 3), col] = val
        rec[t, :m] = r
        rec[t, m:] = r[rng.integers(0, m, slots - m)]
        counts[t] = 0 if t == empty else m
    return rec.view(tu.CORR).reshape(P, slots), counts


def test_constructed_records_48x41(ctx):
    """P = 5, a few hundred records per pair, an empty pair in the middle, duplicates of both kinds, records outside the
    image, padding that would link; then the same with cap below the counts; track_cap 0, one short and exact."""
    W, H, P = 48, 41, 5
    rec, counts = constructed(W, H, P, 340, 400, 11, empty=2)
    assert counts[2] == 0 and counts.max() <= 400 and counts[[0, 1, 3, 4]].min() > 250
    for what, r, c in (("fits", rec, counts), ("cap < counts", np.ascontiguousarray(rec[:, :200]), counts)):
        nxt, tid, rows, n = tu.restate(r, c, W, H)
        assert n > 50 and any(row[2] >= 2 for row in rows) and sum(v >= 0 for v in nxt[0]) > 20
        for track_cap in (0, n - 1, n, n + 3):
            want = tu.expected_arrays(r, c, W, H, FILL, track_cap)
            same(records_device(ctx, r, c, W, H, track_cap), want, (what, track_cap))
    # without the empty pair chains run through the middle: some track has three records or more
    rec, counts = constructed(W, H, P, 340, 400, 12)
    nxt, tid, rows, n = tu.restate(rec, counts, W, H)
    assert max(row[2] for row in rows) >= 3
    same(records_device(ctx, rec, counts, W, H, n), tu.expected_arrays(rec, counts, W, H, FILL, n), "no empty pair")


def test_constructed_records_160x101_many_chunks(ctx):
    """P = 3, about 10 000 records per pair: the heads of a pair lie in five chunks of 2048 records, the last one partial,
    so the numbering crosses chunk boundaries and the scan's tail is partial"""
    W, H, P = 160, 101, 3
    rec, counts = constructed(W, H, P, 10250, 10300, 5)
    assert counts.min() > 8192 and counts.max() % 2048 != 0
    nxt, tid, rows, n = tu.restate(rec, counts, W, H)
    assert n > 3 * 2048
    same(records_device(ctx, rec, counts, W, H, n), tu.expected_arrays(rec, counts, W, H, FILL, n), "10k")
    same(records_device(ctx, rec, counts, W, H, 100), tu.expected_arrays(rec, counts, W, H, FILL, 100), "10k, short table")


def test_one_pair(ctx):
    W, H = 48, 41
    rec, counts = constructed(W, H, 1, 300, 320, 3)
    nxt, tid, rows, n = tu.restate(rec, counts, W, H)
    assert n == counts[0] and all(v == -1 for v in nxt[0])
    same(records_device(ctx, rec, counts, W, H, n), tu.expected_arrays(rec, counts, W, H, FILL, n), "P = 1")


def sequence_device(ctx, frames, s, cap):
    """match_sequence_device -> (records [N-1, cap] as int32 [N-1, cap, 4], counts, ncand)"""
    import torch
    N, H, W = frames.shape
    dev = torch.device("cuda", 0)
    d_f = torch.from_numpy(frames).to(dev)
    d_out = torch.full((N - 1, cap, 4), FILL, dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(N - 1, dtype=torch.int32, device=dev)
    d_nc = torch.zeros(N, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.match_sequence_device(d_f.data_ptr(), W, H, N, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    return d_out.cpu().numpy(), d_cnt.cpu().numpy(), d_nc.cpu().numpy()


def track_device(ctx, frames, s, cap, track_cap):
    import torch
    N, H, W = frames.shape
    dev = torch.device("cuda", 0)
    d_f = torch.from_numpy(frames).to(dev)
    d_out = torch.full((N - 1, cap, 4), FILL, dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(N - 1, dtype=torch.int32, device=dev)
    d_nc = torch.zeros(N, dtype=torch.int32, device=dev)
    d_next, d_id, d_tab, d_n = outputs(N - 1, cap, track_cap)
    torch.cuda.synchronize(dev)
    ctx.track_sequence_device(d_f.data_ptr(), W, H, N, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr(),
                              d_next.data_ptr(), d_id.data_ptr(), d_tab.data_ptr() if track_cap else 0, track_cap, d_n.data_ptr())
    ctx.synchronize()
    return (d_out.cpu().numpy(), d_cnt.cpu().numpy(), d_nc.cpu().numpy()), fetch(d_next, d_id, d_tab, d_n, track_cap)


def check_match_and_track(ctx, frames, s):
    N, H, W = frames.shape
    cap = (W - 26) * (H - 26)
    track_cap = cap * (N - 1)
    rec, cnt, nc = sequence_device(ctx, frames, s, cap)
    (rec2, cnt2, nc2), got = track_device(ctx, frames, s, cap, track_cap)
    assert np.array_equal(cnt, cnt2) and np.array_equal(nc, nc2)
    assert np.array_equal(rec.view(np.uint8), rec2.view(np.uint8))      # padding included: neither call writes it
    r = np.ascontiguousarray(rec2).view(tu.CORR).reshape(N - 1, cap)
    same(got, tu.expected_arrays(r, cnt2, W, H, FILL, track_cap), (W, H, s.epipolar_mode, s.use_hashtable))
    return r, cnt2, got


@pytest.mark.parametrize("W,H", [(160, 101), (1040, 77)])
@pytest.mark.parametrize("epipolar,hashtable", MATCHERS)
def test_match_and_track(ctx, oracle, forest_paths, W, H, epipolar, hashtable):
    """8 translated crops of one texture, zero forest, SSE arithmetic.  The records, counts and candidate counts are those
    of match_sequence_device; links and tracks equal the restatement over them.  Not vacuous: under the sort matchers
    the restatement over the ORACLE's records (CPU) holds tracks of three records and more, tracks that end before the last
    pair and tracks that start after pair 0.  The crops of test_gpu_sequence.py move in y from frame to frame, which leaves
    the epipolar matchers (same row only) a handful of matches per pair and no track of three records in any seed tried
    (seeds 1 .. 3: 3 to 39 593 tracks, none longer than 2), so for them the vertical overlap is enlarged to the whole
    frame (dy = 0); the non-epipolar matchers get the crops as they are.  Seed 1, oracle alone, as (length >= 3, end
    early, start late) of all tracks:
      160x101  epipolar sort, dy = 0: (7432, 5575, 5554) of 12864;   non-epipolar sort: (7098, 6713, 5584) of 12250
      1040x77  epipolar sort, dy = 0: (40914, 22260, 23052) of 61795; non-epipolar sort: (32748, 34855, 31269) of 60516"""
    frames = tu.frames_of(W, H, 8, SEED[(W, H)], 0 if epipolar else 12)
    ctx.load_forest(forest_paths["zero"], W, H)
    r, cnt, got = check_match_and_track(ctx, frames, settings(epipolar, hashtable))
    if not hashtable:
        rc, f = oracle.read_forest(forest_paths["zero"], W, H)
        orec, ocnt, onc = tu.oracle_sequence(oracle, frames, f, epipolar, hashtable)
        nxt, tid, rows, n = tu.restate(orec, ocnt, W, H)
        long_, early, late = tu.shape_of_tracks(rows, 7)
        assert long_ >= 1 and early >= 1 and late >= 1, (long_, early, late, n)
        assert n == got[3] and np.array_equal(ocnt, cnt)


def test_match_and_track_naive_tau(ctx, forest_paths):
    W, H = 160, 101
    frames = tu.frames_of(W, H, 8, SEED[(W, H)])
    ctx.set_arithmetic(True)
    try:
        ctx.load_forest(forest_paths["tau"], W, H)
        r, cnt, got = check_match_and_track(ctx, frames, settings(False, False))
        assert got[3] > 0 and cnt.min() > 0
    finally:
        ctx.set_arithmetic(False)


def test_host_forms_equal_device_forms(ctx, forest_paths):
    """pageable and page-locked inputs; GPC_E_CAPACITY with the defined partial outputs"""
    import opengpc_amd as g
    W, H, P = 48, 41, 5
    rec, counts = constructed(W, H, P, 340, 400, 21)
    n = tu.restate(rec, counts, W, H)[3]
    for what, alloc in (("pageable", np.empty), ("page-locked", ctx.pinned_empty)):   # every array of the call, in and out
        for cap, track_cap, status in ((400, n, 0), (400, n - 1, g.capi.E_CAPACITY), (200, 200 * P, g.capi.E_CAPACITY)):
            rr = alloc((P, cap), g.CORR_DTYPE)
            rr[...] = rec[:, :cap]
            hcnt = alloc((P,), np.int32)
            hcnt[...] = counts
            dn, di, dt, dnum = records_device(ctx, np.asarray(rr), counts, W, H, track_cap)
            nxt = alloc((P, cap), np.int32)
            tid = alloc((P, cap), np.int32)
            tab = alloc((max(track_cap, 1),), g.TRACK_DTYPE)
            nxt[...] = FILL
            tid[...] = FILL
            tab.view(np.int32)[...] = FILL
            hn, hi, ht, hnum, st = ctx.track_records(rr, hcnt, W, H, track_cap, nxt, tid, tab)
            assert st == status, (what, cap, track_cap, st)
            k = min(dnum, track_cap)
            assert hnum == dnum and np.array_equal(nxt, dn) and np.array_equal(tid, di), (what, cap, track_cap)
            assert np.array_equal(tab[:track_cap].view(np.uint8), dt.view(np.uint8)) and len(ht) == k
    # frames in, everything out (the epipolar matcher gets the crops with full vertical overlap, as in
    # test_match_and_track: the crops that move in y leave it at most one match per pair, and nothing to halve below)
    W, H = 160, 101
    ctx.load_forest(forest_paths["zero"], W, H)
    pf = ctx.pinned_empty((8, H, W), np.uint8)
    for epipolar, hashtable in ((True, False), (False, True)):
        frames = tu.frames_of(W, H, 8, SEED[(W, H)], 0 if epipolar else 12)
        pf[...] = frames
        s = settings(epipolar, hashtable)
        cap = (W - 26) * (H - 26)
        (rec, cnt, nc), (dn, di, dt, dnum) = track_device(ctx, frames, s, cap, cap * 7)
        assert cnt.min() > 20 and dnum > 10      # (so that half a pair's count and a table of 10 rows are both too small)
        for what, fr in (("pageable", frames), ("page-locked", pf)):
            out, hc, hnc, hn, hi, ht, hnum, st = ctx.track_sequence(fr, s, cap, cap * 7)
            assert st == 0 and hnum == dnum and np.array_equal(hc, cnt) and np.array_equal(hnc, nc), what
            assert np.array_equal(ht.view(np.uint8), dt[:dnum].view(np.uint8)), what
            for t in range(7):
                m = cnt[t]
                assert np.array_equal(out[t, :m].view(np.int32).reshape(-1, 4), rec[t, :m]), (what, t)
                assert np.array_equal(hn[t, :m], dn[t, :m]) and np.array_equal(hi[t, :m], di[t, :m]), (what, t)
                assert (hn[t, m:] == -1).all() and (hi[t, m:] == -1).all(), (what, t)
        # a pair that does not fit and a table that does not fit: the first cap records of every pair are linked
        small = int(cnt.max()) // 2
        (rec, cnt2, nc), (dn, di, dt, dnum) = track_device(ctx, frames, s, small, 10)
        assert np.array_equal(cnt2, cnt)
        r = np.ascontiguousarray(rec).view(tu.CORR).reshape(7, small)
        same((dn, di, dt, dnum), tu.expected_arrays(r, cnt, W, H, FILL, 10), "capacity")
        out, hc, hnc, hn, hi, ht, hnum, st = ctx.track_sequence(frames, s, small, 10)
        assert st == g.capi.E_CAPACITY and hnum == dnum and np.array_equal(hc, cnt) and len(ht) == 10
        assert np.array_equal(ht.view(np.uint8), dt.view(np.uint8))
        for t in range(7):
            m = min(cnt[t], small)
            assert np.array_equal(hn[t, :m], dn[t, :m]) and np.array_equal(hi[t, :m], di[t, :m]), t


def test_refusals(forest_paths):
    import opengpc_amd as g
    import torch
    W, H = 96, 64
    frames = tu.frames_of(W, H, 3, 1)
    rec, counts = constructed(W, H, 2, 50, 64, 2)
    c = g.Context(0)
    try:
        # the records forms need no forest
        nxt, tid, rows, n, st = c.track_records(rec, counts, W, H)
        assert st == 0 and n == tu.restate(rec, counts, W, H)[3]
        with pytest.raises(g.GpcError) as e:   # the matching forms do
            c.track_sequence(frames, settings(True, False))
        assert e.value.status == g.capi.E_NO_FOREST
        dev = torch.device("cuda", 0)
        d_f = torch.from_numpy(frames).to(dev)
        d_rec = torch.zeros((2, 64, 4), dtype=torch.int32, device=dev)
        d_i = [torch.zeros((2, 64), dtype=torch.int32, device=dev) for _ in range(4)]
        torch.cuda.synchronize(dev)
        s = settings(True, False)
        L = c.L
        seq = lambda nframes=3, cap=64, corr=d_rec.data_ptr(), nx=d_i[1].data_ptr(), track_cap=64, tab=d_rec.data_ptr(): \
            L.gpc_hip_track_sequence_device(c.h, d_f.data_ptr(), W, H, nframes, C.byref(s), corr, cap, d_i[0].data_ptr(), None, nx,
                                            d_i[2].data_ptr(), tab, track_cap, d_i[3].data_ptr())
        recs = lambda npairs=2, cap=64, corr=d_rec.data_ptr(), nx=d_i[1].data_ptr(), track_cap=64, tab=d_rec.data_ptr(), w=W: \
            L.gpc_hip_track_records_device(c.h, corr, cap, d_i[0].data_ptr(), w, H, npairs, nx, d_i[2].data_ptr(), tab, track_cap,
                                           d_i[3].data_ptr())
        assert seq() == g.capi.E_NO_FOREST
        c.load_forest(forest_paths["zero"], W, H)
        assert seq() == 0 and recs() == 0
        c.synchronize()
        for call in (seq, recs):
            assert call(cap=0) == g.capi.E_INVALID and call(track_cap=-1) == g.capi.E_INVALID
            assert call(corr=None) == g.capi.E_INVALID and call(nx=None) == g.capi.E_INVALID
            assert call(tab=None) == g.capi.E_INVALID and call(tab=None, track_cap=0) == 0
        assert recs(npairs=0) == g.capi.E_INVALID and recs(w=0) == g.capi.E_INVALID and seq(nframes=1) == g.capi.E_INVALID
        c.synchronize()
        hrec = np.zeros((2, 64), g.CORR_DTYPE)
        hi = np.zeros((2, 64), np.int32)
        n = C.c_int32()
        assert L.gpc_hip_track_records(c.h, hrec.ctypes.data, 64, hi.ctypes.data, W, H, 0, hi.ctypes.data, hi.ctypes.data,
                                       hrec.ctypes.data, 64, C.byref(n)) == g.capi.E_INVALID
        with pytest.raises(g.GpcError) as e:   # frames of another size than the forest's
            c.track_sequence(np.zeros((3, 64, 112), np.uint8), s)
        assert e.value.status == g.capi.E_INVALID
        # group mode
        st, groups = g.read_forest_groups(os.path.join(ROOT, "forests", "stress16x20Forest.txt"), W, H)
        assert st == 0 and len(groups) == 16
        c.set_forest_groups(groups)
        with pytest.raises(g.GpcError) as e:
            c.track_sequence(frames, s)
        assert e.value.status == g.capi.E_UNSUPPORTED
        assert seq() == g.capi.E_UNSUPPORTED
        assert recs() == 0      # (records need no forest, so group mode does not concern them)
        c.synchronize()
    finally:
        c.close()


@pytest.mark.parametrize("lanes", [1, 2])
def test_batch_and_sequence_after_tracks(oracle, forest_paths, lanes):
    """An ordinary match_batch_device and a match_sequence right after track calls on the same context still equal the
    oracle (the pattern of test_batch_after_sequence)."""
    import opengpc_amd as g
    import torch
    from oracle.pyoracle import sparsematch_settings
    W, H, B = 320, 112, 4
    c = g.Context(0)
    try:
        c.load_forest(forest_paths["zero"], W, H)
        c.set_pipeline(lanes)
        rc, f = oracle.read_forest(forest_paths["zero"], W, H)
        pairs = [oracle.synth_pair(W, H, i, 9 + i) for i in range(B)]
        Lh = np.ascontiguousarray(np.stack([p[0] for p in pairs]))
        Rh = np.ascontiguousarray(np.stack([p[1] for p in pairs]))
        dev = torch.device("cuda", 0)
        cap = (W - 26) * (H - 26)
        d_L, d_R = torch.from_numpy(Lh).to(dev), torch.from_numpy(Rh).to(dev)
        frames = tu.frames_of(W, H, 6, 40)
        for epipolar in (True, False):
            track_device(c, frames, settings(False, False), cap, cap)     # tracks with the device-wide matcher ...
            c.track_sequence(frames, settings(True, False), cap)          # ... and with the epipolar join, host form
            d_out = torch.zeros((B, cap, 3), dtype=torch.int32, device=dev)
            d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
            d_nc = torch.zeros((B, 2), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            c.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, settings(epipolar, False), d_out.data_ptr(), cap,
                                 d_cnt.data_ptr(), d_nc.data_ptr())
            c.synchronize()
            cnt, nc = d_cnt.cpu().numpy(), d_nc.cpu().numpy()
            for p in range(B):
                want, nl, nr = oracle.match_pair(Lh[p], Rh[p], f, sparsematch_settings(5, 128, 0, epipolar))
                rec = d_out[p, :cnt[p]].cpu().numpy().copy().view(g.SUPPORT_DTYPE).reshape(-1)
                assert tuple(nc[p]) == (nl, nr) and cnt[p] == len(want), (epipolar, p)
                assert np.array_equal(rec, want.astype(rec.dtype)), (epipolar, p)
            out, hc, hnc, st = c.match_sequence(frames, settings(epipolar, False), cap)
            orec, ocnt, onc = tu.oracle_sequence(oracle, frames, f, epipolar, False)
            assert st == 0 and np.array_equal(hc, ocnt) and list(hnc) == onc
            for t in range(5):
                assert np.array_equal(out[t, :hc[t]].view(np.uint8), orec[t, :hc[t]].view(np.uint8)), (epipolar, t)
    finally:
        c.close()


def test_cpp_track_sequence(ctx, forest_paths, tmp_path):
    """Forest::trackSequence and gpc::tracking::trackRecords == the points of the Python result (FNV of the points)."""
    W, H, N = 160, 101, 8
    crops = {e: tu.frames_of(W, H, N, SEED[(W, H)], 0 if e else 12) for e in (True, False)}   # (as in test_match_and_track)
    for e in crops:
        (tmp_path / ("f%d.raw" % e)).write_bytes(crops[e].tobytes())
    out = os.path.join(ROOT, "tests", "cpp", "bin", "track_gpu_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "track_gpu_check.cpp"), "-o", out,
                           "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-pthread"])
    ctx.load_forest(forest_paths["tau"], W, H)
    for epipolar, hashtable, min_length in ((True, False, 1), (False, False, 3), (False, True, 2)):
        raw = str(tmp_path / ("f%d.raw" % epipolar))
        rec, cnt, nc, nxt, tid, rows, n, st = ctx.track_sequence(crops[epipolar], settings(epipolar, hashtable))
        assert st == 0 and n == len(rows)
        want = [t for t, row in zip(tu.track_points(rec, nxt, rows.tolist()), rows) if row["length"] >= min_length]
        assert len(want) > 0
        res = subprocess.run([out, forest_paths["tau"], str(W), str(H), str(N), raw, str(int(epipolar)),
                              str(int(hashtable)), str(min_length)], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        lines = {l.split()[0]: (int(l.split()[1]), int(l.split()[2])) for l in res.stdout.splitlines()
                 if l.split() and l.split()[0] in ("TRACKS", "RECORDS")}
        assert lines["TRACKS"] == lines["RECORDS"] == (len(want), tu.fnv_points(want)), (epipolar, hashtable, min_length)
