"""Track streams on the GPU (gpc_hip_track_stream_*): after any sequence of pushes everything delivered so far EQUALS, byte
for byte, what the offline calls return over the concatenated records or frames -- the plain restatement of the rule
(tests/track_util.py) for constructed records, match_sequence_device / track_sequence_device for frames.  prev is the
inverse of the offline next.  Every comparison is integer equality."""
import ctypes as C
import os

import numpy as np
import pytest

import track_util as tu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRESS = os.path.join(ROOT, "forests", "stress16x20Forest.txt")
MATCHERS = [(True, False), (False, False), (True, True), (False, True)]   # (epipolar_mode, use_hashtable)
FILL = -7
SEED = {(160, 101): 1, (1040, 77): 1}   # the frames_of seeds tests/test_gpu_tracks.py uses for these shapes


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def settings(epipolar, hashtable):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epipolar, hashtable, 1)


def dev():
    import torch
    return torch.device("cuda", 0)


def filled(shape, value=FILL):
    import torch
    return torch.full(shape, value, dtype=torch.int32, device=dev())


def constructed(W, H, P, per_pair, slots, seed, empty=None):
    """records [P, slots] and counts with the properties of test_gpu_tracks.constructed: the targets of pair t are drawn
    partly from the sources of pair t + 1, sources and targets repeat, some records lie outside the image, pair `empty` has
    count 0, and every slot beyond a pair's count holds a copy of one of the pair's valid records (which would link if it
    were read)"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((P, slots, 4), np.int32)
    counts = np.zeros(P, np.int32)
    for t in range(P - 1, -1, -1):
        m = int(per_pair * rng.uniform(0.8, 1.0))
        r = np.stack([rng.integers(0, W, m), rng.integers(0, H, m), rng.integers(0, W, m), rng.integers(0, H, m)], 1)
        if t + 1 < P:
            k = rng.random(m) < 0.6
            r[k, 2:] = rec[t + 1, rng.integers(0, slots, int(k.sum())), :2]
        d = rng.integers(0, m, m // 10)
        r[d, :2] = r[rng.integers(0, m, len(d)), :2]
        d = rng.integers(0, m, m // 10)
        r[d, 2:] = r[rng.integers(0, m, len(d)), 2:]
        for col, val in ((0, -1), (1, H), (2, W), (3, -3), (0, W + 5)):
            r[rng.integers(0, m, 3), col] = val
        rec[t, :m] = r
        rec[t, m:] = r[rng.integers(0, m, slots - m)]
        counts[t] = 0 if t == empty else m
    return rec.view(tu.CORR).reshape(P, slots), counts


def prev_of_next(nxt, P, cap, fill=FILL):
    """the inverse of the offline links as the array a stream leaves in outputs that held `fill`: nxt[t] lists of m_t ints"""
    a = np.full((P, cap), fill, np.int32)
    for t in range(P):
        a[t, :len(nxt[t])] = -1
        if t > 0:
            for i, j in enumerate(nxt[t - 1]):
                if j >= 0:
                    assert a[t, j] == -1
                    a[t, j] = i
    return a


def expected_prefix(rec, counts, W, H, Pp, track_cap):
    """(prev [Pp, cap], track_id [Pp, cap], the rows of the table that exist, n_tracks) of the restatement over Pp pairs"""
    r, c = np.ascontiguousarray(rec[:Pp]), counts[:Pp]
    nxt, tid, rows, n = tu.restate(r, c, W, H)
    _, b, tab, _ = tu.expected_arrays(r, c, W, H, FILL, track_cap)
    return prev_of_next(nxt, Pp, rec.shape[1]), b, tab[:min(n, track_cap)], n


def crossing(rows, split, min_len=3):
    """tracks of min_len records or more that have records on both sides of a boundary between two pushes of pairs"""
    bounds = np.cumsum(split)[:-1].tolist()
    return sum(1 for (t, i, length, last) in rows if length >= min_len and any(t < b <= t + length - 1 for b in bounds))


def stream_records(ctx, rec, counts, W, H, split, track_cap, what, check=True):
    """pushes the pairs in groups of `split` through a new stream; after every push the new pairs' prev and track_id, the
    table and the total equal the restatement over the prefix.  -> (prev, track_id) [P, cap] as the device holds them"""
    import torch
    P, cap = rec.shape
    assert sum(split) == P
    d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(P, cap, 4)).to(dev())
    d_cnt = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).to(dev())
    d_prev, d_id = filled((P, cap)), filled((P, cap))
    torch.cuda.synchronize(dev())
    s = ctx.track_stream(W, H, None, cap, track_cap)
    try:
        g = 0
        for k in split:
            s.push_records_device(d_rec[g:].data_ptr(), d_cnt[g:].data_ptr(), k, d_prev[g:].data_ptr(), d_id[g:].data_ptr())
            g += k
            assert s.state()[:2] == (0, g)
            if not check:
                continue
            prev, tid, tab, n = expected_prefix(rec, counts, W, H, g, track_cap)
            got_prev, got_id = d_prev.cpu().numpy(), d_id.cpu().numpy()
            assert np.array_equal(got_prev[:g], prev), (what, split, g, "prev")
            assert np.array_equal(got_id[:g], tid), (what, split, g, "track_id")
            assert (got_prev[g:] == FILL).all() and (got_id[g:] == FILL).all(), (what, split, g, "beyond the push")
            rows, total = s.read_tracks(0, track_cap, fill=FILL)
            assert total == n == s.state()[2], (what, split, g, total, n)
            assert np.array_equal(rows.view(np.uint8), tab.view(np.uint8)), (what, split, g, "table")
        return d_prev.cpu().numpy(), d_id.cpu().numpy()
    finally:
        s.close()


SPLITS7 = ([1, 1, 1, 1, 1, 1, 1], [3, 4], [2, 1, 4], [7])


def test_constructed_records_48x41():
    """7 pairs of a few hundred records (an empty pair, duplicates of both kinds, records outside the image, padding that
    would link) pushed as 7 x 1, 3 + 4, 2 + 1 + 4 and 7; then cap below the counts; then track_cap 0, one short, exact and
    with room.  The empty pair is pair 5, so that tracks of three records cross every boundary of every split."""
    import opengpc_amd as g
    W, H, P = 48, 41, 7
    rec, counts = constructed(W, H, P, 340, 400, 11, empty=5)
    assert counts[5] == 0 and counts.max() <= 400 and counts[[0, 1, 2, 3, 4, 6]].min() > 250
    c = g.Context(0)
    try:
        for what, r in (("fits", rec), ("cap < counts", np.ascontiguousarray(rec[:, :200]))):
            nxt, tid, rows, n = tu.restate(r, counts, W, H)
            assert n > 50 and max(row[2] for row in rows) >= 3
            for split in SPLITS7:
                assert len(split) == 1 or crossing(rows, split) >= 1, (what, split)
                stream_records(c, r, counts, W, H, split, n + 3, what)
            for track_cap in (0, n - 1, n):
                stream_records(c, r, counts, W, H, [2, 1, 4], track_cap, (what, track_cap))
    finally:
        c.close()


def test_more_than_one_chunk(ctx):
    """160x101, 4 pairs of about 5000 records in 5200 slots (three chunks of 2048, the last partial), pushed as 4 x 1 and
    2 + 2: head ranks and the running base across chunk and push boundaries"""
    W, H, P = 160, 101, 4
    rec, counts = constructed(W, H, P, 5190, 5200, 5)
    assert counts.min() > 4096 and counts.max() <= 5200
    n = tu.restate(rec, counts, W, H)[3]
    assert n > 2 * 2048
    for split in ([1, 1, 1, 1], [2, 2]):
        stream_records(ctx, rec, counts, W, H, split, n, "5k")
    stream_records(ctx, rec, counts, W, H, [2, 2], 100, "5k, short table")


def offline(ctx, frames, s, cap, track_cap):
    """match_sequence_device and track_sequence_device over all frames -> (records, counts, ncand) of the first, (records,
    counts, ncand, next, track_id, table rows that exist, n_tracks) of the second"""
    import torch
    N, H, W = frames.shape
    d_f = torch.from_numpy(frames).to(dev())
    res = []
    for tracks in (False, True):
        d_out = filled((N - 1, cap, 4))
        d_cnt = torch.zeros(N - 1, dtype=torch.int32, device=dev())
        d_nc = torch.zeros(N, dtype=torch.int32, device=dev())
        torch.cuda.synchronize(dev())
        if not tracks:
            ctx.match_sequence_device(d_f.data_ptr(), W, H, N, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
            ctx.synchronize()
            res.append((d_out.cpu().numpy(), d_cnt.cpu().numpy(), d_nc.cpu().numpy()))
            continue
        d_next, d_id, d_tab, d_n = filled((N - 1, cap)), filled((N - 1, cap)), filled((max(track_cap, 1), 4)), filled((1,))
        ctx.track_sequence_device(d_f.data_ptr(), W, H, N, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr(),
                                  d_next.data_ptr(), d_id.data_ptr(), d_tab.data_ptr(), track_cap, d_n.data_ptr())
        ctx.synchronize()
        n = int(d_n.cpu().numpy()[0])
        res.append((d_out.cpu().numpy(), d_cnt.cpu().numpy(), d_nc.cpu().numpy(), d_next.cpu().numpy(), d_id.cpu().numpy(),
                    d_tab.cpu().numpy()[:min(n, track_cap)].copy(), n))
    return res


def prev_of_next_array(nxt, cnt, cap):
    P = len(cnt)
    lists = [nxt[t, :min(max(int(cnt[t]), 0), cap)].tolist() for t in range(P)]
    return prev_of_next(lists, P, cap)


def stream_frames(ctx, stream, frames, split, cap, between=None):
    """pushes the frames in groups of `split` -> (records [N-1, cap, 4], counts, ncand [N], prev, track_id) as the device
    holds them after the last push, outputs that held FILL (0 for the counts) everywhere"""
    import torch
    N, H, W = frames.shape
    assert sum(split) == N
    d_f = torch.from_numpy(frames).to(dev())
    d_out, d_prev, d_id = filled((N - 1, cap, 4)), filled((N - 1, cap)), filled((N - 1, cap))
    d_cnt = torch.zeros(N - 1, dtype=torch.int32, device=dev())
    d_nc = torch.zeros(N, dtype=torch.int32, device=dev())
    torch.cuda.synchronize(dev())
    f = 0
    for nf in split:
        g = max(f - 1, 0)
        k = stream.push_device(d_f[f:].data_ptr(), nf, d_out[g:].data_ptr() if g < N - 1 else d_out.data_ptr(),
                               d_cnt[g:].data_ptr() if g < N - 1 else d_cnt.data_ptr(), d_nc[f:].data_ptr(),
                               d_prev[g:].data_ptr() if g < N - 1 else d_prev.data_ptr(),
                               d_id[g:].data_ptr() if g < N - 1 else d_id.data_ptr())
        assert k == (nf if f else nf - 1)
        f += nf
        if between:
            between()
    ctx.synchronize()
    return d_out.cpu().numpy(), d_cnt.cpu().numpy(), d_nc.cpu().numpy(), d_prev.cpu().numpy(), d_id.cpu().numpy()


def check_frames(ctx, frames, s, splits, min_crossing=0, between=None):
    N, H, W = frames.shape
    cap = (W - 26) * (H - 26)
    track_cap = cap * (N - 1)
    (rec, cnt, nc), (rec2, cnt2, nc2, nxt, tid, tab, n) = offline(ctx, frames, s, cap, track_cap)
    assert n > 0 and cnt.min() > 0
    prev = prev_of_next_array(nxt, cnt2, cap)
    for split in splits:
        if min_crossing:   # on the OFFLINE result: the frames' split as a split of pairs
            pairs = [k for k in ([split[0] - 1] + list(split[1:])) if k > 0]
            assert len(pairs) == 1 or crossing(tab.tolist(), pairs) >= min_crossing, split
        st = ctx.track_stream(W, H, s, cap, track_cap)
        try:
            got = stream_frames(ctx, st, frames, split, cap, between)
            assert np.array_equal(got[1], cnt) and np.array_equal(got[2], nc), split
            assert np.array_equal(got[0].view(np.uint8), rec.view(np.uint8)), split     # padding included
            assert np.array_equal(got[3], prev), (split, "prev")
            assert np.array_equal(got[4], tid), (split, "track_id")
            rows, total = st.read_tracks(0, track_cap, fill=FILL)
            assert total == n and st.state() == (N, N - 1, n)
            assert np.array_equal(rows.view(np.int32).reshape(-1, 4), tab), (split, "table")
        finally:
            st.close()
    return tab, n


SPLITS6 = ([1, 1, 1, 1, 1, 1], [2, 4], [6])


@pytest.mark.parametrize("epipolar,hashtable", MATCHERS)
def test_frames_160x101(ctx, forest_paths, epipolar, hashtable):
    """6 translated crops (the seed of test_gpu_tracks.py; full vertical overlap for the epipolar matchers, as there),
    pushed as 6 x 1, 2 + 4 and 6: records, counts and candidate counts are match_sequence_device's, ids, prev and the table
    track_sequence_device's"""
    W, H = 160, 101
    frames = tu.frames_of(W, H, 6, SEED[(W, H)], 0 if epipolar else 12)
    ctx.load_forest(forest_paths["zero"], W, H)
    check_frames(ctx, frames, settings(epipolar, hashtable), SPLITS6)


def test_frames_1040x77_epipolar_long_tracks(ctx, forest_paths):
    """dy = 0, epipolar sort matcher: tracks run through several pairs.  On the offline result, tracks of three records
    and more cross a push boundary in every split (seed 1, the one test_gpu_tracks.py uses for this shape)."""
    W, H = 1040, 77
    frames = tu.frames_of(W, H, 6, SEED[(W, H)], 0)
    ctx.load_forest(forest_paths["zero"], W, H)
    check_frames(ctx, frames, settings(True, False), SPLITS6, min_crossing=1)


@pytest.mark.parametrize("epipolar", [True, False])
def test_frames_naive_32_tests(forest_paths, epipolar):
    """SSE=OFF arithmetic with the stress forest's first 32 tests: the joins read the candidate BYTES of the left image,
    which the stream carries for the last frame"""
    import opengpc_amd as g
    W, H = 160, 101
    frames = tu.frames_of(W, H, 6, SEED[(W, H)], 0 if epipolar else 12)
    c = g.Context(0)
    try:
        c.set_arithmetic(True)
        st, fm = g.read_forest(STRESS, W, H)
        assert st == 0 and fm.num_tests == 32
        c.set_forest(fm)
        check_frames(c, frames, settings(epipolar, False), SPLITS6)
    finally:
        c.close()


def test_every_frame_hashed_once(forest_paths):
    """six single-frame pushes launch k_preprocess and k_hash six times each (overlapping offline windows would need ten)"""
    import opengpc_amd as g
    import torch
    W, H = 160, 101
    frames = tu.frames_of(W, H, 6, SEED[(W, H)], 0)
    cap = (W - 26) * (H - 26)
    c = g.Context(0)
    try:
        c.load_forest(forest_paths["zero"], W, H)
        st = c.track_stream(W, H, settings(True, False), cap, 16)
        c.enable_kernel_timing(True)
        c.reset_kernel_timing()
        stream_frames(c, st, frames, [1] * 6, cap)
        times = c.kernel_times()
        assert times["k_preprocess"][1] == 6 and times["k_hash"][1] == 6, times
        assert times["k_trs_walk"][1] == 5 and times["k_trs_save"][1] == 5 and times["k_track_walk"][1] == 0, times
        torch.cuda.synchronize(dev())
    finally:
        c.close()


def test_isolation(ctx, forest_paths):
    """Between the pushes a match_batch_device of another size and an offline track_records_device run on the same
    context; two streams interleaved on one context each equal their own offline result."""
    import torch
    W, H = 160, 101
    frames = tu.frames_of(W, H, 6, SEED[(W, H)], 12)
    ctx.load_forest(forest_paths["zero"], W, H)
    B, cap = 3, (W - 26) * (H - 26)
    d_L = torch.from_numpy(tu.frames_of(W, H, B, 7)).to(dev())
    d_R = torch.from_numpy(tu.frames_of(W, H, B, 8)).to(dev())
    d_out = torch.zeros((B, cap, 3), dtype=torch.int32, device=dev())
    d_cnt, d_nc = torch.zeros(B, dtype=torch.int32, device=dev()), torch.zeros((B, 2), dtype=torch.int32, device=dev())
    rec, counts = constructed(W, H, 3, 900, 1000, 9)
    d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(3, 1000, 4)).to(dev())
    d_c = torch.from_numpy(counts).to(dev())
    d_a, d_b, d_t, d_n = filled((3, 1000)), filled((3, 1000)), filled((64, 4)), filled((1,))
    torch.cuda.synchronize(dev())

    def other_work():
        ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, settings(True, False), d_out.data_ptr(), cap,
                               d_cnt.data_ptr(), d_nc.data_ptr())
        ctx.track_records_device(d_rec.data_ptr(), 1000, d_c.data_ptr(), W, H, 3, d_a.data_ptr(), d_b.data_ptr(), d_t.data_ptr(), 64,
                                 d_n.data_ptr())

    for epipolar in (True, False):
        fr = tu.frames_of(W, H, 6, SEED[(W, H)], 0 if epipolar else 12)
        check_frames(ctx, fr, settings(epipolar, False), ([1, 1, 1, 1, 1, 1], [2, 4]), between=other_work)
    # two streams, interleaved: one of frames, one of records
    s = settings(False, False)
    (r0, cnt, nc), (r1, c1, n1, nxt, tid, tab, n) = offline(ctx, frames, s, cap, cap * 5)
    P = 5
    rec5, counts5 = constructed(W, H, P, 900, 1000, 10)
    want = expected_prefix(rec5, counts5, W, H, P, 4000)
    d_rec5 = torch.from_numpy(np.ascontiguousarray(rec5).view(np.int32).reshape(P, 1000, 4)).to(dev())
    d_c5 = torch.from_numpy(counts5).to(dev())
    d_p5, d_i5 = filled((P, 1000)), filled((P, 1000))
    torch.cuda.synchronize(dev())
    sa, sb = ctx.track_stream(W, H, s, cap, cap * 5), ctx.track_stream(W, H, None, 1000, 4000)
    try:
        g = [0]

        def push_b():
            if g[0] < P:
                sb.push_records_device(d_rec5[g[0]:].data_ptr(), d_c5[g[0]:].data_ptr(), 1, d_p5[g[0]:].data_ptr(),
                                       d_i5[g[0]:].data_ptr())
                g[0] += 1

        got = stream_frames(ctx, sa, frames, [1] * 6, cap, between=push_b)
        assert g[0] == P
        assert np.array_equal(got[0].view(np.uint8), r0.view(np.uint8)) and np.array_equal(got[1], cnt)
        assert np.array_equal(got[3], prev_of_next_array(nxt, cnt, cap)) and np.array_equal(got[4], tid)
        rows, total = sa.read_tracks(0, cap * 5, fill=FILL)
        assert total == n and np.array_equal(rows.view(np.int32).reshape(-1, 4), tab)
        assert np.array_equal(d_p5.cpu().numpy(), want[0]) and np.array_equal(d_i5.cpu().numpy(), want[1])
        rows, total = sb.read_tracks(0, 4000, fill=FILL)
        assert total == want[3] and np.array_equal(rows.view(np.uint8), want[2].view(np.uint8))
    finally:
        sa.close()
        sb.close()


def test_lifecycle_and_refusals(forest_paths):
    import opengpc_amd as g
    import torch
    E = g.capi
    W, H, N = 96, 64, 4
    cap = (W - 26) * (H - 26)
    frames = tu.frames_of(W, H, N, 1, 0)
    rec, counts = constructed(W, H, 3, 50, 64, 2)
    c, c2 = g.Context(0), g.Context(0)
    try:
        L = c.L
        s = settings(True, False)
        d_f = torch.from_numpy(frames).to(dev())
        d_out, d_prev, d_id = filled((N, cap, 4)), filled((N, cap)), filled((N, cap))
        d_cnt = torch.zeros(N, dtype=torch.int32, device=dev())
        d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(3, 64, 4)).to(dev())
        d_c = torch.from_numpy(counts).to(dev())
        torch.cuda.synchronize(dev())
        k = C.c_int(-5)
        h = C.c_void_p()
        # create
        assert L.gpc_hip_track_stream_create(None, W, H, C.byref(s), cap, 8, C.byref(h)) == E.E_INVALID
        assert L.gpc_hip_track_stream_create(c.h, W, H, C.byref(s), cap, 8, None) == E.E_INVALID
        for bad in ((0, H, cap, 8), (W, 0, cap, 8), (W, H, 0, 8), (W, H, cap, -1)):
            assert L.gpc_hip_track_stream_create(c.h, bad[0], bad[1], C.byref(s), bad[2], bad[3], C.byref(h)) == E.E_INVALID
        assert L.gpc_hip_track_stream_create(c.h, W, H, C.byref(g.Settings(300)), cap, 8, C.byref(h)) == E.E_INVALID
        st = c.track_stream(W, H, s, cap, 4 * cap)

        def push(nf=1, f0=0, stream=None, ctx_h=None, fr=True, out=True, npairs=True):
            return L.gpc_hip_track_stream_push_device(ctx_h or c.h, None if stream == 0 else (stream or st.h), d_f[f0:].data_ptr() if fr else None, nf,
                                                      d_out.data_ptr() if out else None, d_cnt.data_ptr(), None,
                                                      d_prev.data_ptr(), d_id.data_ptr(), C.byref(k) if npairs else None)

        assert push() == E.E_NO_FOREST and st.state() == (0, 0, 0)
        c.load_forest(forest_paths["zero"], W, H)
        c2.load_forest(forest_paths["zero"], W, H)
        assert push(nf=0) == E.E_INVALID and push(fr=False) == E.E_INVALID and push(out=False) == E.E_INVALID
        assert push(npairs=False) == E.E_INVALID and push(ctx_h=c2.h) == E.E_INVALID and push(stream=0) == E.E_INVALID
        assert st.state() == (0, 0, 0) and k.value == -5
        # a first push of one frame is valid and yields no pair
        assert push() == 0 and k.value == 0 and st.state() == (1, 0, 0)
        assert push(nf=2, f0=1) == 0 and k.value == 2
        f_seen, p_seen, n2 = st.state()
        assert (f_seen, p_seen) == (3, 2) and n2 > 0
        first_ids = d_id.cpu().numpy()[:2].copy()
        first_rows = st.read_tracks(0, n2)[0].copy()
        # records into a stream of frames
        assert L.gpc_hip_track_stream_push_records_device(c.h, st.h, d_rec.data_ptr(), d_c.data_ptr(), 1, d_prev.data_ptr(),
                                                          d_id.data_ptr()) == E.E_INVALID
        # another forest between two pushes: refused, nothing changed, until reset
        c.load_forest(forest_paths["tau"], W, H)
        assert push(f0=3) == E.E_INVALID and st.state() == (3, 2, n2)
        c.load_forest(forest_paths["zero"], W, H)        # (the forest it was: still another generation)
        assert push(f0=3) == E.E_INVALID and st.state() == (3, 2, n2)
        c.set_arithmetic(True)
        c.set_arithmetic(False)
        assert push(f0=3) == E.E_INVALID
        # read_tracks beyond the table
        n = C.c_int32(-1)
        row = np.zeros((4, 4), np.int32)
        assert L.gpc_hip_track_stream_read_tracks(c.h, st.h, 4 * cap - 1, 2, row.ctypes.data, C.byref(n)) == E.E_CAPACITY
        assert n.value == n2
        assert L.gpc_hip_track_stream_read_tracks(c.h, st.h, -1, 2, row.ctypes.data, C.byref(n)) == E.E_INVALID
        assert L.gpc_hip_track_stream_read_tracks(c.h, st.h, 0, 2, None, C.byref(n)) == E.E_INVALID
        # reset: ids restart at 0 and the first run comes again
        st.reset()
        assert st.state() == (0, 0, 0)
        d_id.fill_(FILL)
        torch.cuda.synchronize(dev())
        assert push(nf=3) == 0 and k.value == 2
        assert st.state() == (3, 2, n2) and np.array_equal(d_id.cpu().numpy()[:2], first_ids)
        assert np.array_equal(st.read_tracks(0, n2)[0], first_rows)
        tab, tot = st.table()
        assert tab and tot
        # group mode
        stg, groups = g.read_forest_groups(STRESS, W, H)
        c.set_forest_groups(groups)
        assert push(f0=3) == E.E_UNSUPPORTED
        st.reset()
        assert push(nf=2) == E.E_UNSUPPORTED and st.state() == (0, 0, 0)
        # a stream of records needs neither forest nor settings, and takes no frames
        sr = c.track_stream(W, H, None, 64, 16)
        assert push(stream=sr.h) == E.E_INVALID
        sr.push_records_device(d_rec.data_ptr(), d_c.data_ptr(), 2, d_prev.data_ptr(), d_id.data_ptr())
        assert sr.state()[:2] == (0, 2)
        c.load_forest(forest_paths["zero"], W, H)
        assert push(stream=sr.h) == E.E_INVALID      # frames into a stream of records
        assert L.gpc_hip_track_stream_push_records_device(c.h, sr.h, d_rec.data_ptr(), d_c.data_ptr(), 0, d_prev.data_ptr(),
                                                          d_id.data_ptr()) == E.E_INVALID
        assert L.gpc_hip_track_stream_push_records_device(c.h, sr.h, None, d_c.data_ptr(), 1, d_prev.data_ptr(),
                                                          d_id.data_ptr()) == E.E_INVALID
        assert sr.state()[:2] == (0, 2)
        # the per-push limits of the offline form, checked before anything is touched: 65535 pairs, and one fewer once a
        # pair is carried (the window holds it too: one grid row per pair of the window)
        for k_big in (65536, 65535):
            assert L.gpc_hip_track_stream_push_records_device(c.h, sr.h, d_rec.data_ptr(), d_c.data_ptr(), k_big, d_prev.data_ptr(),
                                                              d_id.data_ptr()) == E.E_UNSUPPORTED
        assert sr.state()[:2] == (0, 2)
        # a destroyed stream
        hs = sr.h
        sr.close()
        assert L.gpc_hip_track_stream_destroy(c.h, hs) == E.E_INVALID
        assert L.gpc_hip_track_stream_reset(c.h, hs) == E.E_INVALID
        assert L.gpc_hip_track_stream_state(c.h, hs, None, None, None) == E.E_INVALID
        assert L.gpc_hip_track_stream_destroy(c2.h, st.h) == E.E_INVALID
        st.close()
        c.synchronize()
    finally:
        c.close()
        c2.close()


def test_id_bound_refusal(ctx):
    """Track ids are 31 bits: the host's bound on the total grows by k * min(cap, W * H) per push and a push that could pass
    2^31 - 1 is refused with the stream left as it was.  A records stream of 256x128 with cap = 2^15 (= W * H) is pushed 64
    EMPTY pairs at a time, so the bound grows by 2^21 per push while nothing is read or written beyond the counts: 1023
    pushes are accepted (bound 2^31 - 2^21), the 1024th would reach 2^31 and is refused.  _state reads the true total (0)
    back, which tightens the bound, so the next push is accepted; and a pair of real records pushed after all that gets
    the ids, links and rows the restatement gives, at its global pair index.  About 25 MB of workspace, 7000 short launches."""
    import opengpc_amd as g
    import torch
    W, H, cap, k = 256, 128, 1 << 15, 64
    assert min(cap, W * H) * k == 1 << 21
    d_cnt = torch.zeros(k, dtype=torch.int32, device=dev())
    d_small = filled((1, 64))                     # (records, prev and ids of empty pairs are never touched)
    rec, counts = constructed(W, H, 1, 3000, cap, 31)
    d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(1, cap, 4)).to(dev())
    d_c1 = torch.from_numpy(counts).to(dev())
    d_prev, d_id = filled((1, cap)), filled((1, cap))
    torch.cuda.synchronize(dev())
    s = ctx.track_stream(W, H, None, cap, 4096)
    try:
        L = ctx.L
        push = lambda: L.gpc_hip_track_stream_push_records_device(ctx.h, s.h, d_small.data_ptr(), d_cnt.data_ptr(), k,
                                                                  d_small.data_ptr(), d_small.data_ptr())
        for i in range(1023):
            assert push() == 0, i
        assert push() == g.capi.E_UNSUPPORTED          # 1024 * 2^21 = 2^31 > 2^31 - 1
        assert push() == g.capi.E_UNSUPPORTED
        assert s.state() == (0, 1023 * k, 0)           # nothing changed; the true total tightens the bound to 0 ...
        assert (d_small.cpu().numpy() == FILL).all()
        assert push() == 0 and s.state() == (0, 1024 * k, 0)      # ... so the next push is accepted
        s.push_records_device(d_rec.data_ptr(), d_c1.data_ptr(), 1, d_prev.data_ptr(), d_id.data_ptr())
        nxt, tid, rows, n = tu.restate(rec, counts, W, H)
        assert s.state() == (0, 1024 * k + 1, n) and n == counts[0]
        m = int(counts[0])
        got_prev, got_id = d_prev.cpu().numpy()[0], d_id.cpu().numpy()[0]
        assert (got_prev[:m] == -1).all() and np.array_equal(got_id[:m], np.array(tid[0], np.int32))
        assert (got_prev[m:] == FILL).all() and (got_id[m:] == FILL).all()
        got_rows, total = s.read_tracks(0, 4096, fill=FILL)
        want = np.array([(1024 * k + t, i, length, last) for (t, i, length, last) in rows[:4096]], np.int32)
        assert total == n and np.array_equal(got_rows.view(np.int32).reshape(-1, 4), want)
    finally:
        s.close()


def test_host_form_equals_device_form(ctx, forest_paths):
    """pageable and page-locked frames and outputs; GPC_E_CAPACITY with a small cap"""
    import opengpc_amd as g
    W, H, N = 160, 101, 6
    ctx.load_forest(forest_paths["zero"], W, H)
    pf = ctx.pinned_empty((N, H, W), np.uint8)
    for epipolar, hashtable in ((True, False), (False, True)):
        frames = tu.frames_of(W, H, N, SEED[(W, H)], 0 if epipolar else 12)
        pf[...] = frames
        s = settings(epipolar, hashtable)
        full = (W - 26) * (H - 26)
        cnt0 = offline(ctx, frames, s, full, 1)[0][1]
        for cap, status in ((full, 0), (int(cnt0.max()) // 2, g.capi.E_CAPACITY)):
            (rec, cnt, nc), (r1, c1, n1, nxt, tid, tab, n) = offline(ctx, frames, s, cap, cap * (N - 1))
            prev = prev_of_next_array(nxt, cnt, cap)
            for what, fr, alloc in (("pageable", frames, None), ("page-locked", pf, ctx.pinned_empty)):
                st = ctx.track_stream(W, H, s, cap, cap * (N - 1))
                try:
                    f = g0 = 0
                    for nf in (1, 2, 3):
                        out, hc, hnc, hp, hi, total, code = st.push(fr[f:f + nf], fill=FILL, alloc=alloc)
                        k = nf if f else nf - 1
                        assert len(hc) == k and code == (status if k and (cnt[g0:g0 + k] > cap).any() else 0), (what, cap, f)
                        assert np.array_equal(hc, cnt[g0:g0 + k]) and np.array_equal(hnc, nc[f:f + nf]), (what, cap, f)
                        for t in range(k):
                            m = min(int(cnt[g0 + t]), cap)
                            assert np.array_equal(out[t, :m].view(np.int32).reshape(-1, 4), rec[g0 + t, :m]), (what, cap, f, t)
                        assert np.array_equal(hp, prev[g0:g0 + k]) and np.array_equal(hi, tid[g0:g0 + k]), (what, cap, f)
                        f += nf
                        g0 += k
                        assert total == st.state()[2]
                    rows, total = st.read_tracks(0, cap * (N - 1), fill=FILL)
                    assert total == n and np.array_equal(rows.view(np.int32).reshape(-1, 4), tab), (what, cap)
                finally:
                    st.close()
