"""The host forms of scoring, tracks and filtering share ONE staging block and one upload path (gpc_hip.hip: Stage).  Each host
form here is held equal to its device form on the same inputs, byte for byte, fill bytes and status included, where the
sharing can go wrong: the block grown and reused across features on one context, and a pageable upload longer than the
pieces of the page-locked arena (32 MiB each) whose piece boundaries lie inside a pair."""
import numpy as np
import pytest

import consensus_util as cu
import track_util as tu

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL32 = int(np.array([FILL] * 4, np.uint8).view(np.int32)[0])
THR = [0.5, 1.0, 3.0]


@pytest.fixture(scope="module")
def dctx():
    """the context of the device forms (the host forms under test run on a context of their own)"""
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def filled(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def host_filled(shape, dtype, alloc=np.empty):
    a = alloc(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def special_counts(P, slots, seed):
    """counts near the slots; pair 0 above them, pair 1 negative, pair 2 (where there is one) zero"""
    c = np.random.default_rng(seed).integers(slots * 4 // 5, slots + 1, P).astype(np.int32)
    c[0], c[1] = slots + 7, -3
    if P > 2:
        c[2] = 0
    return c


def constructed(W, H, P, slots, seed):
    """correspondences [P, slots] of tu.CORR, every slot filled, without a loop over records: half of them move by
    (+16, +8), a sixth by (+9, -5), the rest anywhere; half of a pair's targets are sources of the next pair (chains); a few
    lie outside the image"""
    rng = np.random.default_rng(seed)
    sx, sy = rng.integers(0, W, (P, slots)), rng.integers(0, H, (P, slots))
    how = rng.random((P, slots))
    tx = sx + np.where(how < 0.5, 16, np.where(how < 0.67, 9, rng.integers(-W, W, (P, slots))))
    ty = sy + np.where(how < 0.5, 8, np.where(how < 0.67, -5, rng.integers(-H, H, (P, slots))))
    if P > 1:
        k, idx = rng.random((P - 1, slots)) < 0.5, rng.integers(0, slots, (P - 1, slots))
        tx[:-1][k], ty[:-1][k] = np.take_along_axis(sx[1:], idx, 1)[k], np.take_along_axis(sy[1:], idx, 1)[k]
    sx[rng.random((P, slots)) < 0.001] = -1
    ty[rng.random((P, slots)) < 0.001] = H
    rec = np.empty((P, slots), tu.CORR)
    rec["src_x"], rec["src_y"], rec["tar_x"], rec["tar_y"] = sx, sy, tx, ty
    return rec


def tracks_equal(hctx, dctx, rec, counts, W, H, track_cap, what, alloc_rec=np.empty):
    """gpc_hip_track_records == gpc_hip_track_records_device, outputs that held FILL everywhere"""
    import opengpc_amd as g
    import torch
    P, cap = rec.shape
    d_rec, d_cnt = dev(rec.view(np.int32).reshape(P, cap, 4)), dev(counts)
    d_next, d_id, d_tab, d_n = filled(P, cap, 4), filled(P, cap, 4), filled(track_cap, 16), filled(4)
    torch.cuda.synchronize()
    dctx.track_records_device(d_rec.data_ptr(), cap, d_cnt.data_ptr(), W, H, P, d_next.data_ptr(), d_id.data_ptr(),
                              d_tab.data_ptr(), track_cap, d_n.data_ptr())
    dctx.synchronize()
    dnum = int(d_n.cpu().numpy().view(np.int32)[0])
    want = g.capi.E_CAPACITY if (counts > cap).any() or dnum > track_cap else 0
    hrec = alloc_rec(rec.shape, rec.dtype)
    hrec[...] = rec
    nxt, tid, tab = host_filled((P, cap), np.int32), host_filled((P, cap), np.int32), host_filled((track_cap,), g.TRACK_DTYPE)
    _, _, _, hnum, st = hctx.track_records(hrec, counts.copy(), W, H, track_cap, nxt, tid, tab)
    print(what, "tracks", dnum, "status", st)
    assert st == want and hnum == dnum, (what, st, want, hnum, dnum)
    assert dnum > 0 and (nxt != FILL32).any()
    for name, h, d in (("next", nxt, d_next), ("track_id", tid, d_id), ("table", tab, d_tab)):
        assert np.array_equal(h.view(np.uint8).reshape(-1), d.cpu().numpy().reshape(-1)), (what, name)


def consensus_equal(hctx, dctx, rec, counts, W, H, cap_out, what):
    import opengpc_amd as g
    import torch
    P, cap = rec.shape
    prm = g.Consensus(8, 4, 3, 1)
    d_rec, d_cnt = dev(rec.view(np.uint8).reshape(P, cap, 16)), dev(counts)
    d_keep, d_out, d_idx, d_n = filled(P, cap), filled(P, cap_out, 16), filled(P, cap_out, 4), filled(P, 4)
    torch.cuda.synchronize()
    dctx.consensus_records_device(d_rec.data_ptr(), True, cap, d_cnt.data_ptr(), W, H, P, prm, d_keep.data_ptr(), d_out.data_ptr(),
                                  cap_out, d_idx.data_ptr(), d_n.data_ptr())
    dctx.synchronize()
    dn = d_n.cpu().numpy().view(np.int32).reshape(P)
    want = g.capi.E_CAPACITY if (dn > cap_out).any() else 0
    keep, out, idx = host_filled((P, cap), np.uint8), host_filled((P, cap_out), cu.CORR), host_filled((P, cap_out), np.int32)
    _, _, _, hn, st = hctx.consensus_records(rec.copy(), counts.copy(), W, H, prm, cap_out, keep, out, idx)
    print(what, "kept", dn.tolist(), "status", st)
    assert st == want and np.array_equal(hn, dn), (what, st, want)
    assert dn.max() > 0
    for name, h, d in (("keep", keep, d_keep), ("out", out, d_out), ("index", idx, d_idx)):
        assert np.array_equal(h.view(np.uint8).reshape(-1), d.cpu().numpy().reshape(-1)), (what, name)


def truth_planes(P, W, H, seed):
    rng = np.random.default_rng(seed)
    u = np.where(rng.random((P, H, W)) < 0.7, 16, rng.integers(-8, 9, (P, H, W))).astype(np.float32)
    v = np.where(rng.random((P, H, W)) < 0.7, 8, rng.integers(-8, 9, (P, H, W))).astype(np.float32)
    v[rng.random((P, H, W)) < 0.05] = np.float32(-1e10)
    return u, v, (rng.random((P, H, W)) < 0.1).astype(np.uint8)


def scores_equal(hctx, dctx, rec, counts, W, H, what):
    import opengpc_amd as g
    import torch
    P, cap = rec.shape
    u, v, ign = truth_planes(P, W, H, 5)
    d_rec, d_cnt, d_u, d_v, d_i = dev(rec.view(np.int32).reshape(P, cap, 4)), dev(counts), dev(u), dev(v), dev(ign)
    d_sc = filled(P, 120)
    torch.cuda.synchronize()
    dctx.score_correspondences_device(d_rec.data_ptr(), cap, d_cnt.data_ptr(), W, H, P, d_u.data_ptr(), d_v.data_ptr(), d_i.data_ptr(),
                                      THR, d_sc.data_ptr())
    dctx.synchronize()
    want = d_sc.cpu().numpy().copy().view(g.SCORE_DTYPE).reshape(-1)
    got = hctx.score_records(rec.copy(), counts.copy(), u, v, ign, THR)
    print(what, "judged", want["n_judged"].tolist())
    assert got.tobytes() == want.tobytes(), what
    assert want["n_judged"].max() > 0 and want["n_within"].max() > 0
    assert (want["n_records"] == np.clip(counts, 0, cap)).all()


def test_one_block_grown_and_reused_across_features(dctx, forest_paths):
    """filtering 48x41 x 3, tracks 160x101 x 17, scores 48x41 x 17 (two chunks), score_batch 96x64 x 3, filtering 160x101 x 17
    (two chunks), tracks 48x41 x 2 on ONE context, every array pageable: the sizes rise and fall, so a layout computed
    against the previous owner's block, or a stale offset, would show.  Every records call has a pair with a count above
    its capacity, one with a negative count and (but the last, which has two pairs) one with count 0."""
    import opengpc_amd as g
    import torch
    small, large = (48, 41, 400), (160, 101, 3000)
    h = g.Context(0)
    try:
        W, H, slots = small
        consensus_equal(h, dctx, constructed(W, H, 3, slots, 1), special_counts(3, slots, 1), W, H, slots, "filter 48x41 x 3")
        W, H, slots = large
        tracks_equal(h, dctx, constructed(W, H, 17, slots, 2), special_counts(17, slots, 2), W, H, 17 * slots, "tracks 160x101 x 17")
        W, H, slots = small
        scores_equal(h, dctx, constructed(W, H, 17, slots, 3), special_counts(17, slots, 3), W, H, "scores 48x41 x 17")
        W, H = 96, 64
        frames = tu.frames_of(W, H, 4, 1, 0)
        L, R = np.ascontiguousarray(frames[:3]), np.ascontiguousarray(frames[1:])
        u, _, ign = truth_planes(3, W, H, 6)
        u[...] = np.where(ign, u, -4)        # (the crops move left by 1 .. 7 pixels; any truth will do for equality)
        s = g.Settings(5, 128, 0, True, False, 1)
        for c in (h, dctx):
            c.load_forest(forest_paths["zero"], W, H)
        d_L, d_R, d_u, d_i, d_sc = dev(L), dev(R), dev(u), dev(ign), filled(3, 120)
        torch.cuda.synchronize()
        dctx.score_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, 3, s, d_u.data_ptr(), d_i.data_ptr(), THR, d_sc.data_ptr())
        dctx.synchronize()
        want = d_sc.cpu().numpy().copy().view(g.SCORE_DTYPE).reshape(-1)
        assert h.score_batch(L, R, s, u, ign, THR).tobytes() == want.tobytes()
        assert want["n_records"].min() > 0 and want["n_candidates"].min() > 0
        W, H, slots = large
        consensus_equal(h, dctx, constructed(W, H, 17, slots, 4), special_counts(17, slots, 4), W, H, slots // 2, "filter 160x101 x 17")
        W, H, slots = small
        tracks_equal(h, dctx, constructed(W, H, 2, slots, 5), special_counts(2, slots, 5), W, H, 2 * slots, "tracks 48x41 x 2")
    finally:
        h.close()


def test_pageable_upload_longer_than_one_arena_piece(dctx):
    """track_records over 6 pairs of 1024x436 with 4 758 927 valid records of 16 bytes, 76 MB: more than the two pieces of
    32 MiB (2 097 152 records each) that the arena has for a call's pageable uploads.  No prefix sum of the pairs' records
    (799 989, 1 589 988, 2 389 988, 3 186 989, 3 978 928) is a multiple of a piece, nor two records short of one (the counts
    go up first and take 32 bytes), so the first piece fills inside pair 2 and the second inside pair 5, whose rest goes
    into the FIRST piece again, behind the event of the copies that read it.  Every array pageable; then the records
    page-locked, which pass the arena by."""
    W, H, P, cap = 1024, 436, 6, 800000
    counts = np.array([799989, 789999, cap + 3, 797001, 791939, 779999], np.int32)
    ends = np.cumsum(np.clip(counts, 0, cap).astype(np.int64)) * 16
    piece = 32 << 20
    assert 2 * piece < ends[-1] < 3 * piece and ends[4] < 2 * piece
    assert (ends % piece != 0).all() and ((ends + 32) % piece != 0).all()
    import opengpc_amd as g
    rec = constructed(W, H, P, cap, 9)
    h = g.Context(0)
    try:
        tracks_equal(h, dctx, rec, counts, W, H, 1200000, "pageable")
        tracks_equal(h, dctx, rec, counts, W, H, 1200000, "page-locked records", alloc_rec=h.pinned_empty)
    finally:
        h.close()
