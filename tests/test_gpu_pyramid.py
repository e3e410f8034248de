"""Matching over an image pyramid on the GPU (gpc_hip_pyramid_*).  Expected values: the CPU oracle run per level with the
level's settings, and tests/pyramid_util.py's numpy restatement of the downsampling rule and of mapping plus merge.  Outputs
are sentinel-filled and compared byte for byte, spare slots included."""
import os

import numpy as np
import pytest

import pyramid_util as pu
import score_util as su

pytestmark = pytest.mark.gpu

MATCHERS = [(True, False), (False, False), (True, True), (False, True)]   # (epipolar_mode, use_hashtable)
FILL = 0x5A
SPARSE = (5, 128, 0, True, False)
GROUPS_FOREST = os.path.join(pu.ROOT, "forests", "stress16x20Forest.txt")


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def lib_settings(t):
    import opengpc_amd as g
    return g.Settings(t[0], t[1], t[2], int(t[3]), int(t[4]), 1)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def filled(nbytes):
    import torch
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def host(t, dtype):
    return t.cpu().numpy().copy().view(dtype)


def expect_bytes(records, cap, dtype):
    """[P][cap] records as bytes: each pair's first min(n, cap) records, the sentinel behind them"""
    out = np.full((len(records), cap * dtype.itemsize), FILL, np.uint8)
    for p, r in enumerate(records):
        m = min(len(r), cap)
        out[p, :m * dtype.itemsize] = np.ascontiguousarray(r[:m].astype(dtype)).view(np.uint8)
    return out


def run_batch(ctx, L, R, levels, s, cap, ncand=True):
    """pyramid_batch_device on [P, H, W] pairs -> (record bytes [P, cap * 12], counts, level_counts, ncand)"""
    import torch
    P, H, W = L.shape
    d_L, d_R = dev(L), dev(R)
    d_out, d_cnt, d_lc, d_nc = filled(P * cap * 12), filled(P * 4), filled(levels * P * 4), filled(levels * P * 8)
    torch.cuda.synchronize()
    ctx.pyramid_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, levels, s, d_out.data_ptr(), cap, d_cnt.data_ptr(),
                             d_lc.data_ptr(), d_nc.data_ptr() if ncand else 0)
    ctx.synchronize()
    return (host(d_out, np.uint8).reshape(P, cap * 12), host(d_cnt, np.int32), host(d_lc, np.int32).reshape(levels, P),
            host(d_nc, np.int32).reshape(levels, P, 2))


def check_batch(ctx, pairs, forest, levels, st=SPARSE, naive=False, cap=None, need_drops=True):
    """pairs: [(L, R)] of one size.  Preconditions from the restatement, then the call against it."""
    H, W = pairs[0][0].shape
    want = [pu.expected_supports(L, R, forest, levels, st, naive) for L, R in pairs]
    for merged, kept, raw, nc in want:
        assert all(n > 0 for n in raw), raw                          # every level has records
        if need_drops and levels > 1:
            assert 0 < kept[1] < raw[1], (kept, raw)                 # level 1 both keeps and drops
    cap = cap or max(len(w[0]) for w in want) + 7
    ctx.set_arithmetic(naive)
    try:
        ctx.load_forest(pu.FORESTS[forest], W, H)
        got, cnt, lc, nc = run_batch(ctx, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), levels,
                                     lib_settings(st), cap)
    finally:
        ctx.set_arithmetic(False)
    assert cnt.tolist() == [len(w[0]) for w in want]
    assert lc.T.tolist() == [w[1] for w in want]
    assert nc.transpose(1, 0, 2).tolist() == [w[3] for w in want]
    assert np.array_equal(got, expect_bytes([w[0] for w in want], cap, pu.SUPPORT))
    return want


# ---- the downsampling step

@pytest.mark.parametrize("W,H,N", [(32, 2, 1), (64, 31, 3), (96, 60, 2), (16384, 4, 1)])
def test_down_device(ctx, W, H, N):
    import torch
    rng = np.random.default_rng(W + H)
    ramp = (np.arange(N * H * W, dtype=np.int64).reshape(N, H, W) * 37 // 5 % 256).astype(np.uint8)
    ramp[:, 0::2, 0::2] = (np.arange((W + 1) // 2) % 4)[None, None, :]   # sums of every class mod 4 beside whatever follows
    ramp[:, 0::2, 1::2] = 0
    ramp[:, 1::2, :] = 0
    ramp[:, :, W // 2:] = (np.arange(N * H * (W - W // 2)).reshape(N, H, -1) * 7 % 256).astype(np.uint8)
    board = (((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1) * 255).astype(np.uint8)[None].repeat(N, 0)
    cases = {"random": rng.integers(0, 256, (N, H, W)).astype(np.uint8), "all255": np.full((N, H, W), 255, np.uint8),
             "checkerboard": board, "ramp": ramp}
    classes = set(((ramp[0, 0, 0:W // 2:2].astype(int)) % 4).tolist())
    assert classes == {0, 1, 2, 3}
    nout = N * (H // 2) * (W // 2)
    for name, img in cases.items():
        d_src, d_dst = dev(img), filled(nout + 64)
        torch.cuda.synchronize()
        ctx.pyramid_down_device(d_src.data_ptr(), W, H, N, d_dst.data_ptr())
        ctx.synchronize()
        got = host(d_dst, np.uint8)
        assert np.array_equal(got[:nout].reshape(N, H // 2, W // 2), pu.down(img)), name
        assert (got[nout:] == FILL).all(), name
    assert (pu.down(board) == 128).all() and (pu.down(cases["all255"]) == 255).all()


def test_down_device_refusals(ctx):
    import opengpc_amd as g
    d = filled(4096)
    p = d.data_ptr()
    for args in ((p, 48, 4, 1, p + 2048), (p, 32, 1, 1, p + 2048), (p, 32, 4, 0, p + 2048), (p + 4, 32, 4, 1, p + 2048),
                 (p, 32, 4, 1, p + 2050), (0, 32, 4, 1, p), (p, 32, 4, 1, 0)):
        with pytest.raises(g.GpcError) as e:
            ctx.pyramid_down_device(*args)
        assert e.value.status == g.capi.E_INVALID, args


# ---- levels = 1: the plain calls

@pytest.mark.parametrize("epipolar,hashtable", MATCHERS)
def test_one_level_is_the_plain_match(ctx, oracle, epipolar, hashtable):
    import torch
    W, H, P, cap = 160, 101, 2, 9000
    pairs = [oracle.synth_pair(W, H, s, 8 + 4 * s) for s in range(P)]
    L, R = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    s = lib_settings((5, 128, 1, epipolar, hashtable))
    ctx.load_forest(pu.FORESTS["tau"], W, H)
    got, cnt, lc, nc = run_batch(ctx, L, R, 1, s, cap)
    d_L, d_R = dev(L), dev(R)
    d_out, d_cnt, d_nc = filled(P * cap * 12), filled(P * 4), filled(P * 8)
    torch.cuda.synchronize()
    ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    assert np.array_equal(got, host(d_out, np.uint8).reshape(P, -1)) and (cnt > 0).all()
    assert np.array_equal(cnt, host(d_cnt, np.int32)) and np.array_equal(lc[0], cnt)
    assert np.array_equal(nc[0].reshape(-1), host(d_nc, np.int32))
    # frames: against match_sequence_device
    frames = np.stack([L[0], R[0], L[1]])
    d_f = dev(frames)
    outs = []
    for pyramid in (True, False):
        d_o, d_c, d_l, d_n = filled(2 * cap * 16), filled(8), filled(8), filled(12)
        torch.cuda.synchronize()
        if pyramid:
            ctx.pyramid_sequence_device(d_f.data_ptr(), W, H, 3, 1, s, d_o.data_ptr(), cap, d_c.data_ptr(), d_l.data_ptr(), d_n.data_ptr())
        else:
            ctx.match_sequence_device(d_f.data_ptr(), W, H, 3, s, d_o.data_ptr(), cap, d_c.data_ptr(), d_n.data_ptr())
        ctx.synchronize()
        outs.append((host(d_o, np.uint8), host(d_c, np.int32), host(d_n, np.int32), host(d_l, np.int32)))
    assert all(np.array_equal(a, b) for a, b in zip(outs[0][:3], outs[1][:3])) and np.array_equal(outs[0][3], outs[0][1])


# ---- batches

@pytest.mark.parametrize("W,H,levels", [(192, 120, 3), (256, 128, 3), (320, 162, 2), (256, 102, 2), (384, 240, 4)])
def test_batch_shapes(ctx, oracle, W, H, levels):
    check_batch(ctx, [oracle.synth_pair(W, H, 0, 8)], "zero", levels)


@pytest.mark.parametrize("epipolar,hashtable", MATCHERS)
def test_batch_every_matcher(ctx, oracle, epipolar, hashtable):
    check_batch(ctx, [oracle.synth_pair(256, 128, 0, 8)], "zero", 3, (5, 128, 0, epipolar, hashtable))


def test_batch_tau_forest(ctx, oracle):
    check_batch(ctx, [oracle.synth_pair(256, 128, 0, 8)], "tau", 3)


def test_batch_naive_arithmetic(ctx, oracle):
    check_batch(ctx, [oracle.synth_pair(256, 128, 0, 8)], "zero", 3, SPARSE, naive=True)


def test_three_pairs_keep_their_own_occupancy(ctx, oracle):
    """D = 8, 4, 12 in one call: a pair's plane must not leak into its neighbours'"""
    want = check_batch(ctx, [oracle.synth_pair(256, 128, 0, D) for D in (8, 4, 12)], "zero", 3)
    assert len({tuple(w[1]) for w in want}) == 3


def test_level_two_keeps_records(ctx):
    """the right half 4x enlarged: texture only level 2 resolves"""
    want = check_batch(ctx, [pu.enlarged_pair()], "zero", 3)
    kept, raw = want[0][1], want[0][2]
    assert 0 < kept[2] < raw[2], (kept, raw)                          # level 2 both keeps and drops


def test_capacity(ctx, oracle):
    pair = pu.enlarged_pair()
    merged, kept, raw, nc = pu.expected_supports(*pair, "zero", 3)
    assert kept[0] > 10 and kept[1] > 10 and kept[2] > 0
    for cap in (1, kept[0] - 5, kept[0], kept[0] + 3, sum(kept) - 1, sum(kept)):
        check_batch(ctx, [pair], "zero", 3, cap=cap)


# ---- the merge on constructed records

def run_merge(ctx, levels_rec, W, H, cap_out, caps=None, counts=None):
    """levels_rec[l][p]: records of pair p at level l -> (record bytes [P, cap_out * esz], counts, level_counts)"""
    import torch
    P = len(levels_rec[0])
    dtype = levels_rec[0][0].dtype
    corr = dtype == pu.CORR
    caps = caps or [max(max(len(r) for r in lv), 1) for lv in levels_rec]
    d_rec, d_cnt, keep = [], [], []
    for l, lv in enumerate(levels_rec):
        a = np.zeros((P, caps[l]), dtype)
        a.view(np.uint8)[...] = 0xEE                               # slots behind a pair's count are never read
        for p, r in enumerate(lv):
            a[p, :min(len(r), caps[l])] = r[:caps[l]]
        n = np.array([len(r) for r in lv] if counts is None else counts[l], np.int32)
        keep += [dev(a.view(np.uint8)), dev(n)]
        d_rec.append(keep[-2].data_ptr())
        d_cnt.append(keep[-1].data_ptr())
    d_out, d_n, d_lc = filled(P * cap_out * dtype.itemsize), filled(P * 4), filled(len(levels_rec) * P * 4)
    torch.cuda.synchronize()
    ctx.pyramid_merge_device(d_rec, caps, d_cnt, corr, W, H, P, d_out.data_ptr(), cap_out, d_n.data_ptr(), d_lc.data_ptr())
    ctx.synchronize()
    return host(d_out, np.uint8).reshape(P, -1), host(d_n, np.int32), host(d_lc, np.int32).reshape(len(levels_rec), P)


def check_merge(ctx, levels_rec, W, H, cap_out):
    P = len(levels_rec[0])
    want = [pu.merge([lv[p] for lv in levels_rec], W, H) for p in range(P)]
    got, n, lc = run_merge(ctx, levels_rec, W, H, cap_out)
    assert n.tolist() == [len(w[0]) for w in want] and lc.T.tolist() == [w[1] for w in want]
    assert np.array_equal(got, expect_bytes([w[0] for w in want], cap_out, levels_rec[0][0].dtype))
    return want


def sup(*r):
    return np.array(list(r), pu.SUPPORT).reshape(-1)


def test_merge_block_corners_and_outside(ctx):
    """64x40: a coarse record whose block is hit at each corner pixel, and at the pixel just outside each side; one pair per
    probe, so the planes of 8 pairs are tested side by side"""
    W, H = 64, 40
    for l in (1, 2, 3):
        n, x, y = 1 << l, 3, 2
        probes = [(x * n, y * n), (x * n + n - 1, y * n), (x * n, y * n + n - 1), (x * n + n - 1, y * n + n - 1),
                  (x * n - 1, y * n), (x * n + n, y * n), (x * n, y * n - 1), (x * n, y * n + n)]
        levels = [[sup((px, py, 1.0)) for px, py in probes]] + [[sup()] * 8 for _ in range(l - 1)] + [[sup((x, y, 2.0))] * 8]
        want = check_merge(ctx, levels, W, H, 4)
        assert [w[1][-1] for w in want] == [0, 0, 0, 0, 1, 1, 1, 1]


def test_merge_rules_on_constructed_records(ctx):
    W, H = 64, 40
    # (5, 5) is dropped by level 0; both (9, 9) stay and mark (18, 18), which alone suppresses level 2's (4, 4)
    l0 = sup((10, 10, 2.0))
    l1 = sup((5, 5, 1.0), (9, 9, 1.0), (9, 9, 3.0))
    l2 = sup((4, 4, 1.0), (3, 3, 1.0), (15, 9, 0.0))
    want = check_merge(ctx, [[l0], [l1], [l2]], W, H, 8)
    assert want[0][1] == [1, 2, 2]
    # an empty level; all levels empty; correspondences; records outside their level's image; a level-0 pixel in the last column
    check_merge(ctx, [[l0], [sup()], [l2]], W, H, 8)
    check_merge(ctx, [[sup()], [sup()], [sup()]], W, H, 8)
    check_merge(ctx, [[sup((63, 39, 0.0), (70, 3, 0.0))], [sup((31, 19, 0.0), (32, 1, 0.0), (-1, 0, 0.0))], [sup((15, 9, 1.0), (16, 0, 0.0))]],
                W, H, 8)
    c = lambda *r: np.array(list(r), pu.CORR).reshape(-1)
    check_merge(ctx, [[c((10, 10, 12, 10)), c()], [c((5, 5, 6, 5), (9, 9, 11, 9)), c((5, 5, 6, 5))], [c((4, 4, 5, 4)), c((4, 4, 5, 4))]],
                W, H, 8)
    # more than a chunk of records per level: the chunk counts, their scan and the ranks across waves
    rng = np.random.default_rng(7)
    big = [[np.array(list(zip(rng.integers(0, W >> l, m), rng.integers(0, H >> l, m), rng.integers(0, 9, m))), pu.SUPPORT)
            for _ in range(2)] for l, m in enumerate((300, 5000, 5000))]
    check_merge(ctx, big, W, H, 9000)
    check_merge(ctx, big, W, H, 5003)


def test_merge_counts_above_capacity(ctx):
    """a level's count above its capacity reads the capacity; a merged count above cap_out stays true"""
    W, H = 64, 40
    l0, l1 = sup((10, 10, 2.0), (20, 20, 1.0), (30, 30, 1.0)), sup((5, 5, 1.0), (9, 9, 1.0), (11, 11, 1.0))
    got, n, lc = run_merge(ctx, [[l0], [l1]], W, H, 3, caps=[2, 2], counts=[[7], [9]])
    merged, kept = pu.merge([l0[:2], l1[:2]], W, H)
    assert n.tolist() == [3] and lc.T.tolist() == [kept] == [[2, 1]]
    assert np.array_equal(got, expect_bytes([merged], 3, pu.SUPPORT))
    got, n, lc = run_merge(ctx, [[l0], [l1]], W, H, 1, counts=[[-4], [3]])
    merged, kept = pu.merge([l0[:0], l1], W, H)
    assert n.tolist() == [3] and lc.T.tolist() == [[0, 3]] and np.array_equal(got, expect_bytes([merged], 1, pu.SUPPORT))


# ---- sequences

def seq_frames(N=4, W=256, H=128, vertical=True):
    rng = np.random.default_rng(11)
    BW, BH = W + 64, H + 32
    base = (rng.integers(0, 256, (BH // 4 + 1, BW // 4 + 1)).repeat(4, 0).repeat(4, 1)[:BH, :BW] * 3 // 4
            + rng.integers(0, 64, (BH, BW))).astype(np.uint8)
    xs, ys = [0, 8, 12, 24], ([16, 12, 20, 16] if vertical else [16] * 4)
    return np.ascontiguousarray(np.stack([base[ys[t]:ys[t] + H, xs[t]:xs[t] + W] for t in range(N)]))


def expected_sequence(oracle, frames, forest, levels, epipolar, hashtable):
    """per pair (merged correspondences, kept per level, raw per level), and candidates [levels][N]"""
    N, H, W = frames.shape
    per_level, ncand = [], []
    for l, fr in enumerate(pu.pyramid(frames, levels)):
        Hl, Wl = fr.shape[1:]
        rc, f = oracle.read_forest(pu.FORESTS[forest], Wl, Hl)
        pre, desc = [], []
        for img in fr:
            s, gr, m = oracle.preprocess(img, 5)
            pre.append(m)
            desc.append(oracle.descriptors(oracle.hash(s, gr, f), m, Wl, epipolar))
        match = oracle.hash_correspondences if hashtable else oracle.find_correspondences
        recs = []
        for t in range(N - 1):
            r = match(desc[t], pre[t], desc[t + 1], pre[t + 1], Wl)
            out = np.zeros(len(r), pu.CORR)
            for a, b in (("src_x", "sx"), ("src_y", "sy"), ("tar_x", "tx"), ("tar_y", "ty")):
                out[a] = r[b]
            recs.append(out)
        per_level.append(recs)
        ncand.append([len(m) for m in pre])
    out = []
    for t in range(N - 1):
        merged, kept = pu.merge([per_level[l][t] for l in range(levels)], W, H)
        out.append((merged, kept, [len(per_level[l][t]) for l in range(levels)]))
    return out, ncand


@pytest.mark.parametrize("epipolar", [True, False])
def test_sequence(ctx, oracle, epipolar):
    import torch
    frames = seq_frames(vertical=not epipolar)
    N, H, W = frames.shape
    levels = 3
    want, ncw = expected_sequence(oracle, frames, "zero", levels, epipolar, False)
    for merged, kept, raw in want:
        assert all(n > 0 for n in raw) and 0 < kept[1] < raw[1], (kept, raw)
    cap = max(len(w[0]) for w in want) + 5
    ctx.load_forest(pu.FORESTS["zero"], W, H)
    s = lib_settings((5, 128, 0, epipolar, False))
    d_f = dev(frames)
    d_out, d_cnt, d_lc, d_nc = filled((N - 1) * cap * 16), filled((N - 1) * 4), filled(levels * (N - 1) * 4), filled(levels * N * 4)
    torch.cuda.synchronize()
    ctx.pyramid_sequence_device(d_f.data_ptr(), W, H, N, levels, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_lc.data_ptr(),
                                d_nc.data_ptr())
    ctx.synchronize()
    assert host(d_cnt, np.int32).tolist() == [len(w[0]) for w in want]
    assert host(d_lc, np.int32).reshape(levels, N - 1).T.tolist() == [w[1] for w in want]
    assert host(d_nc, np.int32).reshape(levels, N).tolist() == ncw
    dev_bytes = host(d_out, np.uint8).reshape(N - 1, -1)
    assert np.array_equal(dev_bytes, expect_bytes([w[0] for w in want], cap, pu.CORR))
    # the host form: the same bytes, what the device form leaves is left
    out = np.full((N - 1, cap), 0, pu.CORR)
    out.view(np.uint8)[...] = FILL
    got, cnt, lc, nc, st = ctx.pyramid_sequence(frames, levels, s, cap, out=out)
    assert st == 0 and np.array_equal(got.view(np.uint8).reshape(N - 1, -1), dev_bytes)
    assert cnt.tolist() == [len(w[0]) for w in want] and nc.tolist() == ncw and lc.T.tolist() == [w[1] for w in want]


# ---- host forms

@pytest.mark.parametrize("pinned", [False, True])
def test_host_batch_in_two_chunks(ctx, oracle, pinned):
    """19 pairs of 96x60 at 2 levels: chunks of 16 and 3; pageable and page-locked arrays; a short capacity"""
    import opengpc_amd as g
    W, H, P, levels = 96, 60, 19, 2
    pairs = [oracle.synth_pair(W, H, s, 4 + 2 * (s % 3)) for s in range(P)]
    want = [pu.expected_supports(L, R, "zero", levels) for L, R in pairs]
    assert all(all(n > 0 for n in w[2]) for w in want)
    ctx.load_forest(pu.FORESTS["zero"], W, H)
    L, R = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    full = max(len(w[0]) for w in want)
    for cap in (full + 3, full - 20):
        if pinned:
            hl, hr, out = ctx.pinned_empty(L.shape, np.uint8), ctx.pinned_empty(R.shape, np.uint8), ctx.pinned_empty((P, cap), pu.SUPPORT)
            hl[...], hr[...] = L, R
        else:
            hl, hr, out = L, R, np.zeros((P, cap), pu.SUPPORT)
        out.view(np.uint8)[...] = FILL
        got, cnt, lc, nc, st = ctx.pyramid_batch(hl, hr, levels, lib_settings(SPARSE), cap, out=out)
        assert st == (g.capi.E_CAPACITY if cap < full else 0)
        assert cnt.tolist() == [len(w[0]) for w in want] and lc.T.tolist() == [w[1] for w in want]
        assert nc.transpose(1, 0, 2).tolist() == [w[3] for w in want]
        assert np.array_equal(got.view(np.uint8).reshape(P, -1), expect_bytes([w[0] for w in want], cap, pu.SUPPORT))


# ---- state, chain, refusals

def test_context_state_survives_a_pyramid_call(ctx, oracle):
    """a plain match at W x H is byte-equal before and after a pyramid call without a load_forest in between; the pyramid call
    again after an unrelated batch of another size"""
    import torch
    W, H, cap = 256, 128, 16000
    L, R = oracle.synth_pair(W, H, 0, 8)
    s = lib_settings(SPARSE)
    ctx.load_forest(pu.FORESTS["tau"], W, H)
    d_L, d_R = dev(L), dev(R)

    def plain():
        d_out, d_cnt = filled(cap * 12), filled(4)
        torch.cuda.synchronize()
        ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, 1, s, d_out.data_ptr(), cap, d_cnt.data_ptr())
        ctx.synchronize()
        return host(d_out, np.uint8), host(d_cnt, np.int32)
    before = plain()
    first = run_batch(ctx, L[None], R[None], 3, s, cap)
    after = plain()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[1][0] > 0
    merged, kept, raw, nc = pu.expected_supports(L, R, "tau", 3)
    assert first[1].tolist() == [len(merged)] and np.array_equal(first[0], expect_bytes([merged], cap, pu.SUPPORT))
    # an unrelated batch of another size (its own forest size), then the first size again
    L2, R2 = oracle.synth_pair(160, 101, 1, 8)
    ctx.load_forest(pu.FORESTS["tau"], 160, 101)
    run_batch(ctx, L2[None], R2[None], 1, s, 9000)
    ctx.load_forest(pu.FORESTS["tau"], W, H)
    again = run_batch(ctx, L[None], R[None], 3, s, cap)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))


def test_merged_supports_go_to_scoring_unchanged(ctx, oracle):
    import opengpc_amd as g
    import torch
    W, H, levels = 256, 128, 3
    L, R = oracle.synth_pair(W, H, 0, 8)
    merged, kept, raw, nc = pu.expected_supports(L, R, "zero", levels)
    cap = len(merged) + 9
    ctx.load_forest(pu.FORESTS["zero"], W, H)
    d_L, d_R = dev(L), dev(R)
    d_out, d_cnt, d_lc = filled(cap * 12), filled(4), filled(levels * 4)
    rng = np.random.default_rng(2)
    u = (8 + rng.integers(-8, 9, (1, H, W)) / 4.0).astype(np.float32)
    d_u = dev(u)
    d_sc = torch.full((1, 15), -3, dtype=torch.int64, device=torch.device("cuda", 0))
    thr = [0.5, 1.0, 3.0]
    torch.cuda.synchronize()
    ctx.pyramid_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, 1, levels, lib_settings(SPARSE), d_out.data_ptr(), cap,
                             d_cnt.data_ptr(), d_lc.data_ptr())
    ctx.score_supports_device(d_out.data_ptr(), cap, d_cnt.data_ptr(), W, H, 1, d_u.data_ptr(), 0, thr, d_sc.data_ptr())
    ctx.synchronize()
    have = su.as_dict(d_sc.cpu().numpy().copy().view(g.SCORE_DTYPE).reshape(-1)[0])
    rec = np.zeros(cap, pu.SUPPORT)
    rec[:len(merged)] = merged
    want = su.score_records(rec, len(merged), cap, u[0], None, None, thr)
    for k in ("n_records", "n_ignored", "n_no_truth", "n_judged", "n_within", "sum_e2_q8"):
        assert have[k] == want[k], k
    assert have["n_records"] == sum(kept) and have["n_judged"] > 0


def test_refusals(forest_paths):
    import opengpc_amd as g
    import torch
    c = g.Context(0)
    try:
        s = lib_settings(SPARSE)
        d = filled(1 << 20)
        p = d.data_ptr()

        def status(W, H, levels, P=1):
            try:
                c.pyramid_batch_device(p, p + (1 << 18), W, H, P, levels, s, p + (1 << 19), 16, p + (1 << 19) + 4096,
                                       p + (1 << 19) + 8192)
            except g.GpcError as e:
                return e.status
            return 0
        assert status(192, 120, 3) == g.capi.E_NO_FOREST               # no forest yet
        c.load_forest(forest_paths["zero"], 224, 200)
        assert status(224, 200, 3) == g.capi.E_INVALID                 # W % 64 != 0 at 3 levels
        c.load_forest(forest_paths["zero"], 160, 100)
        assert status(160, 100, 3) == g.capi.E_INVALID                 # level 2 would be 40 x 25
        c.load_forest(forest_paths["zero"], 192, 120)
        assert status(192, 120, 0) == g.capi.E_INVALID and status(192, 120, 5) == g.capi.E_INVALID
        assert status(256, 128, 3) == g.capi.E_INVALID                 # a forest of another size
        assert status(192, 120, 3, P=65536) == g.capi.E_UNSUPPORTED
        groups = c.load_forest_groups(GROUPS_FOREST, 192, 120)
        assert len(groups) > 1 and status(192, 120, 3) == g.capi.E_UNSUPPORTED   # group mode
        try:
            c.pyramid_sequence_device(p, 192, 120, 2, 2, s, p + (1 << 19), 16, p + (1 << 19) + 4096, p + (1 << 19) + 8192)
            st = 0
        except g.GpcError as e:
            st = e.status
        assert st == g.capi.E_UNSUPPORTED
        c.synchronize()
        assert (d.cpu().numpy() == FILL).all()                         # a refused call writes nothing
    finally:
        c.close()
