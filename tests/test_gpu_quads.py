"""Quads over a stereo sequence on the GPU (gpc_hip_quads_*, gpc_hip_match_stereo_sequence_device): the quads and their
counts EQUAL the plain restatement of the rule (tests/quad_util.py), byte for byte, for constructed records and for the
records the matching call returns; the matching call equals the three existing device calls byte for byte, with one
k_preprocess and one k_hash launch; the host forms equal the device forms; refusals; the context's state afterwards.
Outputs are pre-filled with -7, so that a byte written where none belongs shows."""
import os
import re
import subprocess

import numpy as np
import pytest

import quad_util as qu
from score_util import write_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FILL = -7


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def dev_of(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def records_device(ctx, sup, nsup, fl, nfl, fr, nfr, W, H, tol, quad_cap, c=None):
    """gpc_hip_quads_records_device over host records: (quads [P, max(quad_cap, 1)] of QUAD, nquads [P]) out of outputs
    that held FILL everywhere"""
    import torch
    c = c or ctx
    N, cap_s = sup.shape
    P, cap_f = fl.shape
    dev = torch.device("cuda", 0)
    d = [dev_of(a) for a in (sup, np.asarray(nsup, np.int32), fl, fr, np.asarray(nfl, np.int32), np.asarray(nfr, np.int32))]
    d_q = torch.full((P, max(quad_cap, 1), 8), FILL, dtype=torch.int32, device=dev)
    d_n = torch.full((P,), FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    c.quads_records_device(d[0].data_ptr(), cap_s, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), cap_f, d[4].data_ptr(),
                           d[5].data_ptr(), W, H, N, tol, d_q.data_ptr() if quad_cap else 0, quad_cap, d_n.data_ptr())
    c.synchronize()
    return d_q.cpu().numpy().view(qu.QUAD).reshape(P, max(quad_cap, 1)), d_n.cpu().numpy()


def same(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, "nquads", got[1], want[1])
    assert np.array_equal(got[0].view(np.uint8), want[0].view(np.uint8)), (what, "quads")


def constructed(W, H, N, per, slots, seed, empty_frame=None, empty_flow=None, negative=None, dmax=6):
    """Supports [N, slots], flows [N - 1, slots] each and their counts, built backwards: most of the supports of frame
    t get a left and a right flow record that lead to a support of frame t + 1 (drawn with repeats, so that some i' are
    contended), with an error of -3 .. 3 pixels between c' and b'.  Left pixels repeat; some d are NaN, infinite or
    non-integral; some right pixels leave the row; some records lie outside the image; every slot beyond a count holds a
    copy of a valid record of its list."""
    rng = np.random.default_rng(seed)
    P = N - 1
    sup = np.zeros((N, slots), qu.SUP)
    fl = np.zeros((P, slots, 4), np.int32)
    fr = np.zeros((P, slots, 4), np.int32)
    nsup, nfl, nfr = np.zeros(N, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    for t in range(N - 1, -1, -1):
        m = int(per * rng.uniform(0.85, 1.0))
        x, y = rng.integers(dmax, W, m), rng.integers(0, H, m)
        d = rng.integers(0, dmax + 1, m).astype(np.float32)
        k = rng.integers(0, m, m // 12)                       # shared left pixels
        src = rng.integers(0, m, len(k))
        x[k], y[k] = x[src], y[src]
        for val in (np.nan, np.inf, -np.inf, 2.5):
            d[rng.integers(0, m, 3)] = val
        d[rng.integers(0, m, 3)] = W + 3.0                     # right pixel left of the row
        d[rng.integers(0, m, 3)] = -(W + 3.0)                  # ... and right of it
        x[rng.integers(0, m, 2)] = -1
        x[rng.integers(0, m, 2)] = W
        y[rng.integers(0, m, 2)] = H
        sup["x"][t, :m], sup["y"][t, :m], sup["d"][t, :m] = x, y, d
        sup[t, m:] = sup[t, rng.integers(0, m, slots - m)]
        nsup[t] = m
        if t == P:
            continue
        mf = int(per * rng.uniform(0.85, 1.0))
        a = np.stack([rng.integers(0, W, mf), rng.integers(0, H, mf), rng.integers(0, W, mf), rng.integers(0, H, mf)], 1)
        b = np.stack([rng.integers(0, W, mf), rng.integers(0, H, mf), rng.integers(0, W, mf), rng.integers(0, H, mf)], 1)
        n1 = int(nsup[t + 1])
        pool = rng.integers(0, n1, max(n1, 1))                  # the i' the circles aim at: drawn with repeats
        for j in range(min(mf, int(0.9 * m))):
            i, i1 = int(rng.integers(0, m)), int(pool[rng.integers(0, len(pool))])
            d0, d1 = sup["d"][t, i], sup["d"][t + 1, i1]
            if not (np.isfinite(d0) and np.isfinite(d1)):
                continue
            e = rng.choice([0, 0, 0, 0, 0, 0, 1, -1, 2, -2, 3, -3], 2)
            a[j] = (sup["x"][t, i], sup["y"][t, i], sup["x"][t + 1, i1], sup["y"][t + 1, i1])
            b[j] = (sup["x"][t, i] - int(d0), sup["y"][t, i], sup["x"][t + 1, i1] - int(d1) + e[0], sup["y"][t + 1, i1] + e[1])
        for r in (a, b):
            for col, val in ((0, -1), (1, H), (2, W), (3, -3)):
                r[rng.integers(0, mf, 2), col] = val
        order = rng.permutation(mf)
        fl[t, :mf], fr[t, :mf] = a[order], b[rng.permutation(mf)]
        fl[t, mf:], fr[t, mf:] = fl[t, rng.integers(0, mf, slots - mf)], fr[t, rng.integers(0, mf, slots - mf)]
        nfl[t] = nfr[t] = mf
    if empty_frame is not None:
        nsup[empty_frame] = 0
    if empty_flow is not None:
        nfl[empty_flow] = 0
    if negative is not None:
        nfr[negative] = -4
    return sup, nsup, fl.view(qu.CORR).reshape(P, slots), nfl, fr.view(qu.CORR).reshape(P, slots), nfr


@pytest.fixture(scope="module")
def small():
    """48 x 41, N = 5: the run the issue describes, checked on the CPU through the restatement before anything is launched"""
    W, H, N = 48, 41, 5
    r = constructed(W, H, N, 300, 340, 21, empty_frame=2, empty_flow=2, negative=1)
    sup, nsup, fl, nfl, fr, nfr = r
    stats = {}
    quads = qu.restate(*r, W, H, 1, stats)
    assert nsup[2] == 0 and nfl[2] == 0 and nfr[1] < 0
    assert [len(q) for q in quads][1:3] == [0, 0] and min(len(quads[0]), len(quads[3])) >= 20, [len(q) for q in quads]
    assert stats["contended"] >= 3 and stats["shared"] >= 1, stats
    d = np.concatenate([sup["d"][t, :max(nsup[t], 0)] for t in range(N)])
    assert np.isnan(d).any() and np.isinf(d).any() and (d[np.isfinite(d)] % 1 != 0).any() and (np.abs(d[np.isfinite(d)]) > W).any()
    assert (sup["x"] < 0).any() and (sup["y"] >= H).any() and (fl["tar_x"] >= W).any() and (fr["src_x"] < 0).any()
    full = qu.restate(sup, np.full(N, 340), fl, np.full(N - 1, 340), fr, np.full(N - 1, 340), W, H, 1)
    assert [len(q) for q in full] != [len(q) for q in quads]       # the padding would close if it were read
    return W, H, r, quads


def test_constructed_records_48x41(ctx, small):
    W, H, r, quads = small
    nmax = max(len(q) for q in quads)
    same(records_device(ctx, *r, W, H, 1, 340), qu.expected_arrays(*r, W, H, 1, FILL, 340), "as it is")
    for quad_cap in (0, nmax - 1, nmax, nmax + 3):
        same(records_device(ctx, *r, W, H, 1, quad_cap), qu.expected_arrays(*r, W, H, 1, FILL, quad_cap), ("quad_cap", quad_cap))
    for tol in (0, 1, 3):
        want = qu.expected_arrays(*r, W, H, tol, FILL, nmax + 3)
        same(records_device(ctx, *r, W, H, tol, nmax + 3), want, ("tol", tol))
    assert len({tuple(qu.expected_arrays(*r, W, H, tol, FILL, 0)[1]) for tol in (0, 1, 3)}) == 3   # the tolerance matters here


def test_capacities_below_the_counts(ctx, small):
    W, H, r, quads = small
    sup, nsup, fl, nfl, fr, nfr = r
    cut = (np.ascontiguousarray(sup[:, :200]), nsup, np.ascontiguousarray(fl[:, :180]), nfl, np.ascontiguousarray(fr[:, :180]), nfr)
    assert nsup.max() > 200 and nfl.max() > 180
    want = qu.expected_arrays(*cut, W, H, 1, FILL, 200)
    assert want[1].max() >= 5
    same(records_device(ctx, *cut, W, H, 1, 200), want, "cap_s, cap_f < counts")


def test_no_empty_frame_and_steps_in_groups(ctx, small, monkeypatch):
    """every step live; then the same through a context that takes the steps in groups of 1, 2 and 3 (GPC_HIP_QUAD_STEPS)"""
    import opengpc_amd as g
    W, H, N = 48, 41, 5
    r = constructed(W, H, N, 300, 340, 22)
    want = qu.expected_arrays(*r, W, H, 1, FILL, 340)
    assert want[1].min() >= 20
    same(records_device(ctx, *r, W, H, 1, 340), want, "all steps")
    for steps in (1, 2, 3):
        monkeypatch.setenv("GPC_HIP_QUAD_STEPS", str(steps))
        c = g.Context(0)
        try:
            same(records_device(ctx, *r, W, H, 1, 340, c=c), want, ("groups of", steps))
            same(records_device(ctx, *small[2], W, H, 1, 340, c=c), qu.expected_arrays(*small[2], W, H, 1, FILL, 340), ("groups, empty", steps))
        finally:
            c.close()


def test_more_than_one_chunk_per_step(ctx):
    """160 x 101, N = 3, about 5000 supports per frame: a step's quads lie in three chunks of 2048 support slots, the last
    one partial, so the numbering crosses chunk boundaries"""
    W, H, N = 160, 101, 3
    r = constructed(W, H, N, 5300, 5400, 5, dmax=9)
    assert r[1].min() > 2 * 2048 and r[1].max() % 2048 != 0
    want = qu.expected_arrays(*r, W, H, 1, FILL, 5400)
    assert want[1].min() > 500
    quads = qu.restate(*r, W, H, 1)
    assert all(any(q[6] >= 4096 for q in qs) and any(q[6] < 2048 for q in qs) for qs in quads)
    same(records_device(ctx, *r, W, H, 1, 5400), want, "5k")
    same(records_device(ctx, *r, W, H, 1, 100), qu.expected_arrays(*r, W, H, 1, FILL, 100), "5k, short")


def test_index_range_16384x64(ctx):
    """the widest image there is: pixels in the last column and the last row, a disparity of the whole row"""
    W, H = 16384, 64
    s0 = [(W - 1, H - 1, 5.0), (W - 1, 0, float(W - 1)), (0, H - 1, 0.0), (9000, 33, -7000.0), (W - 1, H - 1, 1.0), (5, 5, 6.0)]
    s1 = [(W - 1, H - 2, 3.0), (W - 1, H - 1, float(W - 1)), (1, H - 1, 0.0), (16000, 63, 15999.0)]
    rng = np.random.default_rng(3)
    for k in range(30):
        s0.append((int(rng.integers(0, W)), int(rng.integers(0, H)), 0.0))
        s1.append((int(rng.integers(0, W)), int(rng.integers(0, H)), 0.0))
    fl = [(W - 1, H - 1, W - 1, H - 2), (W - 1, 0, W - 1, H - 1), (0, H - 1, 1, H - 1), (9000, 33, 16000, 63)]
    fr = [(W - 6, H - 1, W - 4, H - 2), (0, 0, 0, H - 1), (0, H - 1, 1, H - 1), (16000, 33, 1, 63)]
    for k in range(6, 36):
        fl.append((s0[k][0], s0[k][1], s1[k - 2][0], s1[k - 2][1]))
        fr.append((s0[k][0], s0[k][1], s1[k - 2][0], s1[k - 2][1] + (k % 3 == 0)))
    sup, nsup = qu.sup_array([s0, s1])
    a, na = qu.corr_array([fl])
    b, nb = qu.corr_array([fr])
    want = qu.expected_arrays(sup, nsup, a, na, b, nb, W, H, 0, FILL, 40)
    assert want[1][0] >= 20 and (want[0]["x"][0, :4] == [W - 1, W - 1, 0, 9000]).all(), want[1]
    same(records_device(ctx, sup, nsup, a, na, b, nb, W, H, 0, 40), want, "16384 x 64")


# ---- the matching call

def settings(epipolar, hashtable, thr=5):
    import opengpc_amd as g
    return g.Settings(thr, 128, 0, epipolar, hashtable, 1)


def three_calls(ctx, L, R, ss, fs, cap):
    """the existing device calls: (sup, nsup, ncand [N, 2], flowL, nflowL, ncandL, flowR, nflowR, ncandR) as numpy"""
    import torch
    N, H, W = L.shape
    dev = torch.device("cuda", 0)
    dL, dR = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    d_sup = torch.full((N, cap, 3), FILL, dtype=torch.int32, device=dev)
    d_ns = torch.full((N,), FILL, dtype=torch.int32, device=dev)
    d_nc = torch.full((N, 2), FILL, dtype=torch.int32, device=dev)
    out = []
    torch.cuda.synchronize(dev)
    ctx.match_batch_device(dL.data_ptr(), dR.data_ptr(), W, H, N, ss, d_sup.data_ptr(), cap, d_ns.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    out += [d_sup.cpu().numpy(), d_ns.cpu().numpy(), d_nc.cpu().numpy()]
    for d_f in (dL, dR):
        d_fl = torch.full((N - 1, cap, 4), FILL, dtype=torch.int32, device=dev)
        d_nf = torch.full((N - 1,), FILL, dtype=torch.int32, device=dev)
        d_c = torch.full((N,), FILL, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.match_sequence_device(d_f.data_ptr(), W, H, N, fs, d_fl.data_ptr(), cap, d_nf.data_ptr(), d_c.data_ptr())
        ctx.synchronize()
        out += [d_fl.cpu().numpy(), d_nf.cpu().numpy(), d_c.cpu().numpy()]
    return out


def one_call(ctx, L, R, ss, fs, cap, tol=None, quad_cap=0):
    """gpc_hip_match_stereo_sequence_device (tol None) or gpc_hip_quads_sequence_device: dict of numpy outputs"""
    import torch
    N, H, W = L.shape
    dev = torch.device("cuda", 0)
    dL, dR = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    t = dict(sup=torch.full((N, cap, 3), FILL, dtype=torch.int32, device=dev), nsup=torch.full((N,), FILL, dtype=torch.int32, device=dev),
             flowL=torch.full((N - 1, cap, 4), FILL, dtype=torch.int32, device=dev),
             flowR=torch.full((N - 1, cap, 4), FILL, dtype=torch.int32, device=dev),
             nflowL=torch.full((N - 1,), FILL, dtype=torch.int32, device=dev), nflowR=torch.full((N - 1,), FILL, dtype=torch.int32, device=dev),
             ncand=torch.full((2, N), FILL, dtype=torch.int32, device=dev),
             quads=torch.full((N - 1, max(quad_cap, 1), 8), FILL, dtype=torch.int32, device=dev),
             nquads=torch.full((N - 1,), FILL, dtype=torch.int32, device=dev))
    p = {k: v.data_ptr() for k, v in t.items()}
    torch.cuda.synchronize(dev)
    if tol is None:
        ctx.match_stereo_sequence_device(dL.data_ptr(), dR.data_ptr(), W, H, N, ss, fs, p["sup"], cap, p["nsup"], p["flowL"], p["flowR"],
                                         cap, p["nflowL"], p["nflowR"], p["ncand"])
    else:
        ctx.quads_sequence_device(dL.data_ptr(), dR.data_ptr(), W, H, N, ss, fs, tol, p["sup"], cap, p["nsup"], p["flowL"], p["flowR"],
                                  cap, p["nflowL"], p["nflowR"], p["ncand"], p["quads"] if quad_cap else 0, quad_cap, p["nquads"])
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def records_of(o):
    """the outputs of one_call as the restatement takes them"""
    N, cap = o["sup"].shape[:2]
    return (o["sup"].view(qu.SUP).reshape(N, cap), o["nsup"], o["flowL"].view(qu.CORR).reshape(N - 1, cap), o["nflowL"],
            o["flowR"].view(qu.CORR).reshape(N - 1, cap), o["nflowR"])


FRAMES = {}


def frames(W, H, N, D, dy):
    if (W, H, N, D, dy) not in FRAMES:
        FRAMES[(W, H, N, D, dy)] = qu.stereo_frames_of(W, H, N, 1, D, dy)
    return FRAMES[(W, H, N, D, dy)]


@pytest.mark.parametrize("what", ["sort", "hashtable", "naive tau"])
def test_matching_equals_the_three_existing_calls(ctx, forest_paths, what):
    """160 x 101, N = 4, D = 9, seed 1: records, counts and candidate counts byte for byte, out of one k_preprocess and one
    k_hash launch"""
    W, H, N = 160, 101, 4
    L, R = frames(W, H, N, 9, 0)
    cap = (W - 26) * (H - 26)
    ht = 1 if what == "hashtable" else 0
    ss, fs = settings(1, ht), settings(0, ht)
    naive = what == "naive tau"
    try:
        ctx.set_arithmetic(naive)
        ctx.load_forest(forest_paths["tau" if naive else "zero"], W, H)
        want = three_calls(ctx, L, R, ss, fs, cap)
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_timing()
        got = one_call(ctx, L, R, ss, fs, cap)
        times = ctx.kernel_times()
        ctx.enable_kernel_timing(False)
    finally:
        ctx.set_arithmetic(False)
    assert times["k_preprocess"][1] == 1 and times["k_hash"][1] == 1 and times["k_quad_sides"][1] == 1, times
    assert min(want[1].min(), want[4].min(), want[7].min()) > 1000, (want[1], want[4], want[7])
    for k, (a, b) in {"sup": (got["sup"], want[0]), "nsup": (got["nsup"], want[1]), "flowL": (got["flowL"], want[3]),
                      "nflowL": (got["nflowL"], want[4]), "flowR": (got["flowR"], want[6]), "nflowR": (got["nflowR"], want[7]),
                      "ncand L": (got["ncand"][0], want[5]), "ncand R": (got["ncand"][1], want[8]),
                      "ncand L (batch)": (got["ncand"][0], want[2][:, 0]), "ncand R (batch)": (got["ncand"][1], want[2][:, 1])}.items():
        assert np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), (what, k)


def test_refusals(forest_paths):
    import os
    import torch
    import opengpc_amd as g
    W, H, N = 160, 101, 2
    L, R = frames(W, H, 4, 9, 0)
    L, R = L[:2], R[:2]
    c = g.Context(0)
    try:
        with pytest.raises(g.GpcError) as e:
            one_call(c, L, R, settings(1, 0), settings(0, 0), 64)
        assert e.value.status == g.capi.E_NO_FOREST
        c.load_forest(forest_paths["zero"], W, H)
        with pytest.raises(g.GpcError) as e:
            one_call(c, L, R, settings(1, 0, 5), settings(0, 0, 6), 64)
        assert e.value.status == g.capi.E_INVALID
        for tol in (-1, 256):
            with pytest.raises(g.GpcError) as e:
                one_call(c, L, R, settings(1, 0), settings(0, 0), 64, tol=tol, quad_cap=4)
            assert e.value.status == g.capi.E_INVALID
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        st, groups = g.read_forest_groups(os.path.join(root, "forests", "stress16x20Forest.txt"), W, H)
        assert st == 0 and len(groups) > 1
        c.set_forest_groups(groups)
        with pytest.raises(g.GpcError) as e:
            one_call(c, L, R, settings(1, 0), settings(0, 0), 64)
        assert e.value.status == g.capi.E_UNSUPPORTED
        # the records form needs no forest, so group mode does not concern it
        sup, ns = qu.sup_array([[(10, 5, 3.0)], [(12, 6, 4.0)]])
        a, na = qu.corr_array([[(10, 5, 12, 6)]])
        b, nb = qu.corr_array([[(7, 5, 8, 6)]])
        q, n = records_device(None, sup, ns, a, na, b, nb, 32, 20, 0, 2, c=c)
        assert list(n) == [1] and tuple(q[0, 0]) == (10, 5, 3, 2, 1, 4, 0, 0)
        torch.cuda.synchronize()
    finally:
        c.close()


@pytest.mark.parametrize("W, H, N, D, dy, least", [(160, 101, 4, 9, 12, 1000), (160, 101, 4, 9, 0, 1000), (96, 64, 3, 5, 4, 1000)])
def test_match_and_close(ctx, forest_paths, W, H, N, D, dy, least):
    """The quads of gpc_hip_quads_sequence_device equal the restatement over the records the call returned, with the sort
    matchers (stereo: epipolar; flow: device-wide) and the zero forest, tol = 1; not vacuous: at least 1000 quads per step.
    Counted on an MI355X: 160 x 101, dy = 12: 5611, 5262, 5482; dy = 0: 6086, 5509, 5576; 96 x 64: 1347, 1400."""
    L, R = frames(W, H, N, D, dy)
    cap = (W - 26) * (H - 26)
    ctx.load_forest(forest_paths["zero"], W, H)
    o = one_call(ctx, L, R, settings(1, 0), settings(0, 0), cap, tol=1, quad_cap=cap)
    rec = records_of(o)
    want = qu.expected_arrays(*rec, W, H, 1, FILL, cap)
    print("quads per step", (W, H, dy), list(want[1]))
    same((o["quads"].view(qu.QUAD).reshape(N - 1, cap), o["nquads"]), want, (W, H, dy))
    assert want[1].min() >= least, list(want[1])
    q = o["quads"].view(qu.QUAD).reshape(N - 1, cap)
    for t in range(N - 1):                                        # the construction's truth: disparity D before and after
        m = int(o["nquads"][t])
        assert (q["d0"][t, :m] == D).mean() > 0.95 and (q["d1"][t, :m] == D).mean() > 0.95


def test_host_forms_equal_device_forms(ctx, forest_paths, small):
    import opengpc_amd as g
    W, H, r, quads = small
    sup, nsup, fl, nfl, fr, nfr = r
    nmax = max(len(q) for q in quads)
    for pinned in (False, True):
        for quad_cap, status in ((340, 0), (nmax - 1, g.capi.E_CAPACITY)):
            want = qu.expected_arrays(*r, W, H, 1, FILL, quad_cap)
            args = [np.ascontiguousarray(a) for a in (sup, nsup, fl, nfl, fr, nfr)]
            buf = np.full((4, quad_cap, 8), FILL, np.int32)
            if pinned:
                args = [ctx.pinned_empty(a.shape, a.dtype) for a in args]
                for dst, src in zip(args, (sup, nsup, fl, nfl, fr, nfr)):
                    dst[...] = src
                buf = ctx.pinned_empty((4, quad_cap, 8), np.int32)
                buf[...] = FILL
            q, n, st = ctx.quads_records(*args, W, H, tol=1, quad_cap=quad_cap, quads_out=buf.view(qu.QUAD).reshape(4, quad_cap))
            assert st == status, (pinned, quad_cap, st)
            same((q, n), want, ("host records", pinned, quad_cap))
    # counts above their capacities: GPC_E_CAPACITY, and what is written is the clipped lists' result
    cut = [np.ascontiguousarray(a) for a in (sup[:, :200], nsup, fl[:, :180], nfl, fr[:, :180], nfr)]
    buf = np.full((4, 200, 8), FILL, np.int32)
    q, n, st = ctx.quads_records(*cut, W, H, tol=1, quad_cap=200, quads_out=buf.view(qu.QUAD).reshape(4, 200))
    assert st == g.capi.E_CAPACITY
    same((q, n), qu.expected_arrays(*cut, W, H, 1, FILL, 200), "host records, short lists")
    # the sequence form against the device form
    W, H, N = 96, 64, 3
    L, R = frames(W, H, N, 5, 4)
    cap = (W - 26) * (H - 26)
    ctx.load_forest(forest_paths["zero"], W, H)
    d = one_call(ctx, L, R, settings(1, 0), settings(0, 0), cap, tol=1, quad_cap=cap)
    for alloc in (None, ctx.pinned_empty):
        def make(shape, dtype):
            if alloc is None:
                words = np.dtype(dtype).itemsize // 4
                return np.full(tuple(shape) + (words,), FILL, np.int32).view(dtype).reshape(shape)
            a = alloc(shape, dtype)
            a.view(np.int32)[...] = FILL
            return a
        h = ctx.quads_sequence(L, R, settings(1, 0), settings(0, 0), tol=1, cap_s=cap, cap_f=cap, quad_cap=cap, alloc=make)
        assert h["status"] == 0
        for k in ("sup", "nsup", "flowL", "nflowL", "flowR", "nflowR", "ncand", "quads", "nquads"):
            assert np.array_equal(np.ascontiguousarray(h[k]).view(np.uint8).reshape(-1), d[k].view(np.uint8).reshape(-1)), (k, alloc is None)
    short = int(d["nquads"].max()) - 1
    h = ctx.quads_sequence(L, R, settings(1, 0), settings(0, 0), tol=1, cap_s=cap, cap_f=cap, quad_cap=short)
    assert h["status"] == g.capi.E_CAPACITY and np.array_equal(h["nquads"], d["nquads"])
    for t in range(N - 1):                                        # (arrays made by the call hold zeros behind the valid quads)
        m = min(int(d["nquads"][t]), short)
        assert np.array_equal(h["quads"].view(np.int32).reshape(N - 1, short, 8)[t, :m], d["quads"][t, :m])


def test_batch_after_the_quad_calls(ctx, forest_paths):
    """a plain match_batch_device on the same context gives what it gave before the quad calls"""
    W, H, N = 160, 101, 4
    L, R = frames(W, H, N, 9, 0)
    cap = (W - 26) * (H - 26)
    ctx.load_forest(forest_paths["zero"], W, H)
    before = three_calls(ctx, L, R, settings(1, 0), settings(0, 0), cap)
    one_call(ctx, L, R, settings(1, 0), settings(0, 1), cap, tol=1, quad_cap=cap)
    one_call(ctx, L, R, settings(0, 0), settings(1, 0), cap, tol=0, quad_cap=0)
    after = three_calls(ctx, L, R, settings(1, 0), settings(0, 0), cap)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_cpp_sample_equals_python(ctx, forest_paths, tmp_path):
    """samples/quads (Forest::stereoSequenceQuads of include/gpc/quads.hpp) on four PNGs written here: its quads per step and
    its FNV-1a-64 over the records equal what Context.quads_sequence gives for the same images and settings.  The sample's
    first capacity (a quarter of the pixels) is below the counts, so its second attempt is what answers."""
    W, H, N = 160, 101, 2
    L, R = frames(W, H, 4, 9, 0)
    L, R = np.ascontiguousarray(L[:N]), np.ascontiguousarray(R[:N])
    names = []
    for t in range(N):
        for side, img in (("L", L[t]), ("R", R[t])):
            names.append(str(tmp_path / ("%s%d.png" % (side, t))))
            write_png(names[-1], img)
    ctx.load_forest(forest_paths["zero"], W, H)
    cap = (W - 26) * (H - 26)
    o = ctx.quads_sequence(L, R, settings(1, 0), settings(0, 0), tol=1, cap_s=cap, cap_f=cap, quad_cap=cap)
    assert o["status"] == 0 and o["nquads"][0] >= 1000 and o["nsup"].max() > W * H // 4
    out = subprocess.run([os.path.join(ROOT, "samples", "quads"), forest_paths["zero"]] + names, check=True, capture_output=True,
                         text=True, timeout=120).stdout
    assert [int(v) for v in re.findall(r"step \d+: (\d+) quads", out)] == list(o["nquads"]), out
    assert re.search(r"fnv ([0-9a-f]{16})", out).group(1) == "%016x" % qu.fnv_quads(o["quads"], o["nquads"], cap), out


def test_cpp_close_records_equals_the_restatement(small, tmp_path):
    """gpc::quads::closeRecords over the valid records of the constructed run (tests/cpp/quads_check.cpp, compiled here): the
    four points and the support indices of every quad are the restatement's"""
    W, H, r, _ = small
    sup, nsup, fl, nfl, fr, nfr = r
    N = len(nsup)
    # (the C++ form takes lists, so counts are list lengths: the empty frame and the empty steps stay empty; NaN and
    # infinities travel as text)
    ns, nl, nr = (np.clip(c, 0, None) for c in (nsup, nfl, nfr))
    want = qu.restate(sup, ns, fl, nl, fr, nr, W, H, 1)
    assert want == qu.restate(*r, W, H, 1)
    lines = ["%d %d 1 %d" % (W, H, N)]
    for t in range(N):
        lines.append(str(ns[t]))
        lines += ["%d %d %r" % (sup["x"][t, i], sup["y"][t, i], float(sup["d"][t, i])) for i in range(ns[t])]
    for t in range(N - 1):
        for rec, n in ((fl, nl), (fr, nr)):
            lines.append(str(n[t]))
            lines += ["%d %d %d %d" % tuple(rec[t, i]) for i in range(n[t])]
    exe = str(tmp_path / "quads_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D_INTRINSICS_SSE", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "quads_check.cpp"), "-L" + os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip", "-lz",
                    "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-Wl,-rpath,/opt/rocm/lib", "-lpthread"], check=True, timeout=300)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True, timeout=120).stdout
    got, cur = [], None
    for line in out.splitlines():
        if line.startswith("step"):
            cur = []
            got.append(cur)
        else:
            cur.append(tuple(int(v) for v in line.split()))
    assert got == [[(x, y, x - d0, y, x + u, y + v, x + u - d1, y + v, s0, s1) for (x, y, d0, u, v, d1, s0, s1) in qs] for qs in want]
