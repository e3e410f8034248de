"""Scoring against ground truth on the GPU (gpc_hip_score_*): every output is an integer count, so every comparison here
is equality -- with the numpy restatement of tests/score_util.py, with the reference's own recorded numbers
(tests/golden/appendix_c.json), and between the forms (records already on the device, match-and-score, host)."""
import os
import subprocess

import numpy as np
import pytest

import score_util as su

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCHERS = [(True, False), (False, False), (True, True), (False, True)]   # (epipolar_mode, use_hashtable)
STRESS = os.path.join(ROOT, "forests", "stress16x20Forest.txt")
THR8 = [0.0, 0.5, 1.0, 2.0, 3.0, 5.0, 10.0, 1000.0]


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def settings(epipolar, hashtable):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epipolar, hashtable, 1)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def dev_scores(P):
    import torch
    return torch.full((P, 15), -3, dtype=torch.int64, device=torch.device("cuda", 0))   # (garbage: the calls overwrite it)


def host_scores(d_sc):
    import opengpc_amd as g
    return d_sc.cpu().numpy().copy().view(g.SCORE_DTYPE).reshape(-1)


def score_records_gpu(ctx, rec, cap, counts, W, H, u, v, ign, thr):
    """records [P, cap] (numpy) through the records form -> SCORE_DTYPE [P]"""
    import torch
    P = len(counts)
    d_rec = to_dev(rec.view(np.int32).reshape(P, cap, -1))
    d_cnt = to_dev(np.asarray(counts, np.int32))
    d_u, d_v = to_dev(u), (to_dev(v) if v is not None else None)
    d_i = to_dev(ign) if ign is not None else None
    d_sc = dev_scores(P)
    torch.cuda.synchronize()
    ip = d_i.data_ptr() if d_i is not None else 0
    if v is None:
        ctx.score_supports_device(d_rec.data_ptr(), cap, d_cnt.data_ptr(), W, H, P, d_u.data_ptr(), ip, thr, d_sc.data_ptr())
    else:
        ctx.score_correspondences_device(d_rec.data_ptr(), cap, d_cnt.data_ptr(), W, H, P, d_u.data_ptr(), d_v.data_ptr(), ip,
                                         thr, d_sc.data_ptr())
    ctx.synchronize()
    return host_scores(d_sc)


def same_score(got_row, want, what="", skip=()):
    got = su.as_dict(got_row)
    for k in su.SCORE_FIELDS:
        if k not in skip:
            assert got[k] == want[k], (what, k, got[k], want[k])


SPECIALS = [np.nan, np.inf, -np.inf, 1e10, 1e9, np.float32(1e9) - np.float32(64.0), -1e10]


def random_truth(rng, P, H, W, flow):
    """integer-valued and fractional truth with the special values planted"""
    u = np.where(rng.random((P, H, W)) < 0.5, rng.integers(-6, 7, (P, H, W)), rng.normal(0, 3, (P, H, W))).astype(np.float32)
    v = np.where(rng.random((P, H, W)) < 0.5, rng.integers(-3, 4, (P, H, W)), rng.normal(0, 2, (P, H, W))).astype(np.float32)
    for plane in (u, v):
        k = max(P * H * W // 40, len(SPECIALS))
        at = rng.integers(0, P * H * W, k)
        plane.reshape(-1)[at] = np.array(SPECIALS, np.float32)[np.arange(k) % len(SPECIALS)]
    ign = (rng.random((P, H, W)) < 0.15).astype(np.uint8) * rng.integers(1, 256, (P, H, W)).astype(np.uint8)
    return u, (v if flow else None), ign


def random_records(rng, P, cap, counts, W, H, u, v):
    """records whose values lie near the truth at their pixel (so every threshold catches some)"""
    import opengpc_amd as g
    corr = v is not None
    rec = np.zeros((P, cap), g.CORR_DTYPE if corr else g.SUPPORT_DTYPE)
    for p in range(P):
        x = rng.integers(0, W, cap).astype(np.int32)
        y = rng.integers(0, H, cap).astype(np.int32)
        with np.errstate(all="ignore"):
            tu = np.nan_to_num(u[p, y, x], nan=0.0, posinf=0.0, neginf=0.0).clip(-100, 100)
        if corr:
            with np.errstate(all="ignore"):
                tv = np.nan_to_num(v[p, y, x], nan=0.0, posinf=0.0, neginf=0.0).clip(-100, 100)
            rec[p]["src_x"], rec[p]["src_y"] = x, y
            rec[p]["tar_x"] = x + np.round(tu).astype(np.int32) + rng.integers(-2, 3, cap)
            rec[p]["tar_y"] = y + np.round(tv).astype(np.int32) + rng.integers(-2, 3, cap)
        else:
            rec[p]["x"], rec[p]["y"] = x, y
            rec[p]["d"] = np.where(rng.random(cap) < 0.5, np.round(tu), tu + rng.normal(0, 1.5, cap)).astype(np.float32)
            # d = NaN / +-inf: e2 is NaN / inf -- judged, within no threshold, the clamp added to sum_e2_q8
            rec[p]["d"][7::97] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(len(rec[p]["d"][7::97])) % 3]
    return rec


def plant_fma_cases(rec, u, v, W):
    """the FMA-sensitive inputs of score_util at the first records of pair 0: target == source, truth = (-ex, -ey), so that
    the record's error is exactly (ex, ey); both summand orders"""
    pairs, thr = su.fma_sensitive_corr()
    pairs = np.concatenate([pairs, pairs[:, ::-1]])
    for k, (ex, ey) in enumerate(pairs):
        x, y = 1 + 2 * k, 1
        rec[0, k] = (x, y, x, y)
        u[0, y, x], v[0, y, x] = -ex, -ey
    return len(pairs), thr


@pytest.mark.parametrize("W,H", [(48, 41), (176, 67), (1024, 436)])
@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("flow", [False, True])
def test_records_form_against_numpy(ctx, W, H, P, flow):
    rng = np.random.default_rng(W + H + P + int(flow))
    cap = 3000 if W < 1000 else 70000
    u, v, ign = random_truth(rng, P, H, W, flow)
    counts = [0, cap - 77, cap, cap + 1234, 5][:P] if P > 1 else [cap - 77]
    rec = random_records(rng, P, cap, counts, W, H, u, v)
    thr_all = list(THR8)
    if flow:
        nf, t = plant_fma_cases(rec, u, v, W)
        ign[0, 1, :2 * nf + 2] = 0
        thr_all[4] = t
    for use_ign in (ign, None):
        for thr in (thr_all, [thr_all[4]]):
            got = score_records_gpu(ctx, rec, cap, counts, W, H, u, v, use_ign, thr)
            again = score_records_gpu(ctx, rec, cap, counts, W, H, u, v, use_ign, thr)
            assert got.tobytes() == again.tobytes()
            for p in range(P):
                want = su.score_records(rec[p], counts[p], cap, u[p], v[p] if flow else None,
                                        use_ign[p] if use_ign is not None else None, thr)
                same_score(got[p], want, (p, len(thr), use_ign is None))
                assert got[p]["n_records"] == min(counts[p], cap)
    if P > 1:   # the host records form (chunks of 16 pairs through the arena) gives the device form's bytes
        thr = thr_all[:3]
        dev = score_records_gpu(ctx, rec, cap, counts, W, H, u, v, ign, thr)
        assert ctx.score_records(rec, counts, u, v, ign, thr).tobytes() == dev.tobytes()
        assert ctx.score_records(rec, counts, u, v, None, thr).tobytes() == score_records_gpu(ctx, rec, cap, counts, W, H, u, v, None, thr).tobytes()
    if flow:   # the planted records are what a contracted kernel gets wrong: they are judged, and split by the threshold
        want = su.score_records(rec[0][:nf], nf, nf, u[0], v[0], None, [thr_all[4]])
        assert want["n_judged"] == nf and 0 < want["n_within"][0] < nf


def batch_of(oracle, W, H, B, D0=5):
    pairs = [oracle.synth_pair(W, H, i, D0 + i) for i in range(B)]
    L = np.ascontiguousarray(np.stack([p[0] for p in pairs]))
    R = np.ascontiguousarray(np.stack([p[1] for p in pairs]))
    return L, R, [D0 + i for i in range(B)]


def score_batch_gpu(ctx, L, R, s, u, ign, thr):
    import torch
    P, H, W = L.shape
    d_L, d_R, d_u = to_dev(L), to_dev(R), to_dev(u)
    d_i = to_dev(ign) if ign is not None else None
    d_sc = dev_scores(P)
    torch.cuda.synchronize()
    ctx.score_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, d_u.data_ptr(), d_i.data_ptr() if d_i is not None else 0,
                           thr, d_sc.data_ptr())
    ctx.synchronize()
    return host_scores(d_sc)


def match_batch_gpu(ctx, L, R, s, cap):
    import opengpc_amd as g
    import torch
    P, H, W = L.shape
    d_L, d_R = to_dev(L), to_dev(R)
    d_out = torch.zeros((P, cap, 3), dtype=torch.int32, device=d_L.device)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=d_L.device)
    d_nc = torch.zeros((P, 2), dtype=torch.int32, device=d_L.device)
    torch.cuda.synchronize()
    ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    return d_out.cpu().numpy().copy().view(g.SUPPORT_DTYPE).reshape(P, cap), d_cnt.cpu().numpy(), d_nc.cpu().numpy()


@pytest.mark.parametrize("W,H,D,n", [(1024, 436, 24, 269547), (96, 64, 5, 1044)])
def test_pinned_by_the_references_own_numbers(ctx, oracle, forest_paths, golden, W, H, D, n):
    """SURVEY Appendix C / tests/golden/appendix_c.json: the synthetic pair (s = 0, zero forest, sparsematch settings) has n
    supports, all with d = D."""
    import opengpc_amd as g
    assert n in [case["zero"]["epipolar"]["n"] for case in golden["cases"]]   # (recorded from the compiled reference)
    L, R = oracle.synth_pair(W, H, 0, D)
    ctx.load_forest(forest_paths["zero"], W, H)
    s = g.Settings.sparsematch()
    sc = score_batch_gpu(ctx, L[None], R[None], s, np.full((1, H, W), D, np.float32), None, [0.0, 1.0])[0]
    assert sc["n_records"] == sc["n_judged"] == sc["n_within"][0] == sc["n_within"][1] == n
    assert sc["sum_e2_q8"] == 0 and sc["n_ignored"] == 0 and sc["n_no_truth"] == 0
    sc = score_batch_gpu(ctx, L[None], R[None], s, np.full((1, H, W), D + 1, np.float32), None, [0.0, 1.0])[0]
    assert sc["n_ignored"] == 0 and sc["n_no_truth"] == 0 and sc["n_records"] == sc["n_judged"] == n
    assert sc["n_within"][0] == 0 and sc["n_within"][1] == n and sc["sum_e2_q8"] == 256 * n


def perturbed_truth(W, H, Ds, seed):
    """the pairs' constant D, perturbed per pixel: fractional parts, some unknown, an ignore mask over a known band"""
    rng = np.random.default_rng(seed)
    P = len(Ds)
    u = np.stack([np.full((H, W), D, np.float32) for D in Ds])
    u += np.where(rng.random((P, H, W)) < 0.4, rng.normal(0, 0.8, (P, H, W)), 0).astype(np.float32)
    u[rng.random((P, H, W)) < 0.05] = np.float32(1e10)
    u[rng.random((P, H, W)) < 0.02] = np.nan
    ign = np.zeros((P, H, W), np.uint8)
    ign[:, H // 3:H // 3 + 6, :] = 200
    return u, ign


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("forest", ["zero", "tau"])
@pytest.mark.parametrize("epipolar,hashtable", MATCHERS)
def test_match_and_score_equals_match_then_score(ctx, oracle, forest_paths, epipolar, hashtable, forest, naive):
    from oracle.pyoracle import sparsematch_settings
    W, H, B = 176, 67, 3
    L, R, Ds = batch_of(oracle, W, H, B)
    s = settings(epipolar, hashtable)
    cap = (W - 26) * (H - 26) + 1
    ctx.set_arithmetic(naive)
    try:
        ctx.load_forest(forest_paths[forest], W, H)
        rc, f = oracle.read_forest(forest_paths[forest], W, H)
        rec, cnt, nc = match_batch_gpu(ctx, L, R, s, cap)
        assert (cnt < cap).all()
        const = np.stack([np.full((H, W), D, np.float32) for D in Ds])
        for u, ign in ((const, None), perturbed_truth(W, H, Ds, 4)):
            got = score_batch_gpu(ctx, L, R, s, u, ign, THR8)
            two = score_records_gpu(ctx, rec, cap, cnt, W, H, u, None, ign, THR8)
            for p in range(B):
                want_rec, nl, nr = oracle.match_pair(L[p], R[p], f, sparsematch_settings(5, 128, 0, epipolar, hashtable, naive))
                want = su.score_records(want_rec, len(want_rec), cap, u[p], None, ign[p] if ign is not None else None, THR8)
                pre = oracle.preprocess_naive if naive else oracle.preprocess
                cl, cr = (su.cand_image(pre(img, 5)[2], W, H) for img in (L[p], R[p]))
                want["n_candidates"], want["n_matchable"] = su.matchable(cl, cr, u[p], None, ign[p] if ign is not None else None)
                same_score(got[p], want, (p, "match-and-score"))
                same_score(two[p], want, (p, "match, then score"), skip=("n_candidates", "n_matchable"))
                assert two[p]["n_candidates"] == two[p]["n_matchable"] == 0 and got[p]["n_candidates"] == nl
                if ign is not None:   # every counter is exercised
                    d = su.as_dict(got[p])
                    assert all(d[k] > 0 for k in su.SCORE_FIELDS if k != "n_within") and min(d["n_within"]) > 0, d
    finally:
        ctx.set_arithmetic(False)


def test_group_mode(oracle):
    import opengpc_amd as g
    W, H, B = 176, 67, 2
    L, R, Ds = batch_of(oracle, W, H, B)
    c = g.Context(0)
    try:
        st, groups = g.read_forest_groups(STRESS, W, H)
        assert st == 0 and len(groups) == 16
        c.set_forest_groups(groups)
        cap = 16 * (W - 26) * (H - 26) + 1
        u, ign = perturbed_truth(W, H, Ds, 6)
        for epipolar in (True, False):
            s = settings(epipolar, False)
            rec, cnt, nc = match_batch_gpu(c, L, R, s, cap)
            assert (cnt > 0).all() and (cnt < cap).all()
            got = score_batch_gpu(c, L, R, s, u, ign, THR8)
            two = score_records_gpu(c, rec, cap, cnt, W, H, u, None, ign, THR8)
            for p in range(B):
                want = su.score_records(rec[p], cnt[p], cap, u[p], None, ign[p], THR8)
                cl, cr = (su.cand_image(oracle.preprocess(img, 5)[2], W, H) for img in (L[p], R[p]))
                want["n_candidates"], want["n_matchable"] = su.matchable(cl, cr, u[p], None, ign[p])
                same_score(got[p], want, (epipolar, p))
                same_score(two[p], want, (epipolar, p), skip=("n_candidates", "n_matchable"))
        with pytest.raises(g.GpcError) as e:
            score_batch_gpu(c, L, R, settings(True, True), u, ign, [1.0])
        assert e.value.status == g.capi.E_UNSUPPORTED
    finally:
        c.close()


def make_frames(W, H, N, seed):
    """N crops of one seeded texture at known integer offsets: the true flow of pair t is the constant (dx_t, dy_t)"""
    rng = np.random.default_rng(seed)
    BW, BH = W + 8 * N + 32, H + 40
    noise = rng.integers(0, 64, (BH, BW))
    base = (rng.integers(0, 256, (BH // 4 + 1, BW // 4 + 1)).repeat(4, 0).repeat(4, 1)[:BH, :BW] * 3 // 4 + noise).astype(np.uint8)
    x, y = 16 + 4 * N, 20
    out, at = [], []
    for t in range(N):
        out.append(base[y:y + H, x:x + W])
        at.append((x, y))
        x -= int(rng.integers(1, 5))      # the crop moves left / up or down: the content moves right (u > 0)
        if t % 2:                         # every second pair keeps its rows (dy = 0): the epipolar matchers find those
            y = 20 + int(rng.integers(-6, 7))
    flow = [(at[t][0] - at[t + 1][0], at[t][1] - at[t + 1][1]) for t in range(N - 1)]
    return np.ascontiguousarray(np.stack(out)), flow


def flow_truth(W, H, flow, seed, perturb=True):
    rng = np.random.default_rng(seed)
    P = len(flow)
    u = np.stack([np.full((H, W), f[0], np.float32) for f in flow])
    v = np.stack([np.full((H, W), f[1], np.float32) for f in flow])
    ign = np.zeros((P, H, W), np.uint8)
    if perturb:
        u += np.where(rng.random((P, H, W)) < 0.3, rng.normal(0, 0.7, (P, H, W)), 0).astype(np.float32)
        v[rng.random((P, H, W)) < 0.04] = np.float32(-1e10)
        ign[:, :, W // 2:W // 2 + 9] = 1
    return u, v, ign


def oracle_sequence(oracle, frames, forest, epipolar, hashtable):
    N, H, W = frames.shape
    pre = [oracle.preprocess(f, 5) for f in frames]
    codes = [oracle.hash(p[0], p[1], forest) for p in pre]
    desc = [oracle.descriptors(codes[k], pre[k][2], W, epipolar) for k in range(N)]
    match = oracle.hash_correspondences if hashtable else oracle.find_correspondences
    return [match(desc[t], pre[t][2], desc[t + 1], pre[t + 1][2], W) for t in range(N - 1)], [su.cand_image(p[2], W, H) for p in pre]


def score_sequence_gpu(ctx, frames, s, u, v, ign, thr):
    import torch
    N, H, W = frames.shape
    d_f, d_u, d_v, d_i = to_dev(frames), to_dev(u), to_dev(v), to_dev(ign)
    d_sc = dev_scores(N - 1)
    torch.cuda.synchronize()
    ctx.score_sequence_device(d_f.data_ptr(), W, H, N, s, d_u.data_ptr(), d_v.data_ptr(), d_i.data_ptr(), thr, d_sc.data_ptr())
    ctx.synchronize()
    return host_scores(d_sc)


@pytest.mark.parametrize("epipolar,hashtable", MATCHERS)
def test_sequences(ctx, oracle, forest_paths, epipolar, hashtable):
    import opengpc_amd as g
    import torch
    W, H, N = 176, 67, 5
    frames, flow = make_frames(W, H, N, 3)
    u, v, ign = flow_truth(W, H, flow, 5)
    s = settings(epipolar, hashtable)
    ctx.load_forest(forest_paths["tau"], W, H)
    rc, f = oracle.read_forest(forest_paths["tau"], W, H)
    want_rec, cands = oracle_sequence(oracle, frames, f, epipolar, hashtable)
    got = score_sequence_gpu(ctx, frames, s, u, v, ign, THR8)
    cap = (W - 26) * (H - 26) + 1
    d_f = to_dev(frames)
    d_out = torch.zeros((N - 1, cap, 4), dtype=torch.int32, device=d_f.device)
    d_cnt = torch.zeros(N - 1, dtype=torch.int32, device=d_f.device)
    torch.cuda.synchronize()
    ctx.match_sequence_device(d_f.data_ptr(), W, H, N, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), 0)
    ctx.synchronize()
    rec = d_out.cpu().numpy().copy().view(g.CORR_DTYPE).reshape(N - 1, cap)
    two = score_records_gpu(ctx, rec, cap, d_cnt.cpu().numpy(), W, H, u, v, ign, THR8)
    for t in range(N - 1):
        want = su.score_records(want_rec[t], len(want_rec[t]), cap, u[t], v[t], ign[t], THR8)
        want["n_candidates"], want["n_matchable"] = su.matchable(cands[t], cands[t + 1], u[t], v[t], ign[t])
        same_score(got[t], want, t)
        same_score(two[t], want, t, skip=("n_candidates", "n_matchable"))
        # not vacuous: the epipolar matchers pair pixels of one row only, so they find the pairs without a vertical offset
        assert want["n_matchable"] > 0
        if not epipolar or flow[t][1] == 0:
            assert want["n_judged"] > 0 and want["n_within"][2] > 0, (t, flow[t])
    assert any(f[1] == 0 for f in flow) and any(f[1] != 0 for f in flow)
    # the host form, frames and truth pageable: the same bytes
    host = ctx.score_sequence(frames, s, u, v, ign, THR8)
    assert host.tobytes() == got.tobytes()


def test_host_forms(oracle, forest_paths):
    """pageable and page-locked inputs, a pair count that is not a multiple of the chunk (16), a sequence over several chunks"""
    import opengpc_amd as g
    W, H, B = 96, 64, 19
    L, R, Ds = batch_of(oracle, W, H, B, 3)
    u, ign = perturbed_truth(W, H, Ds, 11)
    old = os.environ.get("GPC_HIP_SEQ_FRAMES")
    os.environ["GPC_HIP_SEQ_FRAMES"] = "4"
    try:
        c = g.Context(0)
    finally:
        if old is None:
            del os.environ["GPC_HIP_SEQ_FRAMES"]
        else:
            os.environ["GPC_HIP_SEQ_FRAMES"] = old
    try:
        c.load_forest(forest_paths["zero"], W, H)
        for epipolar, hashtable in ((True, False), (False, True)):
            s = settings(epipolar, hashtable)
            dev = score_batch_gpu(c, L, R, s, u, ign, THR8)
            assert c.score_batch(L, R, s, u, ign, THR8).tobytes() == dev.tobytes()
            assert c.score_batch(L, R, s, u, None, [1.0]).tobytes() == score_batch_gpu(c, L, R, s, u, None, [1.0]).tobytes()
            pin = [c.pinned_empty(a.shape, a.dtype) for a in (L, R, u, ign)]
            for dst, src in zip(pin, (L, R, u, ign)):
                dst[...] = src
            assert c.score_batch(pin[0], pin[1], s, pin[2], pin[3], THR8).tobytes() == dev.tobytes()
            frames, flow = make_frames(W, H, 9, 2)
            fu, fv, fi = flow_truth(W, H, flow, 8)
            dev = score_sequence_gpu(c, frames, s, fu, fv, fi, THR8)
            assert c.score_sequence(frames, s, fu, fv, fi, THR8).tobytes() == dev.tobytes()
            pin = [c.pinned_empty(a.shape, a.dtype) for a in (frames, fu, fv, fi)]
            for dst, src in zip(pin, (frames, fu, fv, fi)):
                dst[...] = src
            assert c.score_sequence(pin[0], s, pin[1], pin[2], pin[3], THR8).tobytes() == dev.tobytes()
            assert (dev["n_judged"] > 0)[[f[1] == 0 or not epipolar for f in flow]].all()   # (epipolar: the pairs that keep their rows)
    finally:
        c.close()


def test_refusals(oracle, forest_paths):
    import ctypes as C
    import opengpc_amd as g
    import torch
    W, H, B = 96, 64, 2
    L, R, Ds = batch_of(oracle, W, H, B)
    u = np.stack([np.full((H, W), D, np.float32) for D in Ds])
    c = g.Context(0)
    try:
        lib = c.L
        d_L, d_R, d_u = to_dev(L), to_dev(R), to_dev(u)
        d_sc = dev_scores(B)
        d_rec = torch.zeros((B, 8, 3), dtype=torch.int32, device=d_L.device)
        d_cor = torch.zeros((B, 8, 4), dtype=torch.int32, device=d_L.device)
        d_cnt = torch.zeros(B, dtype=torch.int32, device=d_L.device)
        torch.cuda.synchronize()
        s = g.Settings.sparsematch()
        thr = (C.c_float * 9)(*([1.0] * 9))
        tr = g.capi.Truth(d_u.data_ptr(), None, None)
        trv = g.capi.Truth(d_u.data_ptr(), d_u.data_ptr(), None)

        def batch(truth=tr, t=thr, n=2, sc=d_sc.data_ptr(), left=d_L.data_ptr(), w=W):
            return lib.gpc_hip_score_batch_device(c.h, left, d_R.data_ptr(), w, H, B, C.byref(s), C.byref(truth) if truth else None,
                                                  t, n, sc)

        def records(fn, rec, truth, t=thr, n=2, cnt=d_cnt.data_ptr()):
            return fn(c.h, rec, 8, cnt, W, H, B, C.byref(truth) if truth else None, t, n, d_sc.data_ptr())

        # no forest: the match-and-score forms refuse, the records forms need none
        assert batch() == g.capi.E_NO_FOREST
        assert lib.gpc_hip_score_sequence_device(c.h, d_L.data_ptr(), W, H, B, C.byref(s), C.byref(trv), thr, 2,
                                                 d_sc.data_ptr()) == g.capi.E_NO_FOREST
        assert records(lib.gpc_hip_score_supports_device, d_rec.data_ptr(), tr) == 0
        assert records(lib.gpc_hip_score_correspondences_device, d_cor.data_ptr(), trv) == 0
        c.synchronize()
        assert (host_scores(d_sc)["n_records"] == 0).all()
        c.load_forest(forest_paths["zero"], W, H)
        E = g.capi.E_INVALID
        assert batch(truth=None) == E and batch(sc=None) == E and batch(left=None) == E                       # null pointers
        assert batch(truth=g.capi.Truth(None, None, None)) == E and batch(truth=trv) == E                     # no u; v for supports
        assert batch(n=0) == E and batch(n=9) == E and batch(t=None) == E                                     # threshold counts
        for bad in (-1.0, float("nan"), float("inf")):
            assert batch(t=(C.c_float * 2)(1.0, bad)) == E
        assert batch(w=112) == E                                                                              # not the forest's size
        # the matchable pass loads 16 bytes of a truth plane and 4 ignore bytes at a time: misaligned planes are refused
        assert batch(truth=g.capi.Truth(d_u.data_ptr() + 4, None, None)) == E
        assert batch(truth=g.capi.Truth(d_u.data_ptr(), None, d_u.data_ptr() + 1)) == E
        assert lib.gpc_hip_score_sequence_device(c.h, d_L.data_ptr(), W, H, B, C.byref(s), C.byref(g.capi.Truth(d_u.data_ptr(), d_u.data_ptr() + 8, None)),
                                                 thr, 2, d_sc.data_ptr()) == E
        assert records(lib.gpc_hip_score_supports_device, d_rec.data_ptr(), trv) == E
        assert records(lib.gpc_hip_score_correspondences_device, d_cor.data_ptr(), tr) == E
        assert records(lib.gpc_hip_score_supports_device, None, tr) == E
        assert records(lib.gpc_hip_score_supports_device, d_rec.data_ptr(), tr, cnt=None) == E
        assert records(lib.gpc_hip_score_supports_device, d_rec.data_ptr(), tr, n=0) == E
        host_sc = np.zeros(B, g.SCORE_DTYPE)
        host_tr = g.capi.Truth(u.ctypes.data, u.ctypes.data, None)
        assert lib.gpc_hip_score_sequence(c.h, L.ctypes.data, W, H, 1, C.byref(s), C.byref(host_tr), thr, 1,
                                          host_sc.ctypes.data) == E                                          # one frame
        # after the refused calls the next good call is right
        rc, f = oracle.read_forest(forest_paths["zero"], W, H)
        got = score_batch_gpu(c, L, R, s, u, None, [0.0])
        for p in range(B):
            from oracle.pyoracle import sparsematch_settings
            want_rec, nl, nr = oracle.match_pair(L[p], R[p], f, sparsematch_settings())
            assert got[p]["n_records"] == len(want_rec) and got[p]["n_within"][0] == int((want_rec["d"] == Ds[p]).sum())
        # group mode: sequences refuse
        st, groups = g.read_forest_groups(STRESS, W, H)
        c.set_forest_groups(groups)
        assert lib.gpc_hip_score_sequence_device(c.h, d_L.data_ptr(), W, H, B, C.byref(s), C.byref(trv), thr, 2,
                                                 d_sc.data_ptr()) == g.capi.E_UNSUPPORTED
        with pytest.raises(g.GpcError) as e:
            c.score_sequence(L, s, u[:1], u[:1], None, [1.0])
        assert e.value.status == g.capi.E_UNSUPPORTED
    finally:
        c.close()


@pytest.mark.parametrize("lanes", [1, 2])
def test_batch_after_scoring(oracle, forest_paths, lanes):
    """An ordinary match_batch_device right after scoring calls on the same context still equals the oracle."""
    import opengpc_amd as g
    from oracle.pyoracle import sparsematch_settings
    W, H, B = 320, 112, 4
    L, R, Ds = batch_of(oracle, W, H, B, 9)
    u, ign = perturbed_truth(W, H, Ds, 2)
    c = g.Context(0)
    try:
        c.load_forest(forest_paths["zero"], W, H)
        c.set_pipeline(lanes)
        rc, f = oracle.read_forest(forest_paths["zero"], W, H)
        cap = (W - 26) * (H - 26)
        frames, flow = make_frames(W, H, 4, 1)
        fu, fv, fi = flow_truth(W, H, flow, 3)
        for epipolar in (True, False):
            a = score_batch_gpu(c, L, R, settings(epipolar, False), u, ign, THR8)
            b = score_batch_gpu(c, L, R, settings(False, True), u, ign, THR8)
            score_sequence_gpu(c, frames, settings(epipolar, False), fu, fv, fi, [1.0])
            assert (a["n_judged"] > 0).all() and (b["n_judged"] > 0).all()
            rec, cnt, nc = match_batch_gpu(c, L, R, settings(epipolar, False), cap)
            for p in range(B):
                want, nl, nr = oracle.match_pair(L[p], R[p], f, sparsematch_settings(5, 128, 0, epipolar))
                assert tuple(nc[p]) == (nl, nr) and cnt[p] == len(want), (epipolar, p)
                assert np.array_equal(rec[p, :cnt[p]], want.astype(rec.dtype)), (epipolar, p)
                assert a[p]["n_records"] == len(want)
    finally:
        c.close()


def test_kernel_timing_sees_the_score_kernels(ctx, oracle, forest_paths):
    W, H = 96, 64
    L, R, Ds = batch_of(oracle, W, H, 2)
    ctx.load_forest(forest_paths["zero"], W, H)
    ctx.enable_kernel_timing(True, only=["k_score_records", "k_score_matchable"])
    try:
        ctx.reset_kernel_timing()
        import opengpc_amd as g
        score_batch_gpu(ctx, L, R, g.Settings.sparsematch(), np.zeros((2, H, W), np.float32), None, [1.0])
        t = ctx.kernel_times()
        assert t["k_score_records"][1] == 1 and t["k_score_matchable"][1] == 1 and t["k_hash"][1] == 0
        names = ctx.kernel_launch_names()
        assert names["k_score_records"] == "gpc::k_score_records<false>"
        assert names["k_score_matchable"] == "gpc::k_score_matchable<false, true>"
    finally:
        ctx.enable_kernel_timing(False)


def test_evaluate_sample(oracle, forest_paths, tmp_path):
    """samples/evaluate on a small synthetic Sintel tree (two scenes, 1024 x 436; flow and disparity known by construction):
    the printed totals equal the Python API's on the same frames."""
    import opengpc_amd as g
    W, H, N = 1024, 436, 4
    t = str(tmp_path / "training")
    trees = {}
    for si, scene in enumerate(("alley_1", "alley_2")):
        frames, flow = make_frames(W, H, N, 20 + si)
        occ = np.zeros((N + 1, H, W), np.uint8)
        inv = np.zeros((N + 1, H, W), np.uint8)
        for k in range(1, N + 1):
            occ[k, 100 + 10 * k:140 + 10 * k, 300:500] = 255
            inv[k, 250:300, 600 + 20 * k:700 + 20 * k] = 255
        pairs = [oracle.synth_pair(W, H, 10 * si + k, 7 + k) for k in range(1, N + 1)]
        for k in range(1, N + 1):
            name = "frame_%04d" % k
            su.write_png(os.path.join(t, "clean", scene, name + ".png"), frames[k - 1])
            su.write_png(os.path.join(t, "final", scene, name + ".png"), frames[k - 1])
            su.write_png(os.path.join(t, "clean_left", scene, name + ".png"), pairs[k - 1][0])
            su.write_png(os.path.join(t, "clean_right", scene, name + ".png"), pairs[k - 1][1])
            su.write_png(os.path.join(t, "occlusions", scene, name + ".png"), occ[k])
            su.write_png(os.path.join(t, "invalid", scene, name + ".png"), inv[k])
            su.write_png(os.path.join(t, "outofframe", scene, name + ".png"), inv[k])
            D = 7 + k
            rgb = np.zeros((H, W, 3), np.uint8)
            rgb[..., 0], rgb[..., 1], rgb[..., 2] = D // 4, (D % 4) * 64 + 5, 77
            su.write_png(os.path.join(t, "disparities", scene, name + ".png"), rgb)
            if k < N:
                su.write_flo(os.path.join(t, "flow", scene, name + ".flo"), np.full((H, W), flow[k - 1][0], np.float32),
                             np.full((H, W), flow[k - 1][1], np.float32))
        trees[scene] = (frames, flow, occ, inv, pairs)
    exe = os.path.join(ROOT, "samples", "evaluate")
    thr = [1.0, 3.0]

    def totals(kind, scene, first, count):
        res = subprocess.run([exe, forest_paths["tau"], str(tmp_path), kind, scene, str(first), str(count)] + [str(x) for x in thr],
                             capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        w = [l.split() for l in res.stdout.splitlines() if l.startswith("TOTAL ")][0]
        nfr = [int(l.split()[1]) for l in res.stdout.splitlines() if l.startswith("frames ")][0]
        return nfr, {"n_records": int(w[2]), "n_judged": int(w[4]), "n_within": [int(w[6]), int(w[7])], "n_matchable": int(w[9])}

    c = g.Context(0)
    try:
        c.load_forest(forest_paths["tau"], W, H)
        for scene in ("alley_1", "alley_2"):
            frames, flow, occ, inv, pairs = trees[scene]
            nfr, got = totals("flow", scene, 1, N - 1)
            u = np.stack([np.full((H, W), f[0], np.float32) for f in flow])
            v = np.stack([np.full((H, W), f[1], np.float32) for f in flow])
            ign = np.stack([((occ[k] | occ[k + 1] | inv[k] | inv[k + 1]) != 0).astype(np.uint8) for k in range(1, N)])
            sc = c.score_sequence(frames, settings(False, False), u, v, ign, thr)
            assert nfr == N - 1 and sc["n_records"].sum() > 0 and sc["n_within"][:, 0].sum() > 0
            for k in ("n_records", "n_judged", "n_matchable"):
                assert got[k] == int(sc[k].sum()), (scene, k)
            assert got["n_within"] == [int(sc["n_within"][:, 0].sum()), int(sc["n_within"][:, 1].sum())]
            nfr, got = totals("stereo", scene, 2, 2)
            L = np.stack([pairs[k][0] for k in (1, 2)])
            R = np.stack([pairs[k][1] for k in (1, 2)])
            du = np.stack([np.full((H, W), 7 + k, np.float32) for k in (2, 3)])
            ign = np.stack([((occ[k] | inv[k]) != 0).astype(np.uint8) for k in (2, 3)])
            sc = c.score_batch(L, R, g.Settings.sparsematch(), du, ign, thr)
            assert nfr == 2 and sc["n_within"][:, 0].sum() > 0
            for k in ("n_records", "n_judged", "n_matchable"):
                assert got[k] == int(sc[k].sum()), (scene, k)
            assert got["n_within"] == [int(sc["n_within"][:, 0].sum()), int(sc["n_within"][:, 1].sum())]
    finally:
        c.close()


@pytest.mark.parametrize("flow", [False, True])
def test_cpp_score_records(ctx, tmp_path, flow):
    """gpc::evaluation::scoreSupports / scoreCorrespondences (tests/cpp/evaluation_gpu_check.cpp) give the Score of the Python
    records form on the same records, with and without an ignore mask; no records and inconsistent Truth planes are handled."""
    from test_host_api import BIN, compile_cpp, run
    exe = compile_cpp(os.path.join(ROOT, "tests", "cpp", "evaluation_gpu_check.cpp"), os.path.join(BIN, "evaluation_gpu_check"))
    W, H, n = 176, 67, 5000
    rng = np.random.default_rng(11 + int(flow))
    u, v, ign = random_truth(rng, 1, H, W, flow)
    rec = random_records(rng, 1, n, [n], W, H, u, v)
    thr = [0.0, 1.0, 3.0]
    rec[0].tofile(str(tmp_path / "rec.bin"))
    u[0].tofile(str(tmp_path / "u.bin"))
    if flow:
        v[0].tofile(str(tmp_path / "v.bin"))
    ign[0].tofile(str(tmp_path / "ign.bin"))
    for mask in (ign, None):
        out = run(exe, str(W), str(H), str(tmp_path / "rec.bin"), str(n), "corr" if flow else "supports", str(tmp_path / "u.bin"),
                  str(tmp_path / "v.bin") if flow else "-", str(tmp_path / "ign.bin") if mask is not None else "-", *[str(t) for t in thr])
        words = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.splitlines() if l.split() and l.split()[0] in ("SCORE", "EMPTY", "REFUSED")}
        want = score_records_gpu(ctx, rec, n, [n], W, H, u, v, mask, thr)[0]
        assert words["SCORE"] == [int(x) for x in np.frombuffer(want.tobytes(), np.int64)]
        assert want["n_judged"] > 0 and want["n_within"][1] > 0 and (mask is None) == (want["n_ignored"] == 0)
        assert words["EMPTY"] == [0, 0, 0] and words["REFUSED"] == [1, 1, 1]
