"""Group mode on the GPU: every group matched as a forest of its own, united group-major (include/gpc_hip.h,
gpc_hip_set_forest_groups).  Expected values: the oracle run once per group (the group's own forest text), united in numpy."""
import os
import subprocess

import numpy as np
import pytest

from forest_groups_util import forest_text, group_texts, union

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRESS = os.path.join(ROOT, "forests", "stress16x20Forest.txt")
SUPP_KEY = ("x", "y", "d")
CORR_KEY = ("sx", "sy", "tx", "ty")


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def gsettings(epipolar=True, hashtable=False):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epipolar, hashtable, 1)


def oracle_union_pair(oracle, texts, L, R, epipolar=True, naive=False):
    from oracle.pyoracle import sparsematch_settings
    H, W = L.shape
    per = []
    nc = None
    for t in texts:
        rc, f = oracle.parse_forest_text(t, W, H)
        assert rc == 0
        supp, nl, nr = oracle.match_pair(L, R, f, sparsematch_settings(5, 128, 0, epipolar, naive=naive))
        per.append(supp)
        nc = (nl, nr)
    return union(per, SUPP_KEY), nc


def oracle_union_corr(oracle, texts, pl, pr, epipolar):
    H, W = pl[0].shape
    per = []
    for t in texts:
        rc, f = oracle.parse_forest_text(t, W, H)
        cl = oracle.hash(pl[0], pl[1], f)
        cr = oracle.hash(pr[0], pr[1], f)
        per.append(oracle.find_correspondences(oracle.descriptors(cl, pl[2], W, epipolar), pl[2],
                                               oracle.descriptors(cr, pr[2], W, epipolar), pr[2], W))
    return union(per, CORR_KEY)


def same_supports(got, want):
    assert len(got) == len(want)
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["y"], want["y"])
    assert np.array_equal(got["d"], want["d"].astype(got["d"].dtype))


def same_corr(got, want):
    assert len(got) == len(want)
    for a, b in (("src_x", "sx"), ("src_y", "sy"), ("tar_x", "tx"), ("tar_y", "ty")):
        assert np.array_equal(got[a], want[b])


@pytest.mark.parametrize("name", ["defaultZeroForest.txt", "defaultTauForest.txt"])
@pytest.mark.parametrize("epipolar", [True, False])
def test_default_forests_give_todays_results(ctx, oracle, name, epipolar):
    import opengpc_amd as g
    path = os.path.join(ROOT, "forests", name)
    W, H = 320, 120
    L, R = oracle.synth_pair(W, H, 3, 11)
    ctx.load_forest(path, W, H)
    want, n0, nc0, _ = ctx.match_pair(L, R, gsettings(epipolar))
    st, groups = g.read_forest_groups(path, W, H)
    assert st == 0 and len(groups) == 1
    ctx.set_forest_groups(groups)
    got, n, nc, st = ctx.match_pair(L, R, gsettings(epipolar))
    assert st == 0 and n == n0 and nc == nc0 and np.array_equal(got, want)


@pytest.mark.parametrize("W,H", [(256, 96), (1008, 77), (4352, 64)])
@pytest.mark.parametrize("epipolar", [True, False])
def test_stress_forest_match_pair(ctx, oracle, W, H, epipolar):
    L, R = oracle.synth_pair(W, H, 5, 17)
    ctx.load_forest_groups(STRESS, W, H)
    want, nc = oracle_union_pair(oracle, group_texts(open(STRESS).read()), L, R, epipolar)
    got, n, ncg, st = ctx.match_pair(L, R, gsettings(epipolar))
    assert st == 0 and ncg == nc
    same_supports(got, want)


@pytest.mark.parametrize("W,H", [(256, 96), (1008, 77)])
def test_stress_forest_preprocessed_paths(ctx, oracle, W, H):
    L, R = oracle.synth_pair(W, H, 7, 9)
    texts = group_texts(open(STRESS).read())
    ctx.load_forest_groups(STRESS, W, H)
    pl, pr = oracle.preprocess(L, 5), oracle.preprocess(R, 5)
    for epi in (True, False):
        want = oracle_union_corr(oracle, texts, pl, pr, epi)
        got, n, st = ctx.stereo_match(pl, pr, gsettings(epi))       # upload path (copies of the arrays)
        assert st == 0
        same_corr(got, want)
    want, _ = oracle_union_pair(oracle, texts, L, R, True)
    got, n, st = ctx.rectified_match(pl, pr, gsettings(True))
    assert st == 0
    same_supports(got, want)
    # resident path: the arrays the library delivered
    hits = ctx.resident_hits()
    rl, rr = ctx.preprocess_resident(L, 5), ctx.preprocess_resident(R, 5)
    got, n, st = ctx.rectified_match(rl, rr, gsettings(True))
    assert st == 0 and ctx.resident_hits() == hits + 1
    same_supports(got, want)
    got, n, st, _ = ctx.match_async("stereo", rl, rr, gsettings(False))
    assert st == 0
    same_corr(got, oracle_union_corr(oracle, texts, pl, pr, False))


@pytest.mark.parametrize("W,H", [(256, 96), (1008, 77)])
def test_hash_codes_groups(ctx, oracle, W, H):
    import opengpc_amd as g
    L, _ = oracle.synth_pair(W, H, 2, 13)
    sm, gr, _ = oracle.preprocess(L, 5)
    groups = ctx.load_forest_groups(STRESS, W, H)
    codes = ctx.hash_codes_groups(sm, gr)
    assert codes.shape == (16, H, W)
    for k, t in enumerate(group_texts(open(STRESS).read())):
        rc, f = oracle.parse_forest_text(t, W, H)
        assert np.array_equal(codes[k], oracle.hash(sm, gr, f)), k
    with pytest.raises(g.GpcError) as e:
        ctx.hash_codes(sm, gr)
    assert e.value.status == g.capi.E_UNSUPPORTED
    ctx.set_forest(groups[3])   # outside group mode: one plane, the forest's
    one = ctx.hash_codes_groups(sm, gr)
    assert one.shape == (1, H, W) and np.array_equal(one[0], codes[3])


def test_configs4_all_320_tests():
    """BASELINE configs[4] as written: 3840x2160, s = 2, D = 64, the stress forest's 16 trees x 20 tests."""
    import opengpc_amd as g
    from oracle.pyoracle import Oracle
    fast = Oracle(fast=True)
    W, H = 3840, 2160
    L, R = fast.synth_pair(W, H, 2, 64)
    c = g.Context(0)
    try:
        c.load_forest_groups(STRESS, W, H)
        got, n, nc, st = c.match_pair(L, R, gsettings(True))
    finally:
        c.close()
    want, ncw = oracle_union_pair(fast, group_texts(open(STRESS).read()), L, R, True)
    assert st == 0 and nc == ncw and n > 0
    same_supports(got, want)


def test_match_batch_device_32_pairs(ctx):
    import torch
    from opengpc_amd.synth import synth_batch
    from oracle.pyoracle import Oracle
    oracle = Oracle(fast=True)
    W, H, B = 1024, 436, 32
    Lh, Rh = synth_batch(W, H, list(range(B)))
    ctx.load_forest_groups(STRESS, W, H)
    dev = torch.device("cuda", 0)
    cap = 16 * (W - 26) * (H - 26)
    d_L, d_R = torch.from_numpy(Lh).to(dev), torch.from_numpy(Rh).to(dev)
    d_out = torch.empty((B, cap, 3), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    d_nc = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, gsettings(True), d_out.data_ptr(), cap,
                           d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    cnt, nc = d_cnt.cpu().numpy(), d_nc.cpu().numpy()
    texts = group_texts(open(STRESS).read())
    for p in range(B):
        rec = d_out[p, :cnt[p]].cpu().numpy().copy().view(np.dtype([("x", "<i4"), ("y", "<i4"), ("d", "<f4")])).reshape(-1)
        want, ncw = oracle_union_pair(oracle, texts, Lh[p], Rh[p], True)
        assert tuple(nc[p]) == ncw, p
        same_supports(rec, want)
        if p in (0, 17):   # batch == single
            single, n, ncs, st = ctx.match_pair(Lh[p], Rh[p], gsettings(True))
            assert st == 0 and np.array_equal(single.view(np.uint8), rec.view(np.uint8))


def test_naive_two_32_test_groups(oracle):
    """Naive arithmetic, two ferns of 32 tests: both groups use WIDE codes and bit 31."""
    import opengpc_amd as g
    text = forest_text([32, 32], seed=5)
    W, H = 272, 90
    L, R = oracle.synth_pair(W, H, 4, 9)
    c = g.Context(0)
    try:
        c.set_arithmetic(True)
        st, groups = g.parse_forest_groups(text, W, H)
        assert st == 0 and [x.num_tests for x in groups] == [32, 32]
        c.set_forest_groups(groups)
        sm, gr, mk = oracle.preprocess_naive(L, 5)
        codes = c.hash_codes_groups(sm, gr)
        texts = group_texts(text)
        for k, t in enumerate(texts):
            rc, f = oracle.parse_forest_text(t, W, H)
            assert np.array_equal(codes[k], oracle.hash_naive(sm, mk, f)), k
        assert any((codes[k] >> 31).any() for k in range(2))
        got, n, nc, st = c.match_pair(L, R, gsettings(True))
        want, ncw = oracle_union_pair(oracle, texts, L, R, True, naive=True)
        assert st == 0 and nc == ncw
        same_supports(got, want)
    finally:
        c.close()


def test_refusals_capacity_and_leaving_group_mode(ctx, oracle):
    import ctypes as C
    import torch
    import opengpc_amd as g
    W, H = 256, 96
    L, R = oracle.synth_pair(W, H, 3, 11)
    tau = os.path.join(ROOT, "forests", "defaultTauForest.txt")
    ctx.load_forest(tau, W, H)
    before, nb, _, _ = ctx.match_pair(L, R, gsettings(True))
    ctx.load_forest_groups(STRESS, W, H)
    for fn in (lambda: ctx.match_pair(L, R, gsettings(True, True)),
               lambda: ctx.match_batch(L[None], R[None], gsettings(True), 4096),
               lambda: ctx.match_batch_packed(L[None], R[None], gsettings(True), 4096),
               lambda: ctx.set_pipeline(2)):
        with pytest.raises(g.GpcError) as e:
            fn()
        assert e.value.status == g.capi.E_UNSUPPORTED
    dev = torch.device("cuda", 0)
    d_L, d_R = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    buf = torch.zeros(1 << 20, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    with pytest.raises(g.GpcError) as e:
        ctx.match_batch_device_packed(d_L.data_ptr(), d_R.data_ptr(), W, H, 1, gsettings(True), buf.data_ptr(), 4096,
                                      buf.data_ptr() + 4 * 500000, buf.data_ptr() + 4 * 600000)
    assert e.value.status == g.capi.E_UNSUPPORTED
    # capacity: the true union count and its first `cap` records
    full, n, _, st = ctx.match_pair(L, R, gsettings(True))
    assert st == 0 and n > 10
    part, n2, _, st2 = ctx.match_pair(L, R, gsettings(True), cap=n // 3)
    assert st2 == g.capi.E_CAPACITY and n2 == n and np.array_equal(part, full[:n // 3])
    # set_forest leaves group mode: today's results again
    ctx.load_forest(tau, W, H)
    after, na, _, st = ctx.match_pair(L, R, gsettings(True))
    assert st == 0 and na == nb and np.array_equal(after, before)


def test_cpp_read_forest_groups_match_pair(oracle, tmp_path):
    W, H = 320, 112
    L, R = oracle.synth_pair(W, H, 6, 19)
    (tmp_path / "L.raw").write_bytes(L.tobytes())
    (tmp_path / "R.raw").write_bytes(R.tobytes())
    out = os.path.join(ROOT, "tests", "cpp", "bin", "forest_groups_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "forest_groups_check.cpp"), "-o", out,
                           "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-pthread"])
    res = subprocess.run([out, STRESS, str(W), str(H), str(tmp_path / "L.raw"), str(tmp_path / "R.raw")],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = {l.split()[0]: l.split()[1:] for l in res.stdout.splitlines() if l.split() and l.split()[0] in ("GROUPS", "RESULT")}
    assert lines["GROUPS"] == ["16"] + ["20"] * 16
    from oracle.pyoracle import supports_fnv
    want, nc = oracle_union_pair(oracle, group_texts(open(STRESS).read()), L, R, True)
    n, cl, cr, h = (int(v) for v in lines["RESULT"])
    assert (n, cl, cr) == (len(want), nc[0], nc[1]) and h == supports_fnv(oracle, want)


def test_warmup_in_group_mode(oracle):
    """gpc_hip_warmup on a fresh context in group mode (no hash-table matcher, no gpc_hip_match_batch), then a match."""
    import opengpc_amd as g
    W, H = 320, 112
    c = g.Context(0)
    try:
        c.load_forest_groups(STRESS, W, H)
        c.warmup(W, H)
        c.warmup(W, H, gsettings(False))
        L, R = oracle.synth_pair(W, H, 6, 19)
        got, n, nc, st = c.match_pair(L, R, gsettings(True))
    finally:
        c.close()
    want, ncw = oracle_union_pair(oracle, group_texts(open(STRESS).read()), L, R, True)
    assert st == 0 and nc == ncw
    same_supports(got, want)
