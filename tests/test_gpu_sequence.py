"""Frame sequences on the GPU (gpc_hip_match_sequence[_device]): result t is Forest::stereoMatch of (frame t, frame t + 1),
record for record.  Expected values: the oracle's preprocess -> hash -> descriptors -> find_correspondences (or
hash_correspondences for the hash-table matcher) per pair, and the pair entry point itself."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCHERS = [(True, False), (False, False), (True, True), (False, True)]   # (epipolar_mode, use_hashtable)


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def settings(epipolar, hashtable):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epipolar, hashtable, 1)


def frames_of(W, H, N, seed):
    """N crops of one seeded texture at offsets that move in x and y (so non-epipolar matches have ty != sy)."""
    rng = np.random.default_rng(seed)
    BW, BH = W + 8 * N + 32, H + 40
    noise = rng.integers(0, 64, (BH, BW))
    base = (rng.integers(0, 256, (BH // 4 + 1, BW // 4 + 1)).repeat(4, 0).repeat(4, 1)[:BH, :BW] * 3 // 4 + noise).astype(np.uint8)
    out = []
    x, y = 16, 20
    for t in range(N):
        out.append(base[y:y + H, x:x + W])
        x += int(rng.integers(1, 8))
        y = 20 + int(rng.integers(-12, 13))
    return np.ascontiguousarray(np.stack(out))


def oracle_sequence(oracle, frames, forest, epipolar, hashtable, naive=False):
    """[records of pair t] and candidates per frame"""
    N, H, W = frames.shape
    pre, codes = [], []
    for f in frames:
        if naive:
            s, gr, m = oracle.preprocess_naive(f, 5)
            codes.append(oracle.hash_naive(s, m, forest))
        else:
            s, gr, m = oracle.preprocess(f, 5)
            codes.append(oracle.hash(s, gr, forest))
        pre.append(m)
    desc = [oracle.descriptors(codes[k], pre[k], W, epipolar) for k in range(N)]
    match = oracle.hash_correspondences if hashtable else oracle.find_correspondences
    return [match(desc[t], pre[t], desc[t + 1], pre[t + 1], W) for t in range(N - 1)], [len(m) for m in pre]


def same_corr(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for a, b in (("src_x", "sx"), ("src_y", "sy"), ("tar_x", "tx"), ("tar_y", "ty")):
        assert np.array_equal(got[a], want[b]), (what, a)


def run_device(ctx, frames, s, cap):
    """match_sequence_device through torch tensors -> (records [N-1, cap], counts, ncand)"""
    import opengpc_amd as g
    import torch
    N, H, W = frames.shape
    dev = torch.device("cuda", 0)
    d_f = torch.from_numpy(frames).to(dev)
    d_out = torch.full((N - 1, cap, 4), -7, dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(N - 1, dtype=torch.int32, device=dev)
    d_nc = torch.zeros(N, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.match_sequence_device(d_f.data_ptr(), W, H, N, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    rec = d_out.cpu().numpy().copy().view(g.CORR_DTYPE).reshape(N - 1, cap)
    return rec, d_cnt.cpu().numpy(), d_nc.cpu().numpy()


def check_all(ctx, oracle, frames, forest, s, naive=False, cap=None, host=True):
    N, H, W = frames.shape
    cap = cap or (W - 26) * (H - 26)
    want, ncw = oracle_sequence(oracle, frames, forest, s.epipolar_mode, s.use_hashtable, naive)
    rec, cnt, nc = run_device(ctx, frames, s, cap)
    assert list(nc) == ncw
    for t in range(N - 1):
        assert cnt[t] == len(want[t]), t
        same_corr(rec[t, :cnt[t]], want[t], t)
    if host:  # the host form gives the same bytes
        out, hc, hn, st = ctx.match_sequence(frames, s, cap)
        assert st == 0 and np.array_equal(hc, cnt) and np.array_equal(hn, nc)
        for t in range(N - 1):
            assert np.array_equal(out[t, :cnt[t]].view(np.uint8), rec[t, :cnt[t]].view(np.uint8)), t
    return rec, cnt, nc


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("forest", ["zero", "tau"])
@pytest.mark.parametrize("epipolar,hashtable", MATCHERS)
def test_every_matcher_arithmetic_and_forest(ctx, oracle, forest_paths, epipolar, hashtable, forest, naive):
    W, H, N = 176, 67, 5
    frames = frames_of(W, H, N, 3)
    ctx.set_arithmetic(naive)
    try:
        ctx.load_forest(forest_paths[forest], W, H)
        rc, f = oracle.read_forest(forest_paths[forest], W, H)
        check_all(ctx, oracle, frames, f, settings(epipolar, hashtable), naive)
    finally:
        ctx.set_arithmetic(False)


@pytest.mark.parametrize("W,H", [(48, 41), (160, 101), (1936, 120)])
@pytest.mark.parametrize("epipolar,hashtable", MATCHERS)
def test_odd_shapes(ctx, oracle, forest_paths, W, H, epipolar, hashtable):
    frames = frames_of(W, H, 4, W + H)
    ctx.load_forest(forest_paths["tau"], W, H)
    rc, f = oracle.read_forest(forest_paths["tau"], W, H)
    check_all(ctx, oracle, frames, f, settings(epipolar, hashtable))


@pytest.mark.parametrize("epipolar,hashtable", MATCHERS)
def test_33_frames_1024x436(ctx, forest_paths, epipolar, hashtable):
    """33 frames: the device form in one call, the host form in three chunks of <= 16 frames."""
    from oracle.pyoracle import Oracle
    oracle = Oracle(fast=True)
    W, H, N = 1024, 436, 33
    frames = frames_of(W, H, N, 33)
    ctx.load_forest(forest_paths["zero"], W, H)
    rc, f = oracle.read_forest(forest_paths["zero"], W, H)
    check_all(ctx, oracle, frames, f, settings(epipolar, hashtable))


def test_flat_and_saturated_frames(ctx, oracle, forest_paths):
    """Flat frames (no candidates) and saturated ones (heavily repeated codes: the device-wide matchers' radix-sort
    fallbacks) inside one sequence."""
    W, H = 176, 67
    rng = np.random.default_rng(8)
    sat = np.where(rng.random((H, W)) < 0.5, 0, 255).astype(np.uint8)
    flat = np.full((H, W), 77, np.uint8)
    tex = frames_of(W, H, 2, 9)
    frames = np.ascontiguousarray(np.stack([tex[0], flat, flat, sat, sat, np.roll(sat, 3, 1), tex[1]]))
    ctx.load_forest(forest_paths["zero"], W, H)
    rc, f = oracle.read_forest(forest_paths["zero"], W, H)
    for epipolar, hashtable in MATCHERS:
        rec, cnt, nc = check_all(ctx, oracle, frames, f, settings(epipolar, hashtable))
        assert nc[1] == nc[2] == 0 and cnt[1] == 0


def test_host_chunks_and_pinned_frames(oracle, forest_paths):
    """GPC_HIP_SEQ_FRAMES=4: sequences of K + 1 and 2K + 3 frames span chunk boundaries; pageable and page-locked
    frames give the device form's bytes."""
    import opengpc_amd as g
    W, H = 160, 101
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
        c.load_forest(forest_paths["tau"], W, H)
        rc, f = oracle.read_forest(forest_paths["tau"], W, H)
        cap = (W - 26) * (H - 26)
        for N in (5, 11):
            frames = frames_of(W, H, N, N)
            for epipolar, hashtable in ((True, False), (False, False), (False, True)):
                s = settings(epipolar, hashtable)
                rec, cnt, nc = check_all(c, oracle, frames, f, s)
                pinned = c.pinned_empty(frames.shape, np.uint8)
                pinned[...] = frames
                out, hc, hn, st = c.match_sequence(pinned, s, cap)
                assert st == 0 and np.array_equal(hc, cnt) and np.array_equal(hn, nc)
                for t in range(N - 1):
                    assert np.array_equal(out[t, :cnt[t]].view(np.uint8), rec[t, :cnt[t]].view(np.uint8)), (N, t)
    finally:
        c.close()


def test_equals_stereo_match(ctx, forest_paths):
    W, H, N = 176, 67, 4
    frames = frames_of(W, H, N, 12)
    ctx.load_forest(forest_paths["tau"], W, H)
    pre = [ctx.preprocess(fr, 5) for fr in frames]
    for epipolar, hashtable in MATCHERS:
        s = settings(epipolar, hashtable)
        out, cnt, nc, st = ctx.match_sequence(frames, s)
        assert st == 0 and list(nc) == [len(p[2]) for p in pre]
        for t in range(N - 1):
            got, n, st1 = ctx.stereo_match(pre[t], pre[t + 1], s)
            assert st1 == 0 and n == cnt[t]
            assert np.array_equal(got.view(np.uint8), out[t, :n].view(np.uint8)), (epipolar, hashtable, t)


def test_capacity(ctx, oracle, forest_paths):
    """A capacity of half the largest pair, every matcher.  The host form returns GPC_E_CAPACITY, the true counts and each
    pair's first records.  The device form only queues work (the device-wide matchers wait for their plan, not for the
    counts), so it returns GPC_OK and leaves the true counts in d_counts; it runs on outputs filled with 0xA5 that hold a
    spare pair's worth of slots behind the last pair, a spare count and a spare candidate word, and every byte is compared:
    the first min(count, cap) records of each pair, the fill in every other slot."""
    import torch
    import opengpc_amd as g
    from devicewide_util import FILL32, compare, corr_words, expected, filled
    W, H, N = 176, 67, 4
    frames = frames_of(W, H, N, 21)
    ctx.load_forest(forest_paths["zero"], W, H)
    rc, f = oracle.read_forest(forest_paths["zero"], W, H)
    dev = torch.device("cuda", 0)
    d_f = torch.from_numpy(frames).to(dev)
    for epipolar, hashtable in MATCHERS:
        s = settings(epipolar, hashtable)
        want, ncw = oracle_sequence(oracle, frames, f, epipolar, hashtable)
        cap = max(len(w) for w in want) // 2
        assert cap > 10
        out, cnt, nc, st = ctx.match_sequence(frames, s, cap)
        assert st == g.capi.E_CAPACITY and list(cnt) == [len(w) for w in want] and list(nc) == ncw
        d_out, d_cnt, d_nc = filled(N * cap * 16, dev), filled(N * 4, dev), filled((N + 1) * 4, dev)
        torch.cuda.synchronize(dev)
        st = ctx.L.gpc_hip_match_sequence_device(ctx.h, d_f.data_ptr(), W, H, N, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
        assert st == 0, (epipolar, hashtable, st)
        ctx.synchronize()
        dcnt, dnc = d_cnt.cpu().numpy().view(np.int32), d_nc.cpu().numpy().view(np.int32)
        assert list(dcnt[:N - 1]) == list(cnt) and list(dnc[:N]) == ncw
        assert dcnt[N - 1:].view(np.uint32) == FILL32 and dnc[N:].view(np.uint32) == FILL32, "a count behind the sequence's was written"
        words = [corr_words(w) for w in want]
        compare(d_out.cpu().numpy().view(np.uint32).reshape(N, cap, 4), expected(words, cap), words,
                "epipolar %d, hash table %d, cap %d" % (epipolar, hashtable, cap))
        for t in range(N - 1):
            k = min(cap, len(want[t]))
            same_corr(out[t, :k], want[t][:k], t)


def test_refusals(oracle, forest_paths):
    import ctypes as C
    import opengpc_amd as g
    W, H = 96, 64
    frames = frames_of(W, H, 3, 1)
    c = g.Context(0)
    try:
        with pytest.raises(g.GpcError) as e:   # no forest yet
            c.match_sequence(frames, settings(True, False))
        assert e.value.status == g.capi.E_NO_FOREST
        c.load_forest(forest_paths["zero"], W, H)
        with pytest.raises(g.GpcError) as e:   # one frame
            c.match_sequence(frames[:1], settings(True, False))
        assert e.value.status == g.capi.E_INVALID
        with pytest.raises(g.GpcError) as e:   # frames of another size than the forest's
            c.match_sequence(np.zeros((3, 64, 112), np.uint8), settings(True, False))
        assert e.value.status == g.capi.E_INVALID
        # a pending _begin may still write the page-locked arena: it is waited for and ended, the sequence is right
        L = c.L
        assert L.gpc_hip_preprocess_begin(c.h, frames[0].ctypes.data, W, H, 5) == 0
        out, cnt, nc, st = c.match_sequence(frames, settings(True, False))
        assert st == 0
        rc, f = oracle.read_forest(forest_paths["zero"], W, H)
        want, ncw = oracle_sequence(oracle, frames, f, True, False)
        assert list(nc) == ncw and list(cnt) == [len(w) for w in want]
        for t in range(2):
            same_corr(out[t, :cnt[t]], want[t], t)
        sm, gr, mk = np.empty((H, W), np.uint8), np.empty((H, W), np.uint8), np.empty(W * H, np.int32)
        n = C.c_int()
        assert L.gpc_hip_preprocess_fetch(c.h, sm.ctypes.data, gr.ctypes.data, mk.ctypes.data, W * H,
                                          C.byref(n)) == g.capi.E_INVALID
        # group mode
        st, groups = g.read_forest_groups(os.path.join(ROOT, "forests", "stress16x20Forest.txt"), W, H)
        assert st == 0 and len(groups) == 16
        c.set_forest_groups(groups)
        for fn in (lambda: c.match_sequence(frames, settings(True, False)),):
            with pytest.raises(g.GpcError) as e:
                fn()
            assert e.value.status == g.capi.E_UNSUPPORTED
        import torch
        dev = torch.device("cuda", 0)
        d_f = torch.from_numpy(frames).to(dev)
        d_out = torch.zeros((2, 16, 4), dtype=torch.int32, device=dev)
        d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        assert c.L.gpc_hip_match_sequence_device(c.h, d_f.data_ptr(), W, H, 3, settings(True, False), d_out.data_ptr(), 16,
                                                 d_cnt.data_ptr(), None) == g.capi.E_UNSUPPORTED
    finally:
        c.close()


@pytest.mark.parametrize("lanes", [1, 2])
def test_batch_after_sequence(oracle, forest_paths, lanes):
    """An ordinary match_batch_device right after a sequence call on the same context still matches the oracle."""
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
        for epipolar in (True, False):
            frames = frames_of(W, H, 6, 40)
            run_device(c, frames, settings(False, False), cap)      # a sequence with the device-wide matcher ...
            c.match_sequence(frames, settings(True, False), cap)    # ... and one with the epipolar join
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
    finally:
        c.close()


def _fnv_corr(rec):
    h = 1469598103934665603
    for b in np.ascontiguousarray(np.stack([rec["sx"], rec["sy"], rec["tx"], rec["ty"]], 1).astype("<i4")).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_sequence_match(oracle, forest_paths, tmp_path):
    """Forest::sequenceMatch == Forest::stereoMatch per pair == the oracle."""
    W, H, N = 176, 67, 4
    frames = frames_of(W, H, N, 5)
    (tmp_path / "f.raw").write_bytes(frames.tobytes())
    out = os.path.join(ROOT, "tests", "cpp", "bin", "sequence_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sequence_check.cpp"), "-o", out,
                           "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-pthread"])
    rc, f = oracle.read_forest(forest_paths["tau"], W, H)
    for epipolar, hashtable in ((True, False), (False, True)):
        res = subprocess.run([out, forest_paths["tau"], str(W), str(H), str(N), str(tmp_path / "f.raw"), str(int(epipolar)),
                              str(int(hashtable))], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        rows = [l.split() for l in res.stdout.splitlines() if l.split() and l.split()[0] in ("PAIR", "STEREO")]
        seq = {int(r[1]): (int(r[2]), int(r[3])) for r in rows if r[0] == "PAIR"}
        ste = {int(r[1]): (int(r[2]), int(r[3])) for r in rows if r[0] == "STEREO"}
        want, _ = oracle_sequence(oracle, frames, f, epipolar, hashtable)
        assert len(seq) == len(ste) == N - 1
        for t in range(N - 1):
            assert seq[t] == ste[t] == (len(want[t]), _fnv_corr(want[t])), (epipolar, hashtable, t)
