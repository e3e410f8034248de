"""Who frees what, on the GPU: every feature that makes device blocks, page-locked blocks, streams or events of its own
works on a context of its own, the context is destroyed, and the four process-wide counts of gpc_hip_debug_live_resources
(device blocks, device bytes, page-locked blocks, streams + events) are back where they were.  One case per feature, so a
failure names the owner that was forgotten.  96x64 images, at most 4 pairs or 5 frames per call: every lazily made resource
is still created at that size."""
import contextlib
import gc

import numpy as np
import pytest

from devicewide_util import make_ctx

pytestmark = pytest.mark.gpu

W, H, P = 96, 64, 4
CAP = (W - 26) * (H - 26)


def live():
    from opengpc_amd.capi import live_resources
    gc.collect()   # (a context another test dropped without closing goes now, not between two readings)
    return live_resources()


@contextlib.contextmanager
def balanced(env=None, forest="zero", groups=False):
    """a context with a forest; on the way out it is destroyed and the counts must be back.  Yields (ctx, grew), grew() true
    once the counts exceed what the bare context holds."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    before = live()
    ctx = make_ctx(env)
    try:
        if groups:
            assert len(ctx.load_forest_groups(os.path.join(root, "forests", "stress16x20Forest.txt"), W, H)) >= 2
        else:
            ctx.load_forest(os.path.join(root, "forests", "default%sForest.txt" % forest.capitalize()), W, H)
        bare = live()
        yield ctx, lambda: any(a > b for a, b in zip(live(), bare))
        ctx.synchronize()
    finally:
        ctx.close()
    assert live() == before, "left behind (device blocks, device bytes, page-locked blocks, streams + events)"


def pairs(n=P):
    from opengpc_amd.synth import synth_batch
    return synth_batch(W, H, list(range(n)))


def frames(n=5):
    from opengpc_amd.synth import synth_pair
    return np.stack([synth_pair(W, H, 3, 4 + 2 * t)[0] for t in range(n)])


def settings(epipolar=True, hashtable=False):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epipolar, hashtable, 1)


def device_batch(ctx, st, n=P, cap=CAP, corr=False):
    """match_batch_device (corr: match_sequence_device over n + 1 frames) of torch tensors; returns (records, counts) bytes"""
    import torch
    dev = torch.device("cuda", 0)
    d_out = torch.zeros(n * cap * (16 if corr else 12), dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    if corr:
        d_f = torch.from_numpy(frames(n + 1)).to(dev)
        ctx.match_sequence_device(d_f.data_ptr(), W, H, n + 1, st, d_out.data_ptr(), cap, d_cnt.data_ptr())
    else:
        L, R = pairs(n)
        d_L, d_R = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
        ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, n, st, d_out.data_ptr(), cap, d_cnt.data_ptr())
    ctx.synchronize()
    cnt = d_cnt.cpu().numpy()
    assert (cnt > 0).all(), cnt
    return d_out.cpu().numpy(), cnt


@pytest.mark.parametrize("packed", [False, True])
def test_host_batch_of_pageable_images(packed):
    """chunk streams and events, h_stage, h_in, h_cnt, the expansion pool"""
    L, R = pairs()
    with balanced() as (ctx, grew):
        if packed:
            counts = ctx.match_batch_packed(L, R, settings(), CAP)[2]
        else:
            counts = ctx.match_batch(L, R, settings(), CAP)[1]
        assert (counts > 0).all() and grew()


def test_single_pair_and_two_step_forms():
    """h_xfer, h_cnt"""
    L, R = pairs(1)
    with balanced() as (ctx, grew):
        a = ctx.match_pair(L[0], R[0], settings())
        b = ctx.match_async("pair", L[0], R[0], settings())
        assert a[1] > 0 and a[1] == b[1] and np.array_equal(a[0], b[0]) and grew()


def test_preprocess_begin_and_fetch():
    """h_pre, e_pre, the resident images"""
    L, _ = pairs(1)
    with balanced() as (ctx, grew):
        smooth, grad, mask = ctx.preprocess_resident(L[0], 5)
        assert len(mask) > 0 and grew()


def test_group_mode():
    """gforest_dev, vstats, vcand, vout, vcnt, vncand, uplane, ublk, gdense: a forest of 16 groups through
    match_batch_device, epipolar and not, and through the single-pair host form, whose union stays in gdense until it is
    fetched.  (gpc_hip_match_sequence_device refuses group mode: asserted, so that the case grows when that changes.)"""
    import opengpc_amd as g
    L, R = pairs(1)
    with balanced(groups=True) as (ctx, grew):
        device_batch(ctx, settings(True), cap=16 * CAP)
        device_batch(ctx, settings(False), cap=16 * CAP)
        assert ctx.match_pair(L[0], R[0], settings())[1] > 0
        with pytest.raises(g.GpcError) as refused:
            device_batch(ctx, settings(False), cap=16 * CAP, corr=True)
        assert refused.value.status == g.capi.E_UNSUPPORTED and grew()


@pytest.mark.parametrize("hashtable", [False, True])
def test_device_wide_matchers(hashtable):
    """s_aux, e_fork, e_join, e_flag, h_flag, gpart, gkv"""
    with balanced() as (ctx, grew):
        device_batch(ctx, settings(False, hashtable))
        assert grew()


def test_fused_join():
    """jstate, h_err"""
    with balanced({"GPC_HIP_FUSE_ALWAYS": 1}) as (ctx, grew):
        device_batch(ctx, settings())
        assert "fused" in ctx.kernel_launch_names()["k_row_join"] and grew()


def test_two_lanes():
    """the lanes' streams, events and swapped workspaces"""
    with balanced() as (ctx, grew):
        ctx.set_pipeline(2)
        got = [device_batch(ctx, settings()) for _ in range(3)]
        ctx.set_pipeline(1)
        assert all(np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]) for g in got) and grew()


def test_kernel_timing():
    """the event pairs of spans and free_spans"""
    with balanced() as (ctx, grew):
        ctx.enable_kernel_timing(True)
        device_batch(ctx, settings())
        assert ctx.kernel_times()["k_hash"][1] >= 1
        ctx.reset_kernel_timing()
        device_batch(ctx, settings())
        assert grew()


def test_host_forms_of_score_track_consensus_refine_pyramid():
    """stage, e_stage, all_*, tr_*, cs_*, py_*"""
    L, R = pairs()
    f = frames()
    with balanced() as (ctx, grew):
        scores = ctx.score_batch(L, R, settings(), np.zeros((P, H, W), np.float32), None, [1.0])
        assert len(scores) == P
        corr, counts, _, _, _, rows, ntracks, st = ctx.track_sequence(f, settings(False))
        assert st == 0 and (counts > 0).all() and ntracks > 0
        assert ctx.consensus_records(corr, counts, W, H)[4] == 0
        supp, scounts, _, st = ctx.match_batch(L, R, settings(), CAP)
        assert st == 0
        ctx.refine_records(supp, scounts, L, R)
        _, pcounts, _, _, st = ctx.pyramid_batch(L, R, 2, settings(), 2 * CAP)
        assert st == 0 and (pcounts > 0).all() and grew()


def triplets(n=300):
    return np.random.default_rng(5).integers(0, 256, (n, 3, 729), dtype=np.uint8)


def test_train_set():
    from opengpc_amd import SPLIT_DTYPE
    with balanced() as (ctx, grew):
        t = ctx.train_set(triplets())
        t.begin_fern(True)
        cand = np.array([(1, 700, 0), (30, 31, 2), (364, 5, -1), (100, 600, 0)], SPLIT_DTYPE)
        tp, fp, tot = t.eval_level(cand, -2, 3)
        assert tot == 300 and tp.shape == (4, 5) and grew()
        t.marks()
        t.close()


def extracted(ctx):
    L, R = pairs(2)
    rng = np.random.default_rng(9)
    pts = np.stack([rng.integers(21, W - 20, 40), rng.integers(21, H - 20, 40)] * 3, axis=1).astype(np.int32)
    t = ctx.extract_triplets(L, R, pts, [0, 25, 40])
    assert t is not None and t.n == 40
    return t


def test_extract_triplets():
    """ext_* (given back by the call itself), the set's planes and flags"""
    with balanced() as (ctx, grew):
        t = extracted(ctx)
        assert grew()
        t.close()


def test_track_stream():
    f = frames()
    with balanced() as (ctx, grew):
        s = ctx.track_stream(W, H, settings(False), CAP, 4 * CAP)
        assert s.push(f[:3])[6] == 0 and s.push(f[3:])[6] == 0
        assert s.state()[:2] == (5, 4) and grew()
        s.close()


def test_children_left_open():
    """a context destroyed with a train set (made by hand and by extraction) and a track stream still open"""
    with balanced() as (ctx, grew):
        ctx.train_set(triplets(64)).begin_fern(True)
        extracted(ctx)
        s = ctx.track_stream(W, H, settings(False), CAP, 4 * CAP)
        assert s.push(frames(3))[6] == 0 and grew()


def test_two_contexts():
    """both have worked; one goes; the other gives the same records as before, byte for byte"""
    before = live()
    with balanced() as (a, _):
        first = device_batch(a, settings())
        with balanced(forest="tau") as (b, _):
            device_batch(b, settings(False, True))
            device_batch(a, settings())   # (the same call again: nothing of a's grows while b is counted)
            device_batch(b, settings())
        again = device_batch(a, settings())
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    assert live() == before
