"""Match refinement on the GPU (gpc_hip_refine_*): sub-pixel shifts, costs and flags EQUAL the plain restatement of the rule
(tests/refine_util.py) byte for byte -- every output starts out filled with a sentinel, so the entries a call must leave alone
are compared too -- for constructed records at every window border, the extremes of the cost, the records of the four
matchers; the match-and-refine forms write what the plain match writes; the refined supports go to the score call as they
are; the host forms equal the device forms; refusals leave the outputs alone."""
import ctypes as C

import numpy as np
import pytest

import refine_util as ru
import score_util as su
import track_util as tu

pytestmark = pytest.mark.gpu

MATCHERS = [(True, False), (False, False), (True, True), (False, True)]   # (epipolar_mode, use_hashtable)
FILL = 0xA5


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


def refine_device(ctx, rec, counts, imgL, imgR, radius, with_out=True):
    """the records form over host records [P, cap] and images [P, H, W]: (ref, out) read back from sentinel-filled outputs"""
    import torch
    P, cap = rec.shape
    corr = rec.dtype == ru.CORR
    H, W = imgL.shape[1:]
    d_rec = dev(rec.view(np.uint8).reshape(P, cap, rec.dtype.itemsize))
    d_cnt, d_L, d_R = dev(np.asarray(counts, np.int32)), dev(imgL), dev(imgR)
    d_ref, d_out = filled(P, cap, 8), filled(P, cap, 12)
    torch.cuda.synchronize()
    ctx.refine_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), d_L.data_ptr(), d_R.data_ptr(), W, H, P, radius,
                              d_ref.data_ptr(), 0 if corr or not with_out else d_out.data_ptr())
    ctx.synchronize()
    return d_ref.cpu().numpy().view(ru.REFINEMENT).reshape(P, cap), d_out.cpu().numpy().view(ru.SUPPORT).reshape(P, cap)


def same(got, want, what):
    for k, name in enumerate(("ref", "out")):
        if want[k] is not None:
            a, b = np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)
            if not np.array_equal(a, b):
                bad = np.nonzero((a.reshape(-1, got[k].dtype.itemsize) != b.reshape(-1, got[k].dtype.itemsize)).any(axis=1))[0]
                raise AssertionError((what, name, len(bad), bad[:5].tolist(), got[k].reshape(-1)[bad[:5]], want[k].reshape(-1)[bad[:5]]))


def check_records(ctx, rec, counts, imgL, imgR, radius, what):
    want = ru.expected_arrays(rec, counts, imgL, imgR, radius, FILL)
    got = refine_device(ctx, rec, counts, imgL, imgR, radius)
    same(got, want, what)
    if want[1] is None:
        assert (got[1].view(np.uint8) == FILL).all()
    return want


def border_records(W, H, r, corr):
    """every window inequality exactly met and exceeded by one -- source, target, the target's shifts in x (and in y for
    correspondences) -- as (x, y, tx, ty); the last entries are the last admissible windows of the image"""
    cx, cy = W // 2, H // 2
    out = []
    for x in (r - 1, r, W - 1 - r, W - r):
        out.append((x, cy, cx, cy))
    for y in (r - 1, r, H - 1 - r, H - r):
        out.append((cx, y, cx, y if not corr else cy))
    for tx in (r, r + 1, W - 2 - r, W - 1 - r):
        out.append((cx, cy, tx, cy))
    if corr:
        for ty in (r, r + 1, H - 2 - r, H - 1 - r):
            out.append((cx, cy, cx, ty))
        out.append((W - 1 - r, H - 1 - r, W - 2 - r, H - 2 - r))
        out.append((r, r, r + 1, r + 1))
    else:
        out.append((r, r, r + 1, r))
        out.append((W - 2 - r, H - 1 - r, W - 2 - r, H - 1 - r))
        out.append((W - 1 - r, H - 1 - r, W - 2 - r, H - 1 - r))
    return out


def constructed(W, H, r, corr, seed, cap=96):
    """records [3, cap] and counts: pair 0 has a negative count, pair 1 a count above the slots, pair 2 holds the border
    records last (the last admissible window of the LAST image among them); random records near and across every border,
    duplicates, supports with a d that is no whole number, NaN, both infinities, 2^24 and beyond"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((3, cap), ru.CORR if corr else ru.SUPPORT)
    border = border_records(W, H, r, corr)
    for t in range(3):
        m = cap
        x, y = rng.integers(-2, W + 2, m), rng.integers(-2, H + 2, m)
        near = rng.random(m) < 0.5                              # half of them where most windows fit
        x = np.where(near, rng.integers(r, max(W - r, r + 1), m), x)
        y = np.where(near, rng.integers(r, max(H - r, r + 1), m), y)
        tx = np.where(near, np.clip(x + rng.integers(-3, 4, m), r + 1, max(W - 2 - r, r + 1)), x + rng.integers(-W, W, m))
        ty = np.where(near, np.clip(y + rng.integers(-3, 4, m), r + 1, max(H - 2 - r, r + 1)), y + rng.integers(-4, 5, m))
        pts = np.stack([x, y, tx, ty], 1)
        pts[m - len(border):] = border
        dup = rng.integers(0, m - len(border), 8)               # duplicated records
        pts[dup] = pts[dup[::-1]]
        if corr:
            rec[t]["src_x"], rec[t]["src_y"], rec[t]["tar_x"], rec[t]["tar_y"] = pts.T
        else:
            rec[t]["x"], rec[t]["y"], rec[t]["d"] = pts[:, 0], pts[:, 1], (pts[:, 0] - pts[:, 2]).astype(np.float32)
            rec[t]["d"][rng.choice(m - len(border), 9, replace=False)] = (0.5, -3.25, np.nan, np.inf, -np.inf, 2.0 ** 24, -2.0 ** 24,
                                                                          3e38, 16777218.0)
    return rec, np.array([-3, cap + 7, cap], np.int32)


@pytest.mark.parametrize("corr", [False, True])
@pytest.mark.parametrize("r", [1, 3, 6])
@pytest.mark.parametrize("W,H", [(48, 40), (37, 23), (1040, 30)])
def test_constructed_records(ctx, W, H, r, corr):
    """random images; 37 wide: no row starts on a dword; 1040x30: long rows, offsets beyond 2^14"""
    rng = np.random.default_rng(W + r)
    imgL = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    imgR = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    rec, counts = constructed(W, H, r, corr, 100 * r + corr)
    ref, out = check_records(ctx, rec, counts, imgL, imgR, r, (W, H, r, corr))
    assert (ref[0].view(np.uint8) == FILL).all()                         # a negative count: nothing read, nothing written
    assert (ref[1].view(np.uint8) != FILL).any(axis=None) and (ref[1]["flags"] < 8).all()   # a count above the slots reads them all
    ev = (ref[2]["flags"] & 1) != 0
    assert 20 < ev.sum() < len(ev) - 8
    assert ev[-1] and ev[-2]                                             # the last admissible windows of the last image
    nb = len(border_records(W, H, r, corr))
    assert ev[-nb:].sum() == {False: 6 + 3, True: 8 + 2}[corr]           # met: evaluated; exceeded by one: not
    if not corr:
        got = refine_device(ctx, rec, counts, imgL, imgR, r, with_out=False)    # no refined supports wanted: the rest is the same
        same(got, (ref, None), "no out")
        assert (got[1].view(np.uint8) == FILL).all()


def test_extremes(ctx):
    rng = np.random.default_rng(11)
    W, H = 64, 33
    centre = lambda corr, m=40: inner_records(rng, W, H, 6, m, corr)
    for corr in (False, True):
        # all 0 against all 255 at r = 6: the largest cost there is, on every shift -- no minimum
        L, R = np.zeros((1, H, W), np.uint8), np.full((1, H, W), 255, np.uint8)
        rec = centre(corr)
        ref, _ = check_records(ctx, rec, [rec.shape[1]], L, R, 6, ("0 / 255", corr))
        assert (ref["cost"] == 43095).all() and (ref["flags"] == 1).all() and (ref["dx_q8"] == 0).all()
        # a flat pair
        L = R = np.full((1, H, W), 77, np.uint8)
        ref, _ = check_records(ctx, rec, [rec.shape[1]], L, R, 6, ("flat", corr))
        assert (ref["cost"] == 0).all() and (ref["flags"] == 1).all()
        # an image with real 0 pixels inside every window (a masked sum would skip them), against a bright one
        L = rng.integers(1, 256, (1, H, W)).astype(np.uint8)
        L[rng.random((1, H, W)) < 0.4] = 0
        R = rng.integers(128, 256, (1, H, W)).astype(np.uint8)
        for a, b in ((L, R), (R, L), (L, L)):
            for r in (1, 2, 3, 4, 5, 6):
                check_records(ctx, rec, [rec.shape[1]], a, b, r, ("zeros", corr, r))
    # the right image is the left one moved by one pixel: R[y][x] = L[y][x + 1], so a support with d = 1 sits on cost 0
    # and one with d = 0 has its cost 0 at the shift -1: c0 > c-, no minimum
    L = rng.integers(0, 256, (1, H, W)).astype(np.uint8)
    R = np.roll(L, -1, axis=2)
    rec = centre(False)
    rec["d"][0, ::2], rec["d"][0, 1::2] = 1.0, 0.0
    for r in (1, 3, 6):
        ref, out = check_records(ctx, rec, [rec.shape[1]], L, R, r, ("moved", r))
        assert (ref["cost"][0, ::2] == 0).all() and (ref["flags"][0, ::2] == 3).all()
        assert (ref["cost"][0, 1::2] > 0).all() and (ref["flags"][0, 1::2] == 1).all()
    # ... and moved in y for correspondences
    R = np.roll(L, -1, axis=1)
    rec = centre(True)
    rec["tar_x"], rec["tar_y"] = rec["src_x"], rec["src_y"] - 1
    ref, _ = check_records(ctx, rec, [rec.shape[1]], L, R, 3, "moved in y")
    assert (ref["cost"] == 0).all() and (ref["flags"] == 7).all()


def inner_records(rng, W, H, r, m, corr):
    """[1, m] records whose windows all fit, targets within 2 pixels of their sources"""
    x, y = rng.integers(r + 3, W - r - 3, m), rng.integers(r + 3, H - r - 3, m)
    if corr:
        rec = np.zeros((1, m), ru.CORR)
        rec["src_x"], rec["src_y"] = x, y
        rec["tar_x"], rec["tar_y"] = x + rng.integers(-2, 3, m), y + rng.integers(-2, 3, m)
    else:
        rec = np.zeros((1, m), ru.SUPPORT)
        rec["x"], rec["y"], rec["d"] = x, y, rng.integers(-2, 3, m).astype(np.float32)
    return rec


def sequence_device(ctx, frames, s, cap, radius=None):
    """match_sequence_device (radius None) or refine_sequence_device over sentinel-filled outputs"""
    import torch
    N, H, W = frames.shape
    d_f = dev(frames)
    d_out, d_cnt, d_nc, d_ref = filled(N - 1, cap, 16), filled(N - 1, 4), filled(N, 4), filled(N - 1, cap, 8)
    torch.cuda.synchronize()
    if radius is None:
        ctx.match_sequence_device(d_f.data_ptr(), W, H, N, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
    else:
        ctx.refine_sequence_device(d_f.data_ptr(), W, H, N, s, radius, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr(),
                                   d_ref.data_ptr())
    ctx.synchronize()
    return (d_out.cpu().numpy().view(ru.CORR).reshape(N - 1, cap), d_cnt.cpu().numpy().view(np.int32).reshape(-1),
            d_nc.cpu().numpy().view(np.int32).reshape(-1), d_ref.cpu().numpy().view(ru.REFINEMENT).reshape(N - 1, cap))


@pytest.mark.parametrize("W,H", [(160, 101), (1040, 77)])
@pytest.mark.parametrize("epipolar,hashtable", MATCHERS)
def test_match_and_refine_sequence(ctx, forest_paths, W, H, epipolar, hashtable):
    """the frame sets of tests/track_util.py, zero forest: refine_sequence_device writes match_sequence_device's records,
    counts and candidates, and the restatement of their refinement; again after an unrelated batch of another size"""
    import torch
    frames = tu.frames_of(W, H, 6, 1, 0 if epipolar else 12)
    ctx.load_forest(forest_paths["zero"], W, H)
    s = settings(epipolar, hashtable)
    cap = (W - 26) * (H - 26)
    rec, cnt, nc, untouched = sequence_device(ctx, frames, s, cap)
    assert (untouched.view(np.uint8) == FILL).all() and cnt.min() > 50
    want, _ = ru.expected_arrays(rec, cnt, frames[:-1], frames[1:], 3, FILL)
    ev = np.concatenate([(want[t, :cnt[t]]["flags"] & 1) for t in range(len(cnt))])
    mn = np.concatenate([(want[t, :cnt[t]]["flags"] & 6) == 6 for t in range(len(cnt))])
    print("records %d, evaluated %d, minimum on both axes %d" % (len(ev), ev.sum(), mn.sum()))
    assert ev.sum() > len(ev) // 2 and mn.sum() > 0

    def check(what):
        rec2, cnt2, nc2, ref = sequence_device(ctx, frames, s, cap, 3)
        assert np.array_equal(cnt2, cnt) and np.array_equal(nc2, nc), what
        assert np.array_equal(rec2.view(np.uint8), rec.view(np.uint8)), what
        same((ref, None), (want, None), (what, W, H, epipolar, hashtable))

    check("first")
    # an unrelated batch of another size on the same context
    from opengpc_amd import synth
    bw, bh, B = 96, 64, 2
    ctx.load_forest(forest_paths["zero"], bw, bh)
    bl, br = synth.synth_batch(bw, bh, range(B))
    bcap = (bw - 26) * (bh - 26)
    d_l, d_r, d_s, d_c, d_n, d_f = dev(bl), dev(br), filled(B, bcap, 12), filled(B, 4), filled(B, 2, 4), filled(B, bcap, 8)
    torch.cuda.synchronize()
    ctx.refine_batch_device(d_l.data_ptr(), d_r.data_ptr(), bw, bh, B, settings(True, False), 2, d_s.data_ptr(), bcap, d_c.data_ptr(),
                            d_n.data_ptr(), d_f.data_ptr())
    ctx.synchronize()
    ctx.load_forest(forest_paths["zero"], W, H)
    check("again")


@pytest.mark.parametrize("lanes", [1, 2])
def test_match_and_refine_batch(forest_paths, lanes):
    """8 synthetic pairs of 160x101, epipolar: supports, counts and candidates equal a plain match_batch_device, d_ref the
    restatement, and d_out goes to gpc_hip_score_supports_device as it is: the scores equal score_util on the same floats"""
    import opengpc_amd as g
    import torch
    from opengpc_amd import synth
    W, H, B = 160, 101, 8
    c = g.Context(0)
    try:
        c.load_forest(forest_paths["zero"], W, H)
        c.set_pipeline(lanes)
        Lh, Rh = synth.synth_batch(W, H, range(B))
        d_L, d_R = dev(Lh), dev(Rh)
        cap = (W - 26) * (H - 26)
        s = settings(True, False)
        d_sup, d_cnt, d_nc = filled(B, cap, 12), filled(B, 4), filled(B, 2, 4)
        torch.cuda.synchronize()
        c.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, d_sup.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
        c.synchronize()
        rec = d_sup.cpu().numpy().view(ru.SUPPORT).reshape(B, cap)
        cnt, nc = d_cnt.cpu().numpy().view(np.int32).reshape(-1), d_nc.cpu().numpy().view(np.int32).reshape(B, 2)
        assert cnt.min() > 100
        want_ref, want_out = ru.expected_arrays(rec, cnt, Lh, Rh, 3, FILL)
        d_sup2, d_cnt2, d_nc2, d_ref, d_out = filled(B, cap, 12), filled(B, 4), filled(B, 2, 4), filled(B, cap, 8), filled(B, cap, 12)
        torch.cuda.synchronize()
        c.refine_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, 3, d_sup2.data_ptr(), cap, d_cnt2.data_ptr(),
                              d_nc2.data_ptr(), d_ref.data_ptr(), d_out.data_ptr())
        c.synchronize()
        assert np.array_equal(d_sup2.cpu().numpy(), d_sup.cpu().numpy())
        assert np.array_equal(d_cnt2.cpu().numpy(), d_cnt.cpu().numpy()) and np.array_equal(d_nc2.cpu().numpy(), d_nc.cpu().numpy())
        got_out = d_out.cpu().numpy().view(ru.SUPPORT).reshape(B, cap)
        same((d_ref.cpu().numpy().view(ru.REFINEMENT).reshape(B, cap), got_out), (want_ref, want_out), ("batch", lanes))
        moved = sum(int((want_ref[t, :cnt[t]]["dx_q8"] != 0).sum()) for t in range(B))
        print("records %d, with a sub-pixel shift %d" % (cnt.sum(), moved))
        assert moved > 0
        # the refined supports, as they lie on the device, against a truth that is no whole number
        rng = np.random.default_rng(3)
        u = (np.arange(B)[:, None, None] % 64 + 8 + rng.integers(-4, 5, (B, H, W)) / 8.0).astype(np.float32)
        d_u = dev(u)
        d_sc = torch.full((B, 15), -3, dtype=torch.int64, device=torch.device("cuda", 0))
        thr = [0.25, 1.0]
        torch.cuda.synchronize()
        c.score_supports_device(d_out.data_ptr(), cap, d_cnt2.data_ptr(), W, H, B, d_u.data_ptr(), 0, thr, d_sc.data_ptr())
        c.synchronize()
        got = d_sc.cpu().numpy().copy().view(g.SCORE_DTYPE).reshape(-1)
        for t in range(B):
            want = su.score_records(got_out[t], cnt[t], cap, u[t], None, None, thr)
            have = su.as_dict(got[t])
            for k in ("n_records", "n_ignored", "n_no_truth", "n_judged", "n_within", "sum_e2_q8"):
                assert have[k] == want[k], (t, k)
    finally:
        c.close()


def test_host_forms(ctx):
    """19 pairs (two chunks of at most 16) of 48x40: the host forms, from pageable and from page-locked arrays, leave the bytes
    the device forms leave, untouched entries included"""
    W, H, r, P = 48, 40, 2, 19
    rng = np.random.default_rng(23)
    imgL = rng.integers(0, 256, (P, H, W)).astype(np.uint8)
    imgR = np.roll(imgL, 1, axis=2)
    imgR[rng.random((P, H, W)) < 0.2] = 0
    for corr in (False, True):
        rec = np.concatenate([constructed(W, H, r, corr, 7 + k, cap=64)[0] for k in range(7)])[:P]
        counts = rng.integers(0, 64, P).astype(np.int32)
        counts[[1, 5, 17]] = (64 + 9, -1, 64)
        want = ru.expected_arrays(rec, counts, imgL, imgR, r, FILL)
        same(refine_device(ctx, rec, counts, imgL, imgR, r), want, ("device", corr))
        for what, alloc in (("pageable", np.empty), ("page-locked", ctx.pinned_empty)):
            hrec, hl, hr = alloc(rec.shape, rec.dtype), alloc(imgL.shape, np.uint8), alloc(imgR.shape, np.uint8)
            hrec[...], hl[...], hr[...] = rec, imgL, imgR
            ref, out = alloc(rec.shape, ru.REFINEMENT), None if corr else alloc(rec.shape, ru.SUPPORT)
            ref.view(np.uint8)[...] = FILL
            if out is not None:
                out.view(np.uint8)[...] = FILL
            got = ctx.refine_records(hrec, counts, hl, hr, r, ref, out)
            assert got[0] is ref and got[1] is out
            same(got, want, (what, corr))


def test_refusals(forest_paths):
    """every refusal of the group, and the outputs afterwards: not a byte written"""
    import opengpc_amd as g
    import torch
    W, H = 96, 64
    E, U = g.capi.E_INVALID, g.capi.E_UNSUPPORTED
    c = g.Context(0)
    try:
        L = c.L
        d_rec, d_ref, d_out = filled(2, 64, 16), filled(2, 64, 8), filled(2, 64, 12)
        d_cnt = dev(np.array([10, 20], np.int32))
        d_img = dev(tu.frames_of(W, H, 3, 1))
        iL, iR = d_img.data_ptr(), d_img.data_ptr() + W * H
        torch.cuda.synchronize()

        def recs(fn, rec=d_rec.data_ptr(), cap=64, cnt=d_cnt.data_ptr(), l=iL, r_=iR, w=W, h=H, npairs=2, radius=3, ref=d_ref.data_ptr(),
                 out=d_out.data_ptr()):
            args = [c.h, rec, cap, cnt, l, r_, w, h, npairs, radius, ref]
            return fn(*(args + [out] if fn is L.gpc_hip_refine_supports_device else args))

        for fn in (L.gpc_hip_refine_supports_device, L.gpc_hip_refine_correspondences_device):
            for radius in (0, -1, 7, 100):
                assert recs(fn, radius=radius) == E, radius
            assert recs(fn, rec=None) == E and recs(fn, cnt=None) == E and recs(fn, l=None) == E and recs(fn, r_=None) == E
            assert recs(fn, ref=None) == E and recs(fn, npairs=0) == E and recs(fn, cap=0) == E and recs(fn, w=0) == E and recs(fn, h=-1) == E
            assert recs(fn, npairs=65536, cap=1) == U and recs(fn, cap=1 << 20, npairs=2048) == U      # npairs * cap = 2^31
            assert recs(fn, w=1 << 15, h=(1 << 15) + 1, npairs=1) == U                                 # width * height > 2^30
        fn = L.gpc_hip_refine_supports_device
        assert recs(fn, out=d_rec.data_ptr()) == E and recs(fn, out=d_rec.data_ptr() + 12 * 100) == E  # out inside the records
        # host forms: the same checks on host arrays
        hrec, hcnt = np.zeros((2, 64), g.SUPPORT_DTYPE), np.array([3, 4], np.int32)
        himg = np.zeros((3, H, W), np.uint8)
        href, hout = np.full((2, 64, 8), FILL, np.uint8), np.full((2, 64, 12), FILL, np.uint8)
        host = lambda radius=3, out=hout.ctypes.data, npairs=2, ref=href.ctypes.data: L.gpc_hip_refine_supports(
            c.h, hrec.ctypes.data, 64, hcnt.ctypes.data, himg.ctypes.data, himg[1:].ctypes.data, W, H, npairs, radius, ref, out)
        assert host(radius=0) == E and host(radius=7) == E and host(out=hrec.ctypes.data) == E and host(npairs=0) == E
        assert host(ref=None) == E and host(npairs=65536) == U
        assert (href == FILL).all() and (hout == FILL).all()
        # match-and-refine forms: their own refusals and those of the match they wrap
        s = settings(True, False)
        d_corr, d_sup, d_n, d_nc = filled(2, 64, 16), filled(2, 64, 12), filled(2, 4), filled(3, 2, 4)
        seq = lambda nframes=3, radius=3, ref=d_ref.data_ptr(), corr=d_corr.data_ptr(), st=s, w=W: L.gpc_hip_refine_sequence_device(
            c.h, iL, w, H, nframes, C.byref(st), radius, corr, 64, d_n.data_ptr(), d_nc.data_ptr(), ref)
        bat = lambda npairs=2, radius=3, ref=d_ref.data_ptr(), sup=d_sup.data_ptr(), out=d_out.data_ptr(), st=s, w=W: L.gpc_hip_refine_batch_device(
            c.h, iL, iR, w, H, npairs, C.byref(st), radius, sup, 64, d_n.data_ptr(), d_nc.data_ptr(), ref, out)
        assert seq() == g.capi.E_NO_FOREST and bat() == g.capi.E_NO_FOREST
        c.load_forest(forest_paths["zero"], W, H)
        for call in (seq, bat):
            assert call(radius=0) == E and call(radius=7) == E and call(ref=None) == E and call(w=W + 1) == E
        assert seq(nframes=1) == E and seq(corr=None) == E and bat(npairs=0) == E and bat(sup=None) == E
        assert bat(out=d_sup.data_ptr()) == E
        import os
        st, groups = g.read_forest_groups(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "forests",
                                                       "stress16x20Forest.txt"), W, H)
        assert st == 0 and len(groups) == 16
        c.set_forest_groups(groups)
        assert seq() == U                                            # group-mode sequences, as the sequence itself
        assert bat(st=settings(True, True)) == U                     # ... and the hash table in group mode, as the batch itself
        c.synchronize()
        for d in (d_ref, d_out, d_corr, d_sup, d_n, d_nc):
            assert bool((d == FILL).all())
        assert (d_rec == FILL).all()
        # after all of them the calls still work
        c.load_forest(forest_paths["zero"], W, H)
        assert seq() == 0 and bat() == 0 and recs(L.gpc_hip_refine_correspondences_device) == 0
        c.synchronize()
        assert not bool((d_ref == FILL).all())
    finally:
        c.close()
