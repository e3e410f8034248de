"""Dense maps from sparse matches on the GPU (gpc_hip_densify_*): every byte of value and level EQUALS the plain restatement
of the rule (tests/dense_util.py) -- every output starts out filled with a sentinel, and every pixel must be written -- for
random and constructed records at sizes below, across and well above a 32-pixel tile, both record types, every parameter; the
match-and-fill forms equal match, refine and the records form; the host forms equal the device forms; the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import dense_util as du
import track_util as tu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
SIZES = [(1, 1), (7, 5), (33, 17), (96, 64), (130, 67), (200, 90)]   # 200x90: 7 x 3 tiles, levels 6 .. 8 above the tile


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def settings(epipolar, hashtable=False):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epipolar, hashtable, 1)


def P_(prm):
    import opengpc_amd as g
    return g.Densify(*prm)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def filled(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def planes(d_val, d_lev, P, Cn, H, W):
    return d_val.cpu().numpy().view(np.int32).reshape(P, Cn, H, W), d_lev.cpu().numpy().reshape(P, H, W)


def dense_device(ctx, rec, counts, W, H, prm=du.DEFAULTS, ref=None, with_level=True):
    """the records form over host records [P, cap]: (value, level) read back from sentinel-filled outputs"""
    import torch
    P, cap = rec.shape
    corr = rec.dtype == du.CORR
    Cn = 2 if corr else 1
    d_rec = dev(rec.view(np.uint8).reshape(P, cap, rec.dtype.itemsize))
    d_cnt = dev(np.asarray(counts, np.int32))
    d_ref = dev(ref.view(np.uint8).reshape(P, cap, 8)) if ref is not None else None
    d_val, d_lev = filled(P, Cn, H, W, 4), filled(P, H, W)
    torch.cuda.synchronize()
    ctx.densify_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, P_(prm), d_val.data_ptr(),
                               d_lev.data_ptr() if with_level else 0, d_ref.data_ptr() if d_ref is not None else 0)
    ctx.synchronize()
    return planes(d_val, d_lev, P, Cn, H, W)


def same(got, want, what):
    for k, name in enumerate(("value", "level")):
        if not np.array_equal(got[k], want[k]):
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError((what, name, len(bad), bad[:4].tolist(), [got[k][tuple(b)] for b in bad[:4]],
                                  [want[k][tuple(b)] for b in bad[:4]]))


def check(ctx, rec, counts, W, H, prm=du.DEFAULTS, ref=None, what=None):
    want = du.densify(rec, counts, W, H, prm, ref)
    same(dense_device(ctx, rec, counts, W, H, prm, ref), want, (what, W, H, prm))
    return want


@pytest.mark.parametrize("corr", [False, True])
@pytest.mark.parametrize("W,H", SIZES)
def test_random_records_every_parameter(ctx, W, H, corr):
    """two pairs of random records (sources and targets outside the image, duplicates, supports whose d is no whole number
    among them; the right-hand third of the image empty): spread 0 and 1 x min_count 1, 2, unreachable x max_level 1, 3, 15"""
    rng = np.random.default_rng(1000 * W + H + corr)
    m = max(W * H // 7, 1)
    cap = m + 5
    rec = np.stack([du.random_records(rng, W, H, m, corr, cap), du.random_records(rng, W, H, max(m // 9, 1), corr, cap, hole=False)])
    counts = [m, max(m // 9, 1)]
    seen = set()
    for spread in (0, 1):
        for min_count in (1, 2, W * H + 1):
            for max_level in (1, 3, 15):
                _, level = check(ctx, rec, counts, W, H, (max_level, min_count, spread, 0xFFFF), None, corr)
                seen |= set(np.unique(level).tolist())
                if min_count > W * H:
                    assert set(np.unique(level).tolist()) <= {0, 255}
    if W >= 96:
        assert {0, 1, 2, 3, 255} <= seen and max(seen - {255}) >= 6, seen      # pixels filled from above the tile


def test_empty_list_and_counts(ctx):
    """an empty list: everything none, level 255; counts negative, zero and above the slots; pairs of different counts"""
    W, H = 33, 17
    rng = np.random.default_rng(3)
    for corr in (False, True):
        rec = np.stack([du.random_records(rng, W, H, 40, corr, 40, hole=False) for _ in range(5)])
        rec[2] = rec[4]
        counts = [-4, 0, 40 + 11, 7, 40]
        value, level = check(ctx, rec, counts, W, H, du.DEFAULTS, None, ("counts", corr))
        for t in (0, 1):
            assert (value[t] == du.NONE).all() and (level[t] == 255).all()
        assert np.array_equal(value[2], value[4]) and not np.array_equal(value[3], value[4])
        assert (level[2:] != 255).all()


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (33, 17), (130, 67), (200, 90)])
def test_one_record_in_a_corner_fills_the_image(ctx, W, H):
    """min_count 1, max_level 15: the top cell holds the record, so every pixel is valid and equals its value"""
    for corr in (False, True):
        for x, y in {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)}:
            rec = np.zeros((1, 3), du.CORR if corr else du.SUPPORT)
            if corr:
                rec[0, 0] = (x, y, W - 1 - x, H - 1 - y)
                vals = (256 * (W - 1 - 2 * x), 256 * (H - 1 - 2 * y))
            else:
                d = x if x else -(W - 1)
                rec[0, 0] = (x, y, float(d))
                vals = (256 * d,)
            value, level = check(ctx, rec, [1], W, H, du.DEFAULTS, None, ("corner", corr, x, y))
            for c, v in enumerate(vals):
                assert (value[0, c] == v).all()
            assert level[0, y, x] == 0 and level.max() <= du.lmax(W, H)


def test_lowest_index_wins(ctx):
    """several records on one pixel, next to each other and far apart in the list; thousands on pixel (0, 0)"""
    W, H, cap = 96, 64, 6000
    px = [(5, 5), (40, 33), (63, 63)]
    for corr in (False, True):
        rec = np.zeros((1, cap), du.CORR if corr else du.SUPPORT)             # record 0: pixel (0, 0), value 0
        rec[0, 1:] = (0, 0, 1, 0) if corr else (0, 0, -1.0)                    # the later ones would say 256 / -256
        for k, (x, y) in enumerate(px):
            for i, slot in enumerate((3 + 2 * k, 4 + 2 * k, 2900 + k, 5990 + k)):
                rec[0, slot] = (x, y, x + 1 + i, y) if corr else (x, y, float(-1 - i))
        first = 256 if corr else -256
        value, level = check(ctx, rec, [cap], W, H, du.DEFAULTS, None, ("duplicates", corr))
        assert value[0, 0, 0, 0] == 0 and all(value[0, 0, y, x] == first and level[0, y, x] == 0 for x, y in px)
        # the same records in reverse order: the last of each group stands now
        value, level = check(ctx, rec[:, ::-1].copy(), [cap], W, H, du.DEFAULTS, None, ("reversed", corr))
        assert value[0, 0, 0, 0] == first and all(value[0, 0, y, x] == 4 * first for x, y in px)


def test_records_that_do_not_participate(ctx):
    """sources and targets outside the image; supports with a fractional, infinite or NaN d, or one of 2^24: alone they leave
    everything none, beside good records they change nothing"""
    W, H = 33, 17
    sup = np.array([(-1, 3, 0.0), (33, 3, 0.0), (4, -1, 0.0), (4, 17, 0.0), (4, 4, 5.0), (30, 4, -3.0), (4, 4, 0.5), (4, 4, np.nan),
                    (4, 4, np.inf), (4, 4, -np.inf), (4, 4, 2.0 ** 24), (4, 4, -2.0 ** 24), (4, 4, 3e38)], du.SUPPORT)
    cor = np.array([(-1, 3, 3, 3), (33, 3, 3, 3), (4, -1, 3, 3), (4, 17, 3, 3), (4, 4, -1, 4), (4, 4, 33, 4), (4, 4, 4, -1),
                    (4, 4, 4, 17), (2 ** 31 - 1, 4, 4, 4), (4, 4, -2 ** 31, 4)], du.CORR)
    good_s = np.array([(4, 4, 4.0), (32, 16, 32.0), (0, 0, -32.0)], du.SUPPORT)
    good_c = np.array([(4, 4, 0, 0), (32, 16, 32, 16), (0, 0, 32, 16)], du.CORR)
    for bad, good in ((sup, good_s), (cor, good_c)):
        value, level = check(ctx, bad[None], [len(bad)], W, H, du.DEFAULTS, None, "bad alone")
        assert (value == du.NONE).all() and (level == 255).all()
        both = np.concatenate([bad, good])[None]
        with_bad = check(ctx, both, [both.shape[1]], W, H, du.DEFAULTS, None, "bad first")
        alone = check(ctx, good[None], [len(good)], W, H, du.DEFAULTS, None, "good alone")
        assert np.array_equal(with_bad[0], alone[0]) and np.array_equal(with_bad[1], alone[1])
        assert (alone[1] != 255).all() and (alone[1] == 0).sum() == 3


def test_exact_halves_round_away_from_zero(ctx):
    """sums that are an exact half of the count, of both signs, in both channels"""
    W, H = 8, 2
    ref = np.zeros((1, 2), du.REFINEMENT)
    ref["flags"] = 1
    for sign in (1, -1):
        ref["dx_q8"][0], ref["dy_q8"][0] = (sign, 0), (0, -3 * sign)
        rec = np.array([[(0, 0, 0.0), (7, 0, 0.0)]], du.SUPPORT)
        value, level = check(ctx, rec, [2], W, H, (15, 2, 1, 0xFFFF), ref, ("half", sign))
        assert value[0, 0, 1, 3] == -sign and level[0, 1, 3] >= 2             # (-sign + 0) / 2: half a unit, away from zero
        rec = np.array([[(0, 0, 0, 0), (7, 0, 7, 0)]], du.CORR)
        value, level = check(ctx, rec, [2], W, H, (15, 2, 1, 0xFFFF), ref, ("half uv", sign))
        assert value[0, 0, 1, 3] == sign and value[0, 1, 1, 3] == -2 * sign   # 1 / 2 -> 1; -3 / 2 -> -2
    # thirds and larger counts, both signs: the restatement decides
    rng = np.random.default_rng(4)
    for corr in (False, True):
        rec = du.random_records(rng, 33, 17, 60, corr, 60, hole=False)[None]
        ref = du.random_refinements(rng, 60)[None]
        ref["flags"] |= 1
        check(ctx, rec, [60], 33, 17, (15, 3, 1, 0xFFFF), ref, ("fractions", corr))


def test_block_sums_beyond_32_bits(ctx):
    """2048 x 64: 9472 supports of d = +-1900 at one end of the image; the pixels at the other end take their value from
    blocks whose sums are +-4.6e9"""
    W, H = 2048, 64
    xs, ys = np.meshgrid(np.arange(1900, 2048), np.arange(H))
    rec = np.zeros((2, xs.size), du.SUPPORT)
    rec[0]["x"], rec[0]["y"], rec[0]["d"] = xs.ravel(), ys.ravel(), 1900.0
    rec[1]["x"], rec[1]["y"], rec[1]["d"] = 2047 - xs.ravel(), ys.ravel(), -1900.0
    value, level = check(ctx, rec, [xs.size] * 2, W, H, du.DEFAULTS, None, "wide sums")
    assert abs(256 * 1900 * xs.size) > 2 ** 32
    assert (value[0] == 256 * 1900).all() and (value[1] == -256 * 1900).all() and level[0, 0, 0] >= 10 and level[1, 0, 2047] >= 10
    # unequal values, so that the quotient is no summand: d = x - 100 on one side
    rec[0]["d"] = rec[0]["x"] - 100.0
    value, level = check(ctx, rec[:1], [xs.size], W, H, (15, 9000, 1, 0xFFFF), None, "wide sums, min_count 9000")
    assert level[0, 0, 0] >= 10 and 256 * 1800 < value[0, 0, 0, 0] < 256 * 1948


@pytest.mark.parametrize("corr", [False, True])
def test_refinements_shifts_and_cost_ceilings(ctx, corr):
    """ref: shifts of both signs, records that were not evaluated (their shifts must be ignored), ceilings that exclude some
    records, all of them and none"""
    W, H, m = 130, 67, 1500
    rng = np.random.default_rng(21 + corr)
    rec = np.stack([du.random_records(rng, W, H, m, corr, m), du.random_records(rng, W, H, m, corr, m, hole=False)])
    ref = np.stack([du.random_refinements(rng, m), du.random_refinements(rng, m)])
    assert (ref["dx_q8"] < 0).any() and (ref["dx_q8"] > 0).any() and (ref["flags"] == 0).any()
    plain = check(ctx, rec, [m, m], W, H, du.DEFAULTS, None, "no ref")
    open_ = check(ctx, rec, [m, m], W, H, du.DEFAULTS, ref, "no ceiling")
    assert np.array_equal(plain[1], open_[1]) and not np.array_equal(plain[0], open_[0])   # the same owners, shifted values
    some = check(ctx, rec, [m, m], W, H, (15, 1, 1, 1500), ref, "some")
    assert 0 < (some[1] == 0).sum() < (open_[1] == 0).sum()
    most = check(ctx, rec, [m, m], W, H, (15, 1, 1, 0xFFFE), ref, "all evaluated")      # only the unevaluated are out
    assert (some[1] == 0).sum() < (most[1] == 0).sum() < (open_[1] == 0).sum()
    ref["cost"] = np.maximum(ref["cost"], 1)
    none = check(ctx, rec, [m, m], W, H, (15, 1, 1, 0), ref, "all excluded")
    assert (none[0] == du.NONE).all() and (none[1] == 255).all()


def test_level_is_optional(ctx):
    W, H = 130, 67
    rng = np.random.default_rng(8)
    for corr in (False, True):
        rec = du.random_records(rng, W, H, 900, corr, 900)[None]
        want = du.densify(rec, [900], W, H)
        value, level = dense_device(ctx, rec, [900], W, H, with_level=False)
        assert np.array_equal(value, want[0]) and (level == FILL).all()


def test_host_forms(ctx):
    """19 pairs (two chunks of at most 16) of 33x17: the host forms, from pageable and from page-locked arrays, with and
    without ref and level, leave the bytes the device forms leave"""
    W, H, P, cap = 33, 17, 19, 90
    rng = np.random.default_rng(23)
    for corr in (False, True):
        rec = np.stack([du.random_records(rng, W, H, 80, corr, cap, hole=bool(t % 2)) for t in range(P)])
        ref = np.stack([du.random_refinements(rng, cap) for _ in range(P)])
        counts = rng.integers(0, 80, P).astype(np.int32)
        counts[[1, 5, 17]] = (cap + 9, -1, cap)
        for use_ref, prm in ((False, du.DEFAULTS), (True, (3, 2, 0, 1500))):
            want = dense_device(ctx, rec, counts, W, H, prm, ref if use_ref else None)
            same(want, du.densify(rec, counts, W, H, prm, ref if use_ref else None), ("device", corr, use_ref))
            for what, alloc in (("pageable", np.empty), ("page-locked", ctx.pinned_empty)):
                hrec, href = alloc(rec.shape, rec.dtype), alloc(ref.shape, ref.dtype)
                hrec[...], href[...] = rec, ref
                got = ctx.densify_records(hrec, counts, W, H, P_(prm), href if use_ref else None)
                same(got, want, (what, corr, use_ref))
            value, level = ctx.densify_records(rec, counts, W, H, P_(prm), ref if use_ref else None, want_level=False)
            assert level is None and np.array_equal(value, want[0])


def match_batch(c, d_L, d_R, W, H, B, s, cap):
    import torch
    d_sup, d_cnt, d_nc = filled(B, cap, 12), filled(B, 4), filled(B, 2, 4)
    torch.cuda.synchronize()
    c.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, d_sup.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
    c.synchronize()
    return d_sup, d_cnt, d_nc


def records_form(c, d_rec, corr, cap, d_cnt, W, H, P, prm, d_ref=None):
    import torch
    Cn = 2 if corr else 1
    d_val, d_lev = filled(P, Cn, H, W, 4), filled(P, H, W)
    torch.cuda.synchronize()
    c.densify_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, prm, d_val.data_ptr(), d_lev.data_ptr(),
                             d_ref.data_ptr() if d_ref is not None else 0)
    c.synchronize()
    return planes(d_val, d_lev, P, Cn, H, W)


@pytest.mark.parametrize("forest", ["zero", "tau"])
@pytest.mark.parametrize("epipolar", [True, False])
@pytest.mark.parametrize("lanes", [1, 2])
def test_match_and_fill_batch(oracle, forest_paths, forest, epipolar, lanes):
    """synthetic pairs of 96x64 with D = 5: densify_batch_device == match_batch_device then the records form; every support
    has d = 5, so every valid pixel is exactly 256 * 5; with refine_radius 3 == match, refine_batch_device, the records form
    with ref"""
    import opengpc_amd as g
    import torch
    W, H, B, D = 96, 64, 2, 5
    c = g.Context(0)
    try:
        c.load_forest(forest_paths[forest], W, H)
        c.set_pipeline(lanes)
        pairs = [oracle.synth_pair(W, H, i, D) for i in range(B)]
        Lh, Rh = (np.ascontiguousarray(np.stack([q[k] for q in pairs])) for k in (0, 1))
        d_L, d_R = dev(Lh), dev(Rh)
        cap = (W - 26) * (H - 26) + 1
        s = settings(epipolar)
        prm = g.Densify()
        d_sup, d_cnt, d_nc = match_batch(c, d_L, d_R, W, H, B, s, cap)
        cnt = d_cnt.cpu().numpy().view(np.int32).reshape(-1)
        assert cnt.min() > 100
        want = records_form(c, d_sup, False, cap, d_cnt, W, H, B, prm)
        rec = d_sup.cpu().numpy().view(du.SUPPORT).reshape(B, cap)
        same(want, du.densify(rec, cnt, W, H), "records form")
        assert (want[0] == 256 * D).all() and (want[1] != 255).all() and (want[1] == 0).sum() > 200
        for radius in (0, 3):
            d_val, d_lev, d_cnt2, d_nc2 = filled(B, 1, H, W, 4), filled(B, H, W), filled(B, 4), filled(B, 2, 4)
            torch.cuda.synchronize()
            c.densify_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, prm, d_val.data_ptr(), d_lev.data_ptr(), radius,
                                   d_cnt2.data_ptr(), d_nc2.data_ptr())
            c.synchronize()
            assert np.array_equal(d_cnt2.cpu().numpy(), d_cnt.cpu().numpy()) and np.array_equal(d_nc2.cpu().numpy(), d_nc.cpu().numpy())
            got = planes(d_val, d_lev, B, 1, H, W)
            if radius:
                d_sup3, d_cnt3, d_ref = filled(B, cap, 12), filled(B, 4), filled(B, cap, 8)
                torch.cuda.synchronize()
                c.refine_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, radius, d_sup3.data_ptr(), cap, d_cnt3.data_ptr(), 0,
                                      d_ref.data_ptr())
                c.synchronize()
                want = records_form(c, d_sup3, False, cap, d_cnt3, W, H, B, prm, d_ref)
                ref = d_ref.cpu().numpy().view(du.REFINEMENT).reshape(B, cap)
                same(want, du.densify(rec, cnt, W, H, du.DEFAULTS, ref), "records form with ref")
            same(got, want, (forest, epipolar, lanes, radius))
        # the optional outputs left out
        d_val = filled(B, 1, H, W, 4)
        torch.cuda.synchronize()
        c.densify_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, prm, d_val.data_ptr(), 0, 3)
        c.synchronize()
        assert np.array_equal(d_val.cpu().numpy().view(np.int32).reshape(B, 1, H, W), want[0])
    finally:
        c.close()


@pytest.mark.parametrize("epipolar", [True, False])
def test_match_and_fill_sequence(ctx, forest_paths, epipolar):
    """three frames of 96x64: densify_sequence_device == match_sequence_device (then refine) then the records form"""
    import torch
    W, H, N = 96, 64, 3
    frames = tu.frames_of(W, H, N, 1, 0 if epipolar else 3)
    ctx.load_forest(forest_paths["zero"], W, H)
    s = settings(epipolar)
    cap = (W - 26) * (H - 26) + 1
    prm = P_(du.DEFAULTS)
    d_f = dev(frames)
    d_corr, d_cnt, d_nc = filled(N - 1, cap, 16), filled(N - 1, 4), filled(N, 4)
    torch.cuda.synchronize()
    ctx.match_sequence_device(d_f.data_ptr(), W, H, N, s, d_corr.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    cnt = d_cnt.cpu().numpy().view(np.int32).reshape(-1)
    rec = d_corr.cpu().numpy().view(du.CORR).reshape(N - 1, cap)
    assert cnt.min() > 50
    for radius in (0, 3):
        d_ref = None
        if radius:
            d_ref = filled(N - 1, cap, 8)
            torch.cuda.synchronize()
            ctx.refine_records_device(d_corr.data_ptr(), True, cap, d_cnt.data_ptr(), d_f.data_ptr(), d_f.data_ptr() + W * H, W, H, N - 1,
                                      radius, d_ref.data_ptr())
            ctx.synchronize()
        want = records_form(ctx, d_corr, True, cap, d_cnt, W, H, N - 1, prm, d_ref)
        ref = d_ref.cpu().numpy().view(du.REFINEMENT).reshape(N - 1, cap) if radius else None
        same(want, du.densify(rec, cnt, W, H, du.DEFAULTS, ref), ("records form", radius))
        assert (want[1] != 255).all()
        d_val, d_lev, d_cnt2, d_nc2 = filled(N - 1, 2, H, W, 4), filled(N - 1, H, W), filled(N - 1, 4), filled(N, 4)
        torch.cuda.synchronize()
        ctx.densify_sequence_device(d_f.data_ptr(), W, H, N, s, prm, d_val.data_ptr(), d_lev.data_ptr(), radius, d_cnt2.data_ptr(),
                                    d_nc2.data_ptr())
        ctx.synchronize()
        assert np.array_equal(d_cnt2.cpu().numpy(), d_cnt.cpu().numpy()) and np.array_equal(d_nc2.cpu().numpy(), d_nc.cpu().numpy())
        same(planes(d_val, d_lev, N - 1, 2, H, W), want, ("sequence", epipolar, radius))


def test_group_mode_fills_from_the_union(forest_paths, oracle):
    """group mode: the batch form fills from the union's records; the sequence form is refused, as the sequence itself"""
    import opengpc_amd as g
    import torch
    W, H, B = 96, 64, 2
    c = g.Context(0)
    try:
        st, groups = g.read_forest_groups(os.path.join(ROOT, "forests", "stress16x20Forest.txt"), W, H)
        assert st == 0 and len(groups) == 16
        c.set_forest_groups(groups)
        pairs = [oracle.synth_pair(W, H, i, 5) for i in range(B)]
        d_L, d_R = (dev(np.stack([q[k] for q in pairs])) for k in (0, 1))
        cap = 16 * (W - 26) * (H - 26) + 1
        s = settings(True)
        d_sup, d_cnt, d_nc = match_batch(c, d_L, d_R, W, H, B, s, cap)
        cnt = d_cnt.cpu().numpy().view(np.int32).reshape(-1)
        assert cnt.min() > 100
        prm = g.Densify(15, 2, 1)
        want = records_form(c, d_sup, False, cap, d_cnt, W, H, B, prm)
        same(want, du.densify(d_sup.cpu().numpy().view(du.SUPPORT).reshape(B, cap), cnt, W, H, (15, 2, 1, 0xFFFF)), "union")
        d_val, d_lev = filled(B, 1, H, W, 4), filled(B, H, W)
        torch.cuda.synchronize()
        c.densify_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, prm, d_val.data_ptr(), d_lev.data_ptr())
        c.synchronize()
        same(planes(d_val, d_lev, B, 1, H, W), want, "group batch")
        before = d_val.clone()
        assert c.L.gpc_hip_densify_sequence_device(c.h, d_L.data_ptr(), W, H, 2, C.byref(s), 0, C.byref(prm), d_val.data_ptr(),
                                                   d_lev.data_ptr(), None, None) == g.capi.E_UNSUPPORTED
        c.synchronize()
        assert bool((d_val == before).all())
    finally:
        c.close()


def test_refusals(forest_paths):
    """every refusal of the group, and the outputs afterwards: not a byte written"""
    import opengpc_amd as g
    import torch
    W, H = 96, 64
    E, U = g.capi.E_INVALID, g.capi.E_UNSUPPORTED
    c = g.Context(0)
    try:
        L = c.L
        d_rec, d_ref = filled(2, 64, 16), filled(2, 64, 8)
        d_val, d_lev = filled(2, 2, H, W, 4), filled(2, H, W)
        d_cnt = dev(np.array([10, 20], np.int32))
        good = g.Densify()
        torch.cuda.synchronize()

        def recs(fn, rec=d_rec.data_ptr(), cap=64, cnt=d_cnt.data_ptr(), ref=None, w=W, h=H, npairs=2, prm=good, val=d_val.data_ptr(),
                 lev=d_lev.data_ptr()):
            return fn(c.h, rec, cap, cnt, ref, w, h, npairs, C.byref(prm) if prm is not None else None, val, lev)

        for fn in (L.gpc_hip_densify_supports_device, L.gpc_hip_densify_correspondences_device):
            for bad in (g.Densify(0), g.Densify(16), g.Densify(-1), g.Densify(15, 0), g.Densify(15, 65537), g.Densify(15, 1, 2),
                        g.Densify(15, 1, -1), g.Densify(15, 1, 1, -1), g.Densify(15, 1, 1, 0x10000)):
                assert recs(fn, prm=bad, ref=d_ref.data_ptr()) == E, (bad.max_level, bad.min_count, bad.spread, bad.max_cost)
            assert recs(fn, prm=g.Densify(15, 1, 1, 100)) == E and recs(fn, prm=g.Densify(15, 1, 1, 0xFFFE)) == E   # a ceiling needs ref
            assert recs(fn, prm=None) == E and recs(fn, rec=None) == E and recs(fn, cnt=None) == E and recs(fn, val=None) == E
            assert recs(fn, npairs=0) == E and recs(fn, cap=0) == E and recs(fn, w=0) == E and recs(fn, h=-1) == E
            assert recs(fn, w=32769, h=1, npairs=1) == U and recs(fn, w=1, h=32769, npairs=1) == U
            assert recs(fn, w=32768, h=32768 + 1, npairs=1) == U                                       # width * height > 2^30
            assert recs(fn, npairs=65536, cap=1) == U and recs(fn, cap=1 << 20, npairs=2048) == U      # npairs * cap = 2^31
        c.synchronize()
        for d in (d_val, d_lev):
            assert bool((d == FILL).all())
        # host forms: the same checks on host arrays
        hrec, hcnt = np.zeros((2, 64), g.SUPPORT_DTYPE), np.array([3, 4], np.int32)
        hval, hlev = np.full((2, 1, H, W, 4), FILL, np.uint8), np.full((2, H, W), FILL, np.uint8)
        host = lambda prm=good, npairs=2, val=hval.ctypes.data, w=W: L.gpc_hip_densify_supports(
            c.h, hrec.ctypes.data, 64, hcnt.ctypes.data, None, w, H, npairs, C.byref(prm), val, hlev.ctypes.data)
        assert host(prm=g.Densify(0)) == E and host(prm=g.Densify(15, 1, 1, 7)) == E and host(npairs=0) == E and host(val=None) == E
        assert host(npairs=65536) == U and host(w=40000) == U
        assert (hval == FILL).all() and (hlev == FILL).all()
        # match-and-fill forms: their own refusals and those of the match they wrap
        s = settings(True)
        d_f = dev(tu.frames_of(W, H, 3, 1))
        iL, iR = d_f.data_ptr(), d_f.data_ptr() + W * H
        seq = lambda nframes=3, radius=0, prm=good, val=d_val.data_ptr(), st=s, w=W: L.gpc_hip_densify_sequence_device(
            c.h, iL, w, H, nframes, C.byref(st), radius, C.byref(prm), val, d_lev.data_ptr(), None, None)
        bat = lambda npairs=2, radius=0, prm=good, val=d_val.data_ptr(), st=s, w=W: L.gpc_hip_densify_batch_device(
            c.h, iL, iR, w, H, npairs, C.byref(st), radius, C.byref(prm), val, d_lev.data_ptr(), None, None)
        assert seq() == g.capi.E_NO_FOREST and bat() == g.capi.E_NO_FOREST
        c.load_forest(forest_paths["zero"], W, H)
        for call in (seq, bat):
            assert call(radius=-1) == E and call(radius=7) == E and call(val=None) == E and call(w=W + 1) == E
            assert call(prm=g.Densify(15, 1, 3)) == E and call(prm=g.Densify(15, 1, 1, 500)) == E     # a ceiling without refinement
        assert seq(nframes=1) == E and bat(npairs=0) == E
        c.synchronize()
        st, groups = g.read_forest_groups(os.path.join(ROOT, "forests", "stress16x20Forest.txt"), W, H)
        c.set_forest_groups(groups)
        assert seq() == U                                            # group-mode sequences, as the sequence itself
        c.synchronize()
        # after all of them the calls still work, a ceiling with a refinement among them
        c.load_forest(forest_paths["zero"], W, H)
        d_val2, d_lev2 = filled(2, 2, H, W, 4), filled(2, H, W)
        torch.cuda.synchronize()
        assert L.gpc_hip_densify_batch_device(c.h, iL, iR, W, H, 2, C.byref(s), 3, C.byref(g.Densify(15, 1, 1, 500)), d_val2.data_ptr(),
                                              d_lev2.data_ptr(), None, None) == 0
        assert recs(L.gpc_hip_densify_correspondences_device) == 0
        c.synchronize()
        assert not bool((d_lev2 == FILL).any())
    finally:
        c.close()
