"""CPU: the match refinement rule (gpc_hip_refine_*) as tests/refine_util.py restates it -- hand-computed 5x5 cases, the
numpy form equals the per-pixel form, the quotient of the parabola step over its whole range -- and its declarations in the
Python binding."""
import ctypes as C

import numpy as np

import refine_util as ru

MAX_COST = 169 * 255      # the largest window (r = 6), every pixel differing by 255


def support(x, y, d):
    return np.array([(x, y, d)], ru.SUPPORT)


def corr(sx, sy, tx, ty):
    return np.array([(sx, sy, tx, ty)], ru.CORR)


def both(rec, L, R, r=1):
    """the per-pixel form and the numpy form of one record; they must agree"""
    slow = ru.brute_one(rec[0], L, R, r)
    fast = tuple(int(v) for v in ru.refine_pair(rec, L, R, r)[0][0])
    assert slow == fast, (slow, fast)
    return slow


def columns(v):
    """5x5 image whose column c holds v[c]"""
    return np.tile(np.array(v, np.uint8), (5, 1))


def test_flat_image_has_no_minimum():
    L = R = np.full((5, 5), 7, np.uint8)
    assert both(support(2, 2, 0.0), L, R) == (0, 0, 0, ru.EVALUATED)                 # a = 0
    assert both(corr(2, 2, 2, 2), L, R) == (0, 0, 0, ru.EVALUATED)
    R9 = np.full((5, 5), 9, np.uint8)
    assert both(corr(2, 2, 2, 2), L, R9) == (0, 0, 18, ru.EVALUATED)                 # a constant cost: a = 0 again


def test_one_sided_tie_and_the_ends_of_the_range():
    L = np.zeros((5, 5), np.uint8)
    # left image 0: cost(s) = 3 * (v[1 + s] + v[2 + s] + v[3 + s]) for a target at column 2
    R = columns((1, 0, 0, 1, 5))           # c- = 3, c0 = 3, c+ = 18: a tie on the left, a = 15, n = -15 = -a
    assert both(support(2, 2, 0.0), L, R) == (-128, 0, 3, ru.EVALUATED | ru.MIN_X)
    R = columns((5, 1, 0, 0, 1))           # mirrored: n = +a
    assert both(support(2, 2, 0.0), L, R) == (128, 0, 3, ru.EVALUATED | ru.MIN_X)
    R = columns((4, 0, 0, 2, 6))           # c- = 12, c0 = 6, c+ = 24: a = 24, n = -12, (3072 + 24) div 48 = 64
    assert both(support(3, 2, 1.0), L, R) == (-64, 0, 6, ru.EVALUATED | ru.MIN_X)
    R = columns((0, 0, 3, 0, 0))           # c- = c0 = c+ = 9: a = 0
    assert both(support(2, 2, 0.0), L, R) == (0, 0, 9, ru.EVALUATED)
    R = columns((0, 0, 0, 0, 3))           # c- = 0 < c0 = 0 <= ... c+ = 9: c0 <= c-, a = 9, n = -9
    assert both(support(2, 2, 0.0), L, R) == (-128, 0, 0, ru.EVALUATED | ru.MIN_X)
    R = columns((0, 3, 3, 0, 0))           # c- = 18, c0 = 18, c+ = 9: c0 > c+: no minimum although a < 0 is not the reason
    assert both(support(2, 2, 0.0), L, R) == (0, 0, 18, ru.EVALUATED)
    # the same along y for a correspondence, x flat
    assert both(corr(2, 2, 2, 2), L, columns((1, 0, 0, 1, 5)).T.copy()) == (0, -128, 3, ru.EVALUATED | ru.MIN_Y)
    assert both(corr(2, 2, 2, 2), L, columns((5, 1, 0, 0, 1)).T.copy()) == (0, 128, 3, ru.EVALUATED | ru.MIN_Y)


def test_not_evaluated():
    L = R = np.zeros((5, 5), np.uint8)
    for rec in (support(0, 2, -2.0), support(2, 0, 0.0), support(2, 4, 0.0), support(2, 2, 1.0), support(2, 2, -1.0),
                support(2, 2, 0.5), support(2, 2, np.nan), support(2, 2, np.inf), support(2, 2, -np.inf), support(2, 2, 2.0 ** 24),
                corr(2, 2, 2, 1), corr(2, 2, 2, 3), corr(2, 2, 1, 2), corr(2, 2, 3, 2), corr(0, 2, 2, 2), corr(2, 4, 2, 2)):
        assert both(rec, L, R) == ru.NOT_EVALUATED, rec
    for x in (1, 2, 3):                                           # the source may touch the border, the target's shifts not
        assert both(support(x, 1, float(x - 2)), L, R)[3] == ru.EVALUATED
        assert both(corr(x, 3, 2, 2), L, R)[3] == ru.EVALUATED
    assert both(support(2, 2, -0.0), L, R)[3] == ru.EVALUATED
    big = np.zeros((15, 15), np.uint8)
    assert both(support(7, 7, 0.0), big, big, 6)[3] == ru.EVALUATED and both(support(7, 7, 0.0), big[:, :14], big[:, :14], 6) == ru.NOT_EVALUATED


def test_numpy_form_equals_per_pixel_form():
    rng = np.random.default_rng(5)
    for r in (1, 2, 3, 6):
        W, H = 24, 19
        L = rng.integers(0, 256, (H, W)).astype(np.uint8)
        L[rng.random((H, W)) < 0.2] = 0                            # real 0 pixels, and 255s
        L[rng.random((H, W)) < 0.1] = 255
        R = np.roll(L, 2, axis=1)
        R[rng.random((H, W)) < 0.3] = rng.integers(0, 256)
        m = 60
        s = np.zeros(m, ru.SUPPORT)
        s["x"], s["y"] = rng.integers(-1, W + 1, m), rng.integers(-1, H + 1, m)
        s["d"] = rng.integers(-4, 5, m)
        s["d"][:4] = (0.5, np.nan, np.inf, -2.0 ** 24)
        c = np.zeros(m, ru.CORR)
        c["src_x"], c["src_y"] = rng.integers(-1, W + 1, m), rng.integers(-1, H + 1, m)
        c["tar_x"], c["tar_y"] = c["src_x"] + rng.integers(-3, 4, m), c["src_y"] + rng.integers(-3, 4, m)
        for rec in (s, c):
            ref, out = ru.refine_pair(rec, L, R, r)
            for i in range(m):
                assert tuple(int(v) for v in ref[i]) == ru.brute_one(rec[i], L, R, r), (r, i)
            ev = (ref["flags"] & 1) != 0
            if r <= 3:
                assert 0 < ev.sum() < m
            if out is not None:
                assert np.array_equal(out[~ev].view(np.uint8), rec[~ev].view(np.uint8))
                want = rec["d"][ev] - ref["dx_q8"][ev].astype(np.float32) / np.float32(256)
                assert np.array_equal(out["d"][ev], want) and np.array_equal(out["x"], rec["x"]) and np.array_equal(out["y"], rec["y"])


def test_extremes_of_the_cost():
    L, R = np.zeros((15, 15), np.uint8), np.full((15, 15), 255, np.uint8)
    assert both(support(7, 7, 0.0), L, R, 6) == (0, 0, MAX_COST, ru.EVALUATED)
    assert both(corr(7, 7, 7, 7), L, R, 6) == (0, 0, MAX_COST, ru.EVALUATED)
    assert MAX_COST == 43095 < 0xFFFF                              # the cost of a record that is not evaluated is no cost


def test_the_quotient_over_its_whole_range():
    """q = (256 |n| + a) div 2a for every a the costs can give (1 .. 2 * 43 095) and, for each a, every |n| <= a at which the
    quotient can step: the ends and the neighbours of (2q - 1) a / 256, q = 1 .. 128.  q is 128 |n| / a rounded half AWAY
    from zero -- (2q - 1) a <= 256 |n| < (2q + 1) a -- stays within 0 .. 128, and the dividend fits 25 bits (the kernel
    divides unsigned 32-bit integers, exactly)."""
    a = np.arange(1, 2 * MAX_COST + 1, dtype=np.int64)[:, None]
    step = ((2 * np.arange(1, 129, dtype=np.int64)[None, :] - 1) * a) // 256
    n = np.concatenate([np.zeros_like(a), np.ones_like(a), a - 1, a, step - 1, step, step + 1, step + 2], axis=1)
    n = np.clip(n, 0, a)
    num = 256 * n + a
    q = num // (2 * a)
    assert num.max() < 1 << 25 and q.min() == 0 and q.max() == 128
    assert ((2 * q - 1) * a <= 256 * n).all() and (256 * n < (2 * q + 1) * a).all()
    assert (q[n == a] == 128).all() and (q[n == 0] == 0).all()
    # ... and ru.axis, the scalar form, agrees with it where an axis has a minimum: c0 = 0, c- = (a + n) / 2, c+ = (a - n) / 2
    rng = np.random.default_rng(1)
    for _ in range(2000):
        cp = int(rng.integers(0, MAX_COST + 1))
        cm = int(rng.integers(0, MAX_COST + 1))
        c0 = int(rng.integers(0, min(cm, cp) + 1))
        has, got = ru.axis(cm, c0, cp)
        aa, nn = cm + cp - 2 * c0, cm - cp
        assert has == (aa > 0) and abs(nn) <= aa
        if has:
            want = (256 * abs(nn) + aa) // (2 * aa)
            assert got == (want if nn >= 0 else -want) and abs(got) <= 128


def test_binding_declares_the_struct_and_the_entry_points():
    import opengpc_amd as g
    assert g.REFINEMENT_DTYPE.itemsize == 8 and g.REFINEMENT_DTYPE == ru.REFINEMENT
    assert g.REFINEMENT_DTYPE.names == ("dx_q8", "dy_q8", "cost", "flags")
    names = ["gpc_hip_refine_supports_device", "gpc_hip_refine_correspondences_device", "gpc_hip_refine_batch_device",
             "gpc_hip_refine_sequence_device", "gpc_hip_refine_supports", "gpc_hip_refine_correspondences"]
    from opengpc_amd import build
    build.build()
    L = g.load()
    for n in names:
        assert n in g.capi.SYMBOLS and getattr(L, n).argtypes is not None, n
    assert len(L.gpc_hip_refine_supports_device.argtypes) == 12 and len(L.gpc_hip_refine_correspondences_device.argtypes) == 11
    assert len(L.gpc_hip_refine_batch_device.argtypes) == 14 and len(L.gpc_hip_refine_sequence_device.argtypes) == 12
    # the timing mask addresses 32 slots and they are taken: k_refine is a slot behind them, named and timed like the others
    kernels = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_slots())]
    assert "k_refine" in kernels and len(set(kernels)) == len(kernels) and "" not in kernels
    assert L.gpc_hip_kernel_count() == min(len(kernels), 32) and kernels.index("k_refine") >= L.gpc_hip_kernel_count()
    assert ru.CORR == g.CORR_DTYPE and ru.SUPPORT == g.SUPPORT_DTYPE
    for m in ("refine_records_device", "refine_batch_device", "refine_sequence_device", "refine_records"):
        assert callable(getattr(g.Context, m))
    assert C.sizeof(C.c_int16) * 2 + C.sizeof(C.c_uint16) * 2 == 8
