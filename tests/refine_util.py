"""Match refinement (gpc_hip_refine_*), restated plainly from the rule in include/gpc_hip.h for the tests to hold the GPU
result equal to: `refine_pair` with numpy (fast enough for real record lists), `brute_one` with Python loops and integers
(single records).  Neither shares anything with the kernel's method (no packed sums, no shifted words)."""
import numpy as np

CORR = np.dtype([("src_x", "<i4"), ("src_y", "<i4"), ("tar_x", "<i4"), ("tar_y", "<i4")])
SUPPORT = np.dtype([("x", "<i4"), ("y", "<i4"), ("d", "<f4")])
REFINEMENT = np.dtype([("dx_q8", "<i2"), ("dy_q8", "<i2"), ("cost", "<u2"), ("flags", "<u2")])
NOT_EVALUATED = (0, 0, 0xFFFF, 0)
EVALUATED, MIN_X, MIN_Y = 1, 2, 4


def m_of(counts, cap):
    return [min(max(int(c), 0), cap) for c in counts]


def shifts_of(corr):
    return ((-1, 0), (0, 0), (1, 0), (0, -1), (0, 1)) if corr else ((-1, 0), (0, 0), (1, 0))


def ends(r):
    """(usable [m] bool, x, y, tx, ty as int64) of a 1-D record array of either type; usable: a support's d is a whole
    number below 2^24 in magnitude (always true for correspondences)"""
    if r.dtype == CORR:
        x, y, tx, ty = (r[f].astype(np.int64) for f in ("src_x", "src_y", "tar_x", "tar_y"))
        return np.ones(len(r), bool), x, y, tx, ty
    x, y = r["x"].astype(np.int64), r["y"].astype(np.int64)
    d = r["d"].astype(np.float64)
    ok = np.isfinite(d)
    di = np.where(ok, d, 0.0)
    ok &= (di == np.trunc(di)) & (np.abs(di) < 2.0 ** 24)
    di = np.where(ok, di, 0.0).astype(np.int64)
    return ok, x, y, x - di, y


def evaluated(r, W, H, radius):
    """every pixel of every window the record needs lies inside the image"""
    ok, x, y, tx, ty = ends(r)
    ok = ok & (x - radius >= 0) & (x + radius <= W - 1) & (y - radius >= 0) & (y + radius <= H - 1)
    for sx, sy in shifts_of(r.dtype == CORR):
        ok &= (tx + sx - radius >= 0) & (tx + sx + radius <= W - 1) & (ty + sy - radius >= 0) & (ty + sy + radius <= H - 1)
    return ok


def axis(cm, c0, cp):
    """(has a minimum, q) of one axis, Python integers"""
    a, n = cm + cp - 2 * c0, cm - cp
    if not (c0 <= cm and c0 <= cp and a > 0):
        return False, 0
    q = (256 * abs(n) + a) // (2 * a)
    return True, q if n >= 0 else -q


def brute_one(rec, imgL, imgR, radius):
    """(dx_q8, dy_q8, cost, flags) of ONE record (a 0-d element of a record array), by loops over the pixels"""
    H, W = imgL.shape
    r = np.array([rec])
    if not evaluated(r, W, H, radius)[0]:
        return NOT_EVALUATED
    _, x, y, tx, ty = (int(a[0]) for a in ends(r))
    corr = r.dtype == CORR

    def cost(sx, sy):
        return sum(abs(int(imgL[y + j, x + i]) - int(imgR[ty + sy + j, tx + sx + i]))
                   for j in range(-radius, radius + 1) for i in range(-radius, radius + 1))

    c0 = cost(0, 0)
    flags = EVALUATED
    hx, dx = axis(cost(-1, 0), c0, cost(1, 0))
    flags |= MIN_X if hx else 0
    dy = 0
    if corr:
        hy, dy = axis(cost(0, -1), c0, cost(0, 1))
        flags |= MIN_Y if hy else 0
    return dx, dy, c0, flags


def refine_pair(r, imgL, imgR, radius):
    """-> (ref [m] of REFINEMENT, out [m] supports with the refined d or None) of one pair's records (1-D array)"""
    H, W = imgL.shape
    corr = r.dtype == CORR
    ref = np.zeros(len(r), REFINEMENT)
    ref["cost"] = 0xFFFF
    out = None if corr else r.copy()
    idx = np.nonzero(evaluated(r, W, H, radius))[0]
    if len(idx):
        _, x, y, tx, ty = (a[idx] for a in ends(r))
        o = np.arange(-radius, radius + 1)
        J, I = o[None, :, None], o[None, None, :]
        left = imgL[y[:, None, None] + J, x[:, None, None] + I].astype(np.int64)
        c = {}
        for sx, sy in shifts_of(corr):
            right = imgR[(ty + sy)[:, None, None] + J, (tx + sx)[:, None, None] + I].astype(np.int64)
            c[(sx, sy)] = np.abs(left - right).sum(axis=(1, 2))
        c0 = c[(0, 0)]

        def axis_of(cm, cp):
            a, n = cm + cp - 2 * c0, cm - cp
            has = (c0 <= cm) & (c0 <= cp) & (a > 0)
            q = np.sign(n) * ((256 * np.abs(n) + a) // np.where(has, 2 * a, 1))
            return has, np.where(has, q, 0)

        hx, dx = axis_of(c[(-1, 0)], c[(1, 0)])
        flags = EVALUATED + MIN_X * hx
        ref["dx_q8"][idx] = dx
        if corr:
            hy, dy = axis_of(c[(0, -1)], c[(0, 1)])
            flags = flags + MIN_Y * hy
            ref["dy_q8"][idx] = dy
        else:
            out["d"][idx] = r["d"][idx] - dx.astype(np.float32) * np.float32(0.00390625)   # float32 throughout
        ref["cost"][idx] = c0
        ref["flags"][idx] = flags
    return ref, out


def expected_arrays(rec, counts, imgL, imgR, radius, fill):
    """the restatement as the arrays a call leaves in outputs whose every BYTE held `fill`: (ref [P, cap] of REFINEMENT, out
    [P, cap] supports or None for correspondences).  imgL, imgR: [P, H, W] uint8"""
    P, cap = rec.shape
    corr = rec.dtype == CORR
    ref = np.full((P, cap, 8), fill, np.uint8).view(REFINEMENT).reshape(P, cap)
    out = None if corr else np.full((P, cap, 12), fill, np.uint8).view(SUPPORT).reshape(P, cap)
    for t, m in enumerate(m_of(counts, cap)):
        f, o = refine_pair(rec[t, :m], imgL[t], imgR[t], radius)
        ref[t, :m] = f
        if not corr:
            out[t, :m] = o
    return ref, out
