"""The densifier's rule (include/gpc_hip.h, gpc_hip_densify_*) restated plainly, twice: densify_pair with numpy (owner by
minimum index, block sums by np.add.at per level, 3x3 sums by padded shifts) and brute_pixel with Python loops and Python
integers over all records, for single pixels.  Neither shares anything with the kernels' method (tiles, a cell pyramid)."""
import numpy as np

SUPPORT = np.dtype([("x", "<i4"), ("y", "<i4"), ("d", "<f4")])
CORR = np.dtype([("src_x", "<i4"), ("src_y", "<i4"), ("tar_x", "<i4"), ("tar_y", "<i4")])
REFINEMENT = np.dtype([("dx_q8", "<i2"), ("dy_q8", "<i2"), ("cost", "<u2"), ("flags", "<u2")])
NONE = -2 ** 31
DEFAULTS = (15, 1, 1, 0xFFFF)      # max_level, min_count, spread, max_cost


def lmax(W, H):
    l = 1
    while ((W - 1) >> l) or ((H - 1) >> l):
        l += 1
    return l


def valid(count, cap):
    return min(max(int(count), 0), cap)


def participants(rec, count, W, H, ref=None, max_cost=0xFFFF):
    """(index, sx, sy, values [C, n]) of the participating records among rec[:m], in input order; int64 throughout"""
    m = valid(count, len(rec))
    r = rec[:m]
    if rec.dtype == CORR:
        sx, sy, tx, ty = (r[k].astype(np.int64) for k in ("src_x", "src_y", "tar_x", "tar_y"))
        ok = np.ones(m, bool)
        whole_d = None
    else:
        d = r["d"].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(d) & (d == np.trunc(d)) & (np.abs(d) < 2.0 ** 24)
        whole_d = np.where(ok, d, 0).astype(np.int64)
        sx, sy = r["x"].astype(np.int64), r["y"].astype(np.int64)
        tx, ty = sx - whole_d, sy
    ok &= (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H) & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    dx = dy = np.zeros(m, np.int64)
    if ref is not None:
        f = ref[:m]
        ev = (f["flags"] & 1) != 0
        if max_cost < 0xFFFF:
            ok &= ev & (f["cost"].astype(np.int64) <= max_cost)
        dx = np.where(ev, f["dx_q8"].astype(np.int64), 0)
        dy = np.where(ev, f["dy_q8"].astype(np.int64), 0)
    if rec.dtype == CORR:
        vals = np.stack([256 * (tx - sx) + dx, 256 * (ty - sy) + dy])
    else:
        vals = np.stack([256 * whole_d - dx])
    idx = np.nonzero(ok)[0]
    return idx, sx[idx], sy[idx], vals[:, idx]


def densify_pair(rec, count, W, H, prm=DEFAULTS, ref=None):
    """value [C, H, W] int32 and level [H, W] uint8 of one pair"""
    max_level, min_count, spread, max_cost = prm
    C = 2 if rec.dtype == CORR else 1
    idx, sx, sy, vals = participants(rec, count, W, H, ref, max_cost)
    big = np.iinfo(np.int64).max
    owner = np.full(W * H, big, np.int64)
    np.minimum.at(owner, sy * W + sx, idx)
    occ = (owner != big).reshape(H, W)
    where = np.full(len(rec) + 1, -1, np.int64)         # input index -> position among the participants
    where[idx] = np.arange(len(idx))
    val = np.zeros((C, H, W), np.int64)
    oy, ox = np.nonzero(occ)
    val[:, oy, ox] = vals[:, where[owner.reshape(H, W)[oy, ox]]]
    value = np.full((C, H, W), NONE, np.int64)
    level = np.full((H, W), 255, np.int64)
    value[:, occ] = val[:, occ]
    level[occ] = 0
    ys, xs = np.mgrid[0:H, 0:W]
    todo = ~occ
    for l in range(1, min(max_level, lmax(W, H)) + 1):
        gw, gh = ((W - 1) >> l) + 1, ((H - 1) >> l) + 1
        n = np.zeros((gh, gw), np.int64)
        S = np.zeros((C, gh, gw), np.int64)
        np.add.at(n, (oy >> l, ox >> l), 1)
        for c in range(C):
            np.add.at(S[c], (oy >> l, ox >> l), val[c, oy, ox])
        N, T = np.zeros_like(n), np.zeros_like(S)
        pn, pS = np.pad(n, spread), np.pad(S, ((0, 0), (spread, spread), (spread, spread)))
        for j in range(2 * spread + 1):
            for i in range(2 * spread + 1):
                N += pn[j:j + gh, i:i + gw]
                T += pS[:, j:j + gh, i:i + gw]
        Np, Tp = N[ys >> l, xs >> l], T[:, ys >> l, xs >> l]
        take = todo & (Np >= min_count)
        den = np.where(take, Np, 1)
        mean = np.sign(Tp) * ((2 * np.abs(Tp) + den) // (2 * den))
        value[:, take] = mean[:, take]
        level[take] = l
        todo &= ~take
    return value.astype(np.int32), level.astype(np.uint8)


def densify(rec, counts, W, H, prm=DEFAULTS, ref=None):
    """[P, cap] records -> value [P, C, H, W] int32, level [P, H, W] uint8"""
    out = [densify_pair(rec[t], counts[t], W, H, prm, None if ref is None else ref[t]) for t in range(len(rec))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def brute_pixel(rec, count, W, H, x, y, prm=DEFAULTS, ref=None):
    """(values tuple, level) of pixel (x, y): Python loops and integers over every record"""
    max_level, min_count, spread, max_cost = prm
    corr = rec.dtype == CORR
    C = 2 if corr else 1
    first = {}                                           # source pixel -> values of the first participating record
    for i in range(valid(count, len(rec))):
        r = rec[i]
        if corr:
            sx, sy, tx, ty = int(r["src_x"]), int(r["src_y"]), int(r["tar_x"]), int(r["tar_y"])
        else:
            d = float(r["d"])
            if d != d or d in (float("inf"), float("-inf")) or d != float(int(d)) or abs(d) >= 2 ** 24:
                continue
            sx, sy = int(r["x"]), int(r["y"])
            tx, ty = sx - int(d), sy
        if not (0 <= sx < W and 0 <= sy < H and 0 <= tx < W and 0 <= ty < H):
            continue
        dx = dy = 0
        if ref is not None:
            f = ref[i]
            ev = bool(int(f["flags"]) & 1)
            if max_cost < 0xFFFF and not (ev and int(f["cost"]) <= max_cost):
                continue
            if ev:
                dx, dy = int(f["dx_q8"]), int(f["dy_q8"])
        v = (256 * (tx - sx) + dx, 256 * (ty - sy) + dy) if corr else (256 * int(d) - dx,)
        first.setdefault((sx, sy), v)
    if (x, y) in first:
        return first[(x, y)], 0
    for l in range(1, min(max_level, lmax(W, H)) + 1):
        n, s = 0, [0] * C
        for (px, py), v in first.items():
            if abs((px >> l) - (x >> l)) <= spread and abs((py >> l) - (y >> l)) <= spread:
                n += 1
                for c in range(C):
                    s[c] += v[c]
        if n >= min_count:
            sgn = lambda a: (a > 0) - (a < 0)
            return tuple(sgn(a) * ((2 * abs(a) + n) // (2 * n)) for a in s), l
    return (NONE,) * C, 255


def random_records(rng, W, H, m, corr, cap=None, hole=True):
    """[cap] records: m random ones whose sources avoid the right-hand third of the image (so that pixels there reach high
    levels) when `hole`; most targets inside the image; among them sources and targets outside it, duplicates of source
    pixels, and supports with a d that is no whole number, NaN, the infinities, 2^24"""
    cap = m if cap is None else cap
    rec = np.zeros(cap, CORR if corr else SUPPORT)
    xmax = max(1, (2 * W) // 3) if hole else W
    sx, sy = rng.integers(0, xmax, m), rng.integers(0, H, m)
    tx = np.clip(sx + rng.integers(-9, 10, m), 0, W - 1)
    ty = np.clip(sy + rng.integers(-5, 6, m), 0, H - 1)
    bad = rng.random(m) < 0.1
    sx = np.where(bad & (rng.random(m) < 0.5), rng.integers(-3, (xmax if hole else W + 3), m), sx)
    tx = np.where(bad, tx + rng.integers(-W, W + 1, m), tx)
    sy = np.where(bad & (rng.random(m) < 0.3), rng.integers(-2, H + 2, m), sy)
    if m > 8:
        dup = rng.integers(0, m, max(m // 8, 1))
        sx[dup], sy[dup] = sx[dup[::-1]], sy[dup[::-1]]
    if corr:
        rec["src_x"][:m], rec["src_y"][:m], rec["tar_x"][:m], rec["tar_y"][:m] = sx, sy, tx, ty
    else:
        rec["x"][:m], rec["y"][:m], rec["d"][:m] = sx, sy, (sx - tx).astype(np.float32)
        if m > 12:
            rec["d"][rng.choice(m, 6, replace=False)] = (0.5, -3.25, np.nan, np.inf, -np.inf, 2.0 ** 24)
    return rec


def random_refinements(rng, n):
    ref = np.zeros(n, REFINEMENT)
    ev = rng.random(n) < 0.8
    ref["flags"] = np.where(ev, 1 | (rng.integers(0, 4, n) << 1), 0)
    ref["dx_q8"] = rng.integers(-128, 129, n)             # (shifts of records that are not evaluated must be ignored)
    ref["dy_q8"] = rng.integers(-128, 129, n)
    ref["cost"] = np.where(ev, rng.integers(0, 3000, n), 0xFFFF)
    return ref
