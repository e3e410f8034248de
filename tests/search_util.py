"""The local dense search (gpc_hip_search_*), restated with numpy from the rule in include/gpc_hip.h for the tests to hold the
GPU result equal to, as tests/clean_util.py and tests/inpaint_util.py restate their rules.  It shares nothing with the
kernel's method: no staged tile, no packed sums, no shifted words, no second path for the border -- every pixel of every
window is one clamped gather."""
import functools

import numpy as np

NONE = -2 ** 31
IMAX, IMIN1 = 2 ** 31 - 1, -2 ** 31 + 1
DEFAULTS = (2, 1, 1, 0xFFFF)        # radius, range, subpixel, max_cost
TILE_W, TILE_H = 32, 8              # the kernel's tile: SIZES lie below, at and across it in both directions
SIZES = [(1, 1, 1), (7, 5, 1), (31, 33, 1), (33, 31, 1), (64, 32, 1), (70, 45, 3)]   # (W, H, P)
KINDS = ("random", "constant", "shifted")
TRUE_SHIFT = {1: (3, 0), 2: (2, -1)}   # "shifted": the disparity d (imgR[y][x - d] = imgL[y][x]) and the flow (u, v)


def whole(F):
    """sgn(F) * ((|F| + 128) >> 8) of an int64 array"""
    return np.sign(F) * ((np.abs(F) + 128) >> 8)


def base(field):
    """field [C, H, W] -> (valued [H, W], r [C, H, W], bx, by [H, W]) as int64"""
    F = field.astype(np.int64)
    C, H, W = F.shape
    ys, xs = np.mgrid[0:H, 0:W]
    r = whole(F)
    return F[0] != NONE, r, (xs - r[0] if C == 1 else xs + r[0]), (ys if C == 1 else ys + r[1])


def cost_grid(field, imgL, imgR, radius, rng_):
    """cost[dy + R + 1][dx + R + 1] [H, W] int64 of every pixel against the target b + (dx, dy), |dx|, |dy| <= R + 1 (dy = 0
    only with C = 1: then the grid has one row), all addresses clamped.  Holes get whatever their bits give; nobody reads it."""
    C, H, W = field.shape
    _, _, bx, by = base(field)
    ys, xs = np.mgrid[0:H, 0:W]
    o = range(-radius, radius + 1)
    left = {(i, j): imgL[np.clip(ys + j, 0, H - 1), np.clip(xs + i, 0, W - 1)].astype(np.int64) for j in o for i in o}
    K = rng_ + 1
    right = {}
    for dy in (range(-K - radius, K + radius + 1) if C == 2 else o):
        row = np.clip(by + dy, 0, H - 1)
        for dx in range(-K - radius, K + radius + 1):
            right[(dx, dy)] = imgR[row, np.clip(bx + dx, 0, W - 1)].astype(np.int64)
    dys = range(-K, K + 1) if C == 2 else (0,)
    return np.array([[sum(np.abs(left[(i, j)] - right[(dx + i, dy + j)]) for j in o for i in o) for dx in range(-K, K + 1)] for dy in dys])


def candidates(C, rng_):
    """the candidates (kx, ky) in the order of the tie-break: (|kx| + |ky|, ky, kx)"""
    ks = [(kx, ky) for ky in (range(-rng_, rng_ + 1) if C == 2 else (0,)) for kx in range(-rng_, rng_ + 1)]
    return sorted(ks, key=lambda k: (abs(k[0]) + abs(k[1]), k[1], k[0]))


def axis(cm, c0, cp):
    """(has a minimum, q) of one axis, int64 arrays: exactly refine_util.refine_pair's axis_of"""
    a, n = cm + cp - 2 * c0, cm - cp
    has = (c0 <= cm) & (c0 <= cp) & (a > 0)
    q = np.sign(n) * ((256 * np.abs(n) + a) // np.where(has, 2 * a, 1))
    return has, np.where(has, q, 0)


def decide(field, grid, prm, info=None):
    """one pair: field [C, H, W], grid = cost_grid(...) -> out [C, H, W] int32, cost [H, W] uint16, choice [H, W] uint8, stats
    [4] int32.  info (a dict) receives what the condition test of tests/test_search.py asks about."""
    radius, R, subpixel, max_cost = prm
    C, H, W = field.shape
    valued, r, bx, by = base(field)
    K = R + 1
    at = lambda dx, dy: grid[dy + K if C == 2 else 0][dx + K]
    inside = lambda tx, ty: (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    big = np.int64(1) << 40
    best = np.full((H, W), big)
    bkx, bky = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    ties = np.zeros((H, W), bool)
    for kx, ky in candidates(C, R):
        c = np.where(inside(bx + kx, by + ky), at(kx, ky), big)
        ties |= (c == best) & (c < big)
        take = c < best                                     # a later candidate wins only with a strictly smaller cost
        ties &= ~take
        best, bkx, bky = np.where(take, c, best), np.where(take, kx, bkx), np.where(take, ky, bky)
    matched = valued & (best < big)
    tx, ty = bx + bkx, by + bky
    pick = lambda ddx, ddy: sum(np.where((bkx == kx) & (bky == ky), at(kx + ddx, ky + ddy), 0) for kx, ky in candidates(C, R))
    qx, qy = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    hx = hy = ex = ey = np.zeros((H, W), bool)
    if subpixel:
        ex = matched & (tx - 1 >= 0) & (tx + 1 <= W - 1)
        hx, q = axis(pick(-1, 0), best, pick(1, 0))
        hx = hx & ex
        qx = np.where(hx, q, 0)
        if C == 2:
            ey = matched & (ty - 1 >= 0) & (ty + 1 <= H - 1)
            hy, q = axis(pick(0, -1), best, pick(0, 1))
            hy = hy & ey
            qy = np.where(hy, q, 0)
    rejected = matched & (best > max_cost)
    kept = matched & ~rejected
    out = np.full((C, H, W), NONE, np.int64)
    if C == 1:
        out[0] = np.where(kept, 256 * (r[0] - bkx) - qx, NONE)
    else:
        out[0] = np.where(kept, 256 * (r[0] + bkx) + qx, NONE)
        out[1] = np.where(kept, 256 * (r[1] + bky) + qy, NONE)
    cost = np.where(matched, best, 0xFFFF).astype(np.uint16)
    choice = np.where(matched, (bkx + R) if C == 1 else (bky + R) * (2 * R + 1) + bkx + R, 255).astype(np.uint8)
    stats = np.array([kept.sum(), (~valued).sum(), (valued & ~matched).sum(), rejected.sum()], np.int32)
    if info is not None:
        info.update(off_centre=int((matched & ((bkx != 0) | (bky != 0))).sum()), ties=int((matched & ties).sum()),
                    border=int((valued & ~interior(field, radius, R)).sum()),
                    axis_min=int(hx.sum() + hy.sum()), axis_none=int((ex & ~hx).sum() + (ey & ~hy).sum()))
    return out.astype(np.int32), cost, choice, stats


def interior(field, radius, R):
    """[H, W]: no target window of the pixel, the shifts of the parabola included, leaves the image (with C = 1 the rows of
    the target windows are the pixel's own) -- the pixels a kernel may work without clamping"""
    C, H, W = field.shape
    _, _, bx, by = base(field)
    m = radius + R + 1
    ok = (bx - m >= 0) & (bx + m <= W - 1)
    if C == 2:
        return ok & (by - m >= 0) & (by + m <= H - 1)
    ys = np.mgrid[0:H, 0:W][0]
    return ok & (ys - radius >= 0) & (ys + radius <= H - 1)


def search_np(field, imgL, imgR, prm=DEFAULTS, info=None):
    return decide(field, cost_grid(field, imgL, imgR, prm[0], prm[1]), prm, info)


def search(field, imgL, imgR, prm=DEFAULTS):
    """[P, C, H, W], [P, H, W], [P, H, W] -> out [P, C, H, W], cost [P, H, W], choice [P, H, W], stats [P, 4]"""
    res = [search_np(field[t], imgL[t], imgR[t], prm) for t in range(len(field))]
    return tuple(np.stack([r[k] for r in res]) for k in range(4))


def search_plain(field, imgL, imgR, prm, x, y):
    """ONE pixel by Python loops and integers, straight from the numbered steps of the rule: (out [C], cost, choice, state)
    with state 0 kept, 1 hole, 2 unmatched, 3 rejected"""
    radius, R, subpixel, max_cost = prm
    C, H, W = field.shape
    F = [int(field[c, y, x]) for c in range(C)]
    if F[0] == NONE:
        return [NONE] * C, 0xFFFF, 255, 1
    I = lambda img, px, py: int(img[min(max(py, 0), H - 1), min(max(px, 0), W - 1)])
    cost = lambda tx, ty: sum(abs(I(imgL, x + i, y + j) - I(imgR, tx + i, ty + j))
                              for j in range(-radius, radius + 1) for i in range(-radius, radius + 1))
    r = [(-1 if f < 0 else 1) * ((abs(f) + 128) >> 8) for f in F]
    bx, by = (x - r[0], y) if C == 1 else (x + r[0], y + r[1])
    adm = [(cost(bx + kx, by + ky), abs(kx) + abs(ky), ky, kx) for kx, ky in candidates(C, R)
           if 0 <= bx + kx < W and 0 <= by + ky < H]
    if not adm:
        return [NONE] * C, 0xFFFF, 255, 2
    c0, _, ky, kx = min(adm)
    tx, ty = bx + kx, by + ky

    def shift(cm, cp):
        a, n = cm + cp - 2 * c0, cm - cp
        if not (c0 <= cm and c0 <= cp and a > 0):
            return 0
        q = (256 * abs(n) + a) // (2 * a)
        return q if n >= 0 else -q
    qx = shift(cost(tx - 1, ty), cost(tx + 1, ty)) if subpixel and tx - 1 >= 0 and tx + 1 <= W - 1 else 0
    qy = shift(cost(tx, ty - 1), cost(tx, ty + 1)) if subpixel and C == 2 and ty - 1 >= 0 and ty + 1 <= H - 1 else 0
    choice = kx + R if C == 1 else (ky + R) * (2 * R + 1) + kx + R
    if c0 > max_cost:
        return [NONE] * C, c0, choice, 3
    return ([256 * (r[0] - kx) - qx] if C == 1 else [256 * (r[0] + kx) + qx, 256 * (r[1] + ky) + qy]), c0, choice, 0


# ---- data ------------------------------------------------------------------------------------------------------------------

def seed_of(W, H, C):
    return 9000 * W + 10 * H + C


def random_fields(W, H, C, P=1, seed=None):
    """[P, C, H, W] int32: most values point at a target inside the image (with a sub-pixel part), 8 % at one up to a
    window's reach outside it, 4 % far outside, 8 % holes"""
    rng = np.random.default_rng(seed_of(W, H, C) if seed is None else seed)
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.empty((P, C, H, W), np.int64)
    for t in range(P):
        tx, ty = rng.integers(0, W, (H, W)), rng.integers(0, H, (H, W))
        near = rng.random((H, W)) < 0.08
        tx = np.where(near, rng.choice([-1, -2, -7, W, W + 1, W + 6], (H, W)), tx)
        ty = np.where(near & (rng.random((H, W)) < 0.5), rng.choice([-1, -3, H, H + 5], (H, W)), ty)
        far = rng.random((H, W)) < 0.04
        sub = rng.integers(-127, 128, (C, H, W))
        f0 = 256 * (xs - tx if C == 1 else tx - xs) + sub[0]
        f0 = np.where(far, rng.choice([IMAX, IMIN1, 1 << 20, -(1 << 20), 70000, -70000], (H, W)), f0)
        out[t, 0] = np.where(rng.random((H, W)) < 0.08, NONE, f0)
        if C == 2:
            f1 = 256 * (ty - ys) + sub[1]
            out[t, 1] = np.where(rng.random((H, W)) < 0.03, rng.choice([IMAX, IMIN1, NONE, 12345], (H, W)), f1)
    return out.astype(np.int32)


def images(kind, W, H, P, C=1, seed=0):
    """(imgL, imgR) [P, H, W] uint8.  "random": noise on both sides, with flat rectangles (equal costs: ties, axes without a
    minimum) and rectangles of imgR copied from imgL (low costs off the centre).  "constant": one grey level a side.
    "shifted": imgR is imgL moved by TRUE_SHIFT[C], noise where nothing of imgL lands."""
    rng = np.random.default_rng(31 * seed + 7 * W + H + {"random": 0, "constant": 1, "shifted": 2}[kind])
    L = rng.integers(0, 256, (P, H, W)).astype(np.uint8)
    R = rng.integers(0, 256, (P, H, W)).astype(np.uint8)
    if kind == "constant":
        L[:], R[:] = 90, 97
    elif kind == "shifted":
        u, v = TRUE_SHIFT[C]
        if C == 1:
            u = -u                                           # the right pixel of x is x - d
        ys, xs = np.mgrid[0:H, 0:W]
        sy, sx = ys - v, xs - u                              # imgR[y][x] = imgL[y - v][x - u]
        ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
        for t in range(P):
            R[t] = np.where(ok, L[t][np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], R[t])
    else:
        for t in range(P):
            for _ in range(6):
                w, h = int(rng.integers(1, max(2, W // 2 + 1))), int(rng.integers(1, max(2, H // 2 + 1)))
                x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
                if rng.random() < 0.5:
                    L[t, y:y + h, x:x + w] = R[t, y:y + h, x:x + w] = rng.integers(0, 256)
                else:
                    R[t, y:y + h, x:x + w] = L[t, y:y + h, x:x + w]
    return L, R


def shifted_prior(W, H, C, P, R, seed=0):
    """[P, C, H, W]: the true value of "shifted" in 1/256 pixel, off by a whole number of pixels up to R per axis"""
    rng = np.random.default_rng(500 + seed)
    u, v = TRUE_SHIFT[C]
    f = np.empty((P, C, H, W), np.int32)
    f[:, 0] = 256 * (u + rng.integers(-R, R + 1, (P, H, W)))
    if C == 2:
        f[:, 1] = 256 * (v + rng.integers(-R, R + 1, (P, H, W)))
    return f


@functools.lru_cache(maxsize=None)
def case(kind, W, H, P, C):
    """the shared inputs of one (kind, size, C): (field, imgL, imgR), never changed"""
    L, R = images(kind, W, H, P, C)
    f = random_fields(W, H, C, P)
    for a in (f, L, R):
        a.setflags(write=False)
    return f, L, R


@functools.lru_cache(maxsize=None)
def grids(kind, W, H, P, C, radius, R):
    f, L, Rr = case(kind, W, H, P, C)
    return [cost_grid(f[t], L[t], Rr[t], radius, R) for t in range(P)]


def expected(kind, W, H, P, C, prm):
    """search() of case(...), the cost grids shared among the parameter sets that differ only in subpixel and max_cost"""
    f = case(kind, W, H, P, C)[0]
    res = [decide(f[t], g, prm) for t, g in enumerate(grids(kind, W, H, P, C, prm[0], prm[1]))]
    return tuple(np.stack([r[k] for r in res]) for k in range(4))
