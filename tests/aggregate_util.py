"""The scanline aggregation of the search's costs (gpc_hip_aggregate_*), restated from the rule in include/gpc_hip.h for the
tests to hold the GPU result equal to.  Two restatements on search_util.cost_grid: aggregate(), numpy across the pixels of a
scanline front, and aggregate_plain(), one pixel at a time by Python loops.  BOTH take the minimum over all pairs (k, j) of
labels as the rule states it; neither knows the shift form the kernels use."""
import functools

import numpy as np

import search_util as su

NONE = su.NONE
DEFAULTS = (2, 1, 1, 0xFFFF, 128, 512, 15)     # radius, range, subpixel, max_cost, p1, p2, paths
NO_AGG = 0xFFFFFFFF
BIG = np.int64(1) << 40
LANES = 64                                   # chains per workgroup of the path kernels
CHUNKS = (8, 16, 32)                         # columns a horizontal path stages at a time, by the number of labels


def labels(C, R):
    """the labels in the order of `choice`: (kx, ky), index (ky + R)(2R + 1) + kx + R"""
    return [(kx, ky) for ky in (range(-R, R + 1) if C == 2 else (0,)) for kx in range(-R, R + 1)]


def volume(field, grid, R):
    """one pair -> c [K, H, W] int64, adm [K, H, W] bool (valued and the target inside), dx, dy [K, H, W] the displacements"""
    C, H, W = field.shape
    valued, r, bx, by = su.base(field)
    ks = labels(C, R)
    c = np.stack([grid[ky + R + 1 if C == 2 else 0][kx + R + 1] for kx, ky in ks])
    adm = np.stack([valued & (bx + kx >= 0) & (bx + kx < W) & (by + ky >= 0) & (by + ky < H) for kx, ky in ks])
    dx = np.stack([kx - r[0] if C == 1 else r[0] + kx for kx, ky in ks])
    dy = np.stack([np.zeros((H, W), np.int64) if C == 1 else r[1] + ky for kx, ky in ks])
    return c, adm, dx, dy


def penalty(vx, vy, p1, p2):
    ch = np.maximum(np.abs(vx), np.abs(vy))
    return np.where(ch == 0, 0, np.where(ch == 1, p1, p2))


def path_lr(c, adm, dx, dy, p1, p2):
    """L [K, H, W] of the direction whose predecessor is (x - 1, y), a column of pixels at a time; garbage where not adm"""
    K, H, W = c.shape
    live = adm.any(0)
    L = np.zeros((K, H, W), np.int64)
    for x in range(W):
        if x == 0:
            L[:, :, 0] = c[:, :, 0]
            continue
        Lq = np.where(adm[:, :, x - 1], L[:, :, x - 1], BIG)                                   # [j, H]
        V = penalty(dx[:, None, :, x] - dx[None, :, :, x - 1], dy[:, None, :, x] - dy[None, :, :, x - 1], p1, p2)   # [k, j, H]
        L[:, :, x] = np.where(live[:, x - 1][None], c[:, :, x] + (Lq[None] + V).min(1) - Lq.min(0)[None], c[:, :, x])
    return L


def path(bit, c, adm, dx, dy, p1, p2):
    """the four directions through path_lr by mirroring and transposing the arrays (V depends on |v_x|, |v_y| only)"""
    t = (lambda a: a) if bit in (1, 2) else (lambda a: a.transpose(0, 2, 1))
    m = (lambda a: a) if bit in (1, 4) else (lambda a: a[:, :, ::-1])
    return t(m(path_lr(*(m(t(a)) for a in (c, adm, dx, dy)), p1, p2)))


def sums(c, adm, dx, dy, p1, p2, paths):
    if paths == 0:
        return c.copy()
    return sum(path(b, c, adm, dx, dy, p1, p2) for b in (1, 2, 4, 8) if paths & b)


def finish(field, grid, prm, S, adm):
    """the choice over S and steps 5 - 7 of the search on the raw costs: out, cost, choice, stats, agg of one pair"""
    radius, R, subpixel, max_cost = prm[:4]
    C, H, W = field.shape
    valued, r, bx, by = su.base(field)
    K = R + 1
    at = lambda ddx, ddy: grid[ddy + K if C == 2 else 0][ddx + K]
    idx = {k: i for i, k in enumerate(labels(C, R))}
    best, bc = np.full((H, W), BIG), np.zeros((H, W), np.int64)
    bkx, bky = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for kx, ky in su.candidates(C, R):
        i = idx[(kx, ky)]
        take = adm[i] & (S[i] < best)                         # a later candidate wins only with a strictly smaller sum
        best, bc = np.where(take, S[i], best), np.where(take, at(kx, ky), bc)
        bkx, bky = np.where(take, kx, bkx), np.where(take, ky, bky)
    matched = valued & (best < BIG)
    tx, ty = bx + bkx, by + bky
    pick = lambda ddx, ddy: sum(np.where((bkx == kx) & (bky == ky), at(kx + ddx, ky + ddy), 0) for kx, ky in labels(C, R))
    qx, qy = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    if subpixel:
        hx, q = su.axis(pick(-1, 0), bc, pick(1, 0))
        qx = np.where(hx & matched & (tx - 1 >= 0) & (tx + 1 <= W - 1), q, 0)
        if C == 2:
            hy, q = su.axis(pick(0, -1), bc, pick(0, 1))
            qy = np.where(hy & matched & (ty - 1 >= 0) & (ty + 1 <= H - 1), q, 0)
    rejected = matched & (bc > max_cost)
    kept = matched & ~rejected
    out = np.full((C, H, W), NONE, np.int64)
    if C == 1:
        out[0] = np.where(kept, 256 * (r[0] - bkx) - qx, NONE)
    else:
        out[0] = np.where(kept, 256 * (r[0] + bkx) + qx, NONE)
        out[1] = np.where(kept, 256 * (r[1] + bky) + qy, NONE)
    cost = np.where(matched, bc, 0xFFFF).astype(np.uint16)
    choice = np.where(matched, (bkx + R) if C == 1 else (bky + R) * (2 * R + 1) + bkx + R, 255).astype(np.uint8)
    stats = np.array([kept.sum(), (~valued).sum(), (valued & ~matched).sum(), rejected.sum()], np.int32)
    agg = np.where(matched, best, NO_AGG).astype(np.uint32)
    return out.astype(np.int32), cost, choice, stats, agg


def aggregate_pair(field, grid, prm, info=None):
    R, p1, p2, paths = prm[1], prm[4], prm[5], prm[6]
    c, adm, dx, dy = volume(field, grid, R)
    if info is not None and paths:
        info["max_L"] = max(int(np.where(adm, path(b, c, adm, dx, dy, p1, p2), 0).max()) for b in (1, 2, 4, 8) if paths & b)
    return finish(field, grid, prm, sums(c, adm, dx, dy, p1, p2, paths), adm)


def aggregate(field, imgL, imgR, prm=DEFAULTS, info=None):
    """[P, C, H, W], [P, H, W], [P, H, W] -> out [P, C, H, W], cost, choice [P, H, W], stats [P, 4], agg [P, H, W]"""
    res = [aggregate_pair(field[t], su.cost_grid(field[t], imgL[t], imgR[t], prm[0], prm[1]), prm, info) for t in range(len(field))]
    return tuple(np.stack([r[k] for r in res]) for k in range(5))


def aggregate_plain(field, imgL, imgR, prm):
    """ONE pair [C, H, W], one pixel at a time by Python loops and integers, straight from the rule: the minimum over all
    pairs (k, j), literally.  -> out [C, H, W], cost, choice, state [H, W] (0 kept, 1 hole, 2 unmatched, 3 rejected), agg"""
    radius, R, subpixel, max_cost, p1, p2, paths = prm
    C, H, W = field.shape
    grid = su.cost_grid(field, imgL, imgR, radius, R)
    cost_at = lambda x, y, ddx, ddy: int(grid[ddy + R + 1 if C == 2 else 0][ddx + R + 1][y, x])
    rnd = lambda f: (-1 if f < 0 else 1) * ((abs(f) + 128) >> 8)
    ks = labels(C, R)
    A, D, r_of = {}, {}, {}
    for y in range(H):
        for x in range(W):
            F = [int(field[ch, y, x]) for ch in range(C)]
            if F[0] == NONE:
                continue
            r = [rnd(f) for f in F]
            bx, by = (x - r[0], y) if C == 1 else (x + r[0], y + r[1])
            adm = [k for k in ks if 0 <= bx + k[0] < W and 0 <= by + k[1] < H]
            r_of[(x, y)] = (r, bx, by)
            if adm:
                A[(x, y)] = adm
                D[(x, y)] = {k: ((k[0] - r[0], 0) if C == 1 else (r[0] + k[0], r[1] + k[1])) for k in adm}

    def V(a, b):
        m = max(abs(a[0] - b[0]), abs(a[1] - b[1]))
        return 0 if m == 0 else (p1 if m == 1 else p2)

    S = {p: {k: 0 for k in A[p]} for p in A}
    for bit, (qx, qy) in ((1, (-1, 0)), (2, (1, 0)), (4, (0, -1)), (8, (0, 1))):
        if not paths & bit:
            continue
        L = {}
        xs = range(W) if qx <= 0 else range(W - 1, -1, -1)
        ys = range(H) if qy <= 0 else range(H - 1, -1, -1)
        for y in ys:
            for x in xs:
                p, q = (x, y), (x + qx, y + qy)
                if p not in A:
                    continue
                L[p] = {}
                for k in A[p]:
                    c = cost_at(x, y, *k)
                    if q in A:                              # inside the image and live
                        L[p][k] = c + min(L[q][j] + V(D[p][k], D[q][j]) for j in A[q]) - min(L[q][j] for j in A[q])
                    else:
                        L[p][k] = c
                    S[p][k] += L[p][k]
    out = np.full((C, H, W), NONE, np.int64)
    cost, choice = np.full((H, W), 0xFFFF, np.uint16), np.full((H, W), 255, np.uint8)
    state, agg = np.ones((H, W), np.int32), np.full((H, W), NO_AGG, np.uint32)
    for (x, y), (r, bx, by) in r_of.items():
        if (x, y) not in A:
            state[y, x] = 2
            continue
        s, _, ky, kx = min(((S[(x, y)][k] if paths else cost_at(x, y, *k)), abs(k[0]) + abs(k[1]), k[1], k[0]) for k in A[(x, y)])
        c0, tx, ty = cost_at(x, y, kx, ky), bx + kx, by + ky

        def shift(cm, cp):
            a, n = cm + cp - 2 * c0, cm - cp
            if not (c0 <= cm and c0 <= cp and a > 0):
                return 0
            q = (256 * abs(n) + a) // (2 * a)
            return q if n >= 0 else -q
        qx = shift(cost_at(x, y, kx - 1, ky), cost_at(x, y, kx + 1, ky)) if subpixel and tx - 1 >= 0 and tx + 1 <= W - 1 else 0
        qy = shift(cost_at(x, y, kx, ky - 1), cost_at(x, y, kx, ky + 1)) if subpixel and C == 2 and ty - 1 >= 0 and ty + 1 <= H - 1 else 0
        cost[y, x], choice[y, x], agg[y, x] = c0, (kx + R if C == 1 else (ky + R) * (2 * R + 1) + kx + R), s
        state[y, x] = 3 if c0 > max_cost else 0
        if c0 <= max_cost:
            out[:, y, x] = [256 * (r[0] - kx) - qx] if C == 1 else [256 * (r[0] + kx) + qx, 256 * (r[1] + ky) + qy]
    return out.astype(np.int32), cost, choice, state, agg


# ---- data ------------------------------------------------------------------------------------------------------------------

def stepped_fields(W, H, C, P, R, seed=0, holes=0.05, outside=0.04, extremes=0.01):
    """[P, C, H, W] int32: a prior whose whole-pixel base is a[x] + b[y] per channel, a and b walks whose steps are drawn from
    0, 1, R, 2R, 2R + 1, 2R + 2 and 9 with either sign -- so the label bands of neighbours coincide, overlap by one, touch and
    miss each other, in both directions -- kept within a few pixels of zero; a sub-pixel part that never rounds across; holes
    sprinkled through it, priors that point out of the image, and the extremes of int32"""
    rng = np.random.default_rng(7000 + 131 * seed + 17 * W + H + 3 * C + R)
    steps = np.array([0, 0, 0, 1, R, 2 * R, 2 * R + 1, 2 * R + 2, 9])

    def walk(n, lim):
        a, out = 0, []
        for _ in range(n):
            s = int(rng.choice(steps)) * int(rng.choice([-1, 1]))
            if abs(a + s) > lim:
                s = -s
            if abs(a + s) > lim:
                s = 0
            a += s
            out.append(a)
        return np.array(out, np.int64)

    f = np.empty((P, C, H, W), np.int64)
    for t in range(P):
        for ch in range(C):
            lim = max(2, (W if ch == 0 else H) // 3)
            whole = walk(W, lim)[None, :] + walk(H, lim)[:, None]
            f[t, ch] = 256 * whole + rng.integers(-100, 101, (H, W))
        out_x = rng.random((H, W)) < outside
        f[t, 0] = np.where(out_x, 256 * rng.choice([-(W + 1), W + 2, -W, W], (H, W)), f[t, 0])
        ext = rng.random((H, W)) < extremes
        f[t, 0] = np.where(ext, rng.choice([su.IMAX, su.IMIN1], (H, W)), f[t, 0])
        if C == 2:
            ext = rng.random((H, W)) < extremes
            f[t, 1] = np.where(ext, rng.choice([su.IMAX, su.IMIN1, NONE], (H, W)), f[t, 1])
        f[t, 0] = np.where(rng.random((H, W)) < holes, NONE, f[t, 0])
    return f.astype(np.int32)


@functools.lru_cache(maxsize=None)
def stepped_case(W, H, P, C, R, seed=0):
    """the shared inputs of one stepped case: (field, imgL, imgR), never changed"""
    L, Rr = su.images("random", W, H, P, C, seed=seed + 1)
    f = stepped_fields(W, H, C, P, R, seed)
    for a in (f, L, Rr):
        a.setflags(write=False)
    return f, L, Rr


@functools.lru_cache(maxsize=None)
def stepped_grids(W, H, P, C, R, radius, seed=0):
    f, L, Rr = stepped_case(W, H, P, C, R, seed)
    return [su.cost_grid(f[t], L[t], Rr[t], radius, R) for t in range(P)]


def expected_stepped(W, H, P, C, prm, seed=0):
    """aggregate() of stepped_case(...), the cost grids shared among the parameter sets of one radius and range"""
    f = stepped_case(W, H, P, C, prm[1], seed)[0]
    res = [aggregate_pair(f[t], g, prm) for t, g in enumerate(stepped_grids(W, H, P, C, prm[1], prm[0], seed))]
    return tuple(np.stack([r[k] for r in res]) for k in range(5))


def expected_search_case(kind, W, H, P, C, prm):
    """aggregate() of search_util.case(...), on search_util's shared cost grids"""
    f = su.case(kind, W, H, P, C)[0]
    res = [aggregate_pair(f[t], g, prm) for t, g in enumerate(su.grids(kind, W, H, P, C, prm[0], prm[1]))]
    return tuple(np.stack([r[k] for r in res]) for k in range(5))


# ---- the crafted scene -------------------------------------------------------------------------------------------------------
# A disparity pair of 20 columns, every row the same: texture in columns 0 .. 5 and 14 .. 19, one grey level in columns 6 .. 13,
# imgR[x] = imgL[x + 1] (the true disparity is 1), the prior 0 everywhere.  Radius 1, range 1: label kx = -1 (choice 0) is the
# true one.  Where a window sees texture the evidence says so; in columns 7 .. 10 the three windows of a pixel are all grey,
# the three costs tie at 0, and the search keeps the prior (choice 1).  Aggregated along the rows, the band follows its
# neighbours (choice 0).  Column 0 has no target for kx = -1; the last columns see the padding of imgR.
SCENE_ROW = [10, 200, 60, 250, 30, 180, 100, 100, 100, 100, 100, 100, 100, 100, 220, 20, 160, 70, 240, 40]
SCENE_W, SCENE_H = 20, 5
SCENE_PRM = (1, 1, 0, 0xFFFF, 20, 60, 3)
# The winners, written out by hand: choice = kx + 1 per column, every row the same.  Column 0 has no target for kx = -1, and
# of its other two costs (520 for
# kx = 0: |10-200| + |10-200| + |200-60|; 290 for kx = 1: |10-200| + |10-60| + |200-250|) the second is smaller; column 1 sees
# the clamped border too (190 for kx = -1, 130 for kx = 1).  Columns 2 .. 6 and 12 .. 19 see texture: kx = -1 costs 0, the
# others do not.  Columns 7 .. 11: kx = -1 and kx = 0 tie at 0.
SEARCH_WINNERS = [2, 2, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
AGGREGATE_WINNERS = [2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]


def scene():
    """(field [1, 1, H, W], imgL, imgR [1, H, W])"""
    row = np.array(SCENE_ROW, np.uint8)
    L = np.tile(row, (SCENE_H, 1))[None]
    R = np.tile(np.concatenate([row[1:], row[-1:]]), (SCENE_H, 1))[None]
    return np.zeros((1, 1, SCENE_H, SCENE_W), np.int32), L, R
