"""The propagation of field values between neighbours (gpc_hip_propagate_*), restated with numpy from the rule in
include/gpc_hip.h for the tests to hold the GPU result equal to, as tests/search_util.py restates the search.  It shares
nothing with the kernel's method: no staged tile, no packed sums, no skipped duplicates, no second path for the border -- per
iteration every candidate index gets one cost image, every pixel of every window one clamped gather."""
import functools

import numpy as np

import search_util as su

NONE = su.NONE
DEFAULTS = (2, 1, 6, 8)             # radius, span, iterations, neighbours
SIZES = su.SIZES
KINDS = su.KINDS + ("edge",)
OFFSETS = [(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]   # the source of candidate j, in strides
BAND = 6                            # "edge": the prior is wrong this many pixels either side of the line
EDGE_TRUE = {1: ((1, 0), (4, 0)), 2: ((1, 2), (-3, 0))}   # "edge": the disparity d or the flow (u, v) left and right of the line
BIG = np.int64(1) << 40


def stride(span, i):
    return max(1, span >> i)


def displacement(F):
    """[C, H, W] int64 -> (dx, dy) [H, W]: target less pixel, (-r_0, 0) with C = 1 and (r_0, r_1) with C = 2"""
    r = su.whole(F)
    return (-r[0], np.zeros_like(r[0])) if len(F) == 1 else (r[0], r[1])


def left_windows(imgL, radius):
    H, W = imgL.shape
    ys, xs = np.mgrid[0:H, 0:W]
    o = range(-radius, radius + 1)
    return {(i, j): imgL[np.clip(ys + j, 0, H - 1), np.clip(xs + i, 0, W - 1)].astype(np.int64) for j in o for i in o}


def cost_image(left, imgR, tx, ty, radius):
    """cost(p, t) [H, W] int64 with t = (tx, ty) [H, W], all addresses clamped"""
    H, W = tx.shape
    R = imgR.astype(np.int64)
    o = range(-radius, radius + 1)
    total = np.zeros((H, W), np.int64)
    for j in o:
        row = np.clip(ty + j, 0, H - 1)
        for i in o:
            total += np.abs(left[(i, j)] - R[row, np.clip(tx + i, 0, W - 1)])
    return total


def step(F, left, imgR, radius, s, nb, info=None, origin=None):
    """one iteration over one pair: F [C, H, W] int64 -> (new F, cost [H, W] uint16, choice [H, W] uint8, stats [4] int32)"""
    C, H, W = F.shape
    ys, xs = np.mgrid[0:H, 0:W]
    valued = F[0] != NONE
    dx, dy = displacement(F)
    best = np.full((H, W), BIG)
    bj = np.full((H, W), -1, np.int64)
    cand = []                                                # per j: (is a candidate, admissible, dx, dy, cost, source y, source x)
    for j, (ox, oy) in enumerate(OFFSETS[:nb + 1]):
        qx, qy = xs + ox * s, ys + oy * s
        exists = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        cy_, cx_ = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
        is_c = exists & valued[cy_, cx_]
        ddx, ddy = dx[cy_, cx_], dy[cy_, cx_]
        tx, ty = xs + ddx, ys + ddy
        adm = is_c & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        c = np.where(adm, cost_image(left, imgR, tx, ty, radius), BIG)
        take = c < best                                      # a later candidate wins only with a strictly smaller cost
        best, bj = np.where(take, c, best), np.where(take, j, bj)
        cand.append((is_c, adm, ddx, ddy, c, cy_, cx_, exists))
    matched = valued & (bj >= 0)
    moved = matched & (bj > 0)
    out = F.copy()
    for j in range(1, nb + 1):
        w = moved & (bj == j)
        ddx, ddy = cand[j][2], cand[j][3]
        if C == 1:
            out[0] = np.where(w, 256 * -ddx, out[0])
        else:
            out[0], out[1] = np.where(w, 256 * ddx, out[0]), np.where(w, 256 * ddy, out[1])
    cost = np.where(matched, best, 0xFFFF).astype(np.uint16)
    choice = np.where(matched, bj, 255).astype(np.uint8)
    stats = np.array([(matched & ~moved).sum(), (~valued).sum(), (valued & ~matched).sum(), moved.sum()], np.int32)
    if info is not None:
        observe(info, valued, matched, moved, bj, best, cand, radius, nb, origin)
    return out, cost, choice, stats


def observe(info, valued, matched, moved, bj, best, cand, radius, nb, origin):
    """what the condition test of tests/test_propagate.py asks about, counted into info; origin [2, H, W] (updated in place):
    the pixel whose input value a pixel holds"""
    H, W = valued.shape
    ys, xs = np.mgrid[0:H, 0:W]
    add = lambda k, m: info.__setitem__(k, info.get(k, 0) + int(np.sum(m)))
    differs = lambda a, b: (cand[a][2] != cand[b][2]) | (cand[a][3] != cand[b][3])
    for j in range(1, nb + 1):
        add("won_by_%d" % j, moved & (bj == j))
        add("tie_own_wins", matched & (bj == 0) & cand[j][1] & (cand[j][4] == best) & differs(0, j))
        add("source_outside", valued & ~cand[j][7])
        add("source_hole", valued & cand[j][7] & ~cand[j][0])
        add("own_inadmissible_neighbour_admissible", valued & ~cand[0][1] & cand[j][1])
        add("duplicate_of_own", valued & cand[j][0] & ~differs(0, j))
        for k in range(1, j):
            add("tie_between_neighbours", moved & (bj == k) & cand[j][1] & (cand[j][4] == best) & differs(k, j))
            add("duplicate_of_neighbour", valued & cand[j][0] & cand[k][0] & ~differs(k, j) & differs(0, j))
    add("unmatched", valued & ~matched)
    win_dx = sum(np.where(bj == j, cand[j][2], 0) for j in range(nb + 1))
    win_dy = sum(np.where(bj == j, cand[j][3], 0) for j in range(nb + 1))
    tx, ty = xs + win_dx, ys + win_dy
    # the kernel's fast path: the target window inside the image AND the dwords of its last row's load inside the buffer
    # (4 * ceil((2r + 1) / 4) bytes from the row's first byte); every other winner takes the clamped byte-wise path
    interior = (tx - radius >= 0) & (tx + radius <= W - 1) & (ty - radius >= 0) & (ty + radius <= H - 1) & \
        ((ty + radius) * W + (tx - radius) + 4 * ((2 * radius + 1 + 3) // 4) <= W * H)
    tile_edge = (xs % su.TILE_W == 0) | (xs % su.TILE_W == su.TILE_W - 1) | (ys % su.TILE_H == 0) | (ys % su.TILE_H == su.TILE_H - 1)
    add("tile_edge_winner_interior", moved & tile_edge & interior)
    add("tile_edge_winner_clamped", moved & tile_edge & ~interior)
    if origin is not None:
        new = origin.copy()
        for j in range(1, nb + 1):
            w = moved & (bj == j)
            new[:, w] = origin[:, cand[j][5][w], cand[j][6][w]]
        origin[:] = new


def run(field, imgL, imgR, radius, span, iterations, nb, info=None):
    """one pair: field [C, H, W] int32 -> per iteration (field int32, cost, choice, stats): the state after iterations 1 .. N.
    An iteration reads only what the one before it wrote, so the entry of iteration i does not depend on N."""
    F = field.astype(np.int64)
    C, H, W = F.shape
    left = left_windows(imgL, radius)
    origin = np.array(np.mgrid[0:H, 0:W]) if info is not None else None
    moves = np.zeros((H, W), np.int64)
    res = []
    for i in range(iterations):
        F, cost, choice, stats = step(F, left, imgR, radius, stride(span, i), nb, info, origin)
        moves += (choice != 0) & (choice != 255)
        res.append((F.astype(np.int32), cost, choice, stats))
    if info is not None:
        ys, xs = np.mgrid[0:H, 0:W]
        far = np.maximum(np.abs(origin[0] - ys), np.abs(origin[1] - xs)) > stride(span, 0)
        info["travelled_further_than_a_stride"] = info.get("travelled_further_than_a_stride", 0) + int(far.sum())
        info["moved_in_two_iterations"] = info.get("moved_in_two_iterations", 0) + int((moves >= 2).sum())
    return res


def pack(per_pair, N):
    """run() of every pair -> out [P, C, H, W], cost [P, H, W], choice [P, H, W] after iteration N, stats [P, N, 4]"""
    return (np.stack([r[N - 1][0] for r in per_pair]), np.stack([r[N - 1][1] for r in per_pair]),
            np.stack([r[N - 1][2] for r in per_pair]), np.stack([np.stack([r[i][3] for i in range(N)]) for r in per_pair]))


def propagate(field, imgL, imgR, prm=DEFAULTS):
    """[P, C, H, W], [P, H, W], [P, H, W] -> out [P, C, H, W], cost [P, H, W], choice [P, H, W], stats [P, N, 4]"""
    radius, span, N, nb = prm
    return pack([run(field[t], imgL[t], imgR[t], radius, span, N, nb) for t in range(len(field))], N)


def propagate_plain(field, imgL, imgR, prm, x, y):
    """ONE pixel of ONE iteration (prm[1] is that iteration's stride) by Python loops and integers, straight from the numbered
    steps of the rule: (out [C], cost, choice, state) with state 0 kept its own value, 1 hole, 2 unmatched, 3 moved"""
    radius, s, _, nb = prm
    C, H, W = field.shape
    F = lambda qx, qy: [int(field[c, qy, qx]) for c in range(C)]
    own = F(x, y)
    if own[0] == NONE:
        return own, 0xFFFF, 255, 1
    I = lambda img, px, py: int(img[min(max(py, 0), H - 1), min(max(px, 0), W - 1)])
    cost = lambda tx, ty: sum(abs(I(imgL, x + i, y + j) - I(imgR, tx + i, ty + j))
                              for j in range(-radius, radius + 1) for i in range(-radius, radius + 1))
    rnd = lambda f: (-1 if f < 0 else 1) * ((abs(f) + 128) >> 8)
    adm = []
    for j, (ox, oy) in enumerate(OFFSETS[:nb + 1]):
        qx, qy = x + ox * s, y + oy * s
        if not (0 <= qx < W and 0 <= qy < H):
            continue
        v = F(qx, qy)
        if v[0] == NONE:
            continue
        r = [rnd(f) for f in v]
        tx, ty = (x - r[0], y) if C == 1 else (x + r[0], y + r[1])
        if 0 <= tx < W and 0 <= ty < H:
            adm.append((cost(tx, ty), j, r))
    if not adm:
        return own, 0xFFFF, 255, 2
    c0, j, r = min(adm)
    return (own if j == 0 else [256 * v for v in r]), c0, j, (0 if j == 0 else 3)


# ---- data ------------------------------------------------------------------------------------------------------------------

def edge_line(W):
    return W // 2


def edge_pair(W, H, C, seed):
    """one pair of kind "edge": (imgL, imgR, truth [C, H, W] in whole pixels, visible [H, W]).  imgR is imgL moved by
    EDGE_TRUE[C][0] left of the vertical line x = W // 2 and by EDGE_TRUE[C][1] right of it, the right side painted over the
    left where both land, noise where nothing lands.  visible: the pixel's true target lies inside the image and shows it."""
    rng = np.random.default_rng(7700 + 13 * seed + W + 3 * H + C)
    L = rng.integers(0, 256, (H, W)).astype(np.uint8)
    R = rng.integers(0, 256, (H, W)).astype(np.uint8)
    ys, xs = np.mgrid[0:H, 0:W]
    right = xs >= edge_line(W)
    (a0, a1), (b0, b1) = EDGE_TRUE[C]
    t0, t1 = np.where(right, b0, a0), np.where(right, b1, a1)
    tx, ty = (xs - t0, ys) if C == 1 else (xs + t0, ys + t1)
    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    owner = np.full((H, W), -1, np.int64)
    for side in (~right, right):                             # the right side last: it hides what the left side put there
        m = inside & side
        R[ty[m], tx[m]] = L[m]
        owner[ty[m], tx[m]] = (ys * W + xs)[m]
    visible = inside & (owner[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)] == ys * W + xs)
    return L, R, np.stack([t0, t1][:C]), visible


def edge_band(W, H):
    xs = np.mgrid[0:H, 0:W][1]
    return (xs >= edge_line(W) - BAND) & (xs < edge_line(W) + BAND)


def edge_case(W, H, P, C):
    """(field [P, C, H, W] int32, imgL, imgR [P, H, W], truth [P, C, H, W], visible [P, H, W]): the prior takes the WRONG
    side's value in the band and the true value elsewhere"""
    pairs = [edge_pair(W, H, C, t) for t in range(P)]
    xs = np.mgrid[0:H, 0:W][1]
    right = xs >= edge_line(W)
    wrong = np.stack([np.where(right, EDGE_TRUE[C][0][c], EDGE_TRUE[C][1][c]) for c in range(C)])
    band = edge_band(W, H)
    field = np.stack([256 * np.where(band, wrong, q[2]) for q in pairs]).astype(np.int32)
    return field, np.stack([q[0] for q in pairs]), np.stack([q[1] for q in pairs]), np.stack([q[2] for q in pairs]), \
        np.stack([q[3] for q in pairs])


@functools.lru_cache(maxsize=None)
def case(kind, W, H, P, C):
    """the shared inputs of one (kind, size, C): (field, imgL, imgR), never changed"""
    if kind != "edge":
        return su.case(kind, W, H, P, C)
    f, L, R = edge_case(W, H, P, C)[:3]
    for a in (f, L, R):
        a.setflags(write=False)
    return f, L, R


SPANS = (1, 4, 64)
MAX_N = 3


@functools.lru_cache(maxsize=None)
def runs(kind, W, H, P, C, radius, span, nb):
    """run() of every pair of case(...) over MAX_N iterations, with what the condition test asks about: (per pair, info)"""
    f, L, R = case(kind, W, H, P, C)
    info = {}
    return [run(f[t], L[t], R[t], radius, span, MAX_N, nb, info) for t in range(P)], info


def expected(kind, W, H, P, C, prm):
    """propagate() of case(...) for iterations <= MAX_N, the iterations shared among the parameter sets that differ only in N"""
    radius, span, N, nb = prm
    return pack(runs(kind, W, H, P, C, radius, span, nb)[0], N)
