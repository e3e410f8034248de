"""The field cleaner's rule (include/gpc_hip.h, gpc_hip_clean_*) restated twice: clean_plain with Python loops, Python
integers and a breadth-first flood fill for the components, and clean_np with numpy (minimum hooking with pointer jumping
for the components, a sort along the window axis for the median).  Neither shares anything with the kernels' method (tiles,
a union-find in LDS, ranks).  Also the reversed records, and the fields the GPU tests run on: random ones by seed, and
constructed ones that label wrongly when the union across tiles is wrong."""
from collections import deque

import numpy as np

from dense_util import CORR, REFINEMENT, SUPPORT, valid

NONE = -2 ** 31
IMAX, IMIN1 = 2 ** 31 - 1, -2 ** 31 + 1
DEFAULTS = (256, 256, 64, 1)       # check_tol_q8, speckle_diff_q8, speckle_min, median_radius
SIZES = [(1, 1), (1, 40), (40, 1), (7, 5), (33, 17), (96, 64), (130, 67), (200, 90)]
TILE = 32


def rshift(f):
    """sgn(f) * ((|f| + 128) >> 8) of a Python integer"""
    f = int(f)
    r = (abs(f) + 128) >> 8
    return -r if f < 0 else r


def clean_plain(fwd, bwd=None, prm=DEFAULTS, want_label=True):
    """one pair: fwd, bwd [C, H, W] -> out [C, H, W] int32, state [H, W] uint8, label [H, W] int32, stats [4] int32"""
    tol, diff, smin, radius = prm
    C, H, W = fwd.shape
    F = [[[int(fwd[c, y, x]) for x in range(W)] for y in range(H)] for c in range(C)]
    state = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            if F[0][y][x] == NONE:
                state[y][x] = 1
                continue
            if tol < 0:
                continue
            qx = x - rshift(F[0][y][x]) if C == 1 else x + rshift(F[0][y][x])
            qy = y if C == 1 else y + rshift(F[1][y][x])
            if not (0 <= qx < W and 0 <= qy < H) or int(bwd[0, qy, qx]) == NONE:
                state[y][x] = 2
            elif any(abs(F[c][y][x] + int(bwd[c, qy, qx])) > tol for c in range(C)):
                state[y][x] = 2
    label = [[-1] * W for _ in range(H)]
    if want_label or smin > 1:
        for y0 in range(H):
            for x0 in range(W):
                if state[y0][x0] != 0 or label[y0][x0] >= 0:
                    continue
                root = y0 * W + x0                      # scanned in index order: the first pixel met is the lowest
                label[y0][x0] = root
                members, todo = [(x0, y0)], deque([(x0, y0)])
                while todo:
                    x, y = todo.popleft()
                    for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                        if not (0 <= nx < W and 0 <= ny < H) or state[ny][nx] != 0 or label[ny][nx] >= 0:
                            continue
                        if all(abs(F[c][y][x] - F[c][ny][nx]) <= diff for c in range(C)):
                            label[ny][nx] = root
                            members.append((nx, ny))
                            todo.append((nx, ny))
                if smin > 1 and len(members) < smin:
                    for x, y in members:
                        state[y][x] = 3
    out = np.full((C, H, W), NONE, np.int64)
    for y in range(H):
        for x in range(W):
            if state[y][x] != 0:
                continue
            win = [(wx, wy) for wy in range(max(y - radius, 0), min(y + radius, H - 1) + 1)
                   for wx in range(max(x - radius, 0), min(x + radius, W - 1) + 1) if state[wy][wx] == 0]
            for c in range(C):
                vals = sorted(F[c][wy][wx] for wx, wy in win)
                out[c, y, x] = vals[(len(vals) - 1) >> 1]
    st = np.array(state, np.uint8).reshape(H, W)
    lab = np.array(label, np.int32).reshape(H, W)
    if not want_label:
        lab = None
    return out.astype(np.int32), st, lab, np.bincount(st.ravel(), minlength=4)[:4].astype(np.int32)


def components_np(ok, F, diff):
    """ok [H, W] bool, F [C, H, W] int64 -> label [H, W]: the lowest index of each pixel's component, -1 where not ok"""
    C, H, W = F.shape
    idx = np.arange(H * W).reshape(H, W)
    hj = ok[:, 1:] & ok[:, :-1] & (np.abs(F[:, :, 1:] - F[:, :, :-1]) <= diff).all(0)
    vj = ok[1:, :] & ok[:-1, :] & (np.abs(F[:, 1:, :] - F[:, :-1, :]) <= diff).all(0)
    a = np.concatenate([idx[:, 1:][hj], idx[1:, :][vj]])
    b = np.concatenate([idx[:, :-1][hj], idx[:-1, :][vj]])
    L = np.arange(H * W)
    while True:
        la, lb = L[a], L[b]
        m = np.minimum(la, lb)
        n = L.copy()
        for k in (la, lb, a, b):
            np.minimum.at(n, k, m)
        while True:
            j = n[n]
            if np.array_equal(j, n):
                break
            n = j
        if np.array_equal(n, L):
            break
        L = n
    return np.where(ok, L.reshape(H, W), -1)


def clean_np(fwd, bwd=None, prm=DEFAULTS, want_label=True):
    """clean_plain, vectorised"""
    tol, diff, smin, radius = prm
    C, H, W = fwd.shape
    F = fwd.astype(np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    state = np.zeros((H, W), np.int64)
    state[F[0] == NONE] = 1
    if tol >= 0:
        G = bwd.astype(np.int64)
        r = np.sign(F) * ((np.abs(F) + 128) >> 8)
        qx = xs - r[0] if C == 1 else xs + r[0]
        qy = ys if C == 1 else ys + r[1]
        inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
        Gq = G[:, cy, cx]
        bad = ~inside | (Gq[0] == NONE) | (np.abs(F + Gq) > tol).any(0)
        state[(state == 0) & bad] = 2
    label = None
    if want_label or smin > 1:
        label = components_np(state == 0, F, diff)
        if smin > 1:
            size = np.bincount(label[label >= 0], minlength=H * W)
            state[(label >= 0) & (size[np.maximum(label, 0)] < smin)] = 3
    kept = state == 0
    big = np.int64(2) ** 40
    pv = np.pad(np.where(kept[None], F, big), ((0, 0), (radius, radius), (radius, radius)), constant_values=big)
    win = np.stack([pv[:, j:j + H, i:i + W] for j in range(2 * radius + 1) for i in range(2 * radius + 1)])
    win.sort(axis=0)
    n = (win[:, 0] != big).sum(0)
    pick = np.maximum(n - 1, 0) >> 1
    med = np.take_along_axis(win, np.broadcast_to(pick, (1, C, H, W)), 0)[0]
    out = np.where(kept[None], med, NONE).astype(np.int32)
    lab = label.astype(np.int32) if want_label else None
    return out, state.astype(np.uint8), lab, np.bincount(state.ravel(), minlength=4)[:4].astype(np.int32)


def clean(fwd, bwd=None, prm=DEFAULTS, fn=clean_np):
    """[P, C, H, W] -> out [P, C, H, W], state [P, H, W], label [P, H, W], stats [P, 4]"""
    res = [fn(fwd[t], None if bwd is None else bwd[t], prm) for t in range(len(fwd))]
    return tuple(np.stack([r[k] for r in res]) for k in range(4))


def flip(rec, counts, ref=None, rec_out=None, ref_out=None):
    """[P, cap] records read from their target's side, slot i to slot i below the clipped count; the other slots of rec_out
    and ref_out (copies of what the caller pre-filled) stay as they are"""
    P, cap = rec.shape
    out = np.zeros_like(rec) if rec_out is None else rec_out.copy()
    fout = None if ref is None else (np.zeros_like(ref) if ref_out is None else ref_out.copy())
    for t in range(P):
        m = valid(counts[t], cap)
        r = rec[t, :m]
        if rec.dtype == CORR:
            out["src_x"][t, :m], out["src_y"][t, :m], out["tar_x"][t, :m], out["tar_y"][t, :m] = r["tar_x"], r["tar_y"], r["src_x"], r["src_y"]
        else:
            d = r["d"].astype(np.float64)
            with np.errstate(invalid="ignore"):
                ok = np.isfinite(d) & (d == np.trunc(d)) & (np.abs(d) < 2.0 ** 24)
            whole = np.where(ok, d, 0).astype(np.int64)
            x = ((r["x"].astype(np.int64) - whole + 2 ** 31) % 2 ** 32 - 2 ** 31)
            out["x"][t, :m] = np.where(ok, x, -1)
            out["y"][t, :m] = np.where(ok, r["y"], -1)
            out["d"][t, :m] = np.where(ok, -r["d"], np.float32(0))
        if ref is not None:
            f = ref[t, :m]
            fout["dx_q8"][t, :m] = (-f["dx_q8"].astype(np.int64)).astype(np.int16)     # (wraps at -32768)
            fout["dy_q8"][t, :m] = (-f["dy_q8"].astype(np.int64)).astype(np.int16)
            fout["cost"][t, :m], fout["flags"][t, :m] = f["cost"], f["flags"]
    return out, fout


# ---- the fields of the GPU tests -------------------------------------------------------------------------------------

def field_seed(W, H, C):
    return 7000 * W + 10 * H + C


def random_fields(W, H, C, P=3, seed=None):
    """(fwd, bwd) [P, C, H, W]: pair 1 has no value anywhere.  The others: a smooth background that runs through every tile,
    rectangles of other values, 8 % single pixels of far values (INT32_MAX and INT32_MIN + 1 among them), 5 % holes; bwd
    agrees with fwd at most targets, is off by more than any tolerance in use at some, and has holes of its own"""
    rng = np.random.default_rng(field_seed(W, H, C) if seed is None else seed)
    fwd = np.full((P, C, H, W), NONE, np.int64)
    bwd = np.full((P, C, H, W), NONE, np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    for t in range(P):
        if t == 1:
            bwd[t] = rng.integers(-2000, 2000, (C, H, W))
            continue
        base = rng.integers(-3, 4, C) * 256
        F = base[:, None, None] + rng.integers(-60, 61, (C, H, W))
        for _ in range(3):                                  # rectangles: components of their own, some below 64 pixels
            x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
            w, h = int(rng.integers(1, max(W // 3, 2))), int(rng.integers(1, max(H // 3, 2)))
            F[:, y0:y0 + h, x0:x0 + w] = (rng.integers(4, 9, C) * 256 * rng.choice([-1, 1]))[:, None, None] + rng.integers(-60, 61, (C, H, W))[:, y0:y0 + h, x0:x0 + w]
        salt = rng.random((H, W)) < 0.08
        far = rng.integers(-40, 41, (C, H, W)) * 1792 + 77
        F = np.where(salt[None], far, F)
        ext = rng.random((H, W)) < 0.004
        F = np.where(ext[None], rng.choice([IMAX, IMIN1], (C, H, W)), F)
        F[0][F[0] == NONE] = 0
        holes = rng.random((H, W)) < 0.05
        F[:, holes] = NONE
        fwd[t] = F
        r = np.sign(F) * ((np.abs(F) + 128) >> 8)
        qx = xs - r[0] if C == 1 else xs + r[0]
        qy = ys if C == 1 else ys + r[1]
        ok = ~holes & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        e = rng.integers(-256, 257, (C, H, W))
        off = rng.random((H, W)) < 0.1
        e = np.where(off[None], rng.choice([-70000, -257, 257, 5000], (C, H, W)), e)
        G = bwd[t]
        G[:, qy[ok], qx[ok]] = (-F + e)[:, ok]
        G[:, rng.random((H, W)) < 0.05] = NONE
    return np.clip(fwd, NONE, IMAX).astype(np.int32), np.clip(bwd, NONE, IMAX).astype(np.int32)


def spans_three_tiles(label):
    """does some component of label [H, W] have pixels in at least three tiles"""
    H, W = label.shape
    ys, xs = np.nonzero(label >= 0)
    tile = (ys // TILE) * ((W + TILE - 1) // TILE) + xs // TILE
    pairs = np.unique(np.stack([label[ys, xs], tile]), axis=1)
    return len(pairs[0]) > 0 and np.bincount(np.unique(pairs[0], return_inverse=True)[1]).max() >= 3


def spiral(W, H):
    """[H, W] bool: a one-pixel-wide path from (0, 0) inwards with one-pixel gaps between its turns"""
    on = np.zeros((H, W), bool)
    x = y = 0
    on[0, 0] = True
    dirs, k, turns = ((1, 0), (0, 1), (-1, 0), (0, -1)), 0, 0
    while turns < 2:
        dx, dy = dirs[k]
        nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        free = 0 <= nx < W and 0 <= ny < H and not on[ny, nx] and not (0 <= fx < W and 0 <= fy < H and on[fy, fx])
        if free:
            x, y, turns = nx, ny, 0
            on[y, x] = True
        else:
            k, turns = (k + 1) % 4, turns + 1
    return on


def constructed(W=200, H=90, diff=256):
    """name -> (F0 [H, W] int64 with NONE where there is no pixel, number of components expected)"""
    ys, xs = np.mgrid[0:H, 0:W]
    none = np.full((H, W), NONE, np.int64)
    out = {"whole": (np.zeros((H, W), np.int64), 1),
           "checkerboard": (((xs + ys) & 1) * 1000, W * H)}
    snake = (ys % 2 == 0) | ((ys % 4 == 1) & (xs == W - 1)) | ((ys % 4 == 3) & (xs == 0))
    out["serpentine"] = (np.where(snake, 5, none), 1)
    out["spiral"] = (np.where(spiral(W, H), -7, none), 1)
    comb = (xs % 2 == 0) | (ys == H - 1)
    out["comb"] = (np.where(comb, 9, none), 1)
    u = ((xs == 5) | (xs == 70) | (ys == H - 1)) & (xs >= 5) & (xs <= 70)
    out["u"] = (np.where(u, 3, none), 1)
    diag = ((xs < W // 2) & (ys < H // 2)) | ((xs >= W // 2) & (ys >= H // 2))
    out["diagonal"] = (np.where(diag, 0, none), 2)
    out["step"] = (np.where(xs < W // 2, 0, diff + 1), 2)
    out["step at diff"] = (np.where(xs < W // 2, 0, diff), 1)
    return out
