"""Grid motion consensus (gpc_hip_consensus_*), restated plainly from the rule in include/gpc_hip.h for the tests to hold the
GPU result equal to: `restate` with numpy (fast enough for real record lists), `brute` with loops over all pairs of records
(small inputs only).  Neither shares anything with the kernels' method (no sort, no table)."""
import numpy as np

CORR = np.dtype([("src_x", "<i4"), ("src_y", "<i4"), ("tar_x", "<i4"), ("tar_y", "<i4")])
SUPPORT = np.dtype([("x", "<i4"), ("y", "<i4"), ("d", "<f4")])


class Params:
    def __init__(self, cell=16, shifts=4, alpha_num=6, alpha_den=1):
        self.cell, self.shifts, self.alpha_num, self.alpha_den = cell, shifts, alpha_num, alpha_den


def m_of(counts, cap):
    return [min(max(int(c), 0), cap) for c in counts]


def ends(r, W, H):
    """(participates [m] bool, sx, sy, tx, ty as int64) of a 1-D record array of either type"""
    if r.dtype == CORR:
        sx, sy, tx, ty = (r[f].astype(np.int64) for f in ("src_x", "src_y", "tar_x", "tar_y"))
        ok = np.ones(len(r), bool)
    else:
        sx, sy = r["x"].astype(np.int64), r["y"].astype(np.int64)
        d = r["d"].astype(np.float64)
        ok = np.isfinite(d)
        di = np.where(ok, d, 0.0)
        ok &= (di == np.trunc(di)) & (np.abs(di) < 2.0 ** 24)
        di = np.where(ok, di, 0.0).astype(np.int64)
        tx, ty = sx - di, sy
    ok = ok & (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H) & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    return ok, sx, sy, tx, ty


def grid_of(W, H, c, s):
    ox, oy = ((0, 0), (c // 2, 0), (0, c // 2), (c // 2, c // 2))[s]
    return ox, oy, (W - 1 + ox) // c + 1, (H - 1 + oy) // c + 1


def passes(S, T, k, prm):
    """the test, in Python integers (exact)"""
    return S * S * k * prm.alpha_den * prm.alpha_den > prm.alpha_num * prm.alpha_num * T


def keep_of_pair(r, W, H, prm):
    """keep mask [m] uint8 of one pair's records (1-D array of the m records that are read)"""
    ok, sx, sy, tx, ty = ends(r, W, H)
    keep = np.zeros(len(r), np.uint8)
    idx = np.nonzero(ok)[0]
    if not len(idx):
        return keep
    sx, sy, tx, ty = sx[idx], sy[idx], tx[idx], ty[idx]
    c = prm.cell
    for s in range(prm.shifts):
        ox, oy, gx, gy = grid_of(W, H, c, s)
        ax, ay = (sx + ox) // c, (sy + oy) // c
        dx, dy = (tx + ox) // c - ax, (ty + oy) // c - ay
        K = (2 * gx + 1) * (2 * gy + 1)
        cls = (dy + gy) * (2 * gx + 1) + (dx + gx)            # one number per class
        hist = np.zeros((gy + 2, gx + 2), np.int64)           # a border of empty cells
        np.add.at(hist, (ay + 1, ax + 1), 1)
        T = np.zeros(len(idx), np.int64)
        S = np.zeros(len(idx), np.int64)
        k = np.zeros(len(idx), np.int64)
        pairs, cnt = np.unique((ay * gx + ax) * K + cls, return_counts=True)   # (cell, class) -> records
        for ey in (-1, 0, 1):
            for ex in (-1, 0, 1):
                nx, ny = ax + ex, ay + ey
                inside = (nx >= 0) & (nx < gx) & (ny >= 0) & (ny < gy)
                k += inside
                T += hist[ny + 1, nx + 1]
                want = np.where(inside, (ny * gx + nx) * K + cls, -1)
                at = np.minimum(np.searchsorted(pairs, want), len(pairs) - 1)
                S += np.where(pairs[at] == want, cnt[at], 0)
        ad2, an2 = np.uint64(prm.alpha_den ** 2), np.uint64(prm.alpha_num ** 2)
        good = S.astype(np.uint64) * S.astype(np.uint64) * k.astype(np.uint64) * ad2 > an2 * T.astype(np.uint64)
        keep[idx[good]] |= np.uint8(1 << s)
    return keep


def brute_counts(r, W, H, prm, s):
    """(participates, S, T, k) lists of one pair's records under grid s, by comparing every record with every other"""
    ok, sx, sy, tx, ty = (a.tolist() for a in ends(r, W, H))
    c = prm.cell
    ox, oy, gx, gy = grid_of(W, H, c, s)
    m = len(r)
    A = [((sx[i] + ox) // c, (sy[i] + oy) // c) for i in range(m)]
    D = [((tx[i] + ox) // c - A[i][0], (ty[i] + oy) // c - A[i][1]) for i in range(m)]
    S, T, k = [0] * m, [0] * m, [0] * m
    for i in range(m):
        if not ok[i]:
            continue
        k[i] = sum(1 for x in range(gx) for y in range(gy) if max(abs(x - A[i][0]), abs(y - A[i][1])) <= 1)
        for j in range(m):
            if ok[j] and max(abs(A[j][0] - A[i][0]), abs(A[j][1] - A[i][1])) <= 1:
                T[i] += 1
                S[i] += D[j] == D[i]
    return ok, S, T, k


def brute_keep(r, W, H, prm):
    keep = np.zeros(len(r), np.uint8)
    for s in range(prm.shifts):
        ok, S, T, k = brute_counts(r, W, H, prm, s)
        for i in range(len(r)):
            if ok[i] and passes(S[i], T[i], k[i], prm):
                keep[i] |= 1 << s
    return keep


def restate(rec, counts, W, H, prm):
    """-> keep masks: one uint8 array of m_t entries per pair"""
    P, cap = rec.shape
    return [keep_of_pair(rec[t, :m], W, H, prm) for t, m in enumerate(m_of(counts, cap))]


def expected_arrays(rec, counts, W, H, prm, cap_out, fill):
    """the restatement as the arrays a call leaves in outputs whose every BYTE held `fill`: (keep [P, cap] uint8, out
    [P, cap_out] records, index [P, cap_out] int32, out_counts [P] int32)"""
    P, cap = rec.shape
    keep = np.full((P, cap), fill, np.uint8)
    out = np.full((P, cap_out, rec.dtype.itemsize), fill, np.uint8).view(rec.dtype).reshape(P, cap_out)
    index = np.full((P, cap_out, 4), fill, np.uint8).view(np.int32).reshape(P, cap_out)
    n_out = np.zeros(P, np.int32)
    for t, k in enumerate(restate(rec, counts, W, H, prm)):
        keep[t, :len(k)] = k
        kept = np.nonzero(k)[0]
        n_out[t] = len(kept)
        w = min(len(kept), cap_out)
        out[t, :w] = rec[t, kept[:w]]
        index[t, :w] = kept[:w]
    return keep, out, index, n_out


def kept_list(rec, counts, W, H, prm):
    """(records [P, cap] with each pair's kept records first, in order; counts [P]): what a filter call with cap_out = cap
    hands on, unused slots zero"""
    P, cap = rec.shape
    out = np.zeros((P, cap), rec.dtype)
    n = np.zeros(P, np.int32)
    for t, k in enumerate(restate(rec, counts, W, H, prm)):
        kept = np.nonzero(k)[0]
        out[t, :len(kept)] = rec[t, kept]
        n[t] = len(kept)
    return out, n
