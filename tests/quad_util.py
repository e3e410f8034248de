"""Quads over a stereo sequence (gpc_hip_quads_*), restated plainly: the rule of include/gpc_hip.h with dicts and loops, for
the tests to hold the GPU result equal to.  Nothing here is clever and nothing here is fast."""
import math

import numpy as np

SUP = np.dtype([("x", "<i4"), ("y", "<i4"), ("d", "<f4")])
CORR = np.dtype([("src_x", "<i4"), ("src_y", "<i4"), ("tar_x", "<i4"), ("tar_y", "<i4")])
QUAD = np.dtype([("x", "<i4"), ("y", "<i4"), ("d0", "<i4"), ("u", "<i4"), ("v", "<i4"), ("d1", "<i4"), ("support0", "<i4"),
                 ("support1", "<i4")])


def sup_array(frames, cap=None):
    """[[(x, y, d), ...] per frame] -> (records [N, cap] of SUP, counts [N]); unused slots hold (-9, -9, -9.0)"""
    cap = cap or max(1, max(len(f) for f in frames))
    rec = np.zeros((len(frames), cap), SUP)
    rec["x"], rec["y"], rec["d"] = -9, -9, -9.0
    for t, f in enumerate(frames):
        for i, (x, y, d) in enumerate(f[:cap]):
            rec[t, i] = (x, y, d)
    return rec, np.array([len(f) for f in frames], np.int32)


def corr_array(steps, cap=None):
    """[[(sx, sy, tx, ty), ...] per step] -> (records [P, cap] of CORR, counts [P]); unused slots hold -9"""
    cap = cap or max(1, max(len(p) for p in steps))
    rec = np.full((len(steps), cap, 4), -9, np.int32)
    for t, p in enumerate(steps):
        for i, r in enumerate(p[:cap]):
            rec[t, i] = r
    return rec.view(CORR).reshape(len(steps), cap), np.array([len(p) for p in steps], np.int32)


def support_takes_part(x, y, d, W, H):
    """-> the integer disparity, or None"""
    if not (0 <= x < W and 0 <= y < H):
        return None
    d = float(d)
    if math.isnan(d) or math.isinf(d) or d != math.floor(d) or abs(d) > 16384:
        return None
    d = int(d)
    return d if 0 <= x - d < W else None


def restate(sup, nsup, fl, nfl, fr, nfr, W, H, tol, stats=None):
    """-> per step the list of quads (x, y, d0, u, v, d1, support0, support1), by support0 ascending.  stats (a dict):
    receives "contended" (the i' that more than one start closes on) and "shared" (supports that take part and are no
    start, because a lower one has their left pixel), summed over the steps"""
    N, cap_s = sup.shape
    P, cap_f = fl.shape
    assert P == N - 1 and fr.shape == fl.shape

    def clip(c, cap):
        return min(max(int(c), 0), cap)

    first_s, disp = [], []
    for t in range(N):
        lowest, dd = {}, {}
        for i in range(clip(nsup[t], cap_s)):
            x, y = int(sup["x"][t, i]), int(sup["y"][t, i])
            d = support_takes_part(x, y, sup["d"][t, i], W, H)
            if d is None:
                continue
            dd[i] = d
            if y * W + x not in lowest:
                lowest[y * W + x] = i
        first_s.append(lowest)
        disp.append(dd)

    def first_flow(rec, counts, t):
        lowest = {}
        for j in range(clip(counts[t], cap_f)):
            sx, sy, tx, ty = (int(rec[f][t, j]) for f in ("src_x", "src_y", "tar_x", "tar_y"))
            if 0 <= sx < W and 0 <= sy < H and 0 <= tx < W and 0 <= ty < H and sy * W + sx not in lowest:
                lowest[sy * W + sx] = j
        return lowest

    out = []
    for t in range(P):
        ffl, ffr = first_flow(fl, nfl, t), first_flow(fr, nfr, t)
        closing, winner, closers, shared = {}, {}, {}, 0
        for i in range(clip(nsup[t], cap_s)):
            if i not in disp[t]:
                continue
            x, y, d = int(sup["x"][t, i]), int(sup["y"][t, i]), disp[t][i]
            a, b = y * W + x, y * W + x - d
            if first_s[t][a] != i:
                shared += 1
                continue
            if a not in ffl or b not in ffr:
                continue
            j, k = ffl[a], ffr[b]
            ax, ay = int(fl["tar_x"][t, j]), int(fl["tar_y"][t, j])
            bx, by = int(fr["tar_x"][t, k]), int(fr["tar_y"][t, k])
            if ay * W + ax not in first_s[t + 1]:
                continue
            i1 = first_s[t + 1][ay * W + ax]
            d1 = disp[t + 1][i1]
            if abs(ax - d1 - bx) > tol or abs(ay - by) > tol:
                continue
            closing[i] = (x, y, d, ax - x, ay - y, d1, i, i1)
            closers[i1] = closers.get(i1, 0) + 1
            if i1 not in winner:
                winner[i1] = i
        if stats is not None:
            stats["contended"] = stats.get("contended", 0) + sum(1 for v in closers.values() if v > 1)
            stats["shared"] = stats.get("shared", 0) + shared
        out.append([q for i, q in sorted(closing.items()) if winner[q[7]] == i])
    return out


def expected_arrays(sup, nsup, fl, nfl, fr, nfr, W, H, tol, fill, quad_cap):
    """the restatement as the arrays a call leaves in outputs that held `fill` everywhere: (quads [P, max(quad_cap, 1)] of
    QUAD, nquads [P])"""
    quads = restate(sup, nsup, fl, nfl, fr, nfr, W, H, tol)
    P = len(quads)
    tab = np.full((P, max(quad_cap, 1), 8), fill, np.int32)
    for t, qs in enumerate(quads):
        for k, q in enumerate(qs[:quad_cap]):
            tab[t, k] = q
    return tab.view(QUAD).reshape(P, max(quad_cap, 1)), np.array([len(q) for q in quads], np.int32)


def fnv_quads(quads, nquads, quad_cap):
    """FNV-1a 64 over the int32 (step, number of quads written, then their eight words each) of every step, in order"""
    h = 1469598103934665603
    for t in range(len(nquads)):
        m = min(max(int(nquads[t]), 0), quad_cap)
        words = np.concatenate([np.array([t, m], "<i4"), np.ascontiguousarray(quads[t, :m]).view("<i4").reshape(-1)])
        for b in words.astype("<i4").tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def stereo_frames_of(W, H, N, seed, D, dy=12):
    """(left, right) [N, H, W] each: the texture and the walk of track_util.frames_of, widened by D; L_t is the crop at
    (x, y), R_t the crop at (x + D, y), so that the true disparity is D everywhere; x starts at 16 + D"""
    rng = np.random.default_rng(seed)
    BW, BH = W + 8 * N + 32 + 2 * D, H + 40
    noise = rng.integers(0, 64, (BH, BW))
    base = (rng.integers(0, 256, (BH // 4 + 1, BW // 4 + 1)).repeat(4, 0).repeat(4, 1)[:BH, :BW] * 3 // 4 + noise).astype(np.uint8)
    left, right = [], []
    x, y = 16 + D, 20
    for t in range(N):
        left.append(base[y:y + H, x:x + W])
        right.append(base[y:y + H, x + D:x + D + W])
        x += int(rng.integers(1, 8))
        y = 20 + int(rng.integers(-dy, dy + 1))
    return np.ascontiguousarray(np.stack(left)), np.ascontiguousarray(np.stack(right))
