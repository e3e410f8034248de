"""The guided completion's rule (include/gpc_hip.h, gpc_hip_inpaint_*) restated twice: inpaint_plain with Python loops and
Python integers, and inpaint_np with numpy (one shifted copy of the padded planes per window offset, sums in int64).
Neither shares anything with the kernels' method (tiles staged in LDS, a compacted hole list, in-place passes stamped by the
pass plane).  Also the fields and guides the GPU tests run on, by seed."""
import numpy as np

NONE = -2 ** 31
IMAX, IMIN1 = 2 ** 31 - 1, -2 ** 31 + 1
DEFAULTS = (4, 3, 512, 32)         # radius, range_shift, min_weight, passes
SIZES = [(1, 1, 1), (7, 5, 1), (31, 33, 1), (33, 31, 1), (64, 32, 1), (70, 45, 3)]      # W, H, P


def weight(diff, shift):
    return 256 >> min(8, int(diff) >> shift)


def mean(S, Wt):
    """sgn(S) * ((2 |S| + Wt) div (2 Wt)) of Python integers"""
    q = (2 * abs(S) + Wt) // (2 * Wt)
    return -q if S < 0 else q


def inpaint_plain(field, guide, prm=DEFAULTS):
    """one pair: field [C, H, W] int32, guide [H, W] uint8 -> out [C, H, W] int32, pass [H, W] uint8, stats [2] int32"""
    r, shift, minw, passes = prm
    C, H, W = field.shape
    F = [[[int(field[c, y, x]) for x in range(W)] for y in range(H)] for c in range(C)]
    G = [[int(guide[y, x]) for x in range(W)] for y in range(H)]
    pz = [[255 if F[0][y][x] == NONE else 0 for x in range(W)] for y in range(H)]
    for k in range(1, passes + 1):
        new = []
        for y in range(H):
            for x in range(W):
                if pz[y][x] != 255:
                    continue
                Wt, S = 0, [0] * C
                for qy in range(max(y - r, 0), min(y + r, H - 1) + 1):
                    for qx in range(max(x - r, 0), min(x + r, W - 1) + 1):
                        if pz[qy][qx] == 255:
                            continue
                        w = weight(abs(G[y][x] - G[qy][qx]), shift)
                        Wt += w
                        for c in range(C):
                            S[c] += w * F[c][qy][qx]
                if Wt >= minw:
                    new.append((y, x, [mean(s, Wt) for s in S]))
        if not new:
            break                                   # (later passes would see the same state)
        for y, x, v in new:                         # only now: pass k never reads what pass k fills
            pz[y][x] = k
            for c in range(C):
                F[c][y][x] = v[c]
    out = np.array(F, np.int64).reshape(C, H, W)
    pz = np.array(pz, np.uint8).reshape(H, W)
    out[:, pz == 255] = NONE
    return out.astype(np.int32), pz, np.array([((pz > 0) & (pz < 255)).sum(), (pz == 255).sum()], np.int32)


def inpaint_np(field, guide, prm=DEFAULTS):
    """inpaint_plain, vectorised; also over a stack of pairs (field [P, C, H, W], guide [P, H, W]: stats [P, 2])"""
    r, shift, minw, passes = prm
    C, H, W = field.shape[-3:]
    lead = field.shape[:-3]
    F = field.astype(np.int64).reshape((-1, C, H, W))
    P = len(F)
    G = np.pad(guide.astype(np.int64).reshape(P, H, W), ((0, 0), (r, r), (r, r)))
    pz = np.where(F[:, 0] == NONE, 255, 0).astype(np.uint8)
    F = np.where((pz == 255)[:, None], 0, F)
    for k in range(1, passes + 1):
        hole = pz == 255
        if not hole.any():
            break
        V = np.pad(~hole, ((0, 0), (r, r), (r, r)))      # outside the image: no source
        Fp = np.pad(F, ((0, 0), (0, 0), (r, r), (r, r)))
        Wt, S = np.zeros((P, H, W), np.int64), np.zeros((P, C, H, W), np.int64)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                d = np.abs(G[:, r:r + H, r:r + W] - G[:, dy:dy + H, dx:dx + W])
                w = (256 >> np.minimum(8, d >> shift)) * V[:, dy:dy + H, dx:dx + W]
                Wt += w
                S += w[:, None] * Fp[:, :, dy:dy + H, dx:dx + W]
        fill = hole & (Wt >= minw)
        if not fill.any():
            break
        den = np.where(fill, Wt, 1)[:, None]
        q = (2 * np.abs(S) + den) // (2 * den)
        F = np.where(fill[:, None], np.where(S < 0, -q, q), F)
        pz[fill] = k
    F = np.where((pz == 255)[:, None], NONE, F)
    stats = np.stack([((pz > 0) & (pz < 255)).sum((1, 2)), (pz == 255).sum((1, 2))], 1).astype(np.int32)
    return F.astype(np.int32).reshape(lead + (C, H, W)), pz.reshape(lead + (H, W)), stats.reshape(lead + (2,))


def inpaint(field, guide, prm=DEFAULTS):
    """P pairs: field [P, C, H, W], guide [P, H, W] -> out [P, C, H, W], pass [P, H, W], stats [P, 2]"""
    return inpaint_np(field, guide, prm)


def random_fields(W, H, C, P, holes, seed=0):
    """[P, C, H, W] int32: values of a few thousand 1/256 pixel, both signs, a share `holes` of the pixels without a value;
    with C = 2 some holes keep a value in channel 1, which the rule ignores"""
    rng = np.random.default_rng([seed, W, H, C, P, int(holes * 100)])
    f = rng.integers(-6000, 6000, (P, C, H, W)).astype(np.int32)
    hole = rng.random((P, H, W)) < holes
    f[:, 0][hole] = NONE
    if C == 2:
        f[:, 1][hole & (rng.random((P, H, W)) < 0.5)] = NONE
    return f


def guides(kind, W, H, P, seed=0):
    """[P, H, W] uint8: "random", "constant" (77) or "step" (40 left of a slanted edge, 200 right of it)"""
    if kind == "random":
        return np.random.default_rng([seed, W, H, P, 7]).integers(0, 256, (P, H, W)).astype(np.uint8)
    if kind == "constant":
        return np.full((P, H, W), 77, np.uint8)
    ys, xs = np.mgrid[0:H, 0:W]
    return np.broadcast_to(np.where(2 * xs + ys < W, 40, 200).astype(np.uint8), (P, H, W)).copy()
