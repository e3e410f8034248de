"""The scoring rules of include/gpc_hip.h (gpc_score) restated in numpy, for the tests of gpc_hip_score_*.

Everything is an integer count, so the GPU result must EQUAL what these functions give.  The float arithmetic is float32 with
one rounding per operation (numpy's float32 operators do exactly that; nothing here is fused).  Restated from the reference
by citation only: a pixel's truth is usable where the reference's samplers would use it (SintelOpticalFlow.hpp:509-540,
SintelStereo.hpp:416-440: masks read at the SOURCE coordinates), and the true target is rounded with int(round(.)), half
away from zero."""
import os
import struct
import zlib

import numpy as np

MAX_THR = 8
R = 13   # GPC_PATCH_RADIUS: the candidate margin
F32 = np.float32

SCORE_FIELDS = ("n_records", "n_ignored", "n_no_truth", "n_judged", "n_within", "sum_e2_q8", "n_candidates", "n_matchable")


def usable(t):
    """finite and below the .flo "unknown" magnitude 1e9 (float32 compare)"""
    t = np.asarray(t, F32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(t) & (np.abs(t) < F32(1e9))


def thr2(thr):
    t = np.asarray(thr, F32).reshape(-1)
    assert 1 <= len(t) <= MAX_THR and np.isfinite(t).all() and (t >= 0).all()
    return t * t   # float32 product: fl(thr * thr)


def round_half_away(t):
    """roundf for float32 inputs with |t| < 1e9, as int64 (exact in float64: t + 0.5 has no rounding there)"""
    t = np.asarray(t, np.float64)
    return (np.sign(t) * np.floor(np.abs(t) + 0.5)).astype(np.int64)


def e2_support(d, g):
    ex = np.asarray(d, F32) - np.asarray(g, F32)
    return ex * ex


def e2_corr(sx, sy, tx, ty, u, v):
    ex = (np.asarray(tx, np.int32) - np.asarray(sx, np.int32)).astype(F32) - np.asarray(u, F32)
    ey = (np.asarray(ty, np.int32) - np.asarray(sy, np.int32)).astype(F32) - np.asarray(v, F32)
    xx = ex * ex
    yy = ey * ey
    return xx + yy


def q8(e2):
    e2 = np.asarray(e2, F32)
    m = np.where(np.isnan(e2), F32(1048576.0), np.minimum(e2, F32(1048576.0))).astype(F32)   # fminf: NaN gives the clamp
    s = m * F32(256.0)
    return (s + F32(0.5)).astype(np.int64)


def empty_score():
    return {"n_records": 0, "n_ignored": 0, "n_no_truth": 0, "n_judged": 0, "n_within": [0] * MAX_THR, "sum_e2_q8": 0,
            "n_candidates": 0, "n_matchable": 0}


def score_records(rec, count, cap, u, v, ignore, thr):
    """One pair.  rec: structured records (x, y, d) or (src_x / sx, src_y / sy, tar_x / tx, tar_y / ty), at least
    min(count, cap) of them; u, v, ignore: [H, W] planes (v None: supports; ignore may be None)."""
    s = empty_score()
    n = min(max(int(count), 0), int(cap))
    rec = rec[:n]
    s["n_records"] = n
    H, W = u.shape
    names = rec.dtype.names
    corr = "d" not in names
    if corr:
        f = (("src_x", "src_y", "tar_x", "tar_y") if "src_x" in names else ("sx", "sy", "tx", "ty"))
        sx, sy, tx, ty = (rec[k].astype(np.int32) for k in f)
    else:
        sx, sy = rec["x"].astype(np.int32), rec["y"].astype(np.int32)
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    cx, cy = np.where(inside, sx, 0), np.where(inside, sy, 0)
    ign = inside & (ignore[cy, cx] != 0) if ignore is not None else np.zeros(n, bool)
    ok = inside & ~ign & usable(u[cy, cx])
    if corr:
        ok &= usable(v[cy, cx])
    s["n_ignored"] = int(ign.sum())
    s["n_judged"] = int(ok.sum())
    s["n_no_truth"] = n - s["n_ignored"] - s["n_judged"]
    with np.errstate(all="ignore"):
        if corr:
            e2 = e2_corr(sx[ok], sy[ok], tx[ok], ty[ok], u[cy, cx][ok], v[cy, cx][ok])
        else:
            e2 = e2_support(rec["d"][ok], u[cy, cx][ok])
        for k, t2 in enumerate(thr2(thr)):
            s["n_within"][k] = int((e2 <= t2).sum())
        s["sum_e2_q8"] = int(q8(e2).sum())
    return s


def matchable(candL, candR, u, v, ignore):
    """(n_candidates, n_matchable) of one pair.  candL / candR: [H, W] bool candidate images (gradient set, inside the
    margin); v None: stereo (target (x - R(g), y)), else flow (target (x + R(u), y + R(v)))."""
    H, W = candL.shape
    ys, xs = np.nonzero(candL)
    ok = usable(u[ys, xs])
    if v is not None:
        ok &= usable(v[ys, xs])
    if ignore is not None:
        ok &= ignore[ys, xs] == 0
    ys, xs = ys[ok], xs[ok]
    if v is None:
        tx, ty = xs - round_half_away(u[ys, xs]), ys.astype(np.int64)
    else:
        tx, ty = xs + round_half_away(u[ys, xs]), ys + round_half_away(v[ys, xs])
    inm = (tx >= R) & (tx < W - R) & (ty >= R) & (ty < H - R)
    return int(candL.sum()), int(candR[ty[inm], tx[inm]].sum())


def cand_image(mask, W, H):
    """the candidate index list of preprocessImage (oracle / gpc_hip_preprocess) as an [H, W] bool image"""
    c = np.zeros(W * H, bool)
    c[np.asarray(mask, np.int64)] = True
    return c.reshape(H, W)


def as_dict(score_row):
    """one SCORE_DTYPE record -> the dict form used here"""
    d = {k: int(score_row[k]) for k in SCORE_FIELDS if k != "n_within"}
    d["n_within"] = [int(x) for x in score_row["n_within"]]
    return d


def fma_sensitive_corr(seed=0, want=8, thr=F32(3.0)):
    """float32 (ex, ey) pairs for which the two-rounding e2 = fl(fl(ex*ex) + fl(ey*ey)) and a contracted
    fma(ex, ex, fl(ey*ey)) fall on different sides of thr^2 (the fma computed exactly in float64, rounded once)."""
    rng = np.random.default_rng(seed)
    t2 = F32(thr) * F32(thr)
    out = []
    while len(out) < want:
        ang = rng.random(200000) * (np.pi / 2)
        ex = (np.cos(ang) * float(thr)).astype(F32)
        ey = (np.sin(ang) * float(thr)).astype(F32)
        two = ex * ex + ey * ey
        yy = (ey * ey).astype(np.float64)
        fused = (ex.astype(np.float64) * ex.astype(np.float64) + yy).astype(F32)   # (float64 holds the product exactly)
        hit = np.nonzero((two <= t2) != (fused <= t2))[0]
        out.extend((float(ex[i]), float(ey[i])) for i in hit)
    return np.array(out[:want], F32), float(thr)


# --------------------------------------------------------------------------- files of a synthetic Sintel tree
def write_png(path, a):
    a = np.ascontiguousarray(a, np.uint8)
    h, w = a.shape[:2]
    ctype = 2 if a.ndim == 3 else 0
    raw = b"".join(b"\x00" + a[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 1)) + chunk(b"IEND", b""))


def write_flo(path, u, v):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    h, w = u.shape
    with open(path, "wb") as f:
        f.write(np.array([202021.25], "<f4").tobytes() + np.array([w, h], "<i4").tobytes() +
                np.stack([u, v], -1).astype("<f4").tobytes())
