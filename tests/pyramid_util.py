"""The pyramid matcher's two new steps (gpc_hip_pyramid_*) restated in numpy -- the 2x2-mean downsampling and the mapping
plus merge of the levels' records -- and the expected records of a call: the CPU oracle run per level, merged here.
Integers only, as include/gpc_hip.h states the rules."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORT = np.dtype([("x", np.int32), ("y", np.int32), ("d", np.float32)])
CORR = np.dtype([("src_x", np.int32), ("src_y", np.int32), ("tar_x", np.int32), ("tar_y", np.int32)])
MAX_LEVELS = 4
FORESTS = {"zero": os.path.join(ROOT, "forests", "defaultZeroForest.txt"),
           "tau": os.path.join(ROOT, "forests", "defaultTauForest.txt")}


def image_ok(W, H):
    """what the library takes as an image today"""
    return W > 0 and H > 0 and W % 16 == 0 and W >= 42 and H >= 30 and W <= 16384 and W * H <= 1 << 30


def level_sizes(W, H, levels):
    """[(W_l, H_l)] or None where the geometry is refused: W_l = W >> l, H_l = H_{l-1} // 2, every level an image"""
    if not 1 <= levels <= MAX_LEVELS:
        return None
    out = []
    for l in range(levels):
        if l:
            if W & 1:
                return None
            W, H = W >> 1, H // 2
        if not image_ok(W, H):
            return None
        out.append((W, H))
    return out


def down(img):
    """one step: out[y][x] = (a + b + c + d + 2) >> 2 over in[2y .. 2y+1][2x .. 2x+1]; [..., H, W] uint8, an odd last row dropped"""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.shape[-1] % 2 == 0
    H2 = a.shape[-2] // 2
    v = a[..., :2 * H2, :].astype(np.uint16)
    s = v[..., 0::2, 0::2] + v[..., 0::2, 1::2] + v[..., 1::2, 0::2] + v[..., 1::2, 1::2] + 2
    return (s >> 2).astype(np.uint8)


def pyramid(img, levels):
    out = [np.ascontiguousarray(img)]
    for _ in range(levels - 1):
        out.append(np.ascontiguousarray(down(out[-1])))
    return out


def source(rec):
    return (rec["src_x"], rec["src_y"]) if rec.dtype == CORR else (rec["x"], rec["y"])


def map_records(rec, l):
    """level-l records in level 0's coordinates"""
    out = rec.copy()
    if rec.dtype == CORR:
        for f in CORR.names:
            out[f] = rec[f] << l
    else:
        out["x"], out["y"] = rec["x"] << l, rec["y"] << l
        out["d"] = rec["d"] * np.float32(1 << l)
    return out


def block_hit(occ, x, y, l):
    """does the block [x << l, (x << l) + 2^l) x [y << l, (y << l) + 2^l) of the [H, W] plane hold a set pixel?"""
    n = 1 << l
    return bool(occ[y << l:(y << l) + n, x << l:(x << l) + n].any())


def merge(levels_rec, W, H):
    """levels_rec[l]: the unmapped records of level l in the matcher's order -> (merged records, kept count per level).
    Level 0 whole; then level l's mapped records whose block holds the source pixel of no record kept from levels < l.  A
    record whose source lies outside level l's image has no block: kept, marks nothing."""
    occ = np.zeros((H, W), bool)
    out, kept = [], []
    for l, rec in enumerate(levels_rec):
        Wl, Hl = W >> l, H >> l
        x, y = source(rec)
        inside = (x >= 0) & (x < Wl) & (y >= 0) & (y < Hl)
        keep = np.ones(len(rec), bool)
        if l:
            n = 1 << l
            blocks = occ[:Hl << l, :Wl << l].reshape(Hl, n, Wl, n).any(axis=(1, 3))
            keep[inside] = ~blocks[y[inside], x[inside]]
        m = map_records(rec[keep], l)
        mx, my = source(m)
        ins = inside[keep]
        occ[my[ins], mx[ins]] = True          # (after every record of the level has been tested)
        out.append(m)
        kept.append(int(keep.sum()))
    return (np.concatenate(out) if out else np.zeros(0, SUPPORT)), kept


def oracle_settings(thr, disp_high, vtol, epipolar, hashtable, naive, l=0):
    from oracle.pyoracle import sparsematch_settings
    return sparsematch_settings(thr, disp_high >> l, vtol >> l, epipolar, hashtable, naive)


_oracle = None


def the_oracle():
    global _oracle
    if _oracle is None:
        from oracle.pyoracle import Oracle
        _oracle = Oracle()
    return _oracle


_pairs = {}


def remember(L, R):
    """a key for expected_supports: the images are kept so that a result is computed once per test session"""
    key = (L.shape, hash(L.tobytes()), hash(R.tobytes()))
    _pairs[key] = (L, R)
    return key


@functools.lru_cache(maxsize=None)
def level_supports(key, forest, levels, thr, disp_high, vtol, epipolar, hashtable, naive):
    """per level: (records, candidates left, candidates right) of the oracle's match_pair on the level's images"""
    o = the_oracle()
    L, R = _pairs[key]
    out = []
    for l, (a, b) in enumerate(zip(pyramid(L, levels), pyramid(R, levels))):
        H, W = a.shape
        rc, f = o.read_forest(FORESTS[forest], W, H)
        assert rc == 0
        out.append(o.match_pair(a, b, f, oracle_settings(thr, disp_high, vtol, epipolar, hashtable, naive, l)))
    return out


def expected_supports(L, R, forest, levels, settings=(5, 128, 0, True, False), naive=False):
    """-> (merged supports, kept per level, per-level unmerged counts, candidates [levels][2])"""
    per = level_supports(remember(L, R), forest, levels, *settings, naive)
    H, W = L.shape
    merged, kept = merge([p[0].astype(SUPPORT) for p in per], W, H)
    return merged, kept, [len(p[0]) for p in per], [[p[1], p[2]] for p in per]


def enlarged_pair(W=256, H=128, D=8):
    """synth_pair(W, H, 0, D) with the right half of both images replaced by the 4x nearest-neighbour enlargement of
    synth_pair(W / 4, H / 4, 0, D / 4): texture that only level 2 resolves"""
    o = the_oracle()
    L, R = o.synth_pair(W, H, 0, D)
    l, r = o.synth_pair(W // 4, H // 4, 0, D // 4)
    L, R = L.copy(), R.copy()
    L[:, W // 2:] = l.repeat(4, 0).repeat(4, 1)[:, W // 2:]
    R[:, W // 2:] = r.repeat(4, 0).repeat(4, 1)[:, W // 2:]
    return L, R
