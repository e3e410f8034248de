"""Shared by the tests that hold the oracle, the recorded vectors and the GPU library to the reference's own classes
(oracle/_ref/libgpc_ref_full*.so through oracle.pyoracle.RefFull): the case list, the oracle's three levels, and the one
exemption from record-for-record equality, the Q2 tie.

The Q2 tie.  Forest::findCorrespondences sorts both descriptor sets with std::sort and, when its search lands on the
second last target (j == nt - 2), skips the target-uniqueness test.  If the last two sorted targets carry the same
state, which of the two sits at nt - 2 is up to the standard library's sort; the oracle (and the GPU) take the first in
mask order.  `alternatives()` derives, from the reference's own sorted target array and from nothing else, every result
the reference could have produced; `which()` says which of them a result equals.
"""
import os

import numpy as np

from oracle.pyoracle import CORR_DTYPE, SUPPORT_DTYPE, sparsematch_settings
from test_gpu_fuzz import draw_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORESTS = {name: os.path.join(ROOT, "forests", fn) for name, fn in
           (("zero", "defaultZeroForest.txt"), ("tau", "defaultTauForest.txt"), ("stress", "stress16x20Forest.txt"))}
VECTORS = os.path.join(ROOT, "tests", "golden", "ref_full_vectors.json")

FUZZ_SEEDS = 400          # the CPU sweep; the recorded file and the GPU module take the first of them
TIE_CAP = 0.02            # share of the sweep's calls that may use the tie rule
UNDEFINED_CAP = 0.05      # share of the sweep's calls that may be left out as undefined in the reference
MODES = [(True, False), (False, False), (True, True), (False, True)]   # (epipolar, hashtable)


def fuzz_case(seed):
    """The draws of test_gpu_fuzz.test_random_configuration, widths held to 48..944.
    Returns (L, R, forest name, settings)."""
    rng = np.random.default_rng(1000 + seed)
    W = 16 * int(rng.integers(3, 60))
    H = int(rng.integers(30, 150))
    forest = "tau" if seed % 2 else "zero"
    epipolar, hashtable = bool((seed >> 1) & 1), bool((seed >> 2) & 1)
    naive = (seed % 9) == 4
    thr = int(rng.choice([0, 3, 5, 10, 40, 181, 182, 255]))
    disp_high = int(rng.choice([0, 7, 64, 128, 4000]))
    vtol = int(rng.choice([-1, 0, 1, 3]))
    L, R = draw_pair(rng, W, H)
    return L, R, forest, sparsematch_settings(thr, disp_high, vtol, epipolar, hashtable, naive)


def synthetic_case(W, H, seed):
    """A translated blocky pair with a little noise in the right image (duplicates, misses, far disparities)."""
    rng = np.random.default_rng(seed)
    base = (rng.integers(0, 256, (H // 4 + 1, (W + 64) // 4 + 1)).repeat(4, 0).repeat(4, 1)[:H, :W + 64] * 3 // 4
            + rng.integers(0, 64, (H, W + 64))).astype(np.uint8)
    d = int(rng.integers(0, 40))
    L = np.ascontiguousarray(base[:, 32:32 + W])
    R = np.ascontiguousarray(base[:, 32 + d - 20:32 + d - 20 + W])
    R = np.where(rng.random(R.shape) < 0.02, rng.integers(0, 256, R.shape), R).astype(np.uint8)
    return L, R


def striped_case():
    """Few distinct codes: hash buckets overflow their 10-entry cap and the pair / triplet rules decide."""
    W, H = 256, 64
    img = np.tile((np.arange(W) // 3 * 37 % 256).astype(np.uint8), (H, 1))
    return img, np.roll(img, 5, axis=1)


def tail_rows(oracle, nl, nr, seed=40):
    """The constructed rows of test_gpu_parity.test_tail_quirks_epipolar: row H-14 (code 0, the largest epipolar
    states) carries nl source and nr target candidates, so the last sorted targets decide quirks Q1 / Q2."""
    W, H = 96, 64
    rng = np.random.default_rng(seed)
    base = (rng.integers(0, 256, (H // 4 + 1, W // 4 + 1)).repeat(4, 0).repeat(4, 1)[:H, :W] * 3 // 4
            + rng.integers(0, 64, (H, W))).astype(np.uint8)
    smooth, grad, _ = oracle.preprocess(base, 5)
    y = H - 14
    gl, gr = grad.copy(), grad.copy()
    gl[y, :] = 0
    gr[y, :] = 0
    gl[y, 20:20 + nl] = 255
    gr[y, 30:30 + nr] = 255

    def keep(g):
        m = np.flatnonzero(g.reshape(-1)).astype(np.int32)
        return m[(m % W >= 13) & (m % W < W - 13) & (m // W >= 13) & (m // W < H - 13)]
    return (smooth, gl, keep(gl)), (smooth, gr, keep(gr))


TAIL_ROWS = [(1, 1), (1, 2), (1, 3), (2, 2), (0, 2), (1, 0)]


# ---- the oracle, level by level
class Levels:
    def __init__(self, mask_l, mask_r, states_l, states_r, corr, supp):
        self.mask_l, self.mask_r = mask_l, mask_r
        self.states_l, self.states_r = states_l, states_r
        self.corr, self.supp = corr, supp


def oracle_levels_pre(oracle, pl, pr, f, st):
    """descriptors (codes at the candidates, as evalFastMaskOnSubsetSSE returns them), unfiltered correspondences
    and supports from two (smooth, grad, mask) triples."""
    W = pl[0].shape[1]
    raw, keyed = [], []
    for smooth, grad, mask in (pl, pr):
        codes = oracle.hash_naive(smooth, mask, f) if st.naive else oracle.hash(smooth, grad, f)
        raw.append(codes.reshape(-1)[mask].astype(np.uint64))
        keyed.append(oracle.descriptors(codes, mask, W, st.epipolar_mode))
    match = oracle.hash_correspondences if st.use_hashtable else oracle.find_correspondences
    corr = match(keyed[0], pl[2], keyed[1], pr[2], W)
    return Levels(pl[2], pr[2], raw[0], raw[1], corr, oracle.rectified_filter(corr, st))


def oracle_levels(oracle, L, R, f, st):
    pre = oracle.preprocess_naive if st.naive else oracle.preprocess
    lv = oracle_levels_pre(oracle, pre(L, st.gradient_threshold), pre(R, st.gradient_threshold), f, st)
    whole, nl, nr = oracle.match_pair(L, R, f, st)   # the entry point the GPU tests compare with
    assert (nl, nr) == (len(lv.mask_l), len(lv.mask_r)) and np.array_equal(whole, lv.supp)
    return lv


# ---- the reference's filter (inference.hpp:384-391), for the alternatives of a tie
def np_filter(corr, st):
    keep = (np.abs(corr["sy"] - corr["ty"]) <= st.vertical_tolerance) & \
           (np.abs(corr["sx"] - corr["tx"]) <= st.disp_high)
    c = corr[keep]
    out = np.zeros(len(c), SUPPORT_DTYPE)
    out["x"], out["y"], out["d"] = c["sx"], c["sy"], (c["sx"] - c["tx"]).astype(np.float32)
    return out


def alternatives(m, st):
    """[(corr, supp)]: entry 0 is what the reference returned.  More entries exist only where every clause of the tie
    rule holds, each read off the reference's own output: sort matcher; the reference's last record (correspondences
    come out in ascending source state, so the last one belongs to the largest matched state) has as its target the
    descriptor at nt - 2 of the reference's sorted target array; the states at nt - 2 and nt - 1 are equal.  The
    entries differ in the target point of that one record only: one per target carrying that state."""
    alts = [(m.corr, m.supp)]
    ts, txy = m.sorted_t_state, m.sorted_t_xy
    nt = len(ts)
    if st.use_hashtable or nt < 2 or len(m.corr) == 0 or ts[nt - 2] != ts[nt - 1]:
        return alts
    last = m.corr[-1]
    if (int(last["tx"]), int(last["ty"])) != (int(txy[nt - 2][0]), int(txy[nt - 2][1])):
        return alts
    assert np.array_equal(np_filter(m.corr, st), m.supp)
    for k in np.flatnonzero(ts == ts[nt - 1]):
        if k == nt - 2:
            continue
        c = m.corr.copy()
        c["tx"][-1], c["ty"][-1] = txy[k]
        alts.append((c, np_filter(c, st)))
    return alts


def which(alts, corr=None, supp=None):
    """Index of the alternative that `corr` and / or `supp` equal (0: the reference itself); -1 if none.  The source
    point of every record, and every record but the last, are the same in all alternatives, so a result that differs
    anywhere else matches none."""
    for i, (c, s) in enumerate(alts):
        if corr is not None and not (len(corr) == len(c) and np.array_equal(corr, c.astype(corr.dtype))):
            continue
        if supp is not None and not (len(supp) == len(s) and np.array_equal(supp, s.astype(supp.dtype))):
            continue
        return i
    return -1


def as_corr(sx, sy, tx, ty):
    c = np.zeros(len(sx), CORR_DTYPE)
    c["sx"], c["sy"], c["tx"], c["ty"] = sx, sy, tx, ty
    return c


# ---- constructed ties (state level): the largest state twice among the targets, once among the sources
def tie_states(seed, W=1024):
    """(ss, sk, ts, tk, (k_a, k_b)): 40 sources and 41 targets; the two targets at k_a < k_b share the largest state
    with one source.  Linear indices: the tied source sits at (100, 50), the targets at (90, 50) and (60, 50)."""
    rng = np.random.default_rng(seed)
    ss = rng.permutation(1000)[:40].astype(np.uint64) * 3 + 1
    ts = np.concatenate([rng.choice(ss, 20), rng.permutation(1000)[:19].astype(np.uint64) * 3 + 2])
    top = np.uint64(1 << 40)
    ss[7] = top
    sk = (rng.permutation(3000)[:40] + 200 * W).astype(np.int32)
    tk = (rng.permutation(3000)[:41] + 300 * W).astype(np.int32)
    sk[7] = 50 * W + 100
    ts = np.concatenate([ts, [top, top]])
    k_a, k_b = 50 * W + 60, 50 * W + 90
    tk[39], tk[40] = k_a, k_b
    # mask order is ascending linear index: the oracle is handed its candidates that way
    o = np.argsort(tk, kind="stable")
    return ss, sk, ts[o], tk[o], (k_a, k_b)


class StateMatch:
    """A findCorrespondences call on bare states, shaped like RefMatch for alternatives()."""

    def __init__(self, pairs, sorted_ts, sorted_tk, W, st):
        self.corr = as_corr(pairs[:, 0] % W, pairs[:, 0] // W, pairs[:, 1] % W, pairs[:, 1] // W)
        self.supp = np_filter(self.corr, st)
        self.sorted_t_state = sorted_ts
        self.sorted_t_xy = np.stack([sorted_tk % W, sorted_tk // W], 1).astype(np.int32)


# ---- the fixed case list of tests/golden/ref_full_vectors.json (tools/record_ref_full.py writes it from the reference,
# tests/test_oracle_golden.py and tests/test_gpu_vs_reference.py hold the oracle and the GPU library to it)
RECORDED_FUZZ = list(range(96)) + [361]       # 361: the one tie of the 400-seed sweep


def recorded_cases(oracle):
    """(id, L, R, pre, forest, settings): raw pairs (pre None) or two (smooth, grad, mask) triples (L, R None)."""
    for seed in RECORDED_FUZZ:
        L, R, forest, st = fuzz_case(seed)
        yield "fuzz%d" % seed, L, R, None, forest, st
    L, R = synthetic_case(1024, 436, 7)
    for i, (epi, hasht) in enumerate(MODES):
        for naive in (False, True):
            yield ("synth1024x436-e%d-h%d-n%d" % (epi, hasht, naive), L, R, None, "tau" if i % 2 else "zero",
                   sparsematch_settings(5, 128, 1, epi, hasht, naive))
    L, R = striped_case()
    for epi in (True, False):
        yield "striped-e%d" % epi, L, R, None, "zero", sparsematch_settings(5, 128, 1, epi, True)
    for nl, nr in TAIL_ROWS:
        pl, pr = tail_rows(oracle, nl, nr)
        for epi, hasht in MODES:
            yield "tail%d_%d-e%d-h%d" % (nl, nr, epi, hasht), None, None, (pl, pr), "zero", \
                sparsematch_settings(5, 128, 0, epi, hasht)


def hx(v):
    return "%016x" % v


def corr_fnv(oracle, corr):
    a = np.empty((len(corr), 4), np.int32)
    a[:, 0], a[:, 1], a[:, 2], a[:, 3] = corr["sx"], corr["sy"], corr["tx"], corr["ty"]
    return hx(oracle.fnv(a))


def supp_fnv(oracle, supp):
    from oracle.pyoracle import supports_fnv
    return hx(supports_fnv(oracle, supp))


def settings_dict(st):
    return dict(thr=st.gradient_threshold, disp_high=st.disp_high, vtol=st.vertical_tolerance,
                epipolar=st.epipolar_mode, hashtable=st.use_hashtable, naive=st.naive)


def result_record(oracle, corr, supp):
    return dict(n_corr=len(corr), corr=corr_fnv(oracle, corr), n_supp=len(supp), supp=supp_fnv(oracle, supp))


def admissible(rec):
    """The results a recorded case admits: the reference's own, then (tie cases only) the other target's."""
    return [rec["result"]] + rec.get("tie_alternatives", [])


def training_cases():
    """(id, triplets, marks, params, until, w1) on the sets of test_training.py."""
    from test_training import make_cands, make_triplets
    for n, seed in ((1, 1), (257, 2)):
        t = make_triplets(n, seed)
        rng = np.random.default_rng(seed)
        params = make_cands(12, seed + 10)
        params["tau"] = rng.integers(-4, 5, 12)
        for prior, marks in (("none", np.zeros(n, np.uint8)), ("random", rng.integers(0, 4, n).astype(np.uint8))):
            for until in (0, 1, 7, 11):
                for w1 in (0.0, 0.5, 1.0):
                    yield "n%d-%s-l%d-w%g" % (n, prior, until, w1), t, marks, params, until, w1


def ramp_cases():
    """(image, {name: supports}) for getDisparityVisualization: 0, the maximum, negatives, non-integers, the clamp at
    0.8 * 128, supports on the border, one pixel painted twice, and no support at all."""
    W, H = 48, 20
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (H, W), dtype=np.uint8)

    def supports(xy, d):
        s = np.zeros(len(d), SUPPORT_DTYPE)
        s["x"], s["y"], s["d"] = [p[0] for p in xy], [p[1] for p in xy], d
        return s
    steps = np.arange(-8, 273) * 0.5                       # -4.0 .. 136.0 in halves
    grid = [(int(k) % W, int(k) // W) for k in range(len(steps))]
    odd = np.array([0.0, 128.0, 127.99, 102.4, 102.39999, 1e-3, -0.0, -1e9, 1e9, 19.37, 43.9, 63.25, 77.77, 88.1], np.float32)
    border = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (0, H // 2), (W - 1, H // 2), (W // 2, H - 1)]
    return img, {
        "empty": supports([], np.zeros(0, np.float32)),
        "halves": supports(grid, steps.astype(np.float32)),
        "odd values": supports(grid[:len(odd)], odd),
        "border": supports(border, np.linspace(0, 128, len(border)).astype(np.float32)),
        "repainted": supports([(5, 5), (5, 5), (6, 5)], np.array([10, 90, 90], np.float32)),
        "random": supports([(int(x), int(y)) for x, y in zip(rng.integers(0, W, 300), rng.integers(0, H, 300))],
                           (rng.random(300) * 160 - 16).astype(np.float32)),
    }
