"""The harness of the device-wide matchers' tests (test_gpu_devicewide_paths.py, test_gpu_forest_shapes.py,
test_gpu_devicewide_capacity.py): pairs of one shape with the oracle's records and expected results (Case), contexts created
under environment knobs (make_ctx), and one batch call on filled outputs compared byte by byte with oracle.match_pair per pair,
the launch path by name (run); the same for the 16-byte records of a frame sequence [L, R, L] (run_corr).  Both take a
capacity: what a short one must leave in the filled arrays is built by `expected` and compared by `compare`, which need no
device (tests/test_devicewide_harness.py feeds them arrays with a spilt record)."""
import os

import numpy as np

from oracle.pyoracle import sparsematch_settings

FILL = 0xA5
FILL32 = np.uint32(0xA5A5A5A5)
R = 13
HM_BUCKETS = 214673
SLOT = "k_global_match"

VJ4 = "gpc::k_row_join<4, 1024, false, true>"
VJ8 = "gpc::k_row_join<8, 1024, false, true>"
HJ = "gpc::k_ht_join<%d, %d>"


# ---------------------------------------------------------------------------------------------------------------- inputs
def textured(W, H, seed, D):
    from opengpc_amd.synth import synth_pair
    return synth_pair(W, H, seed, D)


def banded(W, H, seed, D, band):
    """a textured pair with `band` striped rows in both images: every striped row alike, so a few codes occur thousands of
    times and share their bins with the textured rows' records, which still have to come out matched and in order"""
    L, Rr = (a.copy() for a in textured(W, H, seed, D))
    s = np.tile((np.arange(W) // 3 * 37 % 256).astype(np.uint8), (band, 1))
    L[20:20 + band], Rr[20:20 + band] = s, np.roll(s, 7, axis=1)
    return L, Rr


class Case:
    """Pairs of one shape, the oracle's forest, and per pair the records (code, row) of either image."""

    def __init__(self, fast, forest, pairs, naive=False, forest_text=None, thr=5):
        self.L, self.R = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        self.B, self.H, self.W = self.L.shape
        self.forest, self.forest_text, self.naive, self.thr = forest, forest_text, naive, thr
        rc, self.f = fast.parse_forest_text(forest_text, self.W, self.H) if forest_text else fast.read_forest(forest, self.W, self.H)
        assert rc == 0
        self.bits = (self.f.num_tests if naive or self.f.num_tests <= 8 else self.f.num_tests - 1)  # code_bits (gpc_hip.hip)
        self.hashed = [[self.hash_image(fast, img) for img in (self.L[i], self.R[i])] for i in range(self.B)]
        self.recs = [[(cd.reshape(-1)[m].astype(np.uint64), (m // self.W).astype(np.uint64)) for cd, m in h] for h in self.hashed]
        self.cap = (self.W - 2 * R) * (self.H - 2 * R)
        self._want = {}

    def hash_image(self, fast, img):
        """(code image, candidate indices) of one image"""
        if self.naive:
            sm, gr, m = fast.preprocess_naive(img, self.thr)
            return fast.hash_naive(sm, m, self.f), m
        sm, gr, m = fast.preprocess(img, self.thr)
        return fast.hash(sm, gr, self.f), m

    def want(self, fast, epi, ht):
        """oracle.match_pair per pair: computed once per setting and shared"""
        if (epi, ht) not in self._want:
            st = sparsematch_settings(self.thr, 128, 1, epi, ht, self.naive)
            self._want[(epi, ht)] = [fast.match_pair(self.L[i], self.R[i], self.f, st) for i in range(self.B)]
        return self._want[(epi, ht)]

    def want_corr(self, fast, i, epi, ht):
        """Forest::stereoMatch of (L_i, R_i) and of (R_i, L_i): the two pairs of the frames [L_i, R_i, L_i], and the frames'
        candidate counts; computed once per setting and shared"""
        if ("corr", i, epi, ht) not in self._want:
            (cl, ml), (cr, mr) = self.hashed[i]
            dl, dr = fast.descriptors(cl, ml, self.W, epi), fast.descriptors(cr, mr, self.W, epi)
            match = fast.hash_correspondences if ht else fast.find_correspondences
            self._want[("corr", i, epi, ht)] = ([match(dl, ml, dr, mr, self.W), match(dr, mr, dl, ml, self.W)], [len(ml), len(mr), len(ml)])
        return self._want[("corr", i, epi, ht)]

    def code_range_of(self, codes, lb=8):
        """bin of a code by its top lb bits (gp_bin<false>)"""
        lb = min(lb, self.bits)  # (run_partition_match: never more bin bits than code bits)
        return (np.asarray(codes, np.uint64) >> np.uint64(self.bits - lb)).astype(np.int64)

    def code_range_hist(self, i, lb=8):
        """per side of pair i the records of every bin"""
        return [np.bincount(self.code_range_of(c, lb), minlength=1 << min(lb, self.bits)) for c, _ in self.recs[i]]

    def code_range_bins(self, i, lb=8):
        """largest bin of pair i, records of one side, by the top lb code bits"""
        return max(int(h.max()) for h in self.code_range_hist(i, lb))

    def bucket_bin_of(self, codes, y, lbits, epi):
        """bin of a record by hm_bucket(code, y or 0) >> lbits (gp_bin<true>)"""
        c, y, m = np.asarray(codes, np.uint64), np.asarray(y, np.uint64), np.uint64(HM_BUCKETS)
        b = ((y * np.uint64(epi) % m) * np.uint64(4585) % m + c % m) % m
        return (b >> np.uint64(lbits)).astype(np.int64)

    def bucket_hist(self, i, lbits, epi):
        """left + right records of pair i in every bin"""
        nb = (HM_BUCKETS + (1 << lbits) - 1) >> lbits
        return sum(np.bincount(self.bucket_bin_of(c, y, lbits, epi), minlength=nb) for c, y in self.recs[i])

    def bucket_bins(self, i, lbits, epi):
        """largest bin of pair i, left + right records"""
        return int(self.bucket_hist(i, lbits, epi).max())


_cases = {}


def shared(key, make):
    """cases are computed once and shared, unchanged, among the tests that need them"""
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


# --------------------------------------------------------------------------------------------------------------- harness
def make_ctx(env=None, naive=False):
    """the knobs are read when a context is created: set, create, remove"""
    import opengpc_amd as g
    env = env or {}
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        c = g.Context(0)
    finally:
        for k in env:
            del os.environ[k]
    if naive:
        c.set_arithmetic(True)
    return c


def load_forest(ctx, c):
    import opengpc_amd as g
    if c.forest_text:
        st, fm = g.parse_forest(c.forest_text, c.W, c.H)
        assert st == 0
        ctx.set_forest(fm)
    else:
        ctx.load_forest(c.forest, c.W, c.H)


def path(ctx):
    return ctx.kernel_launch_names()[SLOT]


def supp_words(w):
    """supports of the oracle as the 12-byte records the library writes: [n, 3] words"""
    out = np.empty((len(w), 3), np.uint32)
    out[:, 0], out[:, 1] = w["x"], w["y"]
    out[:, 2] = np.ascontiguousarray(w["d"], np.float32).view(np.uint32)
    return out


def corr_words(w):
    """correspondences of the oracle as the 16-byte records the library writes: [n, 4] words"""
    out = np.empty((len(w), 4), np.uint32)
    for k, f in enumerate(("sx", "sy", "tx", "ty")):
        out[:, k] = w[f]
    return out


def expected(wants, cap):
    """What a call with `cap` slots per pair must leave in (len(wants) + 1) * cap filled slots: the first min(len, cap) records
    of pair i, in the oracle's order, at the head of pair i's slots, and the fill in every other slot -- behind a pair's
    records, and in the spare pair's worth of slots behind the last pair.  wants: per pair [n, words] words."""
    exp = np.full((len(wants) + 1, cap, wants[0].shape[1]), FILL32, np.uint32)
    for i, w in enumerate(wants):
        k = min(len(w), cap)
        exp[i, :k] = w[:k]
    return exp


def compare(out, exp, wants, what):
    """every word of out against exp (both [pairs + 1, cap, words]); the first slot that differs is named"""
    B, cap = len(wants), exp.shape[1]
    assert out.shape == exp.shape, (out.shape, exp.shape)
    for i in range(B + 1):
        if not np.array_equal(out[i], exp[i]):
            bad = np.flatnonzero((out[i] != exp[i]).any(axis=1))
            raise AssertionError("%s: pair %d of %d: slot %d of %d holds %s, expected %s; %d slots differ (the pair has %d records)" % (
                what, i, B, bad[0], cap, out[i][bad[0]], exp[i][bad[0]], len(bad), len(wants[i]) if i < B else 0))


def filled(nbytes, dev):
    import torch
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev)


def run(ctx, fast, c, epi, ht, name, what, may_be_empty=False, cap=None):
    """One batch call on filled outputs; every byte against the oracle; the path by name (None: whichever, returned).
    A pair without supports fails the case unless the caller expects one (may_be_empty: forests of a few tests).
    cap (default: c.cap, which no pair reaches) may be short of a pair's count: the count stays the true one, the pair's first
    cap records are delivered, and every other slot -- the next pair's, the spare pair's behind the batch -- keeps the fill.
    gpc_hip_match_batch_device returns GPC_OK then as well (match_batch_device raises on every other status)."""
    import torch
    import opengpc_amd as g
    dev = torch.device("cuda", 0)
    B, cap = c.B, c.cap if cap is None else int(cap)
    assert cap >= 1
    want = c.want(fast, epi, ht)
    d_L, d_R = torch.from_numpy(c.L).to(dev), torch.from_numpy(c.R).to(dev)
    d_out, d_cnt, d_nc = filled((B + 1) * cap * 12, dev), filled((B + 1) * 4, dev), filled((B + 1) * 8, dev)
    torch.cuda.synchronize(dev)  # (the library's stream does not wait for torch's)
    ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), c.W, c.H, B, g.Settings(c.thr, 128, 1, epi, ht, 1), d_out.data_ptr(), cap,
                           d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    took = path(ctx)
    assert name is None or took == name, "%s: took %r" % (what, took)
    out = d_out.cpu().numpy().view(np.uint32).reshape(B + 1, cap, 3)
    cnt, nc = d_cnt.cpu().numpy().view(np.int32), d_nc.cpu().numpy().view(np.int32).reshape(B + 1, 2)
    for i in range(B):
        w, nl, nr = want[i]
        assert cnt[i] == len(w) and (len(w) > 0 or may_be_empty), "%s: pair %d counts %d supports, the oracle %d" % (what, i, cnt[i], len(w))
        assert tuple(nc[i]) == (nl, nr), "%s: pair %d: candidates %s, the oracle's %s" % (what, i, tuple(nc[i]), (nl, nr))
    assert cnt[B:].view(np.uint32) == FILL32 and (nc[B:].view(np.uint32) == FILL32).all(), what + ": a count behind the batch's was written"
    words = [supp_words(w[0]) for w in want]
    compare(out, expected(words, cap), words, what)
    return took


def run_corr(ctx, fast, c, i, epi, ht, name, what, cap=None):
    """gpc_hip_match_sequence_device (16-byte records, mode 1) over the frames [L_i, R_i, L_i] of pair i of the case: two pairs,
    so that pair 0 has a neighbour; filled outputs, every byte against the oracle's find_correspondences /
    hash_correspondences per consecutive pair, the frames' candidate counts, the path by name (None: whichever, returned).
    cap as for run.  The device form only queues work and cannot know the counts: it returns GPC_OK at a short capacity too
    (match_sequence_device raises on every other status)."""
    import torch
    import opengpc_amd as g
    dev = torch.device("cuda", 0)
    cap = c.cap if cap is None else int(cap)
    assert cap >= 1
    want, ncand = c.want_corr(fast, i, epi, ht)
    P, N = 2, 3
    d_f = torch.from_numpy(np.ascontiguousarray(np.stack([c.L[i], c.R[i], c.L[i]]))).to(dev)
    d_out, d_cnt, d_nc = filled((P + 1) * cap * 16, dev), filled((P + 1) * 4, dev), filled((N + 1) * 4, dev)
    torch.cuda.synchronize(dev)
    ctx.match_sequence_device(d_f.data_ptr(), c.W, c.H, N, g.Settings(c.thr, 128, 1, epi, ht, 1), d_out.data_ptr(), cap,
                              d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    took = path(ctx)
    assert name is None or took == name, "%s: took %r" % (what, took)
    out = d_out.cpu().numpy().view(np.uint32).reshape(P + 1, cap, 4)
    cnt, nc = d_cnt.cpu().numpy().view(np.int32), d_nc.cpu().numpy().view(np.int32)
    for t in range(P):
        assert cnt[t] == len(want[t]) > 0, "%s: pair %d counts %d correspondences, the oracle %d" % (what, t, cnt[t], len(want[t]))
    assert list(nc[:N]) == ncand, "%s: candidates %s, the oracle's %s" % (what, list(nc[:N]), ncand)
    assert cnt[P:].view(np.uint32) == FILL32 and nc[N:].view(np.uint32) == FILL32, what + ": a count behind the sequence's was written"
    words = [corr_words(w) for w in want]
    compare(out, expected(words, cap), words, what)
    return took
