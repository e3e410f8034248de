"""The harness of the device-wide matchers' tests (test_gpu_devicewide_paths.py, test_gpu_forest_shapes.py): pairs of one shape
with the oracle's records and expected results (Case), contexts created under environment knobs (make_ctx), and one batch
call on filled outputs compared byte by byte with oracle.match_pair per pair, the launch path by name (run)."""
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
        self.recs = [[self.records(fast, img) for img in (self.L[i], self.R[i])] for i in range(self.B)]
        self.cap = (self.W - 2 * R) * (self.H - 2 * R)
        self._want = {}

    def records(self, fast, img):
        if self.naive:
            sm, gr, m = fast.preprocess_naive(img, self.thr)
            codes = fast.hash_naive(sm, m, self.f)
        else:
            sm, gr, m = fast.preprocess(img, self.thr)
            codes = fast.hash(sm, gr, self.f)
        return codes.reshape(-1)[m].astype(np.uint64), (m // self.W).astype(np.uint64)

    def want(self, fast, epi, ht):
        """oracle.match_pair per pair: computed once per setting and shared"""
        if (epi, ht) not in self._want:
            st = sparsematch_settings(self.thr, 128, 1, epi, ht, self.naive)
            self._want[(epi, ht)] = [fast.match_pair(self.L[i], self.R[i], self.f, st) for i in range(self.B)]
        return self._want[(epi, ht)]

    def code_range_bins(self, i, lb=8):
        """largest bin of pair i, records of one side, by the top lb code bits (gp_bin<false>)"""
        lb = min(lb, self.bits)  # (run_partition_match: never more bin bits than code bits)
        return max(int(np.bincount((c >> np.uint64(self.bits - lb)).astype(np.int64), minlength=1).max()) for c, _ in self.recs[i])

    def bucket_bins(self, i, lbits, epi):
        """largest bin of pair i, left + right records, by hm_bucket(code, y or 0) >> lbits (gp_bin<true>)"""
        nb = (HM_BUCKETS + (1 << lbits) - 1) >> lbits
        h = np.zeros(nb, np.int64)
        for c, y in self.recs[i]:
            b = ((y * np.uint64(epi) % np.uint64(HM_BUCKETS)) * np.uint64(4585) % np.uint64(HM_BUCKETS) + c % np.uint64(HM_BUCKETS)) % np.uint64(HM_BUCKETS)
            h += np.bincount((b >> np.uint64(lbits)).astype(np.int64), minlength=nb)
        return int(h.max())


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


def run(ctx, fast, c, epi, ht, name, what, may_be_empty=False):
    """one batch call on filled outputs; every byte against the oracle; the path by name (None: whichever, returned).
    A pair without supports fails the case unless the caller expects one (may_be_empty: forests of a few tests)."""
    import torch
    import opengpc_amd as g
    dev = torch.device("cuda", 0)
    B, cap = c.B, c.cap
    want = c.want(fast, epi, ht)
    d_L, d_R = torch.from_numpy(c.L).to(dev), torch.from_numpy(c.R).to(dev)
    d_out = torch.full(((B + 1) * cap * 12,), FILL, dtype=torch.uint8, device=dev)
    d_cnt = torch.full(((B + 1) * 4,), FILL, dtype=torch.uint8, device=dev)
    d_nc = torch.full(((B + 1) * 8,), FILL, dtype=torch.uint8, device=dev)
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
    for i in range(B + 1):
        exp = np.full((cap, 3), FILL32, np.uint32)
        if i < B:
            w = want[i][0]
            k = len(w)
            exp[:k, 0], exp[:k, 1] = w["x"], w["y"]
            exp[:k, 2] = np.ascontiguousarray(w["d"], np.float32).view(np.uint32)
        if not np.array_equal(out[i], exp):
            bad = np.flatnonzero((out[i] != exp).any(axis=1))
            raise AssertionError("%s: pair %d of %d: slot %d holds %s, expected %s; %d slots differ (the pair has %d records)" % (
                what, i, B, bad[0], out[i][bad[0]], exp[bad[0]], len(bad), len(want[i][0]) if i < B else 0))
    return took
