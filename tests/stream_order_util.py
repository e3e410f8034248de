"""Stream ordering of the *_device entry points (tests/test_gpu_stream_order.py): the harness and the cases.

The contract of include/gpc_hip.h: a call only queues work on the context's stream (the device-wide matchers wait once on
the host inside the call), its inputs are what that stream has produced when the call is made, and its outputs may be read
behind any wait on the stream.  run() holds a call to exactly that on a stream borrowed from torch: the real inputs arrive
behind a delay on the stream, the outputs are copied away on the stream right behind the call, and inputs and outputs are
overwritten behind that copy.  Expected values come from the CPU models the suite trusts (oracle.pyoracle, the *_util.py
restatements), computed once per session and shared."""
import functools
import os

import numpy as np

import clean_util as cu
import consensus_util as co
import dense_util as du
import pyramid_util as pu
import quad_util as qu
import refine_util as ru
import score_util as su
import track_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORESTS = {"zero": os.path.join(ROOT, "forests", "defaultZeroForest.txt"), "tau": os.path.join(ROOT, "forests", "defaultTauForest.txt")}
W, H, B, N = 96, 64, 2, 3                        # the smallest golden shape: 2 pairs, 3 frames
DISP = (5, 7, 3)                                 # the disparity of data set k: the sets differ in what they match, not only where
P = N - 1
CAP = (W - 26) * (H - 26) + 1                    # every record of a pair
FILL = 0xA5                                      # what every output byte holds before the call
MARK = 0x3C                                      # what every output byte is overwritten with behind the snapshot
FILL_I32 = int(np.array([FILL] * 4, np.uint8).view(np.int32)[0])
THR = (1.0, 3.0)
RADIUS = 3
PLACEHOLDER = 2                                  # data set 2: what image inputs hold before the real ones arrive, and what every warm-up call runs on

# The delay every case queues in front of its real inputs, in the ticks torch.cuda._sleep counts.  Measured on an MI355X with
# the library as it stands (`python tests/stream_order_util.py` prints the figures; docs/HISTORY.md, section 8, keeps them):
# _sleep takes 0.42 ms per 10^6 ticks; the host-side duration of the warmed calls at these shapes is 0.004 ms
# (pyramid_down_device) to 0.079 ms in one run and 0.111 ms in another (consensus_batch_device both times; clean_batch_device
# 0.070 / 0.096, consensus_records_device 0.064 / 0.093, the device-wide match_batch_device 0.045 - 0.055).  Ten times the
# longest is 1.1 ms; 50 * 10^6 ticks are 21 ms, 190 times the longest call, so that a host thread that loses its CPU for a
# few milliseconds on a shared machine does not void the premise.  The premise assertions of run() guard the number: a
# delay that ran out fails the case.
DELAY_CYCLES = 50_000_000


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Spec:
    """One call (or a few consecutive ones) under test.
    inputs:  name -> (real, placeholder) or (real, placeholder, warm) numpy arrays of equal size: what the measured call must
             read, what the input holds until then, and what the warm-up call reads (the placeholder if not given);
    outputs: name -> number of bytes, or the name of the input the call writes in place;
    want:    name -> the bytes the output holds after the call(s), given that every byte held FILL before;
    calls:   functions (ctx, p) of the pointers p[name], each one library call;
    waits:   the header documents a host wait inside the call, so the stream may have drained when it returns."""

    def __init__(self, name, inputs, outputs, want, calls, waits=False, forest=None, after_warmup=None, close=None, foreign=None):
        self.name, self.inputs, self.outputs, self.want, self.calls, self.waits = name, inputs, outputs, want, calls, waits
        self.forest, self.after_warmup, self.close = forest, after_warmup, close
        self.foreign = foreign or {}              # name -> (device pointer, bytes): outputs the library owns


class _Foreign:
    """device memory of the library as something torch.as_tensor takes without a copy"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def sleep(st, cycles):
    """a delay on the stream: torch.cuda._sleep, or, where torch has none, a chain of matmuls.  The chain's length is a
    guess that was never measured (no torch without _sleep was at hand); run()'s premise assertions fail the case if it
    is too short."""
    import torch
    with torch.cuda.stream(st):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(int(cycles))
        else:
            a = torch.ones((2048, 2048), device="cuda:0")
            for _ in range(max(1, int(cycles) // 100_000)):
                a = (a @ a) * 0.0 + 1.0


def run(ctx, st, specs, timings=None):
    """The harness.  specs: one Spec, or two for the back-to-back form (queued one after the other behind one delay).
    timings (a dict): receives the host-side duration of each spec's warmed calls (see measure())."""
    try:
        _run(ctx, st, specs, timings)
    finally:
        for s in specs:
            if s.close:
                s.close()


def _run(ctx, st, specs, timings):
    import torch
    dev = torch.device("cuda", 0)
    to_dev = lambda a: torch.from_numpy(u8(a).copy()).to(dev)
    T = []
    for s in specs:
        t = {"real": {n: to_dev(v[0]) for n, v in s.inputs.items()}, "ph": {n: to_dev(v[1]) for n, v in s.inputs.items()}}
        for n, v in s.inputs.items():
            assert u8(v[0]).nbytes == u8(v[1]).nbytes == u8(v[-1]).nbytes, (s.name, n)
            assert not np.array_equal(u8(v[0]), u8(v[-1])), (s.name, n, "the warm-up data must differ from the real data")
        t["in"] = {n: to_dev(v[-1]) for n, v in s.inputs.items()}            # the warm-up call sees OTHER valid data
        t["out"] = {n: (t["in"][nb] if isinstance(nb, str) else torch.full((nb,), FILL, dtype=torch.uint8, device=dev))
                    for n, nb in s.outputs.items()}
        for n, (ptr, nb) in s.foreign.items():
            t["out"][n] = torch.as_tensor(_Foreign(ptr, nb), device=dev)
        t["snap"] = {n: torch.zeros_like(o) for n, o in t["out"].items()}
        p = {n: x.data_ptr() for n, x in list(t["in"].items()) + list(t["out"].items())}
        T.append((t, p))
    torch.cuda.synchronize(dev)
    # warm-up: one untimed, fully synchronised call of the same shape, so that no workspace grows (and waits) inside the
    # measured call -- on ANOTHER valid data set (PLACEHOLDER), so that every workspace of the context and every table of a
    # track stream holds valid but wrong state when the measured call is queued: a launch that runs too early, or on another
    # stream, reads that state and the bytes come out wrong
    for s, (t, p) in zip(specs, T):
        if s.forest:
            ctx.load_forest(FORESTS[s.forest], W, H)
        for call in s.calls:
            call(ctx, p)
        ctx.synchronize()
        if timings is not None:                                             # the host-side duration of the warmed calls
            import time
            if s.after_warmup:
                s.after_warmup()
            t0 = time.perf_counter()
            for call in s.calls:
                call(ctx, p)
            timings[s.name] = (time.perf_counter() - t0) / len(s.calls)
            ctx.synchronize()
        if s.after_warmup:
            s.after_warmup()
        for n, x in t["in"].items():
            x.copy_(t["ph"][n])
        for n, nb in s.outputs.items():
            if not isinstance(nb, str):
                t["out"][n].fill_(FILL)
    ctx.synchronize()
    torch.cuda.synchronize(dev)
    # the real inputs exist only in stream order, behind the delay
    sleep(st, DELAY_CYCLES)
    with torch.cuda.stream(st):
        for t, _ in T:
            for n, x in t["in"].items():
                x.copy_(t["real"][n], non_blocking=True)
    for s, (t, p) in zip(specs, T):
        for k, call in enumerate(s.calls):
            assert not st.query(), (s.name, k, "the delay ran out before the call: the case proves nothing")
            call(ctx, p)
            assert s.waits or not st.query(), (s.name, k, "the call is documented to only queue work, but the stream had drained when it returned")
    # no host wait: the outputs are copied away in stream order, then inputs and outputs are overwritten behind the copy
    with torch.cuda.stream(st):
        for t, _ in T:
            for n, o in t["out"].items():
                t["snap"][n].copy_(o, non_blocking=True)
        for s, (t, _) in zip(specs, T):
            for n, x in t["in"].items():
                x.copy_(t["ph"][n], non_blocking=True)
            for n, nb in s.outputs.items():
                if not isinstance(nb, str):
                    t["out"][n].fill_(MARK)
    st.synchronize()
    got = [{n: x.cpu().numpy() for n, x in t["snap"].items()} for t, _ in T]
    ctx.synchronize()                                                       # (raises on a status other than 0)
    for s, g in zip(specs, got):
        assert set(s.want) == set(g), (s.name, sorted(s.want), sorted(g))
        for n, w in s.want.items():
            w = u8(w)
            assert w.nbytes == g[n].nbytes, (s.name, n, w.nbytes, g[n].nbytes)
            if not np.array_equal(g[n], w):
                bad = np.flatnonzero(g[n] != w)
                raise AssertionError("%s: output %s: %d of %d bytes differ, the first at %d: %s, expected %s" % (
                    s.name, n, len(bad), w.nbytes, bad[0], g[n][bad[0]:bad[0] + 16].tolist(), w[bad[0]:bad[0] + 16].tolist()))


# ---- data: computed once, shared, never changed ---------------------------------------------------------------------------

def oracle():
    return pu.the_oracle()


@functools.lru_cache(maxsize=None)
def forest(name):
    rc, f = oracle().read_forest(FORESTS[name], W, H)
    assert rc == 0
    return f


@functools.lru_cache(maxsize=None)
def pairs(k):
    q = [oracle().synth_pair(W, H, 10 * k + i, DISP[k]) for i in range(B)]
    return np.stack([a[0] for a in q]), np.stack([a[1] for a in q])


@functools.lru_cache(maxsize=None)
def frames(k):
    return tu.frames_of(W, H, N, 1 + k, 0)


@functools.lru_cache(maxsize=None)
def stereo(k):
    return qu.stereo_frames_of(W, H, N, 1 + k, DISP[k], 0)


def settings(epi=True, ht=False):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, epi, ht, 1)


def filled(shape, dtype):
    dtype = np.dtype(dtype)
    n = int(np.prod(shape))
    return np.full(n * dtype.itemsize, FILL, np.uint8).view(dtype).reshape(shape)


def slots(lists, dtype, cap=CAP, fill=True):
    """per-pair record lists -> ([len(lists), cap] of dtype: the records, then FILL bytes (or zeros), counts [len(lists)])"""
    out = filled((len(lists), cap), dtype) if fill else np.zeros((len(lists), cap), dtype)
    for t, r in enumerate(lists):
        k = min(len(r), cap)
        out[t, :k] = np.ascontiguousarray(r[:k]).view(dtype)
    return out, np.array([len(r) for r in lists], np.int32)


@functools.lru_cache(maxsize=None)
def match(images, k, fname="zero", epi=True, ht=False):
    """the oracle's Forest::rectifiedMatch of every pair of pairs(k) (images "pairs") or of (L_t, R_t) of stereo(k) ("stereo"):
    (supports per pair, candidate counts [n, 2])"""
    from oracle.pyoracle import sparsematch_settings
    L, R = pairs(k) if images == "pairs" else stereo(k)
    res = [oracle().match_pair(L[i], R[i], forest(fname), sparsematch_settings(5, 128, 0, epi, ht, False)) for i in range(len(L))]
    return [r[0] for r in res], np.array([[r[1], r[2]] for r in res], np.int32)


@functools.lru_cache(maxsize=None)
def flow(images, k, fname="zero", epi=True, ht=False):
    """the oracle's Forest::stereoMatch of consecutive frames: (correspondences per pair, candidates per frame [N])"""
    f = {"frames": lambda: frames(k), "left": lambda: stereo(k)[0], "right": lambda: stereo(k)[1]}[images]()
    rec, cnt, nc = tu.oracle_sequence(oracle(), f, forest(fname), epi, ht)
    return [rec[t, :cnt[t]] for t in range(len(cnt))], np.array(nc, np.int32)


@functools.lru_cache(maxsize=None)
def sup_in(k):
    """supports as a record-form input: [B, CAP] with zeros behind the records, counts [B]"""
    return slots(match("pairs", k)[0], ru.SUPPORT, fill=False)


@functools.lru_cache(maxsize=None)
def corr_in(k):
    return slots(flow("frames", k)[0], ru.CORR, fill=False)


@functools.lru_cache(maxsize=None)
def truth(k, with_v):
    """disparity (or flow) truth planes around the construction's, with pixels off by more than a threshold, and an ignore mask"""
    rng = np.random.default_rng(900 + k)
    n = P if with_v else B
    u = (DISP[k] if not with_v else 3) + rng.choice([0.0, 0.0, 0.0, 0.5, -2.0, 4.0], (n, H, W))
    v = rng.choice([0.0, 0.0, 1.0, -3.5], (n, H, W))
    ign = (rng.random((n, H, W)) < 0.1).astype(np.uint8)
    return u.astype(np.float32), v.astype(np.float32), ign


def score_rows(recs, cnts, u, v, ign, extra=None):
    import opengpc_amd as g
    out = np.zeros(len(recs), g.SCORE_DTYPE)
    for t in range(len(recs)):
        s = su.score_records(recs[t], cnts[t], CAP, u[t], None if v is None else v[t], ign[t], np.array(THR, np.float32))
        if extra:
            s["n_candidates"], s["n_matchable"] = extra[t]
        for f in su.SCORE_FIELDS:
            out[f][t] = s[f]
    return out


@functools.lru_cache(maxsize=None)
def refinement(k):
    """refinements and refined supports of sup_in(k) over the raw pairs, in FILL-filled arrays"""
    rec, cnt = sup_in(k)
    L, R = pairs(k)
    return ru.expected_arrays(rec, cnt, L, R, RADIUS, FILL)


@functools.lru_cache(maxsize=None)
def ref_in(k):
    """the refinements as an input: zeros behind the records"""
    ref = refinement(k)[0].copy()
    for t, m in enumerate(ru.m_of(sup_in(k)[1], CAP)):
        ref[t, m:] = np.zeros(1, ru.REFINEMENT)[0]
    return ref


@functools.lru_cache(maxsize=None)
def fields(k):
    return cu.random_fields(W, H, 1, 3, seed=100 + k)


@functools.lru_cache(maxsize=None)
def track_want(images, k, track_cap):
    lists, _ = flow(images, k)
    rec, cnt = slots(lists, tu.CORR, fill=False)
    return tu.expected_arrays(rec, cnt, W, H, FILL_I32, track_cap)


def prev_of(nxt, cnt):
    """prev [P, CAP]: the inverse of next, FILL behind a pair's records"""
    prev = np.full(nxt.shape, FILL_I32, np.int32)
    for t, m in enumerate(ru.m_of(cnt, CAP)):
        prev[t, :m] = -1
        if t:
            i = np.flatnonzero(nxt[t - 1, :ru.m_of(cnt, CAP)[t - 1]] >= 0)
            prev[t, nxt[t - 1, i]] = i
    return prev


@functools.lru_cache(maxsize=None)
def quads_in(k):
    sup, nsup = slots(match("stereo", k)[0], qu.SUP, fill=False)
    fl, nfl = slots(flow("left", k)[0], qu.CORR, fill=False)
    fr, nfr = slots(flow("right", k)[0], qu.CORR, fill=False)
    return sup, nsup, fl, nfl, fr, nfr


@functools.lru_cache(maxsize=None)
def quads_want(k):
    q, n = qu.expected_arrays(*quads_in(k), W, H, 1, FILL_I32, CAP)
    assert n.min() > 0, n
    return q, n


@functools.lru_cache(maxsize=None)
def pyramid_levels(k):
    """per pair the oracle's (records, candidates left, candidates right) of both levels"""
    L, R = pairs(k)
    return [pu.level_supports(pu.remember(L[i], R[i]), "zero", 2, 5, 128, 0, True, False, False) for i in range(B)]


CAP1 = (W // 2 - 26) * (H // 2 - 26) + 1
CAPM = CAP + CAP1


@functools.lru_cache(maxsize=None)
def pyramid_want(k):
    per = pyramid_levels(k)
    merged, kept = zip(*[pu.merge([l[0].astype(pu.SUPPORT) for l in p], W, H) for p in per])
    out, cnt = slots(merged, pu.SUPPORT, CAPM)
    ncand = np.array([[[p[l][1], p[l][2]] for p in per] for l in range(2)], np.int32)
    return out, cnt, np.array(kept, np.int32).T.copy(), ncand


# ---- the cases ------------------------------------------------------------------------------------------------------------

def rec_inputs(make, k, *names):
    """record-form inputs: name -> (array of set k, zeros, array of the warm-up set); make(k) returns the arrays in order"""
    return {n: (a, np.zeros_like(a), w) for n, a, w in zip(names, make(k), make(PLACEHOLDER))}


def score_supports(ctx, k):
    (rec, cnt), (u, _, ign) = sup_in(k), truth(k, False)
    return Spec("score_supports_device", rec_inputs(lambda j: sup_in(j) + truth(j, False)[::2], k, "rec", "cnt", "u", "ign"),
                dict(scores=B * 120), dict(scores=score_rows(rec, cnt, u, None, ign)),
                [lambda c, p: c.score_supports_device(p["rec"], CAP, p["cnt"], W, H, B, p["u"], p["ign"], THR, p["scores"])])


def score_correspondences(ctx, k):
    (rec, cnt), (u, v, ign) = corr_in(k), truth(k, True)
    return Spec("score_correspondences_device",
                rec_inputs(lambda j: corr_in(j) + truth(j, True), k, "rec", "cnt", "u", "v", "ign"),
                dict(scores=P * 120), dict(scores=score_rows(rec, cnt, u, v, ign)),
                [lambda c, p: c.score_correspondences_device(p["rec"], CAP, p["cnt"], W, H, P, p["u"], p["v"], p["ign"], THR, p["scores"])])


TRACK_CAP = P * CAP


def track_records(ctx, k):
    rec, cnt = corr_in(k)
    nxt, tid, tab, n = track_want("frames", k, TRACK_CAP)
    return Spec("track_records_device", rec_inputs(corr_in, k, "rec", "cnt"),
                dict(next=P * CAP * 4, tid=P * CAP * 4, tracks=TRACK_CAP * 16, n=4),
                dict(next=nxt, tid=tid, tracks=tab, n=np.array([n], np.int32)),
                [lambda c, p: c.track_records_device(p["rec"], CAP, p["cnt"], W, H, P, p["next"], p["tid"], p["tracks"], TRACK_CAP, p["n"])])


def consensus_records(corr):
    def make(ctx, k):
        import opengpc_amd as g
        rec, cnt = corr_in(k) if corr else sup_in(k)
        n = len(rec)
        keep, out, index, n_out = co.expected_arrays(rec, cnt, W, H, co.Params(), CAP, FILL)
        return Spec("consensus_records_device(%s)" % ("correspondences" if corr else "supports"),
                    rec_inputs(corr_in if corr else sup_in, k, "rec", "cnt"),
                    dict(keep=n * CAP, out=n * CAP * rec.dtype.itemsize, index=n * CAP * 4, n=n * 4),
                    dict(keep=keep, out=out, index=index, n=n_out),
                    [lambda c, p: c.consensus_records_device(p["rec"], corr, CAP, p["cnt"], W, H, n, g.Consensus(), p["keep"], p["out"], CAP,
                                                             p["index"], p["n"])])
    return make


def refine_records(ctx, k):
    (rec, cnt), (L, R), (ref, out) = sup_in(k), pairs(k), refinement(k)
    pL, pR = pairs(PLACEHOLDER)
    return Spec("refine_records_device", dict(rec_inputs(sup_in, k, "rec", "cnt"), L=(L, pL), R=(R, pR)),
                dict(ref=B * CAP * 8, out=B * CAP * 12), dict(ref=ref, out=out),
                [lambda c, p: c.refine_records_device(p["rec"], False, CAP, p["cnt"], p["L"], p["R"], W, H, B, RADIUS, p["ref"], p["out"])])


def pyramid_down(ctx, k):
    L, pL = pairs(k)[0], pairs(PLACEHOLDER)[0]
    return Spec("pyramid_down_device", dict(src=(L, pL)), dict(dst=B * (H // 2) * (W // 2)), dict(dst=pu.down(L)),
                [lambda c, p: c.pyramid_down_device(p["src"], W, H, B, p["dst"])])


def merge_in(k):
    """both levels' unmapped records and counts, zeros behind the records"""
    per = pyramid_levels(k)
    return slots([p[0][0] for p in per], pu.SUPPORT, CAP, fill=False) + slots([p[1][0] for p in per], pu.SUPPORT, CAP1, fill=False)


def pyramid_merge(ctx, k):
    r0, c0, r1, c1 = merge_in(k)
    out, cnt, kept, _ = pyramid_want(k)
    assert kept[1].min() >= 0 and c1.min() > 0
    return Spec("pyramid_merge_device", rec_inputs(merge_in, k, "r0", "c0", "r1", "c1"),
                dict(out=B * CAPM * 12, cnt=B * 4, levels=2 * B * 4), dict(out=out, cnt=cnt, levels=kept),
                [lambda c, p: c.pyramid_merge_device([p["r0"], p["r1"]], [CAP, CAP1], [p["c0"], p["c1"]], False, W, H, B, p["out"], CAPM,
                                                     p["cnt"], p["levels"])])


def densify_records(ctx, k):
    import opengpc_amd as g
    (rec, cnt), ref = sup_in(k), ref_in(k)
    value, level = du.densify(rec, cnt, W, H, du.DEFAULTS, ref)
    return Spec("densify_records_device", rec_inputs(lambda j: sup_in(j) + (ref_in(j),), k, "rec", "cnt", "ref"),
                dict(value=B * H * W * 4, level=B * H * W), dict(value=value, level=level),
                [lambda c, p: c.densify_records_device(p["rec"], False, CAP, p["cnt"], W, H, B, g.Densify(), p["value"], p["level"], p["ref"])])


def clean_fields(with_bwd):
    def make(ctx, k):
        import opengpc_amd as g
        fwd, bwd = fields(k)
        pf, pb = fields(PLACEHOLDER)
        prm = cu.DEFAULTS if with_bwd else (-1, 256, 64, 1)
        out, state, label, stats = cu.clean(fwd, bwd if with_bwd else None, prm)
        n = len(fwd)
        inputs = dict(fwd=(fwd, pf), bwd=(bwd, pb)) if with_bwd else dict(fwd=(fwd, pf))
        return Spec("clean_fields_device(%s)" % ("cross-check" if with_bwd else "no backward field"), inputs,
                    dict(out=n * H * W * 4, state=n * H * W, label=n * H * W * 4, stats=n * 16),
                    dict(out=out, state=state, label=label, stats=stats),
                    [lambda c, p: c.clean_fields_device(p["fwd"], 1, W, H, n, g.Clean(*prm), p["out"], p.get("bwd", 0), p["state"], p["label"],
                                                        p["stats"])])
    return make


def flip_records(in_place):
    def make(ctx, k):
        (rec, cnt), ref = sup_in(k), ref_in(k)
        if in_place:
            w_rec, w_ref = cu.flip(rec, cnt, ref, rec, ref)
            return Spec("flip_records_device(in place)", rec_inputs(lambda j: sup_in(j) + (ref_in(j),), k, "rec", "cnt", "ref"),
                        dict(rec_out="rec", ref_out="ref"), dict(rec_out=w_rec, ref_out=w_ref),
                        [lambda c, p: c.flip_records_device(p["rec"], False, CAP, p["cnt"], B, p["rec"], p["ref"], p["ref"])])
        w_rec, w_ref = cu.flip(rec, cnt, ref, filled((B, CAP), du.SUPPORT), filled((B, CAP), du.REFINEMENT))
        return Spec("flip_records_device", rec_inputs(lambda j: sup_in(j) + (ref_in(j),), k, "rec", "cnt", "ref"),
                    dict(rec_out=B * CAP * 12, ref_out=B * CAP * 8), dict(rec_out=w_rec, ref_out=w_ref),
                    [lambda c, p: c.flip_records_device(p["rec"], False, CAP, p["cnt"], B, p["rec_out"], p["ref"], p["ref_out"])])
    return make


def quads_records(ctx, k):
    sup, nsup, fl, nfl, fr, nfr = quads_in(k)
    q, n = quads_want(k)
    return Spec("quads_records_device", rec_inputs(quads_in, k, "sup", "nsup", "fl", "nfl", "fr", "nfr"),
                dict(quads=P * CAP * 32, n=P * 4), dict(quads=q, n=n),
                [lambda c, p: c.quads_records_device(p["sup"], CAP, p["nsup"], p["fl"], p["fr"], CAP, p["nfl"], p["nfr"], W, H, N, 1,
                                                     p["quads"], CAP, p["n"])])


def stream_push_records(ctx, k):
    rec, cnt = corr_in(k)
    nxt, tid, tab, n = track_want("frames", k, TRACK_CAP)
    ts = ctx.track_stream(W, H, None, CAP, TRACK_CAP)
    d_tab, d_n = ts.table()
    # the table is the library's memory: rows at n and beyond are never written, so only the rows that exist are compared
    return Spec("TrackStream.push_records_device", rec_inputs(corr_in, k, "rec", "cnt"),
                dict(prev=P * CAP * 4, tid=P * CAP * 4), dict(prev=prev_of(nxt, cnt), tid=tid, table=tab[:n], total=np.array([n], np.int32)),
                [lambda c, p: ts.push_records_device(p["rec"], p["cnt"], P, p["prev"], p["tid"])],
                after_warmup=ts.reset, close=ts.close, foreign=dict(table=(d_tab, n * 16), total=(d_n, 4)))


RECORD_FORMS = {
    "score_supports": score_supports, "score_correspondences": score_correspondences, "track_records": track_records,
    "consensus_supports": consensus_records(False), "consensus_correspondences": consensus_records(True),
    "refine_records": refine_records, "pyramid_down": pyramid_down, "pyramid_merge": pyramid_merge, "densify_records": densify_records,
    "clean_fields": clean_fields(True), "clean_fields_no_bwd": clean_fields(False), "flip_records": flip_records(False),
    "flip_records_in_place": flip_records(True), "quads_records": quads_records, "stream_push_records": stream_push_records,
}


def image_inputs(k, what="pairs"):
    if what == "pairs":
        (L, R), (pL, pR) = pairs(k), pairs(PLACEHOLDER)
        return dict(L=(L, pL), R=(R, pR))
    if what == "stereo":
        (L, R), (pL, pR) = stereo(k), stereo(PLACEHOLDER)
        return dict(L=(L, pL), R=(R, pR))
    return dict(F=(frames(k), frames(PLACEHOLDER)))


def match_batch(fname, epi, ht):
    def make(ctx, k):
        lists, nc = match("pairs", k, fname, epi, ht)
        out, cnt = slots(lists, ru.SUPPORT)
        assert cnt.min() > 0
        return Spec("match_batch_device(%s, epipolar %d, hashtable %d)" % (fname, epi, ht), image_inputs(k),
                    dict(out=B * CAP * 12, cnt=B * 4, nc=B * 8), dict(out=out, cnt=cnt, nc=nc),
                    [lambda c, p: c.match_batch_device(p["L"], p["R"], W, H, B, settings(epi, ht), p["out"], CAP, p["cnt"], p["nc"])],
                    waits=not (epi and not ht), forest=fname)
    return make


def match_batch_packed(ctx, k):
    lists, nc = match("pairs", k)
    packed, rows = filled((B, CAP), np.uint32), filled((B, H), np.int32)
    for t, r in enumerate(lists):
        x = r["x"].astype(np.int64)
        packed[t, :len(r)] = (x | ((x - r["d"].astype(np.int64)) << 16)).astype(np.uint32)
        rows[t, 13:H - 13] = np.bincount(r["y"], minlength=H)[13:H - 13]
        assert (np.diff(r["y"]) >= 0).all()
    return Spec("match_batch_device_packed", image_inputs(k), dict(packed=B * CAP * 4, rows=B * H * 4, cnt=B * 4, nc=B * 8),
                dict(packed=packed, rows=rows, cnt=np.array([len(r) for r in lists], np.int32), nc=nc),
                [lambda c, p: c.match_batch_device_packed(p["L"], p["R"], W, H, B, settings(), p["packed"], CAP, p["rows"], p["cnt"], p["nc"])],
                forest="zero")


def match_sequence(ctx, k):
    lists, nc = flow("frames", k)
    out, cnt = slots(lists, ru.CORR)
    assert cnt.min() > 0
    return Spec("match_sequence_device", image_inputs(k, "frames"), dict(out=P * CAP * 16, cnt=P * 4, nc=N * 4), dict(out=out, cnt=cnt, nc=nc),
                [lambda c, p: c.match_sequence_device(p["F"], W, H, N, settings(), p["out"], CAP, p["cnt"], p["nc"])], forest="zero")


def stereo_outputs(k):
    (sl, snc), (ll, lnc), (rl, rnc) = match("stereo", k), flow("left", k), flow("right", k)
    (sup, nsup), (fl, nfl), (fr, nfr) = slots(sl, qu.SUP), slots(ll, qu.CORR), slots(rl, qu.CORR)
    assert (snc[:, 0] == lnc).all() and (snc[:, 1] == rnc).all()
    sizes = dict(sup=N * CAP * 12, nsup=N * 4, fl=P * CAP * 16, fr=P * CAP * 16, nfl=P * 4, nfr=P * 4, nc=2 * N * 4)
    return sizes, dict(sup=sup, nsup=nsup, fl=fl, fr=fr, nfl=nfl, nfr=nfr, nc=np.stack([lnc, rnc]))


def match_stereo_sequence(ctx, k):
    sizes, want = stereo_outputs(k)
    return Spec("match_stereo_sequence_device", image_inputs(k, "stereo"), sizes, want,
                [lambda c, p: c.match_stereo_sequence_device(p["L"], p["R"], W, H, N, settings(), settings(), p["sup"], CAP, p["nsup"], p["fl"],
                                                             p["fr"], CAP, p["nfl"], p["nfr"], p["nc"])], forest="zero")


def quads_sequence(ctx, k):
    sizes, want = stereo_outputs(k)
    q, n = quads_want(k)
    return Spec("quads_sequence_device", image_inputs(k, "stereo"), dict(sizes, quads=P * CAP * 32, n=P * 4), dict(want, quads=q, n=n),
                [lambda c, p: c.quads_sequence_device(p["L"], p["R"], W, H, N, settings(), settings(), 1, p["sup"], CAP, p["nsup"], p["fl"],
                                                      p["fr"], CAP, p["nfl"], p["nfr"], p["nc"], p["quads"], CAP, p["n"])], forest="zero")


def score_batch(ctx, k):
    (lists, nc), (u, _, ign), (L, R) = match("pairs", k), truth(k, False), pairs(k)
    rec, cnt = slots(lists, ru.SUPPORT, fill=False)
    cand = lambda img: su.cand_image(oracle().preprocess(img, 5)[2], W, H)
    extra = [su.matchable(cand(L[t]), cand(R[t]), u[t], None, ign[t]) for t in range(B)]
    assert min(e[1] for e in extra) > 0
    inputs = dict(image_inputs(k), **rec_inputs(lambda j: truth(j, False)[::2], k, "u", "ign"))
    return Spec("score_batch_device", inputs, dict(scores=B * 120), dict(scores=score_rows(rec, cnt, u, None, ign, extra)),
                [lambda c, p: c.score_batch_device(p["L"], p["R"], W, H, B, settings(), p["u"], p["ign"], THR, p["scores"])], forest="zero")


def track_sequence(ctx, k):
    lists, nc = flow("frames", k)
    out, cnt = slots(lists, ru.CORR)
    nxt, tid, tab, n = track_want("frames", k, TRACK_CAP)
    return Spec("track_sequence_device", image_inputs(k, "frames"),
                dict(out=P * CAP * 16, cnt=P * 4, nc=N * 4, next=P * CAP * 4, tid=P * CAP * 4, tracks=TRACK_CAP * 16, n=4),
                dict(out=out, cnt=cnt, nc=nc, next=nxt, tid=tid, tracks=tab, n=np.array([n], np.int32)),
                [lambda c, p: c.track_sequence_device(p["F"], W, H, N, settings(), p["out"], CAP, p["cnt"], p["nc"], p["next"], p["tid"],
                                                      p["tracks"], TRACK_CAP, p["n"])], forest="zero")


def stream_push(ctx, k):
    """two pushes: frames 0 and 1 (one pair), then frame 2 (the second pair)"""
    lists, nc = flow("frames", k)
    out, cnt = slots(lists, ru.CORR)
    nxt, tid, tab, n = track_want("frames", k, TRACK_CAP)
    ts = ctx.track_stream(W, H, settings(), CAP, TRACK_CAP)
    d_tab, d_n = ts.table()

    def push(first, nf, pair):
        def call(c, p):
            got = ts.push_device(p["F"] + first * W * H, nf, p["out"] + pair * CAP * 16, p["cnt"] + pair * 4, p["nc"] + first * 4,
                                 p["prev"] + pair * CAP * 4, p["tid"] + pair * CAP * 4)
            assert got == 1, got
        return call
    return Spec("TrackStream.push_device", image_inputs(k, "frames"), dict(out=P * CAP * 16, cnt=P * 4, nc=N * 4, prev=P * CAP * 4, tid=P * CAP * 4),
                dict(out=out, cnt=cnt, nc=nc, prev=prev_of(nxt, cnt), tid=tid, table=tab[:n], total=np.array([n], np.int32)),
                [push(0, 2, 0), push(2, 1, 1)], forest="zero", after_warmup=ts.reset, close=ts.close,
                foreign=dict(table=(d_tab, n * 16), total=(d_n, 4)))


def consensus_batch(ctx, k):
    import opengpc_amd as g
    lists, nc = match("pairs", k)
    rec, cnt = slots(lists, co.SUPPORT, fill=False)
    _, out, _, n_out = co.expected_arrays(rec, cnt, W, H, co.Params(), CAP, FILL)
    assert n_out.min() > 0
    return Spec("consensus_batch_device", image_inputs(k), dict(out=B * CAP * 12, n=B * 4, raw=B * 4, nc=B * 8),
                dict(out=out, n=n_out, raw=cnt, nc=nc),
                [lambda c, p: c.consensus_batch_device(p["L"], p["R"], W, H, B, settings(), g.Consensus(), p["out"], CAP, p["n"], p["raw"],
                                                       p["nc"])], forest="zero")


def refine_batch(ctx, k):
    lists, nc = match("pairs", k)
    sup, cnt = slots(lists, ru.SUPPORT)
    ref, out = refinement(k)
    return Spec("refine_batch_device", image_inputs(k), dict(sup=B * CAP * 12, cnt=B * 4, nc=B * 8, ref=B * CAP * 8, out=B * CAP * 12),
                dict(sup=sup, cnt=cnt, nc=nc, ref=ref, out=out),
                [lambda c, p: c.refine_batch_device(p["L"], p["R"], W, H, B, settings(), RADIUS, p["sup"], CAP, p["cnt"], p["nc"], p["ref"],
                                                    p["out"])], forest="zero")


def pyramid_batch(ctx, k):
    out, cnt, kept, ncand = pyramid_want(k)
    return Spec("pyramid_batch_device", image_inputs(k), dict(out=B * CAPM * 12, cnt=B * 4, levels=2 * B * 4, nc=2 * B * 8),
                dict(out=out, cnt=cnt, levels=kept, nc=ncand),
                [lambda c, p: c.pyramid_batch_device(p["L"], p["R"], W, H, B, 2, settings(), p["out"], CAPM, p["cnt"], p["levels"], p["nc"])],
                forest="zero")


@functools.lru_cache(maxsize=None)
def dense_want(k):
    (rec, cnt), ref = sup_in(k), ref_in(k)
    return du.densify(rec, cnt, W, H, du.DEFAULTS, ref)


def densify_batch(ctx, k):
    import opengpc_amd as g
    value, level = dense_want(k)
    return Spec("densify_batch_device", image_inputs(k), dict(value=B * H * W * 4, level=B * H * W, cnt=B * 4, nc=B * 8),
                dict(value=value, level=level, cnt=sup_in(k)[1], nc=match("pairs", k)[1]),
                [lambda c, p: c.densify_batch_device(p["L"], p["R"], W, H, B, settings(), g.Densify(), p["value"], p["level"], RADIUS, p["cnt"],
                                                     p["nc"])], forest="zero")


def clean_batch(ctx, k):
    import opengpc_amd as g
    (rec, cnt), ref = sup_in(k), ref_in(k)
    fwd, level = dense_want(k)
    r_rec, r_ref = cu.flip(rec, cnt, ref, rec, ref)
    bwd, _ = du.densify(r_rec, cnt, W, H, du.DEFAULTS, r_ref)
    out, state, label, stats = cu.clean(fwd, bwd, cu.DEFAULTS)
    assert (stats[:, 0] > 0).all()
    return Spec("clean_batch_device", image_inputs(k),
                dict(out=B * H * W * 4, state=B * H * W, label=B * H * W * 4, stats=B * 16, fwd=B * H * W * 4, level=B * H * W, cnt=B * 4, nc=B * 8),
                dict(out=out, state=state, label=label, stats=stats, fwd=fwd, level=level, cnt=cnt, nc=match("pairs", k)[1]),
                [lambda c, p: c.clean_batch_device(p["L"], p["R"], W, H, B, settings(), g.Densify(), g.Clean(), p["out"], p["state"], p["label"],
                                                   p["stats"], p["fwd"], p["level"], RADIUS, p["cnt"], p["nc"])], forest="zero")


IMAGE_FORMS = {
    "match_batch_epipolar": match_batch("zero", True, False), "match_batch_global": match_batch("zero", False, False),
    "match_batch_hashtable": match_batch("zero", True, True),
    "match_batch_epipolar_tau": match_batch("tau", True, False), "match_batch_global_tau": match_batch("tau", False, False),
    "match_batch_hashtable_tau": match_batch("tau", True, True),
    "match_batch_packed": match_batch_packed, "match_sequence": match_sequence, "match_stereo_sequence": match_stereo_sequence,
    "score_batch": score_batch, "track_sequence": track_sequence, "stream_push": stream_push, "consensus_batch": consensus_batch,
    "refine_batch": refine_batch, "pyramid_batch": pyramid_batch, "densify_batch": densify_batch, "clean_batch": clean_batch,
    "quads_sequence": quads_sequence,
}


def measure():
    """python tests/stream_order_util.py: the figures behind DELAY_CYCLES (docs/HISTORY.md, section 8), on the GPU at hand:
    what torch.cuda._sleep takes per 10^6 ticks, and the host-side duration of the warmed calls of every case"""
    import sys
    import time
    sys.path.insert(0, ROOT)
    import torch
    torch.cuda.init()
    import opengpc_amd as g
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    for cycles in (1_000_000, 10_000_000, 10_000_000):                       # (the first launch pays for the code object)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sleep(st, cycles)
        st.synchronize()
        print("_sleep: %.3f ms per 10^6 ticks" % ((time.perf_counter() - t0) * 1e9 / cycles))
    c = g.Context(0)
    c.set_stream(st.cuda_stream)
    timings = {}
    try:
        for forms in (RECORD_FORMS, IMAGE_FORMS):
            for name in sorted(forms):
                for _ in range(2):
                    t = {}
                    run(c, st, [forms[name](c, 0)], timings=t)
                    for k, v in t.items():
                        timings[k] = max(timings.get(k, 0.0), v)
    finally:
        st.synchronize()
        c.set_stream(None)
        c.close()
    for k, v in timings.items():
        print("%-60s %.4f ms" % (k, v * 1e3))
    print("longest: %.4f ms; DELAY_CYCLES = %d" % (max(timings.values()) * 1e3, DELAY_CYCLES))


if __name__ == "__main__":
    measure()
