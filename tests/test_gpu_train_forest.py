"""gpc_hip_train_forest on the GPU: a whole forest trained over ONE resident training set, every fern's bootstrap a
multiplicity per triplet (opengpc_amd/csrc/k_train_forest.h), against the CPU oracle on a host gather.

One meaning, held by every case: fern f's parameters and per-level statistics are exactly what Fern::train gives for the
triplets t[draws[f]] with all marks cleared -- oracle.train_fern(t[draws[f]], zeros, ...).  Integers equal, doubles equal.

Shapes are the smallest at which the kernels take another path: n in {1, 255, 257, 1025, 4097} (one lane; the 256 padding
boundary from both sides; the 1024-triplet iteration boundary from both sides), 1 / 3 / 7 ferns, depth <= 4, <= 6 resamples.
The oracle's result per (n, draws, settings) is computed once per case; the device sets are made once per n and shared."""
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import SPLIT_DTYPE
from test_host_api import BIN, ROOT, compile_cpp
from test_training import make_triplets, stats_equal

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 257, 1025, 4097)


def cands(nferns, depth, nres, seed):
    """[nferns][depth][nres] hyperplanes, i != j like sampleHyperplane; the tau field is noise the call must ignore"""
    rng = np.random.default_rng(seed)
    c = np.zeros((nferns, depth, nres), SPLIT_DTYPE)
    c["i"] = rng.integers(0, 729, c.shape)
    c["j"] = (c["i"] + rng.integers(1, 729, c.shape)) % 729
    c["tau"] = rng.integers(-15, 16, c.shape)
    return c


def bootstrap(n, nferns, per_fern, seed):
    return np.random.default_rng(seed).integers(0, n, (nferns, per_fern)).astype(np.int32)


def oracle_forest(oracle, t, draws, cand, taulo, tauhi, only, w1):
    """the CPU oracle fern by fern on a host gather: [(params, stats)] per fern"""
    nferns, depth, nres = cand.shape
    out = []
    for f in range(nferns):
        sub = t if draws is None else np.ascontiguousarray(t[draws[f]])
        out.append(oracle.train_fern(sub, np.zeros(len(sub), np.uint8), depth, cand[f].reshape(-1), nres, taulo, tauhi,
                                     bool(only), w1))
    return out


def same(got, want):
    fp, st = got
    assert len(fp) == len(st) == len(want)
    for f, (wfp, wst) in enumerate(want):
        assert np.array_equal(fp[f], wfp), (f, fp[f], wfp)
        for level in range(len(wfp)):
            stats_equal(st[f][level], wst[level])


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets(ctx):
    """n -> (triplets, device set); made on first use, shared by every case of the module"""
    made = {}

    def get(n):
        if n not in made:
            t = make_triplets(n, 100 + n)
            made[n] = (t, ctx.train_set(t))
        return made[n]
    yield get
    for _, ts in made.values():
        ts.close()


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("nferns", [1, 3, 7])
@pytest.mark.parametrize("n", SIZES)
def test_every_size_and_fern_count(sets, oracle, n, nferns):
    t, ts = sets(n)
    cand = cands(nferns, 3, 5, 7 * n + nferns)
    draws = bootstrap(n, nferns, max(1, int(0.7 * n)), n + nferns)
    got = ts.train_forest(nferns, 3, cand, 5, -3, 4, True, 0.5, draws)
    same(got, oracle_forest(oracle, t, draws, cand, -3, 4, True, 0.5))


@pytest.mark.parametrize("w1", [0.5, 0.8])
@pytest.mark.parametrize("only", [0, 1])
@pytest.mark.parametrize("taulo,tauhi", [(0, 1), (-3, 4), (-32, 32)])
def test_optimizers(sets, oracle, taulo, tauhi, only, w1):
    n, nferns, depth, nres = 1025, 3, 4, 6
    t, ts = sets(n)
    cand = cands(nferns, depth, nres, 11 + tauhi)
    draws = bootstrap(n, nferns, int(0.7 * n), 12 + only)
    got = ts.train_forest(nferns, depth, cand, nres, taulo, tauhi, only, w1, draws)
    same(got, oracle_forest(oracle, t, draws, cand, taulo, tauhi, only, w1))


@pytest.mark.parametrize("kind", ["one", "bootstrap", "n", "2n"])
@pytest.mark.parametrize("n", SIZES)
def test_draws_per_fern(sets, oracle, n, kind):
    """1, int(0.7 n), n and 2 n draws per fern (oversampling is legal through the C ABI); zero and tau optimizer in turn"""
    import opengpc_amd as g
    t, ts = sets(n)
    per_fern = {"one": 1, "bootstrap": int(0.7 * n), "n": n, "2n": 2 * n}[kind]
    taulo, tauhi = ((0, 1), (-3, 4))[(n + len(kind)) % 2]
    cand = cands(3, 3, 4, n + len(kind))
    if per_fern == 0:  # int(0.7 * 1): no draws with a draws array is refused
        with pytest.raises(g.GpcError) as e:
            ts.train_forest(3, 3, cand, 4, taulo, tauhi, True, 0.5, np.zeros((3, 0), np.int32))
        assert e.value.status == g.capi.E_INVALID
        return
    draws = bootstrap(n, 3, per_fern, 5 * n + per_fern)
    got = ts.train_forest(3, 3, cand, 4, taulo, tauhi, True, 0.5, draws)
    same(got, oracle_forest(oracle, t, draws, cand, taulo, tauhi, True, 0.5))


@pytest.mark.parametrize("n", SIZES)
def test_no_draws_is_every_fern_on_the_whole_set(sets, oracle, n):
    """draws=None: each fern equals the existing TrainSet.train_fern on the same set with its marks cleared"""
    t, ts = sets(n)
    cand = cands(3, 4, 5, 3 * n)
    for only, (taulo, tauhi) in ((0, (0, 1)), (1, (-3, 4))):
        fp, st = ts.train_forest(3, 4, cand, 5, taulo, tauhi, only, 0.5)
        for f in range(3):
            ts.marks(np.zeros(n, np.uint8))
            wfp, wst = ts.train_fern(4, cand[f].reshape(-1), 5, taulo, tauhi, only, 0.5)
            assert np.array_equal(fp[f], wfp)
            for level in range(4):
                stats_equal(st[f][level], wst[level])
        same((fp, st), oracle_forest(oracle, t, None, cand, taulo, tauhi, only, 0.5))
    ts.marks(np.zeros(n, np.uint8))


def test_equals_train_fern_on_the_gathered_set(ctx, sets):
    """the path this call replaces: t[draws[f]] uploaded as a set of its own and trained by gpc_hip_train_fern"""
    n = 1025
    t, ts = sets(n)
    cand = cands(3, 4, 6, 41)
    draws = bootstrap(n, 3, int(0.7 * n), 42)
    fp, st = ts.train_forest(3, 4, cand, 6, -3, 4, True, 0.8, draws)
    for f in range(3):
        gathered = ctx.train_set(np.ascontiguousarray(t[draws[f]]))
        wfp, wst = gathered.train_fern(4, cand[f].reshape(-1), 6, -3, 4, True, 0.8)
        gathered.close()
        assert np.array_equal(fp[f], wfp)
        for level in range(4):
            stats_equal(st[f][level], wst[level])


# ------------------------------------------------------------------------------------------------ multiplicity edges
def test_one_triplet_drawn_255_times_is_exact(sets, oracle):
    n = 257
    t, ts = sets(n)
    cand = cands(2, 3, 5, 51)
    draws = np.stack([np.concatenate([np.full(255, 5), np.arange(100, 200)]),
                      np.concatenate([np.arange(156, 256), np.full(255, 256)])]).astype(np.int32)
    for taulo, tauhi in ((0, 1), (-3, 4)):
        got = ts.train_forest(2, 3, cand, 5, taulo, tauhi, True, 0.5, draws)
        want = oracle_forest(oracle, t, draws, cand, taulo, tauhi, True, 0.5)
        same(got, want)
        assert int(want[0][1][0]["tot"]) == 355   # every draw counts, the 255 copies among them


def test_one_triplet_drawn_256_times_is_refused(ctx, sets, oracle):
    """documented in include/gpc_hip.h: above 255 copies the call returns GPC_E_UNSUPPORTED before it launches anything;
    the context and the set go on working"""
    import opengpc_amd as g
    n = 257
    t, ts = sets(n)
    cand = cands(2, 3, 5, 52)
    draws = np.stack([np.arange(356) % n, np.concatenate([np.full(256, 5), np.arange(100, 200)])]).astype(np.int32)
    with pytest.raises(g.GpcError) as e:
        ts.train_forest(2, 3, cand, 5, 0, 1, True, 0.5, draws)
    assert e.value.status == g.capi.E_UNSUPPORTED
    draws[1, 0] = 6  # 255 copies
    same(ts.train_forest(2, 3, cand, 5, 0, 1, True, 0.5, draws), oracle_forest(oracle, t, draws, cand, 0, 1, True, 0.5))


def test_a_fern_whose_draws_all_name_one_triplet(sets, oracle):
    n = 1025
    t, ts = sets(n)
    cand = cands(2, 3, 5, 53)
    draws = np.stack([np.full(200, 1024), np.full(200, 0)]).astype(np.int32)
    for taulo, tauhi in ((0, 1), (-32, 32)):
        want = oracle_forest(oracle, t, draws, cand, taulo, tauhi, True, 0.5)
        same(ts.train_forest(2, 3, cand, 5, taulo, tauhi, True, 0.5, draws), want)
        assert int(want[0][1][0]["tot"]) == 200


def test_same_candidates_other_draws_differ_where_the_oracle_says(sets, oracle):
    """two ferns with identical hyperplanes and different bootstraps; the seed is chosen here, on the CPU, as the first for
    which the oracle's two ferns do differ in their parameters, so the case cannot pass by both ferns being one"""
    n = 255
    t, ts = sets(n)
    one = cands(1, 4, 6, 54)
    cand = np.concatenate([one, one])
    for seed in range(200):
        draws = bootstrap(n, 2, int(0.7 * n), 1000 + seed)
        want = oracle_forest(oracle, t, draws, cand, -3, 4, True, 0.5)
        if not np.array_equal(want[0][0], want[1][0]):
            break
    else:
        pytest.fail("no seed separates the two ferns")
    fp, st = ts.train_forest(2, 4, cand, 6, -3, 4, True, 0.5, draws)
    same((fp, st), want)
    assert not np.array_equal(fp[0], fp[1])


# ------------------------------------------------------------------------------------------------ independence
def test_a_fern_does_not_depend_on_its_neighbours_or_on_the_grouping(sets, oracle):
    """fern f alone, the ferns permuted, and the ferns split into groups of 3 (GPC_HIP_TRAIN_GROUP) give fern f the same
    result; the set's own marks, preset to a pattern, are what they were"""
    import opengpc_amd as g
    from devicewide_util import make_ctx
    n, nferns, depth, nres = 1025, 7, 3, 5
    t, ts = sets(n)
    cand = cands(nferns, depth, nres, 61)
    draws = bootstrap(n, nferns, int(0.7 * n), 62)
    marks = np.random.default_rng(63).integers(0, 4, n).astype(np.uint8)
    assert np.array_equal(ts.marks(marks), marks)
    fp, st = ts.train_forest(nferns, depth, cand, nres, -3, 4, True, 0.5, draws)
    same((fp, st), oracle_forest(oracle, t, draws, cand, -3, 4, True, 0.5))
    perm = np.random.default_rng(64).permutation(nferns)
    pfp, pst = ts.train_forest(nferns, depth, cand[perm], nres, -3, 4, True, 0.5, draws[perm])
    assert np.array_equal(pfp, fp[perm]) and np.array_equal(pst, st[perm])
    for f in (0, 4, 6):
        ofp, ost = ts.train_forest(1, depth, cand[f:f + 1], nres, -3, 4, True, 0.5, draws[f:f + 1])
        assert np.array_equal(ofp[0], fp[f]) and np.array_equal(ost[0], st[f])
    assert np.array_equal(ts.marks(), marks)
    ts.marks(np.zeros(n, np.uint8))
    grouped = make_ctx({"GPC_HIP_TRAIN_GROUP": 3})
    try:
        gts = grouped.train_set(t)
        gfp, gst = gts.train_forest(nferns, depth, cand, nres, -3, 4, True, 0.5, draws)
        assert np.array_equal(gfp, fp) and np.array_equal(gst, st)
        # the multiplicities of EVERY group are checked before the first group is launched
        many = draws.copy()
        many[6, :256] = 9
        with pytest.raises(g.GpcError) as e:
            gts.train_forest(nferns, depth, cand, nres, -3, 4, True, 0.5, many)
        assert e.value.status == g.capi.E_UNSUPPORTED
    finally:
        grouped.close()


# ------------------------------------------------------------------------------------------------ errors
def test_bad_arguments_are_refused_before_anything_runs(ctx, sets, oracle):
    """argument checks only: every call returns before a launch, and the context works afterwards"""
    import ctypes as C
    import opengpc_amd as g
    from opengpc_amd.capi import STATS_DTYPE, _ptr
    n = 257
    t, ts = sets(n)
    cand = cands(2, 3, 4, 71)
    draws = bootstrap(n, 2, 100, 72)

    def status(**kw):
        a = dict(nferns=2, depth=3, cand=cand, nres=4, taulo=0, tauhi=1, draws=draws, per_fern=100,
                 fp=np.zeros((2, 3), SPLIT_DTYPE), st=np.zeros((2, 3), STATS_DTYPE))
        a.update(kw)
        return ctx.L.gpc_hip_train_forest(ctx.h, ts.h, a["nferns"], a["depth"], _ptr(a["cand"]), a["nres"], a["taulo"],
                                          a["tauhi"], 1, C.c_double(0.5), _ptr(a["draws"]), a["per_fern"], _ptr(a["fp"]),
                                          _ptr(a["st"]))

    assert status() == g.capi.OK
    for at, value in ((0, n), (150, -1), (199, 2 ** 31 - 1)):
        bad = draws.copy()
        bad.reshape(-1)[at] = value
        assert status(draws=bad) == g.capi.E_INVALID, (at, value)
    assert status(nferns=0) == g.capi.E_INVALID
    assert status(depth=0) == g.capi.E_INVALID
    assert status(per_fern=0) == g.capi.E_INVALID
    assert status(fp=None) == g.capi.E_INVALID and status(st=None) == g.capi.E_INVALID and status(cand=None) == g.capi.E_INVALID
    outside = cand.copy()
    outside["j"][1, 2, 3] = 729
    assert status(cand=outside) == g.capi.E_INVALID
    assert ctx.L.gpc_hip_train_forest(ctx.h, None, 2, 3, _ptr(cand), 4, 0, 1, 1, C.c_double(0.5), None, 0, None, None) == g.capi.E_INVALID
    deep = cands(2, 65, 1, 73)
    assert status(depth=65, cand=deep, nres=1, fp=np.zeros((2, 65), SPLIT_DTYPE), st=np.zeros((2, 65), STATS_DTYPE)) == g.capi.E_UNSUPPORTED
    assert status(taulo=-32, tauhi=33) == g.capi.E_UNSUPPORTED
    # nothing to evaluate: zeros, as Fern::train leaves them
    fp, st = ts.train_forest(2, 3, cand, 4, 2, 2, True, 0.5, draws)
    assert not fp["i"].any() and not fp["j"].any() and not st["tot"].any()
    same(ts.train_forest(2, 3, cand, 4, 0, 1, True, 0.5, draws), oracle_forest(oracle, t, draws, cand, 0, 1, True, 0.5))


# ------------------------------------------------------------------------------------------------ who frees what
def test_workspaces_are_released_before_the_call_returns():
    """in the style of tests/test_gpu_resources.py: after train_forest nothing but the set is held, and after ctx.close()
    the counts of gpc_hip_debug_live_resources are back where they were"""
    import gc
    import opengpc_amd as g
    from opengpc_amd.capi import live_resources

    def live():
        gc.collect()
        return live_resources()
    before = live()
    ctx = g.Context(0)
    try:
        t = make_triplets(1025, 81)
        ts = ctx.train_set(t)
        ts.train_fern(2, cands(1, 2, 3, 82).reshape(-1), 3, 0, 1, True, 0.5)  # (the set's own scratch exists from here on)
        held = live()
        assert any(a > b for a, b in zip(held, before))
        ts.train_forest(3, 3, cands(3, 3, 4, 83), 4, -3, 4, True, 0.5, bootstrap(1025, 3, 700, 84))
        assert live() == held
        with pytest.raises(g.GpcError):
            ts.train_forest(1, 3, cands(1, 3, 4, 85), 4, 0, 1, True, 0.5, np.full((1, 300), 3, np.int32))
        assert live() == held
    finally:
        ctx.close()
    assert live() == before, "left behind (device blocks, device bytes, page-locked blocks, streams + events)"


def test_timing_slots_of_the_new_kernels(ctx, sets):
    n = 1025
    t, ts = sets(n)
    ctx.enable_kernel_timing(True)
    try:
        ctx.reset_kernel_timing()
        ts.train_forest(3, 3, cands(3, 3, 4, 91), 4, -3, 4, True, 0.5, bootstrap(n, 3, 700, 92))
        times = ctx.kernel_times()
    finally:
        ctx.enable_kernel_timing(False)
    assert [times[k][1] for k in ("k_tf_begin", "k_tf_eval", "k_tf_tot", "k_tf_commit")] == [1, 3, 3, 2]
    assert times["k_train_eval"][1] == 0


# ------------------------------------------------------------------------------------------------ the C++ overload
@pytest.fixture(scope="module")
def forest_bin():
    from opengpc_amd import build
    build.build()
    return compile_cpp(os.path.join(ROOT, "tests", "cpp", "train_forest_check.cpp"), os.path.join(BIN, "train_forest_check"))


@pytest.mark.parametrize("taulo,tauhi,only", [(0, 1, 1), (-2, 3, 0)])
def test_cpp_forest_over_a_device_set(forest_bin, tmp_path, oracle, taulo, tauhi, only):
    """Forest::trainAndExport(DeviceTrainingSet&, ...): the exported parameters equal the oracle's, fern by fern, for the
    hyperplanes and bootstraps the run dumped; a second run with the same seeds writes the same file; the file reads back"""
    n, depth, nres, w1 = 2000, 3, 4, 0.5
    t = make_triplets(n, 5)
    path = str(tmp_path / "triplets.bin")
    t.tofile(path)
    outs = []
    for run in range(2):
        fpath, cdump, ddump = (str(tmp_path / ("%s%d.txt" % (k, run))) for k in ("forest", "cand", "draws"))
        env = dict(os.environ, GPC_TRAIN_DUMP_CANDIDATES=cdump, GPC_TRAIN_DUMP_DRAWS=ddump)
        out = subprocess.run([forest_bin, path, fpath, "17", "23", str(taulo), str(tauhi), str(only), str(w1)], check=True,
                             capture_output=True, text=True, env=env).stdout
        outs.append((out, open(fpath).read(), open(cdump).read(), open(ddump).read()))
    out, text, cdump, ddump = outs[0]
    assert outs[1][1:] == (text, cdump, ddump)
    assert "SIZE 2000" in out and "Fern(3/3) num samples:1400" in out and "Exporting forest" in out
    assert out.count("ERR: Training set is empty. Aborting.") == 1 and not os.path.exists(str(tmp_path / "forest0.txt.none"))
    ij = np.array(cdump.split(), np.int32).reshape(3, depth, nres, 2)
    cand = np.zeros((3, depth, nres), SPLIT_DTYPE)
    cand["i"], cand["j"] = ij[..., 0], ij[..., 1]
    draws = np.array(ddump.split(), np.int32).reshape(3, 1400)
    assert draws.min() >= 0 and draws.max() < 1400     # the reference draws from the first sampleFraction * N triplets
    want = oracle_forest(oracle, t, draws, cand, taulo, tauhi, only, w1)
    words = text.split()
    assert words[0] == "3"
    at = 1
    for f, scale in enumerate("sml"):
        assert words[at:at + 3] == [str(f), scale, str(depth)]
        at += 3
        for level in range(depth):
            i, j, tau = (int(want[f][0][k][level]) for k in ("i", "j", "tau"))
            assert [int(w) for w in words[at:at + 6]] == [level, i % 27 - 13, i // 27 - 13, j % 27 - 13, j // 27 - 13, tau]
            at += 6
    assert at == len(words)
    # the tables the run printed carry the oracle's per-level statistics, fern after fern
    table = [l.split() for l in out.splitlines() if l.split() and l.split()[0].isdigit() and len(l.split()) == 12]
    assert len(table) == 3 * depth
    for k, row in enumerate(table):
        s = want[k // depth][1][k % depth]
        assert [int(v) for v in row[4:8]] == [s["tot"], s["tp"], s["fp"], s["fn"]]
    rc, f = oracle.read_forest(str(tmp_path / "forest0.txt"), 1024, 436)
    taus = np.concatenate([w[0]["tau"] for w in want])
    assert rc == 0 and f.num_tests == 9 and f.type == int(taus.any())
