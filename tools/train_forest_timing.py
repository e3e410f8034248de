#!/usr/bin/env python3
"""Times forest training over ONE resident set (gpc_hip_train_forest) against the path it replaces, in the same process
on one MI355X, for the settings of samples/train.cpp: six ferns, depth 5, 10 resamples, 70 % bootstraps drawn from the
first 70 % of the set, zero and tau (-10 .. 10) optimizer, 2^18 synthetic triplets built as in tools/train_bench.py.

Per optimizer, each leg the median of five repetitions after one warm-up (host clock around synchronous calls):
  * forest_resident_ms      train_forest with the set already on the device;
  * forest_with_upload_ms   one upload (ctx.train_set) + train_forest + release;
  * per_fern_path_ms        per fern: host gather of its bootstrap, ctx.train_set of the copy, train_fern, release -- with
                            its parts.  (The C++ host-vector overload copies every bootstrap TWICE on the host before the
                            upload; this leg copies it once, so it flatters the old path.)
  * speedup_resident / speedup_with_upload = per_fern_path_ms over the two new legs.
Kernel times (HIP events, in runs of their own, not inside the legs above), per level:
  * k_tf_eval_ms_per_level                  one launch for all six ferns over the resident set and the multiplicities;
  * k_train_eval_six_gathered_ms_per_level  six launches of the existing kernel, one per gathered bootstrap (0.7 x the rows);
  * k_train_eval_six_resident_ms_per_level  six launches of the existing kernel over the whole resident set.
The two paths' parameters and statistics are compared (they must be equal) before anything is written.
Output: train_forest_timing.json in $BENCH_OUT (default bench_out/) and a copy in profiles/train_forest_timing.json.
The run ends itself after --limit seconds (default 540)."""
import argparse
import json
import os
import shutil
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import opengpc_amd as g  # noqa: E402
from opengpc_amd.capi import SPLIT_DTYPE  # noqa: E402

NFERNS, DEPTH, NRES, FRACTION, REPS = 6, 5, 10, 0.7, 5


def median_ms(fn):
    fn()  # warm-up
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 3), [round(v, 3) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triplets", type=int, default=1 << 18)
    ap.add_argument("--limit", type=int, default=540)
    a = ap.parse_args()
    signal.alarm(a.limit)
    n = a.triplets
    rng = np.random.default_rng(7)
    t = rng.integers(0, 256, (n, 3, 729), dtype=np.uint8)
    t[:, 1] = t[:, 0] ^ rng.integers(0, 4, (n, 729), dtype=np.uint8)  # pos ~ ref
    per_fern = int(FRACTION * n)
    draws = rng.integers(0, per_fern, (NFERNS, per_fern)).astype(np.int32)  # training.hpp:113-121
    cand = np.zeros((NFERNS, DEPTH, NRES), SPLIT_DTYPE)
    cand["i"] = rng.integers(0, 729, cand.shape)
    cand["j"] = (cand["i"] + rng.integers(1, 729, cand.shape)) % 729
    ctx = g.Context(0)
    ts = ctx.train_set(t)
    res = {"triplets": n, "set_bytes": int(t.nbytes), "ferns": NFERNS, "depth": DEPTH, "resamples": NRES,
           "draws_per_fern": per_fern, "repetitions": REPS, "runs": []}
    for name, taulo, tauhi in (("zero optimizer", 0, 1), ("tau optimizer", -10, 10)):
        args = (NRES, taulo, tauhi, False, 0.5)
        parts = {"gather": [], "upload": [], "train_fern": []}

        def forest():
            return ts.train_forest(NFERNS, DEPTH, cand, *args, draws)

        def forest_with_upload():
            s = ctx.train_set(t)
            s.train_forest(NFERNS, DEPTH, cand, *args, draws)
            s.close()

        def per_fern_path(keep=None):
            for f in range(NFERNS):
                t0 = time.perf_counter()
                sub = np.ascontiguousarray(t[draws[f]])
                t1 = time.perf_counter()
                s = ctx.train_set(sub)
                t2 = time.perf_counter()
                out = s.train_fern(DEPTH, cand[f].reshape(-1), *args)
                t3 = time.perf_counter()
                s.close()
                parts["gather"].append(t1 - t0), parts["upload"].append(t2 - t1), parts["train_fern"].append(t3 - t2)
                if keep is not None:
                    keep.append(out)

        # the two paths compute the same forest
        old = []
        per_fern_path(old)
        fp, st = forest()
        equal = all(np.array_equal(fp[f], old[f][0]) and np.array_equal(st[f], old[f][1]) for f in range(NFERNS))
        assert equal, "the forest call and the per-fern path disagree"
        for v in parts.values():
            v.clear()
        run = {"config": name, "taus": tauhi - taulo, "results_equal": equal}
        run["forest_resident_ms"], run["forest_resident_all"] = median_ms(forest)
        run["forest_with_upload_ms"], run["forest_with_upload_all"] = median_ms(forest_with_upload)
        run["per_fern_path_ms"], run["per_fern_path_all"] = median_ms(per_fern_path)
        calls = len(parts["gather"]) // NFERNS
        run["per_fern_path_parts_ms"] = {k: round(sum(v) / calls * 1e3, 3) for k, v in parts.items()}
        run["speedup_resident"] = round(run["per_fern_path_ms"] / run["forest_resident_ms"], 2)
        run["speedup_with_upload"] = round(run["per_fern_path_ms"] / run["forest_with_upload_ms"], 2)
        # kernel times, in runs of their own
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_timing()
        forest()
        ms, launches = ctx.kernel_times()["k_tf_eval"]
        run["k_tf_eval_ms_per_level"] = round(ms / launches, 4)
        run["k_tf_other_ms_per_call"] = {k: round(ctx.kernel_times()[k][0], 4) for k in ("k_tf_begin", "k_tf_tot", "k_tf_commit")}
        ctx.reset_kernel_timing()
        per_fern_path()
        ms, launches = ctx.kernel_times()["k_train_eval"]
        run["k_train_eval_six_gathered_ms_per_level"] = round(ms / launches * NFERNS, 4)
        ctx.reset_kernel_timing()
        for f in range(NFERNS):
            ts.train_fern(DEPTH, cand[f].reshape(-1), *args)
        ms, launches = ctx.kernel_times()["k_train_eval"]
        run["k_train_eval_six_resident_ms_per_level"] = round(ms / launches * NFERNS, 4)
        ctx.enable_kernel_timing(False)
        ctx.reset_kernel_timing()
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    ts.close()
    ctx.close()
    out = os.path.join(os.environ.get("BENCH_OUT", os.path.join(ROOT, "bench_out")), "train_forest_timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    shutil.copyfile(out, os.path.join(ROOT, "profiles", "train_forest_timing.json"))


if __name__ == "__main__":
    main()
