"""Frame sequences (gpc_hip_match_sequence[_device]) against the batch entry points over the expanded pairs.

Cases: 33 frames of 1024x436 and 9 frames of 1920x1080 (crops of one texture moving in x and y), the non-epipolar sort
matcher and the hash-table matcher (epipolar_mode = 0).  For each, one JSON object with
  * device: a warmed match_sequence_device call against match_batch_device over rawL = f[:-1], rawR = f[1:] (same
    settings; its records are 12-byte supports, the sequence's 16-byte correspondences), HIP events around `iters`
    calls, and the per-kernel us per call (gpc_hip_kernel_time) of both;
  * host: match_sequence (pageable frames) against match_batch on the same expanded pairs, wall clock per call.
usage: python tools/sequence_timing.py [--iters N] [--out FILE] [--no-host]
(per-kernel times under the profiler: rocprofv3 --kernel-trace --stats -- python tools/sequence_timing.py --no-host)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames_of(W, H, N, seed):
    rng = np.random.default_rng(seed)
    BW, BH = W + 8 * N + 32, H + 40
    base = (rng.integers(0, 256, (BH // 4 + 1, BW // 4 + 1)).repeat(4, 0).repeat(4, 1)[:BH, :BW] * 3 // 4
            + rng.integers(0, 64, (BH, BW))).astype(np.uint8)
    out, x = [], 16
    for _ in range(N):
        y = 20 + int(rng.integers(-12, 13))
        out.append(base[y:y + H, x:x + W])
        x += int(rng.integers(1, 8))
    return np.ascontiguousarray(np.stack(out))


def timed(torch, ctx, fn, iters):
    for _ in range(3):
        fn()
    ctx.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    ctx.synchronize()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_timing()
    for _ in range(iters):
        fn()
    ctx.synchronize()
    kt = {k: round(1e3 * v[0] / v[1], 1) for k, v in ctx.kernel_times().items() if v[1]}
    names = {k: v for k, v in ctx.kernel_launch_names().items() if v}
    ctx.enable_kernel_timing(False)
    return {"us_per_call": round(1e3 * ms, 1), "kernels_us": kt, "launch_names": names}


def case(g, torch, W, H, N, hashtable, iters, host):
    dev = torch.device("cuda", 0)
    s = g.Settings(5, 128, 0, False, hashtable, 1)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    f = frames_of(W, H, N, N)
    P = N - 1
    cap = (W - 26) * (H - 26)
    d_f = torch.from_numpy(f).to(dev)
    d_L, d_R = d_f[:-1].contiguous(), d_f[1:].contiguous()
    d_corr = torch.empty((P, cap, 4), dtype=torch.int32, device=dev)
    d_supp = torch.empty((P, cap, 3), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    d_nc = torch.zeros(N, dtype=torch.int32, device=dev)
    d_nc2 = torch.zeros((P, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    res = {"width": W, "height": H, "frames": N, "pairs": P, "matcher": "hashtable" if hashtable else "sort"}
    res["sequence_device"] = timed(torch, ctx, lambda: ctx.match_sequence_device(
        d_f.data_ptr(), W, H, N, s, d_corr.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr()), iters)
    seq_counts = d_cnt.cpu().numpy().copy()
    res["batch_device"] = timed(torch, ctx, lambda: ctx.match_batch_device(
        d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, d_supp.data_ptr(), cap, d_cnt.data_ptr(), d_nc2.data_ptr()), iters)
    res["records"] = int(seq_counts.sum())
    res["device_ratio"] = round(res["sequence_device"]["us_per_call"] / res["batch_device"]["us_per_call"], 3)
    if host:
        L, R = np.ascontiguousarray(f[:-1]), np.ascontiguousarray(f[1:])
        for name, fn in (("sequence_host", lambda: ctx.match_sequence(f, s, cap)),
                         ("batch_host", lambda: ctx.match_batch(L, R, s, cap))):
            fn()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            res[name] = {"ms_per_call": round(1e3 * (time.perf_counter() - t0) / iters, 3)}
        res["host_ratio"] = round(res["sequence_host"]["ms_per_call"] / res["batch_host"]["ms_per_call"], 3)
        res["upload_bytes"] = {"sequence": int(f.nbytes), "batch": int(L.nbytes + R.nbytes)}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    import opengpc_amd as g
    out = []
    for W, H, N in ((1024, 436, 33), (1920, 1080, 9)):
        for hashtable in (False, True):
            out.append(case(g, torch, W, H, N, hashtable, a.iters, not a.no_host))
            print(json.dumps(out[-1], sort_keys=True), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
