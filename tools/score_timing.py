"""Scoring on the device (gpc_hip_score_*) against what it replaces: the records' way over the host link.

Cases: the bench batch (256 pairs of 1024x436, zero forest, sparsematch settings, truth g = D), 32 such pairs, 8 pairs of
1920x1080, and a 33-frame sequence of 1024x436 (non-epipolar sort matcher, constant true flow).  For each, one JSON object:
  * match_us / score_us: a warmed match_batch_device (match_sequence_device) call and the score_batch_device
    (score_sequence_device) call on the same inputs, HIP events around `iters` calls each, median and min .. max of `reps`
    repetitions;
  * kernels_us: per-kernel us per call (gpc_hip_kernel_time) of the scoring call, k_score_records and k_score_matchable
    among them;
  * bytes: the compulsory bytes of the two scoring kernels (records x (12 | 16 B + 4 | 8 B of truth + 1 B of mask);
    per pair W*H*(4 | 8 + 1) B + both candidate images) and the rate they imply, beside 8 TB/s and the measured
    device copy rate;
  * link: 12 B (16 B) x records / the measured page-locked device-to-host rate: what copying the records out to score them
    on the host would cost.  The derived condition is score kernels' time < link time.
usage: python tools/score_timing.py [--iters N] [--reps N] [--out FILE] [--stats-csv FILE] [--only NAME]
(counters, in a run of their own: rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum
 --kernel-include-regex k_score_records -- python tools/score_timing.py --only sequence --iters 2 --reps 1)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames_of(W, H, N, seed):
    rng = np.random.default_rng(seed)
    BW, BH = W + 8 * N + 32, H + 40
    base = (rng.integers(0, 256, (BH // 4 + 1, BW // 4 + 1)).repeat(4, 0).repeat(4, 1)[:BH, :BW] * 3 // 4
            + rng.integers(0, 64, (BH, BW))).astype(np.uint8)
    out, at, x = [], [], 16 + 8 * N
    for _ in range(N):
        y = 20 + int(rng.integers(-12, 13))
        out.append(base[y:y + H, x:x + W])
        at.append((x, y))
        x -= int(rng.integers(1, 8))
    flow = [(at[t][0] - at[t + 1][0], at[t][1] - at[t + 1][1]) for t in range(N - 1)]
    return np.ascontiguousarray(np.stack(out)), flow


def events_us(torch, ctx, fn, iters, reps):
    for _ in range(3):
        fn()
    ctx.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        ctx.synchronize()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / iters)
    return {"median": round(float(np.median(out)), 1), "min": round(min(out), 1), "max": round(max(out), 1)}


def kernel_us(ctx, fn, iters):
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_timing()
    for _ in range(iters):
        fn()
    ctx.synchronize()
    kt = {k: round(1e3 * v[0] / v[1], 1) for k, v in ctx.kernel_times().items() if v[1]}
    names = {k: v for k, v in ctx.kernel_launch_names().items() if v}
    ctx.enable_kernel_timing(False)
    return kt, names


def copy_rates(torch, dev, nbytes=1 << 28):
    """(device-to-device copy, page-locked device-to-host copy) in GB/s; the copy counts read + written bytes once each"""
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    h = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    res = []
    for dst in (b, h):
        best = 1e30
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(a, non_blocking=True)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        res.append(nbytes / best / 1e6)
    return round(2 * res[0], 1), round(res[1], 1)


def case(g, torch, name, W, H, P, iters, reps, rates, sequence=False):
    from opengpc_amd.synth import synth_batch
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    cap = (W - 26) * (H - 26) + 1
    d_sc = torch.zeros((P, 15), dtype=torch.int64, device=dev)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    thr = [0.0, 1.0, 3.0]
    if sequence:
        s = g.Settings(5, 128, 0, False, False, 1)
        f, flow = frames_of(W, H, P + 1, P + 1)
        d_f = torch.from_numpy(f).to(dev)
        d_u = torch.from_numpy(np.stack([np.full((H, W), a, np.float32) for a, b in flow])).to(dev)
        d_v = torch.from_numpy(np.stack([np.full((H, W), b, np.float32) for a, b in flow])).to(dev)
        d_out = torch.empty((P, cap, 4), dtype=torch.int32, device=dev)
        match = lambda: ctx.match_sequence_device(d_f.data_ptr(), W, H, P + 1, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), 0)
        score = lambda: ctx.score_sequence_device(d_f.data_ptr(), W, H, P + 1, s, d_u.data_ptr(), d_v.data_ptr(), 0, thr,
                                                  d_sc.data_ptr())
        rec_bytes, truth_bytes = 16, 8
    else:
        s = g.Settings.sparsematch()
        idx = list(range(P))
        L, R = synth_batch(W, H, idx)
        d_L, d_R = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
        d_u = torch.from_numpy(np.stack([np.full((H, W), 8 + i % 64, np.float32) for i in idx])).to(dev)
        d_out = torch.empty((P, cap, 3), dtype=torch.int32, device=dev)
        match = lambda: ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), 0)
        score = lambda: ctx.score_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, d_u.data_ptr(), 0, thr, d_sc.data_ptr())
        rec_bytes, truth_bytes = 12, 4
    torch.cuda.synchronize(dev)
    res = {"case": name, "width": W, "height": H, "pairs": P}
    res["match_us"] = events_us(torch, ctx, match, iters, reps)
    res["score_us"] = events_us(torch, ctx, score, iters, reps)
    kt, names = kernel_us(ctx, score, iters)
    res["kernels_us"], res["launch_names"] = kt, names
    sc = d_sc.cpu().numpy().view(g.SCORE_DTYPE).reshape(-1)
    nrec = int(sc["n_records"].sum())
    res["records"], res["within"], res["matchable"] = nrec, [int(x) for x in sc["n_within"].sum(0)[:3]], int(sc["n_matchable"].sum())
    bits = names.get("k_score_matchable", "").endswith("true>")
    b_rec = nrec * (rec_bytes + truth_bytes)                     # (no ignore mask in these cases)
    b_mat = P * W * H * truth_bytes + P * 2 * W * H // (8 if bits else 1)
    d2d, d2h = rates
    res["bytes"] = {"records_pass": b_rec, "matchable_pass": b_mat,
                    "records_GBps": round(b_rec / kt["k_score_records"] / 1e3, 1),
                    "matchable_GBps": round(b_mat / kt["k_score_matchable"] / 1e3, 1),
                    "at_8TBps_us": [round(b_rec / 8e6, 1), round(b_mat / 8e6, 1)],
                    "at_copy_rate_us": [round(b_rec / d2d / 1e3, 1), round(b_mat / d2d / 1e3, 1)], "copy_GBps": d2d}
    link_us = nrec * rec_bytes / d2h / 1e3
    both = kt["k_score_records"] + kt["k_score_matchable"]
    res["link"] = {"d2h_GBps": d2h, "records_over_link_us": round(link_us, 1), "score_kernels_us": round(both, 1),
                   "margin": round(link_us / both, 1), "condition_met": bool(both < link_us)}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--only", default=None, help="run the cases whose name contains this (e.g. under rocprofv3 --pmc)")
    a = ap.parse_args()
    import torch
    import opengpc_amd as g
    rates = copy_rates(torch, torch.device("cuda", 0))
    out = []
    for name, W, H, P, seq in (("bench batch", 1024, 436, 256, False), ("32 pairs", 1024, 436, 32, False),
                               ("8 x 1920x1080", 1920, 1080, 8, False), ("33-frame sequence", 1024, 436, 32, True)):
        if a.only and a.only not in name:
            continue
        out.append(case(g, torch, name, W, H, P, a.iters, a.reps, rates, seq))
        print(json.dumps(out[-1], sort_keys=True), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")
    if a.stats_csv:
        with open(a.stats_csv, "w") as fo:
            fo.write("case,kernel,us_per_call\n")
            for r in out:
                for k, v in sorted(r["kernels_us"].items()):
                    fo.write("%s,%s,%s\n" % (r["case"], k, v))


if __name__ == "__main__":
    main()
