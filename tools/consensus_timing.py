"""The consensus filter (gpc_hip_consensus_*) beside the match that produced its records.

Cases: 15 pairs of 1024x436 from match_sequence_device (16 frames moving in x and y, zero forest, non-epipolar sort matcher)
and 256 pairs of 1024x436 from match_batch_device (the benchmark's synthetic pairs, the reference's sparsematch settings).
For each, one JSON object:
  * match_us / filter_us: a warmed match call into an every-record array, and the records form of the filter over what it
    left (documented defaults: cell 16, shifts 4, alpha 6 / 1); HIP events around `iters` calls, median and min .. max of
    `reps` repetitions; ratio = filter / match (medians);
  * kernels_us: per-kernel us per filter call (gpc_hip_kernel_time): the six k_cons_* kernels, the first four launched once
    per grid; k_cons_scan's figure is the mean over BOTH of its uses (the histogram scan of each grid and the one scan of
    the chunk counts), which share one timing slot;
  * records / kept: the totals over the pairs;
  * precision (the sequence, whose frames are crops of one texture so that the true flow is known): the share of the
    judged records within 1 and 3 pixels of the truth (gpc_hip_score_correspondences_device) before and after the filter.
usage: python tools/consensus_timing.py [--iters N] [--reps N] [--out FILE] [--only NAME]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from score_timing import events_us, frames_of, kernel_us  # noqa: E402

CONS_KERNELS = ("k_cons_cells", "k_cons_scan", "k_cons_scatter", "k_cons_count", "k_cons_blocks", "k_cons_write")
THR = [1.0, 3.0]


def precision(g, torch, ctx, d_rec, cap, d_cnt, W, H, P, d_u, d_v):
    d_sc = torch.zeros((P, 15), dtype=torch.int64, device=d_rec.device)
    ctx.score_correspondences_device(d_rec.data_ptr(), cap, d_cnt.data_ptr(), W, H, P, d_u.data_ptr(), d_v.data_ptr(), 0, THR,
                                     d_sc.data_ptr())
    ctx.synchronize()
    sc = d_sc.cpu().numpy().copy().view(g.SCORE_DTYPE).reshape(-1)
    judged = int(sc["n_judged"].sum())
    return {"judged": judged, "within_1px": round(float(sc["n_within"][:, 0].sum()) / max(judged, 1), 4),
            "within_3px": round(float(sc["n_within"][:, 1].sum()) / max(judged, 1), 4)}


def case(g, torch, name, W, H, P, sequence, iters, reps):
    from opengpc_amd.synth import synth_batch
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    cap = (W - 26) * (H - 26) + 1
    prm = g.Consensus()
    words = 4 if sequence else 3
    d_rec = torch.empty((P, cap, words), dtype=torch.int32, device=dev)
    d_out = torch.empty((P, cap, words), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    d_n = torch.zeros(P, dtype=torch.int32, device=dev)
    if sequence:
        frames, flow = frames_of(W, H, P + 1, P + 1)
        d_f = torch.from_numpy(frames).to(dev)
        s = g.Settings(5, 128, 0, False, False, 1)
        match = lambda: ctx.match_sequence_device(d_f.data_ptr(), W, H, P + 1, s, d_rec.data_ptr(), cap, d_cnt.data_ptr(), 0)
    else:
        L, R = synth_batch(W, H, range(P))
        d_L, d_R = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
        s = g.Settings.sparsematch()
        match = lambda: ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, d_rec.data_ptr(), cap, d_cnt.data_ptr(), 0)
    filt = lambda: ctx.consensus_records_device(d_rec.data_ptr(), sequence, cap, d_cnt.data_ptr(), W, H, P, prm, 0, d_out.data_ptr(),
                                                cap, 0, d_n.data_ptr())
    torch.cuda.synchronize(dev)
    res = {"case": name, "width": W, "height": H, "pairs": P, "cell": prm.cell, "shifts": prm.shifts,
           "alpha": [prm.alpha_num, prm.alpha_den]}
    res["match_us"] = events_us(torch, ctx, match, iters, reps)
    res["filter_us"] = events_us(torch, ctx, filt, iters, reps)
    res["ratio_filter_to_match"] = round(res["filter_us"]["median"] / res["match_us"]["median"], 3)
    kt, names = kernel_us(ctx, filt, iters)
    res["kernels_us"] = {k: kt.get(k) for k in CONS_KERNELS}
    res["records"], res["kept"] = int(d_cnt.cpu().numpy().astype(np.int64).sum()), int(d_n.cpu().numpy().astype(np.int64).sum())
    if sequence:
        u = np.empty((P, H, W), np.float32)
        v = np.empty((P, H, W), np.float32)
        for t, (fx, fy) in enumerate(flow):
            u[t], v[t] = fx, fy
        d_u, d_v = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
        res["precision"] = {"before": precision(g, torch, ctx, d_rec, cap, d_cnt, W, H, P, d_u, d_v),
                            "after": precision(g, torch, ctx, d_out, cap, d_n, W, H, P, d_u, d_v)}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="run the cases whose name contains this")
    a = ap.parse_args()
    import torch
    import opengpc_amd as g
    out = []
    for name, P, sequence in (("15 pairs of 1024x436, match_sequence_device", 15, True),
                              ("256 pairs of 1024x436, match_batch_device", 256, False)):
        if a.only and a.only not in name:
            continue
        out.append(case(g, torch, name, 1024, 436, P, sequence, a.iters, a.reps))
        print(json.dumps(out[-1], sort_keys=True), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
