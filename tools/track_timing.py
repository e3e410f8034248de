"""Linking a sequence's matches into tracks on the device (gpc_hip_track_*) against what it replaces: the records' way
over the host link.

Cases: 33 frames of 1024x436 and 9 frames of 1920x1080 (zero forest, frames moving in x and y), each with the non-epipolar
sort matcher and with the hash-table matcher.  For each, one JSON object:
  * match_us / track_us / link_only_us: a warmed match_sequence_device call, the track_sequence_device call on the same
    frames, and track_records_device over the records the former left; HIP events around `iters` calls, median and
    min .. max of `reps` repetitions;
  * kernels_us: per-kernel us per call (gpc_hip_kernel_time) of the track call, the six k_track_* kernels among them;
  * bytes: each linking kernel's compulsory bytes (R records, n tracks, P pairs of W x H):
      fill 4 W H (P-1);  scatter 16 R + 4 R (pred) + 4 R' (plane, R' = records of pairs 1 ..);  link 16 R + 4 R + 4 R + 4 R;
      settle 12 R;  walk 12 R + 16 n;  scan 8 per chunk
    with the rate they imply and their time at the device copy rate measured in the same run;
  * link: 16 B x records / the page-locked device-to-host rate measured in the same run.  The derived condition is
    sum of the k_track_* kernels < that time.
usage: python tools/track_timing.py [--iters N] [--reps N] [--out FILE] [--only NAME]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from score_timing import copy_rates, events_us, kernel_us  # noqa: E402
from sequence_timing import frames_of  # noqa: E402  (the frames of DESIGN.md 4.7's cases)

TRACK_KERNELS = ("k_track_fill", "k_track_scatter", "k_track_link", "k_track_settle", "k_track_scan", "k_track_walk")


def case(g, torch, name, W, H, N, hashtable, iters, reps, rates):
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    P, cap = N - 1, (W - 26) * (H - 26) + 1
    s = g.Settings(5, 128, 0, False, hashtable, 1)
    d_f = torch.from_numpy(frames_of(W, H, N, N)).to(dev)
    d_out = torch.empty((P, cap, 4), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    d_next = torch.empty((P, cap), dtype=torch.int32, device=dev)
    d_id = torch.empty((P, cap), dtype=torch.int32, device=dev)
    d_tab = torch.empty((P * cap, 4), dtype=torch.int32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    match = lambda: ctx.match_sequence_device(d_f.data_ptr(), W, H, N, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), 0)
    track = lambda: ctx.track_sequence_device(d_f.data_ptr(), W, H, N, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), 0,
                                              d_next.data_ptr(), d_id.data_ptr(), d_tab.data_ptr(), P * cap, d_n.data_ptr())
    link = lambda: ctx.track_records_device(d_out.data_ptr(), cap, d_cnt.data_ptr(), W, H, P, d_next.data_ptr(), d_id.data_ptr(),
                                            d_tab.data_ptr(), P * cap, d_n.data_ptr())
    torch.cuda.synchronize(dev)
    res = {"case": name, "width": W, "height": H, "frames": N, "matcher": "hashtable" if hashtable else "sort"}
    res["match_us"] = events_us(torch, ctx, match, iters, reps)
    res["track_us"] = events_us(torch, ctx, track, iters, reps)
    res["link_only_us"] = events_us(torch, ctx, link, iters, reps)
    kt, names = kernel_us(ctx, track, iters)
    res["kernels_us"] = kt
    cnt = d_cnt.cpu().numpy().astype(np.int64)
    R, R1, n = int(cnt.sum()), int(cnt[1:].sum()), int(d_n.cpu().numpy()[0])
    tab = d_tab[:n].cpu().numpy()
    res["records"], res["tracks"] = R, n
    res["length_histogram"] = {str(k): int(v) for k, v in zip(*np.unique(tab[:, 2], return_counts=True))}
    nchunk = (cap + 2047) // 2048
    b = {"k_track_fill": 4 * W * H * (P - 1), "k_track_scatter": 20 * R + 4 * R1, "k_track_link": 28 * R,
         "k_track_settle": 12 * R, "k_track_scan": 8 * nchunk * P, "k_track_walk": 12 * R + 16 * n}
    d2d, d2h = rates
    missing = [k for k in TRACK_KERNELS if not kt.get(k)]    # (kernel_us leaves out what was never launched; P > 1 here)
    if missing:
        raise RuntimeError("no time for %s" % ", ".join(missing))
    res["bytes"] = {k: {"bytes": v, "GBps": round(v / kt[k] / 1e3, 1), "at_copy_rate_us": round(v / d2d / 1e3, 1)}
                    for k, v in b.items()}
    res["copy_GBps"] = d2d
    link_us = 16 * R / d2h / 1e3
    total = sum(kt[k] for k in TRACK_KERNELS)
    res["link"] = {"d2h_GBps": d2h, "records_over_link_us": round(link_us, 1), "track_kernels_us": round(total, 1),
                   "margin": round(link_us / total, 1), "condition_met": bool(total < link_us)}
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
    rates = copy_rates(torch, torch.device("cuda", 0))
    out = []
    for name, W, H, N, ht in (("33 x 1024x436, sort", 1024, 436, 33, False), ("33 x 1024x436, hash table", 1024, 436, 33, True),
                              ("9 x 1920x1080, sort", 1920, 1080, 9, False), ("9 x 1920x1080, hash table", 1920, 1080, 9, True)):
        if a.only and a.only not in name:
            continue
        out.append(case(g, torch, name, W, H, N, ht, a.iters, a.reps, rates))
        print(json.dumps(out[-1], sort_keys=True), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
