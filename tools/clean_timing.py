"""The field cleaner (gpc_hip_clean_*) in one run on one card: gpc_hip_clean_fields_device over the fields of real match
output, per kernel, beside the fill that made those fields.

Cases: 16 pairs of 1024x436 with the zero forest, sparsematch settings, the documented fill and clean parameters: C = 1
(the benchmark's synthetic stereo pairs) and C = 2 (a sequence of 17 frames that alternates the two images of one pair, so
that every step moves by the pair's disparity).  The forward and backward fields are made once by the records forms
(gpc_hip_densify_*_device, gpc_hip_flip_*_device); then, for each case, one JSON object:
  * clean_us / fill_us: warmed calls; HIP events around `iters` calls, median and min .. max of `reps` repetitions.  fill =
    the records form of the densifier over the same records (what tools/dense_timing.py reports as fill_us, here at 16 pairs
    and in the same run);
  * kernel_us_per_call: every timing slot of the cleaner (gpc_hip_kernel_time), two runs of `iters` calls each; the memset of
    the stats not among them;
  * bytes_per_call: what each kernel must move, from the shapes alone (px = pixels of all pairs, b = pixels on inner tile
    edges, C = channels, e = (32 + 2 r)^2 / 32^2 for the median's halo):
      k_clean_check    4 C px read (fwd)  +  4 C px gathered (bwd)  +  8 px written (labels, sizes)
      k_clean_tile     (4 + 4 C) px read  +  4 px written
      k_clean_border   (8 + 8 C) b read (twice that where the previous pixel of the edge is looked at) + the atomics
      k_clean_flatten  4 px read  +  at most 4 px written
      k_clean_sizes    4 px read + one atomic per root and tile
      k_clean_apply    (8 + 4 C) e px read (values, labels, sizes at the labels)  +  (4 C + 1) px written
    and roof_fraction = bytes / kernel time / 6.3 TB/s (the HBM rate a streaming kernel reaches on an MI355X; the planes of
    16 pairs fit the 256 MiB Infinity Cache, so part of the traffic may never reach HBM);
  * stats: pixels by state, summed over the pairs.
usage: python tools/clean_timing.py [--iters N] [--reps N] [--out FILE] [--only NAME]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from score_timing import events_us  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def case(g, torch, name, W, H, P, corr, iters, reps):
    from opengpc_amd.synth import synth_batch, synth_pair
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    cap = (W - 26) * (H - 26) + 1
    Cn = 2 if corr else 1
    s, fill, prm = g.Settings.sparsematch(), g.Densify(), g.Clean()
    d_rec = torch.empty((P, cap, 4 if corr else 3), dtype=torch.int32, device=dev)
    d_rev = torch.empty_like(d_rec)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    if corr:
        a, b = synth_pair(W, H, 0, 5)
        d_f = torch.from_numpy(np.stack([a, b] * (P // 2 + 1))[:P + 1].copy()).to(dev)
        ctx.match_sequence_device(d_f.data_ptr(), W, H, P + 1, s, d_rec.data_ptr(), cap, d_cnt.data_ptr(), 0)
    else:
        L, R = synth_batch(W, H, range(P))
        d_L, d_R = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
        ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, d_rec.data_ptr(), cap, d_cnt.data_ptr(), 0)
    d_fwd, d_bwd, d_out = (torch.empty((P, Cn, H, W), dtype=torch.int32, device=dev) for _ in range(3))
    d_state = torch.empty((P, H, W), dtype=torch.uint8, device=dev)
    d_stats = torch.empty((P, 4), dtype=torch.int32, device=dev)
    fwd_fill = lambda: ctx.densify_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, fill, d_fwd.data_ptr())
    fwd_fill()
    ctx.flip_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), P, d_rev.data_ptr())
    ctx.densify_records_device(d_rev.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, fill, d_bwd.data_ptr())
    clean = lambda: ctx.clean_fields_device(d_fwd.data_ptr(), Cn, W, H, P, prm, d_out.data_ptr(), d_bwd.data_ptr(), d_state.data_ptr(), 0,
                                            d_stats.data_ptr())
    ctx.synchronize()
    res = {"case": name, "width": W, "height": H, "pairs": P, "channels": Cn,
           "clean": [prm.check_tol_q8, prm.speckle_diff_q8, prm.speckle_min, prm.median_radius]}
    res["fill_us"] = events_us(torch, ctx, fwd_fill, iters, reps)
    res["clean_us"] = events_us(torch, ctx, clean, iters, reps)
    res["ratio_clean_to_fill"] = round(res["clean_us"]["median"] / res["fill_us"]["median"], 3)
    ctx.enable_kernel_timing(True)
    runs = []
    for _ in range(2):
        ctx.reset_kernel_timing()
        for _ in range(iters):
            clean()
        ctx.synchronize()
        times = {k: v for k, v in ctx.kernel_times().items() if v[1] and k.startswith("k_clean")}
        runs.append({k: round(1e3 * v[0] / iters, 1) for k, v in times.items()})
    res["kernel_us_per_call"] = runs
    res["kernels"] = {k: v for k, v in ctx.kernel_launch_names().items() if k in runs[0]}
    ctx.enable_kernel_timing(False)
    res["stats"] = d_stats.cpu().numpy().astype(np.int64).sum(0).tolist()
    px = W * H * P
    b = (((W + 31) // 32 - 1) * H + ((H + 31) // 32 - 1) * W) * P
    e = (32 + 2 * prm.median_radius) ** 2 / 1024.0
    need = {"k_clean_check": (8 * Cn + 8) * px, "k_clean_tile": (8 + 4 * Cn) * px, "k_clean_border": (8 + 8 * Cn) * b,
            "k_clean_flatten": 8 * px, "k_clean_sizes": 4 * px, "k_clean_apply": int((8 + 4 * Cn) * e * px) + (4 * Cn + 1) * px}
    res["bytes_per_call"] = need
    best = {k: min(r[k] for r in runs if k in r) for k in need if any(k in r for r in runs)}
    res["roof_fraction"] = {k: round(need[k] / (best[k] * 1e-6) / HBM_BYTES_PER_S, 3) for k in best if best[k]}
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
    for name, corr in (("16 pairs of 1024x436, C = 1", False), ("16 steps of 1024x436, C = 2", True)):
        if a.only and a.only not in name:
            continue
        out.append(case(g, torch, name, 1024, 436, 16, corr, a.iters, a.reps))
        print(json.dumps(out[-1], sort_keys=True), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
