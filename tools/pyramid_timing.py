"""The pyramid matcher (gpc_hip_pyramid_batch_device, 3 levels) beside the plain gpc_hip_match_batch_device of level 0, in
the same run on the same card.

Cases: 32 pairs of 1024x436 with the zero forest (the benchmark's synthetic pairs) and one 1920x1080 pair with the tau
forest, sparsematch settings.  For each, one JSON object:
  * plain_us / pyramid_us: warmed calls into every-record arrays; HIP events around `iters` calls, median and min .. max of
    `reps` repetitions; ratio = pyramid / plain (medians).  By pixel count the levels cost 1 + 1/4 + 1/16 = 1.31 of level 0;
    the rest is launches (3 matches instead of 1, the downsampling steps, 3 merge launches per level) and the merge's pass
    over level 0's records, which a plain call writes once and the pyramid call writes, reads and writes again;
  * kernel_us_per_call / launches_per_call: every timing slot the pyramid call uses (gpc_hip_kernel_time), summed over
    the launches of one call, the new k_pyr_* among them;
  * level_counts: supports each level adds, summed over the pairs.
usage: python tools/pyramid_timing.py [--iters N] [--reps N] [--out FILE] [--only NAME]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from score_timing import events_us  # noqa: E402

LEVELS = 3


def case(g, torch, name, W, H, P, forest, iters, reps):
    from opengpc_amd.synth import synth_batch
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", forest), W, H)
    cap0 = (W - 26) * (H - 26) + 1
    cap = cap0 + cap0 // 2
    L, R = synth_batch(W, H, range(P))
    d_L, d_R = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    d_out = torch.empty((P, cap, 3), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    d_lc = torch.zeros((LEVELS, P), dtype=torch.int32, device=dev)
    s = g.Settings.sparsematch()
    plain = lambda: ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), 0)
    pyr = lambda: ctx.pyramid_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, LEVELS, s, d_out.data_ptr(), cap,
                                           d_cnt.data_ptr(), d_lc.data_ptr(), 0)
    torch.cuda.synchronize(dev)
    res = {"case": name, "width": W, "height": H, "pairs": P, "levels": LEVELS, "forest": forest}
    res["plain_us"] = events_us(torch, ctx, plain, iters, reps)
    res["pyramid_us"] = events_us(torch, ctx, pyr, iters, reps)
    res["ratio_pyramid_to_plain"] = round(res["pyramid_us"]["median"] / res["plain_us"]["median"], 3)
    res["ratio_by_pixels"] = round(sum((W >> l) * (H >> l) for l in range(LEVELS)) / float(W * H), 3)
    # per CALL, not per launch: a pyramid call launches most kernels once per level
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_timing()
    for _ in range(iters):
        pyr()
    ctx.synchronize()
    res["kernel_us_per_call"] = {k: round(1e3 * v[0] / iters, 1) for k, v in ctx.kernel_times().items() if v[1]}
    res["launches_per_call"] = {k: round(v[1] / iters, 2) for k, v in ctx.kernel_times().items() if v[1]}
    res["kernels"] = {k: v for k, v in ctx.kernel_launch_names().items() if k.startswith("k_pyr")}
    ctx.enable_kernel_timing(False)
    res["level_counts"] = [int(v) for v in d_lc.cpu().numpy().astype(np.int64).sum(axis=1)]
    res["supports"] = int(d_cnt.cpu().numpy().astype(np.int64).sum())
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
    for name, W, H, P, forest in (("32 pairs of 1024x436, zero forest", 1024, 436, 32, "defaultZeroForest.txt"),
                                  ("1 pair of 1920x1080, tau forest", 1920, 1080, 1, "defaultTauForest.txt")):
        if a.only and a.only not in name:
            continue
        out.append(case(g, torch, name, W, H, P, forest, a.iters, a.reps))
        print(json.dumps(out[-1], sort_keys=True), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
