"""The guided completion (gpc_hip_inpaint_*) in one run on one card: gpc_hip_inpaint_fields_device over the cleaned fields of
real match output, per kernel and per call, beside the cleaner that made those fields.

Cases: 16 pairs of 1024x436 with the zero forest, sparsematch settings, the documented fill, clean and inpaint parameters:
C = 1 (the benchmark's synthetic stereo pairs, guided by the left images) and C = 2 (a sequence of 17 frames that alternates
the two images of one pair, guided by frame t).  Forward and backward fields and the cleaned field are made once by the
records forms; then, for each case, one JSON object:
  * inpaint_us / clean_us: warmed calls; HIP events around `iters` calls, median and min .. max of `reps` repetitions;
  * kernel_us_per_call: the two timing slots of the completion (gpc_hip_kernel_time), two runs of `iters` calls each;
    k_inpaint_pass is the sum over the `passes` launches of a call, and launches_per_call counts them.  The two clears of the
    control words are not among them;
  * passes_that_filled: the highest pass number in the pass plane; hole_share: holes of the cleaned field over all pixels;
    fill_stats: pixels filled and holes left, summed over the pairs.
usage: python tools/inpaint_timing.py [--iters N] [--reps N] [--out FILE] [--only NAME]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from score_timing import events_us  # noqa: E402


def case(g, torch, name, W, H, P, corr, iters, reps):
    from opengpc_amd.synth import synth_batch, synth_pair
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    cap = (W - 26) * (H - 26) + 1
    Cn = 2 if corr else 1
    s, fill, prm, ip = g.Settings.sparsematch(), g.Densify(), g.Clean(), g.Inpaint()
    d_rec = torch.empty((P, cap, 4 if corr else 3), dtype=torch.int32, device=dev)
    d_rev = torch.empty_like(d_rec)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    if corr:
        a, b = synth_pair(W, H, 0, 5)
        d_guide = torch.from_numpy(np.stack([a, b] * (P // 2 + 1))[:P + 1].copy()).to(dev)
        ctx.match_sequence_device(d_guide.data_ptr(), W, H, P + 1, s, d_rec.data_ptr(), cap, d_cnt.data_ptr(), 0)
    else:
        L, R = synth_batch(W, H, range(P))
        d_guide, d_R = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
        ctx.match_batch_device(d_guide.data_ptr(), d_R.data_ptr(), W, H, P, s, d_rec.data_ptr(), cap, d_cnt.data_ptr(), 0)
    d_fwd, d_bwd, d_cleaned, d_out = (torch.empty((P, Cn, H, W), dtype=torch.int32, device=dev) for _ in range(4))
    d_pass = torch.empty((P, H, W), dtype=torch.uint8, device=dev)
    d_stats = torch.empty((P, 2), dtype=torch.int32, device=dev)
    ctx.densify_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, fill, d_fwd.data_ptr())
    ctx.flip_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), P, d_rev.data_ptr())
    ctx.densify_records_device(d_rev.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, fill, d_bwd.data_ptr())
    clean = lambda: ctx.clean_fields_device(d_fwd.data_ptr(), Cn, W, H, P, prm, d_cleaned.data_ptr(), d_bwd.data_ptr())
    inpaint = lambda: ctx.inpaint_fields_device(d_cleaned.data_ptr(), d_guide.data_ptr(), Cn, W, H, P, ip, d_out.data_ptr(),
                                                d_pass.data_ptr(), d_stats.data_ptr())
    clean()
    ctx.synchronize()
    res = {"case": name, "width": W, "height": H, "pairs": P, "channels": Cn,
           "inpaint": [ip.radius, ip.range_shift, ip.min_weight, ip.passes]}
    res["clean_us"] = events_us(torch, ctx, clean, iters, reps)
    res["inpaint_us"] = events_us(torch, ctx, inpaint, iters, reps)
    res["ratio_inpaint_to_clean"] = round(res["inpaint_us"]["median"] / res["clean_us"]["median"], 3)
    ctx.enable_kernel_timing(True)
    runs, launches = [], {}
    for _ in range(2):
        ctx.reset_kernel_timing()
        for _ in range(iters):
            inpaint()
        ctx.synchronize()
        times = {k: v for k, v in ctx.kernel_times().items() if v[1] and k.startswith("k_inpaint")}
        runs.append({k: round(1e3 * v[0] / iters, 1) for k, v in times.items()})
        launches = {k: v[1] // iters for k, v in times.items()}
    res["kernel_us_per_call"] = runs
    res["launches_per_call"] = launches
    res["kernels"] = {k: v for k, v in ctx.kernel_launch_names().items() if k in runs[0]}
    ctx.enable_kernel_timing(False)
    pz = d_pass.cpu().numpy()
    res["passes_that_filled"] = int(pz[pz < 255].max())
    res["hole_share"] = round(float((d_cleaned[:, 0] == -2 ** 31).sum().item()) / (W * H * P), 5)
    res["fill_stats"] = d_stats.cpu().numpy().astype(np.int64).sum(0).tolist()
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
