"""The densifier (gpc_hip_densify_*) in one run on one card: the fill alone over real match output, and the match-and-fill
form beside the plain gpc_hip_match_batch_device call on the same inputs.

Cases: 32 pairs of 1024x436 with the zero forest (the benchmark's synthetic pairs) and one 1920x1080 pair with the tau
forest, sparsematch settings, the documented fill parameters.  For each, one JSON object:
  * plain_us / fill_us / batch_us: warmed calls; HIP events around `iters` calls, median and min .. max of `reps`
    repetitions.  fill = gpc_hip_densify_supports_device over the records the plain call left on the device; batch =
    gpc_hip_densify_batch_device (match into the every-record workspace, then the fill);
  * kernel_us_per_call: every timing slot of the fill (gpc_hip_kernel_time), the memset of the owner plane not among them;
  * bytes_per_call: what each kernel must move, from the shapes alone (px = pixels, m = records, c = cells of all levels):
      k_dense_claim  12 m read (the records)  +  4 m atomics
      k_dense_pull   4 px read (owners)  +  12 * occupied read (their records)  +  4 px written (values)  +  12 c written
      k_dense_top    the cells of the levels above the tile, read and written: a few KiB
      k_dense_push   4 px read (values)  +  12 c read  +  5 px written (values and levels)
    and roof_fraction = bytes / kernel time / 6.3 TB/s (the HBM rate a streaming kernel reaches on an MI355X; the planes of 32
    pairs, 57 MB each, fit the 256 MiB Infinity Cache, so part of the traffic may never reach HBM);
  * occupied / filled / none: pixels by kind, and the highest level used.
usage: python tools/dense_timing.py [--iters N] [--reps N] [--out FILE] [--only NAME]"""
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


def cells(W, H):
    n, l = 0, 1
    while True:
        gw, gh = ((W - 1) >> l) + 1, ((H - 1) >> l) + 1
        n += gw * gh
        if gw == 1 and gh == 1:
            return n
        l += 1


def case(g, torch, name, W, H, P, forest, iters, reps):
    from opengpc_amd.synth import synth_batch
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", forest), W, H)
    cap = (W - 26) * (H - 26) + 1
    L, R = synth_batch(W, H, range(P))
    d_L, d_R = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    d_out = torch.empty((P, cap, 3), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    d_val = torch.empty((P, 1, H, W), dtype=torch.int32, device=dev)
    d_lev = torch.empty((P, H, W), dtype=torch.uint8, device=dev)
    s, prm = g.Settings.sparsematch(), g.Densify()
    plain = lambda: ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), 0)
    fill = lambda: ctx.densify_records_device(d_out.data_ptr(), False, cap, d_cnt.data_ptr(), W, H, P, prm, d_val.data_ptr(),
                                              d_lev.data_ptr())
    batch = lambda: ctx.densify_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, prm, d_val.data_ptr(), d_lev.data_ptr())
    torch.cuda.synchronize(dev)
    res = {"case": name, "width": W, "height": H, "pairs": P, "forest": forest}
    res["plain_us"] = events_us(torch, ctx, plain, iters, reps)
    res["fill_us"] = events_us(torch, ctx, fill, iters, reps)
    res["batch_us"] = events_us(torch, ctx, batch, iters, reps)
    res["ratio_batch_to_plain"] = round(res["batch_us"]["median"] / res["plain_us"]["median"], 3)
    plain()
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_timing()
    for _ in range(iters):
        fill()
    ctx.synchronize()
    times = {k: v for k, v in ctx.kernel_times().items() if v[1] and k.startswith("k_dense")}
    res["kernel_us_per_call"] = {k: round(1e3 * v[0] / iters, 1) for k, v in times.items()}
    res["kernels"] = {k: v for k, v in ctx.kernel_launch_names().items() if k in times}
    ctx.enable_kernel_timing(False)
    lev = d_lev.cpu().numpy()
    m = int(d_cnt.cpu().numpy().astype(np.int64).sum())
    px, occ, c = W * H * P, int((lev == 0).sum()), cells(W, H) * P
    res.update(supports=m, occupied=occ, filled=int(((lev > 0) & (lev < 255)).sum()), none=int((lev == 255).sum()),
               highest_level=int(lev[lev < 255].max()) if occ else -1)
    need = {"k_dense_claim": 16 * m, "k_dense_pull": 8 * px + 12 * occ + 12 * c, "k_dense_push": 9 * px + 12 * c}
    res["bytes_per_call"] = need
    res["roof_fraction"] = {k: round(need[k] / (res["kernel_us_per_call"][k] * 1e-6) / HBM_BYTES_PER_S, 3) for k in need
                            if res["kernel_us_per_call"].get(k)}
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
