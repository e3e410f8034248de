"""The scanline aggregation (gpc_hip_aggregate_fields_device) in one run on one card, over the filled fields of real match
output, beside k_search on the same fields in the same run.

Cases: 32 pairs of 1024x436 with the zero forest, sparsematch settings and the documented fill: C = 1 (the benchmark's
synthetic stereo pairs) and C = 2 (a sequence of 33 frames that alternates the two images of one pair), the documented
parameters, paths = 3, 12 and 15.  One JSON object per case and paths:
  * aggregate_ms: events on the context's stream around the call, per call, two runs of `iters` calls each -- the whole stage:
    the clear of the stats and every launch of every group of pairs;
  * search_ms: the same events around gpc_hip_search_fields_device; k_search_ms: its timing slot (gpc_hip_kernel_time), from
    calls of their own, since the slots are bracketed only while timing is on;
  * times_search: aggregate_ms over search_ms, the slower run of each;
  * bytes: what the stage moves per call by its layout -- see DESIGN.md 4.20 -- and the pairs per workspace group.
The kernels have no timing slot; each kernel's share comes from a rocprofv3 --kernel-trace --stats run of this tool.
usage: python tools/aggregate_timing.py [--iters N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, ctx, st, fn, iters):
    """ms per call of fn, by events on the context's stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters):
        fn()
    e1.record(st)
    e1.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def case(g, torch, name, W, H, P, corr, iters):
    from opengpc_amd.synth import synth_batch, synth_pair
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    st = torch.cuda.Stream(device=dev)
    ctx.set_stream(st.cuda_stream)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    cap = (W - 26) * (H - 26) + 1
    Cn = 2 if corr else 1
    s, fill = g.Settings.sparsematch(), g.Densify()
    d_rec = torch.empty((P, cap, 4 if corr else 3), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    if corr:
        a, b = synth_pair(W, H, 0, 5)
        d_L = torch.from_numpy(np.stack([a, b] * (P // 2 + 1))[:P + 1].copy()).to(dev)
        iL, iR = d_L.data_ptr(), d_L.data_ptr() + W * H
        ctx.match_sequence_device(iL, W, H, P + 1, s, d_rec.data_ptr(), cap, d_cnt.data_ptr(), 0)
    else:
        L, R = synth_batch(W, H, range(P))
        d_L, d_R = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
        iL, iR = d_L.data_ptr(), d_R.data_ptr()
        ctx.match_batch_device(iL, iR, W, H, P, s, d_rec.data_ptr(), cap, d_cnt.data_ptr(), 0)
    d_fwd, d_out = (torch.empty((P, Cn, H, W), dtype=torch.int32, device=dev) for _ in range(2))
    d_stats = torch.empty((P, 4), dtype=torch.int32, device=dev)
    ctx.densify_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, fill, d_fwd.data_ptr())
    sr = g.Search()
    search = lambda: ctx.search_fields_device(d_fwd.data_ptr(), iL, iR, Cn, W, H, P, sr, d_out.data_ptr(), 0, 0, d_stats.data_ptr())
    search()
    ctx.synchronize()
    search_ms = [timed(torch, ctx, st, search, iters) for _ in range(2)]
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_timing()
    for _ in range(iters):
        search()
    ctx.synchronize()
    k_search_ms = round(ctx.kernel_times()["k_search"][0] / iters, 4)
    ctx.enable_kernel_timing(False)
    n, out = W * H, []
    K, cells = (9, 21) if corr else (3, 5)                                    # labels; cost cells written (the ring's corners are not)
    for paths in (3, 12, 15):
        ag = g.Aggregate(paths=paths)
        run = lambda: ctx.aggregate_fields_device(d_fwd.data_ptr(), iL, iR, Cn, W, H, P, ag, d_out.data_ptr(), 0, 0, d_stats.data_ptr())
        run()
        ctx.synchronize()
        ms = [timed(torch, ctx, st, run, iters) for _ in range(2)]
        dirs = bin(paths).count("1")
        per_pixel = {"cost": 4 * Cn + 2 + 2 * cells, "paths": dirs * (2 * K + 4 * Cn + 2 * K), "choose": 4 * Cn + 2 * cells + 2 * K * dirs + 4 * Cn}
        space = 2 * ((25 if corr else 5) + dirs * K) * n
        out.append({"case": name, "width": W, "height": H, "pairs": P, "channels": Cn, "paths": paths, "aggregate": [2, 1, 1, 0xFFFF, ag.p1, ag.p2],
                    "aggregate_ms": ms, "search_ms": search_ms, "k_search_ms": k_search_ms,
                    "times_search": round(max(ms) / max(search_ms), 2), "bytes_per_pixel": per_pixel,
                    "bytes": sum(per_pixel.values()) * n * P, "pairs_per_group": min(P, max(1, (1 << 30) // space)),
                    "stats": d_stats.cpu().numpy().astype(np.int64).sum(0).tolist()})
        print(json.dumps(out[-1], sort_keys=True), flush=True)
    ctx.set_stream(None)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import opengpc_amd as g
    out = case(g, torch, "32 pairs of 1024x436, C = 1", 1024, 436, 32, False, a.iters)
    out += case(g, torch, "32 steps of 1024x436, C = 2", 1024, 436, 32, True, a.iters)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
