"""The local dense search (gpc_hip_search_*) in one run on one card: k_search over the filled fields of real match output, by
the library's kernel timing, beside k_dense_push of the fill that made those fields.

Cases: 32 pairs of 1024x436 with the zero forest, sparsematch settings and the documented fill: C = 1 (the benchmark's
synthetic stereo pairs) at the documented search parameters, C = 2 (a sequence of 33 frames that alternates the two images
of one pair) at the documented parameters and at radius 4, range 2.  One JSON object per case:
  * k_search_ms / k_dense_push_ms: the timing slots (gpc_hip_kernel_time), per call, two runs of `iters` calls each;
  * bytes: what the kernel must move -- the field in and out (4 C bytes a pixel each) and the two images (1 byte each);
  * share_of_8TBps: bytes over the HBM peak of 8 TB/s, over the slower run's time: a roof the kernel does not aim at (it is
    bound by its byte SADs, not by memory); sads_per_pixel: the byte differences the rule needs per pixel -- the candidates
    and the parabola's neighbours, times the window (the kernel evaluates the whole grid of shifts, corners included);
  * stats: pixels kept, hole, unmatched, rejected, summed over the pairs.
usage: python tools/search_timing.py [--iters N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def case(g, torch, name, W, H, P, corr, prms, iters):
    from opengpc_amd.synth import synth_batch, synth_pair
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
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
    densify = lambda: ctx.densify_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, fill, d_fwd.data_ptr())
    densify()
    ctx.synchronize()
    out = []
    for prm in prms:
        sr = g.Search(*prm)
        search = lambda: ctx.search_fields_device(d_fwd.data_ptr(), iL, iR, Cn, W, H, P, sr, d_out.data_ptr(), 0, 0, d_stats.data_ptr())
        search()                                                              # warm-up: the code object, the shape
        ctx.synchronize()
        ctx.enable_kernel_timing(True)
        runs = []
        for _ in range(2):
            ctx.reset_kernel_timing()
            for _ in range(iters):
                densify()
                search()
            ctx.synchronize()
            t = ctx.kernel_times()
            assert t["k_search"][1] == iters, t["k_search"]
            runs.append({k: round(t[k][0] / iters, 4) for k in ("k_search", "k_dense_push")})
        ctx.enable_kernel_timing(False)
        need = (2 * 4 * Cn + 2) * W * H * P
        ms = max(r["k_search"] for r in runs)
        cands = (2 * prm[1] + 1) ** (2 if corr else 1) + (4 if corr else 2) * prm[2]
        out.append({"case": name, "width": W, "height": H, "pairs": P, "channels": Cn, "search": list(prm),
                    "kernel": ctx.kernel_launch_names()["k_search"], "k_search_ms": [r["k_search"] for r in runs],
                    "k_dense_push_ms": [r["k_dense_push"] for r in runs], "bytes": need,
                    "share_of_8TBps": round(need / 8e12 / (ms * 1e-3), 4), "sads_per_pixel": cands * (2 * prm[0] + 1) ** 2,
                    "stats": d_stats.cpu().numpy().astype(np.int64).sum(0).tolist()})
        print(json.dumps(out[-1], sort_keys=True), flush=True)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import opengpc_amd as g
    out = case(g, torch, "32 pairs of 1024x436, C = 1", 1024, 436, 32, False, [(2, 1, 1, 0xFFFF)], a.iters)
    out += case(g, torch, "32 steps of 1024x436, C = 2", 1024, 436, 32, True, [(2, 1, 1, 0xFFFF), (4, 2, 1, 0xFFFF)], a.iters)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
