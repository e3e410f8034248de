"""Group mode (all trees of a forest) against today's 32-test truncation, device-resident (gpc_hip_match_batch_device).

For BASELINE configs[4] (one 3840x2160 pair, s = 2, D = 64) and for 32 pairs of 1024x436 (synth_batch: pair i has
s = i, D = 8 + i mod 64), both with forests/stress16x20Forest.txt (16 groups of 20 tests), prints one JSON object:
  * per-kernel us per call (gpc_hip_kernel_time) in group mode and truncated;
  * end-to-end device time per pair in both modes (HIP events around whole calls, timing of kernels off);
  * the multi-group k_hash beside the sum of the 16 single-group k_hash launches over the same images, and the code
    planes it writes per second against the 8 TB/s peak;
  * supports with d == D and d != D in both modes (the pairs' true disparity is D everywhere; for information).
usage: python tools/forest_groups_timing.py [--iters N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STRESS = os.path.join(ROOT, "forests", "stress16x20Forest.txt")


def run(ctx, d_L, d_R, W, H, B, s, d_out, cap, d_cnt, d_nc):
    ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, d_out.data_ptr(), cap, d_cnt.data_ptr(),
                           d_nc.data_ptr())


def case(g, torch, name, W, H, Ls, Rs, Ds, iters):
    dev = torch.device("cuda", 0)
    B = len(Ls)
    s = g.Settings(5, 128, 0, True, False, 1)
    ctx = g.Context(0)
    groups = g.read_forest_groups(STRESS, W, H)[1]
    G = len(groups)
    cap = G * (W - 26) * (H - 26)
    d_L, d_R = torch.from_numpy(np.ascontiguousarray(Ls)).to(dev), torch.from_numpy(np.ascontiguousarray(Rs)).to(dev)
    d_out = torch.empty((B, cap, 3), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    d_nc = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    res = {"pairs": B, "width": W, "height": H, "groups": G}
    for mode in ("groups", "truncated"):
        if mode == "groups":
            ctx.set_forest_groups(groups)
        else:
            ctx.load_forest(STRESS, W, H)
        for _ in range(3):
            run(ctx, d_L, d_R, W, H, B, s, d_out, cap, d_cnt, d_nc)
        ctx.synchronize()
        # end to end (no per-kernel events)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        e0.record()
        for _ in range(iters):
            run(ctx, d_L, d_R, W, H, B, s, d_out, cap, d_cnt, d_nc)
        ctx.synchronize()
        e1.record()
        torch.cuda.synchronize(dev)
        ms = e0.elapsed_time(e1) / iters
        # per kernel
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_timing()
        for _ in range(iters):
            run(ctx, d_L, d_R, W, H, B, s, d_out, cap, d_cnt, d_nc)
        ctx.synchronize()
        kt = {k: round(1e3 * v[0] / v[1], 1) for k, v in ctx.kernel_times().items() if v[1]}
        ctx.enable_kernel_timing(False)
        cnt = d_cnt.cpu().numpy()
        # d == D counted on the device: truth D everywhere, threshold 0 (gpc_hip_score_batch_device)
        d_u = torch.from_numpy(np.stack([np.full((H, W), D, np.float32) for D in Ds])).to(d_out.device)
        d_sc = torch.zeros((B, 15), dtype=torch.int64, device=d_out.device)
        torch.cuda.synchronize()
        ctx.score_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, B, s, d_u.data_ptr(), 0, [0.0], d_sc.data_ptr())
        ctx.synchronize()
        sc = d_sc.cpu().numpy().view(g.SCORE_DTYPE).reshape(-1)
        assert int(sc["n_records"].sum()) == int(cnt.sum())
        right = int(sc["n_within"][:, 0].sum())
        wrong = int(sc["n_judged"].sum()) - right
        res[mode] = {"us_per_call": round(1e3 * ms, 1), "us_per_pair": round(1e3 * ms / B, 2), "kernels_us": kt,
                     "launch_names": {k: v for k, v in ctx.kernel_launch_names().items() if v},
                     "supports": int(cnt.sum()), "supports_d_eq_D": right, "supports_d_ne_D": wrong}
    # the multi-group k_hash beside G single-group launches over the same images
    single = 0.0
    for grp in groups:
        ctx.set_forest(grp)
        run(ctx, d_L, d_R, W, H, B, s, d_out, cap, d_cnt, d_nc)
        ctx.synchronize()
        ctx.enable_kernel_timing(True, only=["k_hash"])
        ctx.reset_kernel_timing()
        for _ in range(iters):
            run(ctx, d_L, d_R, W, H, B, s, d_out, cap, d_cnt, d_nc)
        ctx.synchronize()
        v = ctx.kernel_times()["k_hash"]
        single += 1e3 * v[0] / v[1]
        ctx.enable_kernel_timing(False)
    multi = res["groups"]["kernels_us"]["k_hash"]
    written = 4.0 * W * H * 2 * B * G
    res["k_hash"] = {"multi_group_us": multi, "sum_single_group_us": round(single, 1),
                     "ratio": round(multi / single, 3), "code_bytes_written": int(written),
                     "write_TBps": round(written / (multi * 1e-6) / 1e12, 2), "peak_TBps": 8.0}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["configs4", "batch32"], default=None)
    a = ap.parse_args()
    import torch
    import opengpc_amd as g
    from opengpc_amd.synth import synth_batch, synth_pair
    out = {}
    if a.only in (None, "configs4"):
        L, R = synth_pair(3840, 2160, 2, 64)
        out["configs4"] = case(g, torch, "configs4", 3840, 2160, L[None], R[None], [64], a.iters)
    if a.only in (None, "batch32"):
        idx = list(range(32))
        L, R = synth_batch(1024, 436, idx)
        out["batch32"] = case(g, torch, "batch32", 1024, 436, L, R, [8 + i % 64 for i in idx], a.iters)
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
