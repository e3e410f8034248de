"""The propagation (gpc_hip_propagate_fields_device) in one run on one card, over the filled fields of real match output,
beside gpc_hip_search_fields_device at its defaults on the same fields in the same run.

Cases: 32 pairs of 1024x436 with the zero forest, sparsematch settings and the documented fill: C = 1 (the benchmark's
synthetic stereo pairs) and C = 2 (a sequence of 33 frames that alternates the two images of one pair); radius 2, 4
iterations, neighbours 4 and 8, spans 1 and 8.  One JSON object per case and parameter set:
  * propagate_ms: events on the context's stream around the call, per call, two windows of `iters` calls each -- the whole
    stage: the clear of the stats and every iteration's launch (out apart from the field, no cost, no choice);
  * search_ms: the same events around gpc_hip_search_fields_device;
  * times_search, times_search_per_iteration: propagate_ms over search_ms, the slower window of each, whole and divided by the
    iterations;
  * moved_share: the share of pixels moved per iteration, from the stats, summed over the pairs;
  * evaluated_lanes: per iteration the share of valued pixels (of the first 4 pairs) that had to evaluate 0, 1, 2, ...
    candidates, counted on the host from the call's own intermediate fields (each iteration run as a call of one iteration
    at its stride) by the kernel's rule: the distinct admissible displacements among the neighbours that differ from the pixel's own, plus the own
    one when there is any (no cost was asked for).
The kernel has no timing slot, and the launches' own times apart from the clear of the stats were not measured: no
rocprofv3 --kernel-trace --stats run of this tool was made.
usage: python tools/propagate_timing.py [--iters N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OFFSETS = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]
NONE = -2 ** 31
LANE_PAIRS = 4                                                  # evaluated_lanes is counted over the first pairs only


def timed(torch, ctx, st, fn, iters):
    """ms per call of fn, by events on the context's stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters):
        fn()
    e1.record(st)
    e1.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def evaluated(F, s, nb):
    """field [P, C, H, W] int64 -> the histogram of candidates evaluated per valued pixel at stride s (index = how many)"""
    P, C, H, W = F.shape
    whole = np.sign(F) * ((np.abs(F) + 128) >> 8)
    dx, dy = (-whole[:, 0], np.zeros_like(whole[:, 0])) if C == 1 else (whole[:, 0], whole[:, 1])
    valued = F[:, 0] != NONE
    ys, xs = np.mgrid[0:H, 0:W]
    seen = [(dx, dy)]
    count = np.zeros((P, H, W), np.int64)
    for ox, oy in OFFSETS[:nb]:
        qx, qy = xs + ox * s, ys + oy * s
        ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
        is_c = ok[None] & valued[:, cy, cx]
        ddx, ddy = np.where(is_c, dx[:, cy, cx], dx), np.where(is_c, dy[:, cy, cx], dy)
        fresh = (xs + ddx >= 0) & (xs + ddx < W) & (ys + ddy >= 0) & (ys + ddy < H)
        for a, b in seen:
            fresh &= (a != ddx) | (b != ddy)
        seen.append((ddx, ddy))
        count += fresh
    own = (xs + dx >= 0) & (xs + dx < W) & (ys + dy >= 0) & (ys + dy < H)
    count += own & (count > 0)
    h = np.bincount(count[valued], minlength=nb + 2)
    return [round(float(v) / max(1, int(valued.sum())), 5) for v in h]


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
    d_fwd, d_out, d_mid = (torch.empty((P, Cn, H, W), dtype=torch.int32, device=dev) for _ in range(3))
    d_sstats = torch.empty((P, 4), dtype=torch.int32, device=dev)
    ctx.densify_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, fill, d_fwd.data_ptr())
    sr = g.Search()
    search = lambda: ctx.search_fields_device(d_fwd.data_ptr(), iL, iR, Cn, W, H, P, sr, d_out.data_ptr(), 0, 0, d_sstats.data_ptr())
    search()
    ctx.synchronize()
    search_ms = [timed(torch, ctx, st, search, iters) for _ in range(2)]
    out = []
    N = 4
    for nb in (4, 8):
        for span in (1, 8):
            pg = g.Propagate(2, span, N, nb)
            d_stats = torch.empty((P, N, 4), dtype=torch.int32, device=dev)
            run = lambda: ctx.propagate_fields_device(d_fwd.data_ptr(), iL, iR, Cn, W, H, P, pg, d_out.data_ptr(), 0, 0, d_stats.data_ptr())
            run()
            ctx.synchronize()
            ms = [timed(torch, ctx, st, run, iters) for _ in range(2)]
            stats = d_stats.cpu().numpy().astype(np.int64).sum(0)
            lanes = []
            d_mid.copy_(d_fwd)
            for i in range(N):                                  # the field each iteration read, one iteration a call
                stride = max(1, span >> i)
                ctx.synchronize()
                torch.cuda.synchronize()
                lanes.append(evaluated(d_mid[:LANE_PAIRS].cpu().numpy().astype(np.int64), stride, nb))
                ctx.propagate_fields_device(d_mid.data_ptr(), iL, iR, Cn, W, H, P, g.Propagate(2, stride, 1, nb), d_mid.data_ptr())
            ctx.synchronize()
            assert bool((d_mid == d_out).all()), "the iterations run one a call give what the call gives"
            out.append({"case": name, "width": W, "height": H, "pairs": P, "channels": Cn, "propagate": [2, span, N, nb],
                        "propagate_ms": ms, "search_ms": search_ms, "times_search": round(max(ms) / max(search_ms), 2),
                        "times_search_per_iteration": round(max(ms) / max(search_ms) / N, 2), "stats": stats.tolist(),
                        "moved_share": [round(float(r[3]) / max(1, int(r.sum())), 5) for r in stats], "evaluated_lanes": lanes})
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
