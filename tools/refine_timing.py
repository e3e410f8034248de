"""Match refinement (gpc_hip_refine_*) beside the match that produced its records, radius 3.

Cases: 256 pairs of 1024x436 from match_batch_device (the benchmark's synthetic pairs, the reference's sparsematch settings:
epipolar, records arrive row by row) and 15 pairs of 1024x436 from match_sequence_device (16 frames moving in x and y, zero
forest, non-epipolar sort matcher: records arrive in code order).  For each, one JSON object:
  * match_us / refine_us: a warmed match call into an every-record array, and the records form of the refinement over what it
    left; HIP events around `iters` calls, median and min .. max of `reps` repetitions; ratio = refine / match (medians);
  * kernel_us: k_refine's own time per call (gpc_hip_kernel_time) and the instantiation launched;
  * records, ns_per_record, and the bytes the kernel must move -- 12 | 16 B in and 8 (+ 12) B out per record, both images
    once -- with the rate that kernel_us implies for them;
  * refine_us_sorted: the same records sorted by source row and column on the host first, refined again: what binning the
    records by source row on the device could gain at the most (its own cost not counted).
Then the sub-pixel check: pairs with the true disparity D + k / 4, k = 1, 2, 3 -- synth's texture rendered at four times the
width, box-averaged over 4 columns, the right image from columns 4 D + k further on -- matched (epipolar), refined, and both
the integer supports and the refined ones scored against the true disparity by gpc_hip_score_supports_device: sum_e2_q8
before and after, over the judged records.
usage: python tools/refine_timing.py [--iters N] [--reps N] [--out FILE] [--only NAME]
(which unit binds the kernel: rocprofv3 --kernel-trace --stats -- python tools/refine_timing.py --iters 2 --reps 1, and
counters in a run of their own: rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCP_TCC_READ_REQ_sum SQ_INSTS_VALU SQ_WAIT_INST_ANY
--kernel-include-regex k_refine -- python tools/refine_timing.py --only sequence --iters 2 --reps 1)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from score_timing import events_us, frames_of, kernel_us  # noqa: E402

RADIUS = 3


def case(g, torch, name, W, H, P, sequence, iters, reps):
    from opengpc_amd.synth import synth_batch
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    cap = (W - 26) * (H - 26) + 1
    words = 4 if sequence else 3
    d_rec = torch.zeros((P, cap, words), dtype=torch.int32, device=dev)
    d_out = torch.empty((P, cap, 3), dtype=torch.int32, device=dev)
    d_ref = torch.empty((P, cap, 2), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    if sequence:
        frames, _ = frames_of(W, H, P + 1, P + 1)
        d_f = torch.from_numpy(frames).to(dev)
        d_L, d_R = d_f, d_f[1:]
        s = g.Settings(5, 128, 0, False, False, 1)
        match = lambda: ctx.match_sequence_device(d_f.data_ptr(), W, H, P + 1, s, d_rec.data_ptr(), cap, d_cnt.data_ptr(), 0)
    else:
        L, R = synth_batch(W, H, range(P))
        d_L, d_R = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
        s = g.Settings.sparsematch()
        match = lambda: ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, d_rec.data_ptr(), cap, d_cnt.data_ptr(), 0)

    def refine_of(d_records):
        return lambda: ctx.refine_records_device(d_records.data_ptr(), sequence, cap, d_cnt.data_ptr(), d_L.data_ptr(), d_R.data_ptr(),
                                                 W, H, P, RADIUS, d_ref.data_ptr(), 0 if sequence else d_out.data_ptr())

    torch.cuda.synchronize(dev)
    res = {"case": name, "width": W, "height": H, "pairs": P, "radius": RADIUS}
    res["match_us"] = events_us(torch, ctx, match, iters, reps)
    res["refine_us"] = events_us(torch, ctx, refine_of(d_rec), iters, reps)
    res["ratio_refine_to_match"] = round(res["refine_us"]["median"] / res["match_us"]["median"], 3)
    kt, names = kernel_us(ctx, refine_of(d_rec), iters)
    res["kernel_us"], res["kernel"] = kt.get("k_refine"), names.get("k_refine")
    cnt = np.minimum(d_cnt.cpu().numpy().astype(np.int64), cap)
    n = int(cnt.sum())
    ref = d_ref.cpu().numpy().view(g.REFINEMENT_DTYPE).reshape(P, cap)
    fl = np.concatenate([ref[t, :cnt[t]]["flags"] for t in range(P)])
    res["records"], res["evaluated"], res["minimum_in_x"] = n, int((fl & 1).sum()), int(((fl & 2) != 0).sum())
    res["ns_per_record"] = round(1e3 * res["kernel_us"] / max(n, 1), 3)
    per_rec = (16 + 8) if sequence else (12 + 8 + 12)
    res["bytes"] = n * per_rec + (P + 1 if sequence else 2 * P) * W * H
    res["GBps_of_those_bytes"] = round(res["bytes"] / (res["kernel_us"] * 1e-6) / 1e9, 1)
    # the same records in source order
    rec = d_rec.cpu().numpy()
    srt = rec.copy()
    for t in range(P):
        r = rec[t, :cnt[t]]
        srt[t, :cnt[t]] = r[np.lexsort((r[:, 0], r[:, 1]))]
    d_srt = torch.from_numpy(srt).to(dev)
    res["refine_us_sorted"] = events_us(torch, ctx, refine_of(d_srt), iters, reps)
    ctx.close()
    return res


def fractional_pair(W, H, s, D, k):
    """(left, right) with the true disparity D + k / 4 everywhere: synth's texture at four times the width, box-averaged"""
    from opengpc_amd.synth import _texture
    fine = _texture(4 * (W + 2 * D + 2), H, s, 0).astype(np.int64)
    box = lambda first: ((fine[:, first:first + 4 * W].reshape(H, W, 4).sum(axis=2) + 2) // 4).astype(np.uint8)
    return box(4 * D), box(4 * D + 4 * D + k)


def subpixel(g, torch, W, H, npairs):
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    cap = (W - 26) * (H - 26) + 1
    s = g.Settings.sparsematch()
    out = []
    for k in (1, 2, 3):
        D = [8 + 3 * i for i in range(npairs)]
        pairs = [fractional_pair(W, H, i, D[i], k) for i in range(npairs)]
        d_L = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
        d_R = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
        u = np.empty((npairs, H, W), np.float32)
        for i in range(npairs):
            u[i] = D[i] + k / 4.0
        d_u = torch.from_numpy(u).to(dev)
        d_sup = torch.zeros((npairs, cap, 3), dtype=torch.int32, device=dev)
        d_out = torch.zeros((npairs, cap, 3), dtype=torch.int32, device=dev)
        d_ref = torch.zeros((npairs, cap, 2), dtype=torch.int32, device=dev)
        d_cnt = torch.zeros(npairs, dtype=torch.int32, device=dev)
        ctx.refine_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, npairs, s, RADIUS, d_sup.data_ptr(), cap, d_cnt.data_ptr(), 0,
                                d_ref.data_ptr(), d_out.data_ptr())
        row = {"true_disparity_fraction": k / 4.0, "pairs": npairs}
        for what, d_rec in (("integer", d_sup), ("refined", d_out)):
            d_sc = torch.zeros((npairs, 15), dtype=torch.int64, device=dev)
            ctx.score_supports_device(d_rec.data_ptr(), cap, d_cnt.data_ptr(), W, H, npairs, d_u.data_ptr(), 0, [0.25, 0.5, 1.0],
                                      d_sc.data_ptr())
            ctx.synchronize()
            sc = d_sc.cpu().numpy().copy().view(g.SCORE_DTYPE).reshape(-1)
            row[what] = {"judged": int(sc["n_judged"].sum()), "sum_e2_q8": int(sc["sum_e2_q8"].sum()),
                         "within_quarter_half_one_px": [int(v) for v in sc["n_within"][:, :3].sum(axis=0)]}
        out.append(row)
    ctx.close()
    return {"case": "sub-pixel check, %dx%d, radius %d" % (W, H, RADIUS), "rows": out}


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
    for name, P, sequence in (("256 pairs of 1024x436, match_batch_device, epipolar", 256, False),
                              ("15 pairs of 1024x436, match_sequence_device, non-epipolar", 15, True)):
        if a.only and a.only not in name:
            continue
        out.append(case(g, torch, name, 1024, 436, P, sequence, a.iters, a.reps))
        print(json.dumps(out[-1], sort_keys=True), flush=True)
    if not a.only or a.only in "sub-pixel check":
        out.append(subpixel(g, torch, 1024, 436, 8))
        print(json.dumps(out[-1], sort_keys=True), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
