"""Stereo sequences (gpc_hip_match_stereo_sequence_device, gpc_hip_quads_*) on one MI355X: N = 16 stereo frames of 1024x436,
zero forest, stereo settings (5, 128, 0, epipolar, sort), flow settings (5, 128, 0, non-epipolar, sort).
  1. one_call_us: gpc_hip_match_stereo_sequence_device (one k_preprocess and one k_hash over the 2 N images), against
     three_calls_us: gpc_hip_match_batch_device + gpc_hip_match_sequence_device (left) + gpc_hip_match_sequence_device (right)
     queued back to back, which preprocess and hash 4 N images; both warmed, HIP events around `iters` calls, median and
     min .. max of `reps` (>= 20).  The three existing calls are timed on THIS commit (assumed, not measured, to
     take what they take on the parent: none of their kernels or launchers changed).  The per-slot times of
     both say where the difference comes from (k_quad_sides is the price of the single hashing).
  2. closing: the launches of gpc_hip_quads_records_device over the records of (1), from the kernel-timing table, and the
     call's time by events.
usage: python tools/quads_timing.py [--iters N] [--reps N] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from score_timing import events_us  # noqa: E402
from track_stream_timing import slot_times  # noqa: E402
from quad_util import stereo_frames_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import opengpc_amd as g
    W, H, N, D = 1024, 436, 16, 24
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    ss, fs = g.Settings(5, 128, 0, 1, 0, 1), g.Settings(5, 128, 0, 0, 0, 1)
    L, R = stereo_frames_of(W, H, N, 1, D, 12)
    dL, dR = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    P, cap = N - 1, (W - 26) * (H - 26) + 1
    d_sup = torch.empty((N, cap, 3), dtype=torch.int32, device=dev)
    d_fl = torch.empty((P, cap, 4), dtype=torch.int32, device=dev)
    d_fr = torch.empty((P, cap, 4), dtype=torch.int32, device=dev)
    d_ns = torch.zeros(N, dtype=torch.int32, device=dev)
    d_nl, d_nr, d_nq = (torch.zeros(P, dtype=torch.int32, device=dev) for _ in range(3))
    d_nc = torch.zeros((2, N), dtype=torch.int32, device=dev)
    d_q = torch.empty((P, cap, 8), dtype=torch.int32, device=dev)

    def three():
        ctx.match_batch_device(dL.data_ptr(), dR.data_ptr(), W, H, N, ss, d_sup.data_ptr(), cap, d_ns.data_ptr(), 0)
        ctx.match_sequence_device(dL.data_ptr(), W, H, N, fs, d_fl.data_ptr(), cap, d_nl.data_ptr(), d_nc[0].data_ptr())
        ctx.match_sequence_device(dR.data_ptr(), W, H, N, fs, d_fr.data_ptr(), cap, d_nr.data_ptr(), d_nc[1].data_ptr())

    def one():
        ctx.match_stereo_sequence_device(dL.data_ptr(), dR.data_ptr(), W, H, N, ss, fs, d_sup.data_ptr(), cap, d_ns.data_ptr(),
                                         d_fl.data_ptr(), d_fr.data_ptr(), cap, d_nl.data_ptr(), d_nr.data_ptr(), d_nc.data_ptr())

    def close():
        ctx.quads_records_device(d_sup.data_ptr(), cap, d_ns.data_ptr(), d_fl.data_ptr(), d_fr.data_ptr(), cap, d_nl.data_ptr(),
                                 d_nr.data_ptr(), W, H, N, 1, d_q.data_ptr(), cap, d_nq.data_ptr())

    torch.cuda.synchronize(dev)
    res = {"width": W, "height": H, "frames": N, "disparity": D, "iters": a.iters, "reps": a.reps}
    res["three_calls_us"] = events_us(torch, ctx, three, a.iters, a.reps)
    res["one_call_us"] = events_us(torch, ctx, one, a.iters, a.reps)
    res["three_calls_us_again"] = events_us(torch, ctx, three, a.iters, a.reps)     # (order of measurement: the same either way?)
    res["ratio_one_over_three"] = round(res["one_call_us"]["median"] / res["three_calls_us"]["median"], 3)
    res["three_calls_slots"] = slot_times(ctx, three, a.iters)
    res["one_call_slots"] = slot_times(ctx, one, a.iters)
    res["closing_us"] = events_us(torch, ctx, close, a.iters, a.reps)
    res["closing_slots"] = slot_times(ctx, close, a.iters)
    res["closing_timed_us"] = round(sum(v["us_per_pass"] for v in res["closing_slots"].values()), 1)
    ctx.synchronize()
    res["supports"], res["flow_left"], res["flow_right"] = (int(t.sum().item()) for t in (d_ns, d_nl, d_nr))
    res["quads_per_step"] = d_nq.cpu().numpy().tolist()
    ctx.close()
    print(json.dumps(res, sort_keys=True), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(res, sort_keys=True, indent=1) + "\n")


if __name__ == "__main__":
    main()
