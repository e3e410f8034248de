"""A track stream (gpc_hip_track_stream_*) against the offline call it equals: time per pair for pushes of 1, 8 and
all-but-the-first frames, and gpc_hip_track_sequence_device over the same frames in the same run.

Cases: 33 frames of 1024x436 and 9 frames of 1920x1080 (zero forest, frames moving in x and y, the frames of
tools/track_timing.py), sort matcher, non-epipolar.  For each, one JSON object:
  * offline_us: a warmed track_sequence_device call; HIP events around `iters` calls, median and min .. max of `reps`;
  * push_1 / push_8 / push_all: one pass over the video = reset, a push of the first frame, then pushes of 1 / 8 / N - 1
    frames; us per pass and per pair, and per timing slot (gpc_hip_kernel_time) its us per PASS, its launches per pass and
    its mean us per LAUNCH; largest_per_launch names the slot whose single launch takes longest;
  * first_frame_us: reset + the push of the first frame alone (preprocess, hash, save the codes: no pair);
  * derived: the push of N - 1 frames (push_all - first_frame) does the offline call's work plus the carry's bytes --
    restoring and saving the code image, 4 B per pixel each way, read and written, and 20 B per carried record, read and
    written -- and five dependent launches more (two copies in, two out, k_trs_save).  expected_us = offline + those bytes
    at the device copy rate of the same run + 6 us per added launch; ratio = measured / expected.
usage: python tools/track_stream_timing.py [--iters N] [--reps N] [--out FILE] [--only NAME]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from score_timing import copy_rates, events_us  # noqa: E402
from sequence_timing import frames_of  # noqa: E402

LAUNCH_US = 6.0      # a dependent launch
ADDED_LAUNCHES = 5


def slot_times(ctx, fn, iters):
    """{slot: {"us_per_pass", "launches_per_pass", "us_per_launch"}} over `iters` passes of fn, slots never launched left out"""
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_timing()
    for _ in range(iters):
        fn()
    ctx.synchronize()
    out = {k: {"us_per_pass": round(1e3 * ms / iters, 1), "launches_per_pass": round(n / iters, 2), "us_per_launch": round(1e3 * ms / n, 1)}
           for k, (ms, n) in ctx.kernel_times().items() if n}
    ctx.enable_kernel_timing(False)
    return out


def case(g, torch, name, W, H, N, iters, reps, rates):
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    P, cap = N - 1, (W - 26) * (H - 26) + 1
    s = g.Settings(5, 128, 0, False, False, 1)
    d_f = torch.from_numpy(frames_of(W, H, N, N)).to(dev)
    d_out = torch.empty((P, cap, 4), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    d_link = torch.empty((P, cap), dtype=torch.int32, device=dev)
    d_id = torch.empty((P, cap), dtype=torch.int32, device=dev)
    d_tab = torch.empty((P * cap, 4), dtype=torch.int32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    st = ctx.track_stream(W, H, s, cap, P * cap)
    offline = lambda: ctx.track_sequence_device(d_f.data_ptr(), W, H, N, s, d_out.data_ptr(), cap, d_cnt.data_ptr(), 0,
                                                d_link.data_ptr(), d_id.data_ptr(), d_tab.data_ptr(), P * cap, d_n.data_ptr())

    def passes(step):
        def run():
            st.reset()
            st.push_device(d_f.data_ptr(), 1, d_out.data_ptr(), d_cnt.data_ptr(), 0, d_link.data_ptr(), d_id.data_ptr())
            f = 1
            while step and f < N:
                nf = min(step, N - f)
                st.push_device(d_f[f:].data_ptr(), nf, d_out[f - 1:].data_ptr(), d_cnt[f - 1:].data_ptr(), 0,
                               d_link[f - 1:].data_ptr(), d_id[f - 1:].data_ptr())
                f += nf
        return run

    torch.cuda.synchronize(dev)
    res = {"case": name, "width": W, "height": H, "frames": N, "pairs": P, "matcher": "sort", "copy_GBps": rates[0]}
    res["offline_us"] = events_us(torch, ctx, offline, iters, reps)
    res["offline_us_per_pair"] = round(res["offline_us"]["median"] / P, 1)
    res["offline_slots"] = slot_times(ctx, offline, iters)
    n_off = int(d_n.cpu().numpy()[0])
    cnt = d_cnt.cpu().numpy().astype(np.int64)
    res["records"], res["tracks"] = int(cnt.sum()), n_off
    res["first_frame_us"] = events_us(torch, ctx, passes(0), iters, reps)
    for key, step in (("push_1", 1), ("push_8", 8), ("push_all", N - 1)):
        t = events_us(torch, ctx, passes(step), iters, reps)
        kt = slot_times(ctx, passes(step), iters)
        res[key] = {"pass_us": t, "us_per_pair": round(t["median"] / P, 1), "pushes": 1 + (P + step - 1) // step, "slots": kt,
                    "largest_per_launch": max(kt, key=lambda q: kt[q]["us_per_launch"]),
                    "largest_per_pass": max(kt, key=lambda q: kt[q]["us_per_pass"]),
                    "timed_us_per_pass": round(sum(v["us_per_pass"] for v in kt.values()), 1)}
        assert st.state() == (N, P, n_off), (key, st.state(), n_off)     # the same tracks as offline, every time
    carry_bytes = 16 * W * H + 40 * int(min(cnt[-1], cap))
    measured = res["push_all"]["pass_us"]["median"] - res["first_frame_us"]["median"]
    expected = res["offline_us"]["median"] + carry_bytes / rates[0] / 1e3 + LAUNCH_US * ADDED_LAUNCHES
    res["derived"] = {"carry_bytes": carry_bytes, "carry_at_copy_rate_us": round(carry_bytes / rates[0] / 1e3, 1),
                      "added_launches": ADDED_LAUNCHES, "measured_us": round(measured, 1), "expected_us": round(expected, 1),
                      "ratio": round(measured / expected, 3)}
    st.close()
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
    rates = copy_rates(torch, torch.device("cuda", 0))
    out = []
    for name, W, H, N in (("33 x 1024x436, sort", 1024, 436, 33), ("9 x 1920x1080, sort", 1920, 1080, 9)):
        if a.only and a.only not in name:
            continue
        out.append(case(g, torch, name, W, H, N, a.iters, a.reps, rates))
        print(json.dumps(out[-1], sort_keys=True), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
