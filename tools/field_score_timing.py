"""The dense field scorer (gpc_hip_score_fields_device) in one run on one card.  Its kernel has no timing slot (the slot
table is closed), so the call is bracketed with events on the context's stream, a stream borrowed from torch: `reps` calls
between two events, `windows` windows, the median and the fastest window per call.  A call is a 512-byte-per-pair clear
and one launch, so the figure holds both and the launch gaps between calls.

Case: 32 pairs of 1024x436.  The fields are real ones: match, fill and search over the benchmark's synthetic stereo pairs
(C = 1) and over a sequence that alternates the two images of one pair (C = 2); k_search and k_dense_push of that very run
are read from their timing slots and stand beside the scorer.  Truth is a constant plane with scattered pixels without
truth, the ignore mask covers the left columns, the class plane is random.  Inputs exist in `copies` copies that the calls
rotate through, so that the working set (stated) exceeds the 256 MiB Infinity Cache and the bytes come from HBM.
Per variant (C, error plane, bins): ms per call, the bytes the rule must move (8 C + 1 read per pixel, + 1 with a class
plane, + 2 written with the error plane) and their share of the 8 TB/s roof.
usage: python tools/field_score_timing.py [--reps N] [--windows N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROOF = 8e12


def fields(g, torch, ctx, W, H, P, corr):
    """-> (searched forward field on the device, {k_search, k_dense_push: ms per call})"""
    from opengpc_amd.synth import synth_batch, synth_pair
    dev = torch.device("cuda", 0)
    cap = (W - 26) * (H - 26) + 1
    Cn = 2 if corr else 1
    s, fill, sr = g.Settings.sparsematch(), g.Densify(), g.Search()
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
    d_fwd = torch.empty((P, Cn, H, W), dtype=torch.int32, device=dev)
    run = lambda: (ctx.densify_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, fill, d_fwd.data_ptr()),
                   ctx.search_fields_device(d_fwd.data_ptr(), iL, iR, Cn, W, H, P, sr, d_fwd.data_ptr()))
    run()
    ctx.synchronize()
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_timing()
    for _ in range(10):
        run()
    ctx.synchronize()
    t = ctx.kernel_times()
    ctx.enable_kernel_timing(False)
    return d_fwd, {k: round(t[k][0] / t[k][1], 4) for k in ("k_search", "k_dense_push")}


def case(g, torch, W, H, P, corr, reps, windows, copies):
    dev = torch.device("cuda", 0)
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    Cn = 2 if corr else 1
    d_fwd, beside = fields(g, torch, ctx, W, H, P, corr)
    rng = np.random.default_rng(3)
    truth = np.full((P, H, W), 5.0, np.float32)
    truth[rng.random((P, H, W)) < 0.01] = np.nan
    ign = np.zeros((P, H, W), np.uint8)
    ign[:, :, :13] = 1
    cls = rng.integers(0, 4, (P, H, W)).astype(np.uint8)
    sets = []
    for _ in range(copies):
        sets.append(dict(f=d_fwd.clone(), u=torch.from_numpy(truth).to(dev), v=torch.from_numpy(truth).to(dev) if corr else None,
                         i=torch.from_numpy(ign).to(dev), c=torch.from_numpy(cls).to(dev),
                         e=torch.empty((P, H, W), dtype=torch.int16, device=dev)))
    d_scores = torch.empty((P, 512), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ctx.set_stream(st.cuda_stream)
    out = []
    for name, err, bins, prm in (("plain", False, False, g.FieldScorePrm()), ("error plane", True, False, g.FieldScorePrm()),
                                 ("class bins", False, True, g.FieldScorePrm()), ("error plane and class bins", True, True, g.FieldScorePrm()),
                                 ("speed bins", False, False, g.FieldScorePrm(speed_q8=(2560, 10240)))):
        def call(k):
            q = sets[k % copies]
            ctx.score_fields_device(q["f"].data_ptr(), Cn, W, H, P, q["u"].data_ptr(), q["v"].data_ptr() if corr else 0, q["i"].data_ptr(),
                                    prm, d_scores.data_ptr(), q["c"].data_ptr() if bins else 0, q["e"].data_ptr() if err else 0)
        for k in range(2 * copies):                                             # warm-up: the code object, every copy
            call(k)
        ctx.synchronize()
        ms = []
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for k in range(reps):
                call(k)
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
        ctx.synchronize()
        words = d_scores.cpu().numpy().view(np.int64).reshape(P, 64).sum(axis=0)
        need = (8 * Cn + 1 + (1 if bins else 0) + (2 if err else 0)) * W * H * P
        med, best = float(np.median(ms)), float(min(ms))
        out.append({"width": W, "height": H, "pairs": P, "channels": Cn, "variant": name,
                    "kernel": "gpc::k_field_score<%d, %s>" % (Cn, "true" if bins or prm.n_speed else "false"),
                    "ms_per_call_median": round(med, 5), "ms_per_call_fastest_window": round(best, 5), "reps": reps, "windows": windows,
                    "bytes": need, "working_set_bytes": need * copies, "share_of_8TBps": round(need / ROOF / (med * 1e-3), 4),
                    "TBps": round(need / (med * 1e-3) / 1e12, 3), "beside_ms": beside,
                    "pixels": {"ignored": int(words[1]), "no_truth": int(words[2]), "hole": int(words[3]), "judged": int(words[4])}})
        print(json.dumps(out[-1], sort_keys=True), flush=True)
    st.synchronize()
    ctx.set_stream(None)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import opengpc_amd as g
    out = case(g, torch, 1024, 436, 32, False, a.reps, a.windows, a.copies)
    out += case(g, torch, 1024, 436, 32, True, a.reps, a.windows, a.copies)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
