"""The scanline hole closing (gpc_hip_gapfill_fields_device) in one run on one card, over the cleaned fields of real match
output, beside gpc_hip_inpaint_fields_device at its defaults on the same fields in the same run.

Cases: 32 pairs of 1024x436 with the zero forest, sparsematch settings, the documented fill and search in both directions and
the documented cleaner with its cross-check: C = 1 (the benchmark's synthetic stereo pairs) and C = 2 (a sequence of 33
frames that alternates the two images of one pair).  One JSON object per case and parameter set (the documented defaults, the
same with select = 1, and the same with max_gap = 16, which shortens the look-back of the column scan's bands):
  * gapfill_ms: events on the context's stream around the call, per call, five windows of `iters` calls each -- the whole
    stage: the clear of the stats and the three launches (out apart from the field, how and stats asked for); the inputs
    rotate through eight copies of field and guide, 0.57 GB with C = 1 and 1.03 GB with C = 2 against the 256 MiB of the
    last-level cache, so that a call's inputs were evicted before it reads them again; that they come from HBM is inferred
    from these sizes, not measured (no counter run);
  * inpaint_ms: the same events around gpc_hip_inpaint_fields_device on the same fields;
  * must_bytes: what the rule must move -- the field read once, out and how written once -- and roof_share: must_bytes over
    the slowest window's time, over 8 TB/s.  The call as built moves more: design_bytes adds the two extra reads of channel 0
    by the scans and the four distance planes written and read;
  * stats: pixels filled continuous, discontinuous, border, holes left, summed over the pairs; holes_share of all pixels.
The kernels have no timing slot, and the launches' own times were not measured: no rocprofv3 --kernel-trace --stats run of
this tool was made.
usage: python tools/gapfill_timing.py [--iters N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROOF = 8e12
COPIES, WINDOWS = 8, 5


def timed(torch, st, fn, iters):
    """ms per call of fn(k), by events on the context's stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for k in range(iters):
        fn(k)
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
    d_flip = torch.empty_like(d_rec)
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
    d_f, d_b, d_out = (torch.empty((P, Cn, H, W), dtype=torch.int32, device=dev) for _ in range(3))
    d_clean = torch.empty((COPIES, P, Cn, H, W), dtype=torch.int32, device=dev)
    d_guide = torch.empty((COPIES, P, H, W), dtype=torch.uint8, device=dev)
    d_how = torch.empty((P, H, W), dtype=torch.uint8, device=dev)
    d_stats = torch.empty((P, 4), dtype=torch.int32, device=dev)
    ctx.densify_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, fill, d_f.data_ptr())
    ctx.flip_records_device(d_rec.data_ptr(), corr, cap, d_cnt.data_ptr(), P, d_flip.data_ptr(), 0, 0)
    ctx.densify_records_device(d_flip.data_ptr(), corr, cap, d_cnt.data_ptr(), W, H, P, fill, d_b.data_ptr())
    ctx.search_fields_device(d_f.data_ptr(), iL, iR, Cn, W, H, P, g.Search(), d_f.data_ptr())
    ctx.search_fields_device(d_b.data_ptr(), iR, iL, Cn, W, H, P, g.Search(), d_b.data_ptr())
    ctx.clean_fields_device(d_f.data_ptr(), Cn, W, H, P, g.Clean(), d_clean[0].data_ptr(), d_b.data_ptr())
    ctx.synchronize()
    for k in range(1, COPIES):
        d_clean[k].copy_(d_clean[0])
    for k in range(COPIES):
        d_guide[k].copy_(d_L[:P] if corr else d_L)
    torch.cuda.synchronize()
    n = W * H * P
    holes = int((d_clean[0][:, 0] == -2 ** 31).sum())
    ip = g.Inpaint()
    inpaint = lambda k: ctx.inpaint_fields_device(d_clean[k % COPIES].data_ptr(), d_guide[k % COPIES].data_ptr(), Cn, W, H, P, ip,
                                                  d_out.data_ptr())
    inpaint(0)
    ctx.synchronize()
    inpaint_ms = [timed(torch, st, inpaint, iters) for _ in range(WINDOWS)]
    out = []
    d = g.Gapfill()
    for mg, sel in ((d.max_gap, 0), (d.max_gap, 1), (16, 0)):
        gf = g.Gapfill(mg, d.discon_q8, sel, d.border)
        run = lambda k: ctx.gapfill_fields_device(d_clean[k % COPIES].data_ptr(), d_guide[k % COPIES].data_ptr(), Cn, W, H, P, gf,
                                                  d_out.data_ptr(), d_how.data_ptr(), d_stats.data_ptr())
        run(0)
        ctx.synchronize()
        ms = [timed(torch, st, run, iters) for _ in range(WINDOWS)]
        must = n * (4 * Cn + 4 * Cn + 1)
        design = must + n * (2 * 4 + 4 * 2 * 2)
        out.append({"case": name, "width": W, "height": H, "pairs": P, "channels": Cn,
                    "gapfill": [gf.max_gap, gf.discon_q8, gf.select, gf.border], "gapfill_ms": ms, "inpaint_ms": inpaint_ms,
                    "times_inpaint": round(max(ms) / max(inpaint_ms), 3), "must_bytes": must, "design_bytes": design,
                    "roof_share": round(must / (max(ms) * 1e-3) / ROOF, 4), "design_roof_share": round(design / (max(ms) * 1e-3) / ROOF, 4),
                    "stats": d_stats.cpu().numpy().astype(np.int64).sum(0).tolist(), "holes_share": round(holes / n, 5),
                    "iters": iters, "windows": WINDOWS})
        print(json.dumps(out[-1], sort_keys=True), flush=True)
    ctx.set_stream(None)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
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
