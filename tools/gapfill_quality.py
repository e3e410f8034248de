"""The quality record of the scanline hole closing (gpc_hip_gapfill_fields_device): what it does to the error against ground
truth between the cleaner and the completion, on the four scenes, forest and settings of tools/dense_quality.py (DESIGN.md
4.19), scored on the device by gpc_hip_score_fields_device.

The cleaned field is today's chain at the documented defaults of every stage: match, fill, propagate, search (in place), the
same over the records read from the right image's side with the two images exchanged, then the cleaner with its cross-check.
Arms over that one field: clean -> complete (today's); clean -> gapfill; clean -> gapfill -> complete.  The gapfill arms run
over the grid max_gap {8, 16, 32, 64, 128} x discon_q8 {128, 256, 512} x select {0, 1} x border {0, 1}.  Per arm, over all
judged pixels, the visible and the occluded ones: density, EPE, within 1 / 3 / 5 pixels; a gapfill row also carries its stats
(pixels filled continuous, discontinuous, border, holes left).

"chosen": the grid point with the lowest all-pixel EPE after gapfill -> complete, ties to the smaller max_gap, then select 0
(then, the rule being silent, the smaller discon_q8 and border 0); and what the occluded pixels gain against today's arm.
usage: python tools/gapfill_quality.py [--scenes N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
MAX_GAPS, DISCONS, SELECTS, BORDERS = (8, 16, 32, 64, 128), (128, 256, 512), (0, 1), (0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import opengpc_amd as g
    from dense_quality import W, H, figures, scene
    dev, P = torch.device("cuda", 0), a.scenes
    sc = [scene(k) for k in range(P)]
    up = lambda i: torch.from_numpy(np.stack([s[i] for s in sc])).to(dev)
    d_L, d_R, d_u, d_ign, d_cls = (up(i) for i in range(5))
    iL, iR = d_L.data_ptr(), d_R.data_ptr()
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    cap = (W - 26) * (H - 26) + 1
    d_rec = torch.empty((P, cap, 3), dtype=torch.int32, device=dev)
    d_flip = torch.empty_like(d_rec)
    d_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    field = lambda: torch.empty((P, 1, H, W), dtype=torch.int32, device=dev)
    d_f, d_b, d_clean, d_gap, d_done = (field() for _ in range(5))
    ctx.match_batch_device(iL, iR, W, H, P, g.Settings.sparsematch(), d_rec.data_ptr(), cap, d_cnt.data_ptr(), 0)
    ctx.densify_records_device(d_rec.data_ptr(), False, cap, d_cnt.data_ptr(), W, H, P, g.Densify(), d_f.data_ptr())
    ctx.flip_records_device(d_rec.data_ptr(), False, cap, d_cnt.data_ptr(), P, d_flip.data_ptr(), 0, 0)
    ctx.densify_records_device(d_flip.data_ptr(), False, cap, d_cnt.data_ptr(), W, H, P, g.Densify(), d_b.data_ptr())
    for d, x, y in ((d_f, iL, iR), (d_b, iR, iL)):
        ctx.propagate_fields_device(d.data_ptr(), x, y, 1, W, H, P, g.Propagate(), d.data_ptr())
        ctx.search_fields_device(d.data_ptr(), x, y, 1, W, H, P, g.Search(), d.data_ptr())
    ctx.clean_fields_device(d_f.data_ptr(), 1, W, H, P, g.Clean(), d_clean.data_ptr(), d_b.data_ptr())
    d_scores = torch.empty((2, P, 512), dtype=torch.uint8, device=dev)
    d_stats = torch.zeros((P, 4), dtype=torch.int32, device=dev)

    def scored(fields, names):
        for k, d in enumerate(fields):
            ctx.score_fields_device(d.data_ptr(), 1, W, H, P, d_u.data_ptr(), 0, d_ign.data_ptr(), g.FieldScorePrm(), d_scores[k].data_ptr(),
                                    d_cls.data_ptr())
        ctx.synchronize()
        words = d_scores.cpu().numpy().view(np.int64).reshape(2, P, 64)
        out = {}
        for k, name in enumerate(names):
            t = g.FieldScore.from_buffer_copy(words[k].sum(axis=0).tobytes())
            out[name] = {"holes": int(t.n_hole), "all": figures(t, None), "visible": figures(t, 0), "occluded": figures(t, 1)}
        return out

    ctx.inpaint_fields_device(d_clean.data_ptr(), iL, 1, W, H, P, g.Inpaint(), d_done.data_ptr())
    today = scored((d_clean, d_done), ("clean", "complete"))
    out = {"width": W, "height": H, "scenes": [{"d_bg": q[5][0], "d_fg": q[5][1], "rectangle": q[5][2]} for q in sc],
           "forest": "defaultZeroForest.txt",
           "settings": "sparsematch, refine radius 0, fill -> propagate -> search -> clean at the documented defaults of every stage",
           "score": {"thr_q8": [256, 768, 1280], "out_abs_q8": 768, "out_rel_pm": 50}, "clean": today["clean"],
           "clean_complete": today["complete"], "grid": []}
    for name in ("clean", "clean_complete"):
        print(name, json.dumps(out[name], sort_keys=True), flush=True)
    for mg in MAX_GAPS:
        for dq in DISCONS:
            for sel in SELECTS:
                for b in BORDERS:
                    ctx.gapfill_fields_device(d_clean.data_ptr(), iL, 1, W, H, P, g.Gapfill(mg, dq, sel, b), d_gap.data_ptr(), 0, d_stats.data_ptr())
                    ctx.inpaint_fields_device(d_gap.data_ptr(), iL, 1, W, H, P, g.Inpaint(), d_done.data_ptr())
                    r = dict(scored((d_gap, d_done), ("gapfill", "gapfill_complete")), max_gap=mg, discon_q8=dq, select=sel, border=b,
                             stats=d_stats.cpu().numpy().astype(np.int64).sum(0).tolist())
                    out["grid"].append(r)
                    print(json.dumps({k: r[k] for k in ("max_gap", "discon_q8", "select", "border", "stats")}), "gapfill all/vis/occ",
                          [r["gapfill"][c]["epe_px"] for c in ("all", "visible", "occluded")], "density", r["gapfill"]["all"]["density"],
                          "then complete", [r["gapfill_complete"][c]["epe_px"] for c in ("all", "visible", "occluded")], flush=True)
    best = min(out["grid"], key=lambda r: (r["gapfill_complete"]["all"]["epe_px"], r["max_gap"], r["select"], r["discon_q8"], r["border"]))
    t, n = out["clean_complete"], best["gapfill_complete"]
    out["chosen"] = {"max_gap": best["max_gap"], "discon_q8": best["discon_q8"], "select": best["select"], "border": best["border"],
                     "epe_px": n["all"]["epe_px"], "today_epe_px": t["all"]["epe_px"],
                     "occluded_epe_px": n["occluded"]["epe_px"], "today_occluded_epe_px": t["occluded"]["epe_px"],
                     "occluded_within_1": n["occluded"]["within_1_3_5"][0], "today_occluded_within_1": t["occluded"]["within_1_3_5"][0],
                     "beats_today": bool(n["all"]["epe_px"] < t["all"]["epe_px"]),
                     "occluded_gain": bool(n["occluded"]["epe_px"] < t["occluded"]["epe_px"])}
    print("chosen", json.dumps(out["chosen"], sort_keys=True), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
