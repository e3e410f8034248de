"""The quality record of the propagation (gpc_hip_propagate_fields_device): what it does to the error against ground truth
between the fill and the search, on the four scenes, forest and settings of tools/dense_quality.py, scored
on the device by gpc_hip_score_fields_device.

Rows: fill; fill -> search (today's chain); fill -> propagate -> search over the grid span {1, 2, 4, 8, 16} x iterations
{1, 2, 4, 6} x neighbours {4, 8} at radius 2.  Every row is the same chain of device calls: match, fill, [propagate,] search
(in place), and for the cleaner's cross-check the same over the records read from the right image's side with the two
images exchanged; then clean and complete with the documented defaults.  Per row the figures after the stage (the searched
forward field; the filled one in the row "fill"), after the cleaner and after the completion, each over all judged pixels,
the visible and the occluded ones: density, EPE, within 1 / 3 / 5 pixels.  A propagate row also carries the share of pixels
moved per iteration (from the stats) and its nominal candidate evaluations per pixel, iterations x (1 + neighbours).

"chosen": the grid point with the lowest all-pixel EPE after propagate -> search, ties to the fewer nominal evaluations; and
whether it beats fill -> search.
usage: python tools/propagate_quality.py [--scenes N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SPANS, ITERATIONS, NEIGHBOURS, RADIUS = (1, 2, 4, 8, 16), (1, 2, 4, 6), (4, 8), 2


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
    d_fill_f, d_fill_b, d_f, d_b, d_clean, d_done = (field() for _ in range(6))
    ctx.match_batch_device(iL, iR, W, H, P, g.Settings.sparsematch(), d_rec.data_ptr(), cap, d_cnt.data_ptr(), 0)
    ctx.densify_records_device(d_rec.data_ptr(), False, cap, d_cnt.data_ptr(), W, H, P, g.Densify(), d_fill_f.data_ptr())
    ctx.flip_records_device(d_rec.data_ptr(), False, cap, d_cnt.data_ptr(), P, d_flip.data_ptr(), 0, 0)
    ctx.densify_records_device(d_flip.data_ptr(), False, cap, d_cnt.data_ptr(), W, H, P, g.Densify(), d_fill_b.data_ptr())
    d_scores = torch.empty((3, P, 512), dtype=torch.uint8, device=dev)

    def row(prm, search=True):
        """the figures of one row; prm = None: no propagation"""
        d_f.copy_(d_fill_f)
        d_b.copy_(d_fill_b)
        torch.cuda.synchronize()
        moved = None
        if prm is not None:
            d_stats = torch.zeros((P, prm.iterations, 4), dtype=torch.int32, device=dev)
            ctx.propagate_fields_device(d_f.data_ptr(), iL, iR, 1, W, H, P, prm, d_f.data_ptr(), 0, 0, d_stats.data_ptr())
            ctx.propagate_fields_device(d_b.data_ptr(), iR, iL, 1, W, H, P, prm, d_b.data_ptr())
        if search:
            ctx.search_fields_device(d_f.data_ptr(), iL, iR, 1, W, H, P, g.Search(), d_f.data_ptr())
            ctx.search_fields_device(d_b.data_ptr(), iR, iL, 1, W, H, P, g.Search(), d_b.data_ptr())
        ctx.clean_fields_device(d_f.data_ptr(), 1, W, H, P, g.Clean(), d_clean.data_ptr(), d_b.data_ptr())
        ctx.inpaint_fields_device(d_clean.data_ptr(), iL, 1, W, H, P, g.Inpaint(), d_done.data_ptr())
        for k, d in enumerate((d_f, d_clean, d_done)):
            ctx.score_fields_device(d.data_ptr(), 1, W, H, P, d_u.data_ptr(), 0, d_ign.data_ptr(), g.FieldScorePrm(), d_scores[k].data_ptr(),
                                    d_cls.data_ptr())
        ctx.synchronize()
        words = d_scores.cpu().numpy().view(np.int64).reshape(3, P, 64)
        out = {}
        for k, name in enumerate(("stage", "clean", "complete")):
            t = g.FieldScore.from_buffer_copy(words[k].sum(axis=0).tobytes())
            out[name] = {"holes": int(t.n_hole), "all": figures(t, None), "visible": figures(t, 0), "occluded": figures(t, 1)}
        if prm is not None:
            st = d_stats.cpu().numpy().astype(np.int64).sum(0)
            out["moved_share_per_iteration"] = [round(float(r[3]) / max(1, int(r.sum())), 5) for r in st]
        return out

    out = {"width": W, "height": H, "scenes": [{"d_bg": q[5][0], "d_fg": q[5][1], "rectangle": q[5][2]} for q in sc],
           "forest": "defaultZeroForest.txt", "settings": "sparsematch, refine radius 0, documented defaults of every other stage",
           "score": {"thr_q8": [256, 768, 1280], "out_abs_q8": 768, "out_rel_pm": 50}, "radius": RADIUS,
           "fill": row(None, search=False), "fill_search": row(None), "grid": []}
    for name in ("fill", "fill_search"):
        print(name, json.dumps(out[name], sort_keys=True), flush=True)
    for span in SPANS:
        for it in ITERATIONS:
            for nb in NEIGHBOURS:
                r = dict(row(g.Propagate(RADIUS, span, it, nb)), span=span, iterations=it, neighbours=nb, evaluations=it * (1 + nb))
                out["grid"].append(r)
                print(json.dumps({k: r[k] for k in ("span", "iterations", "neighbours", "moved_share_per_iteration")}),
                      "epe all/visible/occluded", [r["stage"][c]["epe_px"] for c in ("all", "visible", "occluded")],
                      "clean", r["clean"]["all"]["epe_px"], "complete", r["complete"]["all"]["epe_px"], flush=True)
    best = min(out["grid"], key=lambda r: (r["stage"]["all"]["epe_px"], r["evaluations"]))
    out["chosen"] = {"radius": RADIUS, "span": best["span"], "iterations": best["iterations"], "neighbours": best["neighbours"],
                     "epe_px": best["stage"]["all"]["epe_px"], "fill_search_epe_px": out["fill_search"]["stage"]["all"]["epe_px"],
                     "beats_fill_search": bool(best["stage"]["all"]["epe_px"] < out["fill_search"]["stage"]["all"]["epe_px"])}
    print("chosen", json.dumps(out["chosen"], sort_keys=True), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
