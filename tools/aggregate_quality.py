"""What the scanline aggregation (gpc_hip_aggregate_*) does to the error of the dense chain, beside the fill and the search:
the four scenes of tools/dense_quality.py (its scene()), the same forest and settings, scored on the device by
gpc_hip_score_fields_device.

Rows: fill; search; aggregate at paths = 15 over a small grid of (p1, p2); aggregate at paths = 3 at the best of them (lowest
EPE over all pixels after the stage).  Of every row but the fill: the forward field after the stage, after the cleaner
(cross-checked against the backward field of the same stage) and after the completion.  Per field: density, EPE over all,
visible and occluded pixels, the share within 1 px.
usage: python tools/aggregate_quality.py [--scenes N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GRID = ((4, 16), (8, 32), (16, 64), (32, 128), (64, 256), (128, 512), (64, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import opengpc_amd as g
    from dense_quality import H, W, scene
    dev, P = torch.device("cuda", 0), a.scenes
    sc = [scene(k) for k in range(P)]
    up = lambda i: torch.from_numpy(np.stack([s[i] for s in sc])).to(dev)
    d_L, d_R, d_u, d_ign, d_cls = (up(i) for i in range(5))
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    s = g.Settings.sparsematch()
    field = lambda: torch.empty((P, 1, H, W), dtype=torch.int32, device=dev)
    d_scores = torch.empty((P, 512), dtype=torch.uint8, device=dev)

    def score(d_f):
        ctx.score_fields_device(d_f.data_ptr(), 1, W, H, P, d_u.data_ptr(), 0, d_ign.data_ptr(), g.FieldScorePrm(), d_scores.data_ptr(),
                                d_cls.data_ptr())
        ctx.synchronize()
        t = g.FieldScore.from_buffer_copy(d_scores.cpu().numpy().view(np.int64).reshape(P, 64).sum(axis=0).tobytes())
        r = lambda x: None if x != x else round(x, 5)
        return {"density": r(t.density(None)), "epe_px": r(t.epe(None)), "epe_visible_px": r(t.epe(0)), "epe_occluded_px": r(t.epe(1)),
                "within_1": r(t.within(0, None)), "within_1_visible": r(t.within(0, 0))}

    def chain(run):
        """run(d_clean, d_fwd) is a match form; -> the figures after the stage, the cleaner and the completion"""
        d_fwd, d_clean, d_done = field(), field(), field()
        run(d_clean, d_fwd)
        ctx.inpaint_fields_device(d_clean.data_ptr(), d_L.data_ptr(), 1, W, H, P, g.Inpaint(), d_done.data_ptr())
        return {"stage": score(d_fwd), "clean": score(d_clean), "complete": score(d_done)}

    args = (d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, g.Densify())
    d_fill = field()
    ctx.densify_batch_device(*args, d_fill.data_ptr(), 0)
    rows = {"fill": {"stage": score(d_fill)}}
    rows["search"] = chain(lambda d_c, d_f: ctx.search_batch_device(*args, g.Search(), g.Clean(), d_c.data_ptr(), d_fwd=d_f.data_ptr()))
    agg = lambda p1, p2, paths: chain(lambda d_c, d_f: ctx.aggregate_batch_device(
        *args, g.Aggregate(2, 1, 1, 0xFFFF, p1, p2, paths), g.Clean(), d_c.data_ptr(), d_fwd=d_f.data_ptr()))
    for p1, p2 in GRID:
        rows["aggregate p1=%d p2=%d paths=15" % (p1, p2)] = agg(p1, p2, 15)
    best = min(GRID, key=lambda q: rows["aggregate p1=%d p2=%d paths=15" % q]["stage"]["epe_px"])
    rows["aggregate p1=%d p2=%d paths=3" % best] = agg(best[0], best[1], 3)
    for name, r in rows.items():
        print(name, json.dumps(r, sort_keys=True), flush=True)
    ctx.close()
    out = {"width": W, "height": H, "scenes": P, "forest": "defaultZeroForest.txt", "best_p1_p2": list(best),
           "settings": "sparsematch, refine radius 0, radius 2, range 1, sub-pixel, no ceiling; documented defaults of every other stage",
           "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
