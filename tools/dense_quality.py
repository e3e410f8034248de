"""The first quality record of the dense chain: what each stage does to the error against ground truth, scored on the
device by gpc_hip_score_fields_device with the library's defaults throughout (no figure is demanded of these; they exist).

Scenes (512 x 256, `--scenes` of them): a foreground rectangle of disparity D_fg over a background of D_bg, both of the
value-noise texture of opengpc_amd/synth.py.  L(x) = P(x + D) and R(x) = P(x + 2 D) per layer, the right image composed with
the rectangle moved by D_fg, so truth is known per left pixel: D_fg inside the rectangle, D_bg outside.  Background pixels
that the foreground hides in the right view are class 1 (occluded), everything else class 0; pixels whose true target lies
left of the right image are ignored.

Stages, forward field of each: fill (densify_batch_device), search (search_batch_device's d_fwd), clean (its d_out),
complete (inpaint_fields_device over the cleaned field, guided by the left image).  Per stage and class (all, visible,
occluded), summed over the scenes: density, EPE, within 1 / 3 / 5 pixels, the outlier rate (3 px and 5 %).
usage: python tools/dense_quality.py [--scenes N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 512, 256


def scene(k):
    """(left, right, truth, ignore, cls, (D_bg, D_fg, rectangle)) of scene k"""
    from opengpc_amd.synth import _texture
    rng = np.random.default_rng(700 + k)
    d_bg, d_fg = int(rng.integers(4, 12)), int(rng.integers(16, 40))
    x0, y0 = int(rng.integers(120, 200)), int(rng.integers(40, 80))
    x1, y1 = x0 + int(rng.integers(120, 220)), y0 + int(rng.integers(90, 140))
    xs, ys = np.arange(W)[None, :], np.arange(H)[:, None]
    rect = lambda x: (x >= x0) & (x < x1) & (ys >= y0) & (ys < y1)
    fg_left, fg_right = rect(xs), rect(xs + d_fg)
    left = np.where(fg_left, _texture(W, H, 1000 + k, d_fg), _texture(W, H, k, d_bg))
    right = np.where(fg_right, _texture(W, H, 1000 + k, 2 * d_fg), _texture(W, H, k, 2 * d_bg))
    truth = np.where(fg_left, d_fg, d_bg).astype(np.float32)
    ignore = (xs - truth < 0).astype(np.uint8)
    cls = (~fg_left & rect(xs - d_bg + d_fg)).astype(np.uint8)
    return left.astype(np.uint8), right.astype(np.uint8), truth, ignore, cls, (d_bg, d_fg, [x0, y0, x1, y1])


def figures(s, b):
    r = lambda x: None if x != x else round(x, 5)
    return {"judged": int(s.tally(b).n_judged), "density": r(s.density(b)), "epe_px": r(s.epe(b)), "rms_px": r(s.rms(b)),
            "within_1_3_5": [r(s.within(k, b)) for k in range(3)], "outlier_rate": r(s.outlier_rate(b))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import opengpc_amd as g
    dev, P = torch.device("cuda", 0), a.scenes
    sc = [scene(k) for k in range(P)]
    up = lambda i: torch.from_numpy(np.stack([s[i] for s in sc])).to(dev)
    d_L, d_R, d_u, d_ign, d_cls = (up(i) for i in range(5))
    ctx = g.Context(0)
    ctx.load_forest(os.path.join(ROOT, "forests", "defaultZeroForest.txt"), W, H)
    s = g.Settings.sparsematch()
    field = lambda: torch.empty((P, 1, H, W), dtype=torch.int32, device=dev)
    d_fill, d_search, d_clean, d_done = field(), field(), field(), field()
    ctx.densify_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, g.Densify(), d_fill.data_ptr(), 0)
    ctx.search_batch_device(d_L.data_ptr(), d_R.data_ptr(), W, H, P, s, g.Densify(), g.Search(), g.Clean(), d_clean.data_ptr(),
                            d_fwd=d_search.data_ptr())
    ctx.inpaint_fields_device(d_clean.data_ptr(), d_L.data_ptr(), 1, W, H, P, g.Inpaint(), d_done.data_ptr())
    d_scores = torch.empty((4, P, 512), dtype=torch.uint8, device=dev)
    stages = (("fill", d_fill), ("search", d_search), ("clean", d_clean), ("complete", d_done))
    for k, (_, d_f) in enumerate(stages):
        ctx.score_fields_device(d_f.data_ptr(), 1, W, H, P, d_u.data_ptr(), 0, d_ign.data_ptr(), g.FieldScorePrm(), d_scores[k].data_ptr(),
                                d_cls.data_ptr())
    ctx.synchronize()
    words = d_scores.cpu().numpy().view(np.int64).reshape(4, P, 64)
    out = {"width": W, "height": H, "scenes": [{"d_bg": q[5][0], "d_fg": q[5][1], "rectangle": q[5][2]} for q in sc],
           "forest": "defaultZeroForest.txt", "settings": "sparsematch, refine radius 0, documented defaults of every stage",
           "score": {"thr_q8": [256, 768, 1280], "out_abs_q8": 768, "out_rel_pm": 50},
           "pixels": {"all": int(words[0, :, 0].sum()), "ignored": int(words[0, :, 1].sum()),
                      "occluded": int(sum(((q[4] != 0) & (q[3] == 0)).sum() for q in sc))}, "stages": {}}
    for k, (name, _) in enumerate(stages):
        t = g.FieldScore.from_buffer_copy(words[k].sum(axis=0).tobytes())
        out["stages"][name] = {"holes": int(t.n_hole), "all": figures(t, None), "visible": figures(t, 0), "occluded": figures(t, 1)}
        print(name, json.dumps(out["stages"][name], sort_keys=True), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
