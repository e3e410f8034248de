#!/usr/bin/env python3
"""Writes tests/golden/ref_full_vectors.json: what the reference's own classes (oracle/_ref/libgpc_ref_full*.so, built by
oracle/Makefile where the reference tree is present) return on the fixed case list of tests/ref_full_util.py.

Recorded results only: per matching case the settings, the candidate counts, counts and FNV-1a-64 of the descriptors,
of stereoMatch's correspondences (int32 sx, sy, tx, ty) and of rectifiedMatch's supports (int32 x, y, d, the
Appendix C convention); for a Q2 tie the other admissible result beside the reference's own; for a call the reference
leaves undefined a flag and nothing else.  Training: the eight statistics of evalSplit (doubles as hex) and the FNV of
the marks after markSplitSamples.  Colour ramp: the FNV of the RGB image.  Needs no GPU."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle.pyoracle import Oracle, RefFull  # noqa: E402
import ref_full_util as U  # noqa: E402


def main():
    o = Oracle()          # for its FNV and the constructed rows' smooth images only
    refs = {False: RefFull(False), True: RefFull(True)}
    out = {"about": "results of the reference's Forest / Fern / Buffer classes; written by tools/record_ref_full.py",
           "matching": [], "training": [], "ramp": []}
    for cid, L, R, pre, forest, st in U.recorded_cases(o):
        reff = refs[bool(st.naive)]
        m = reff.match_pre(pre[0], pre[1], U.FORESTS[forest], st) if pre else reff.match_pair(L, R, U.FORESTS[forest], st)
        H, W = (pre[0][0] if pre else L).shape
        rec = dict(id=cid, W=W, H=H, forest=forest, settings=U.settings_dict(st), n_cand=[len(m.mask_l), len(m.mask_r)],
                   mask=[U.hx(o.fnv(m.mask_l)), U.hx(o.fnv(m.mask_r))],
                   states=[U.hx(o.fnv(m.states_l)), U.hx(o.fnv(m.states_r))], undefined=bool(m.undefined))
        if not m.undefined:
            alts = U.alternatives(m, st)
            rec["result"] = U.result_record(o, *alts[0])
            if len(alts) > 1:
                rec["tie_alternatives"] = [dict(U.result_record(o, c, s), target=[int(c["tx"][-1]), int(c["ty"][-1])])
                                           for c, s in alts[1:]]
        out["matching"].append(rec)
    for cid, t, marks, params, until, w1 in U.training_cases():
        s = refs[False].eval_split(t, marks, params, until, w1)
        after = marks.copy()
        refs[False].mark_split_samples(t, after, params, until + 1)
        out["training"].append(dict(id=cid, counts=[int(s[k]) for k in ("tp", "fp", "fn", "tot")],
                                    stats=[float(s[k]).hex() for k in ("prec", "rec", "hmean", "convcomb")],
                                    marks=U.hx(o.fnv(after))))
    img, cases = U.ramp_cases()
    for name, supp in cases.items():
        out["ramp"].append(dict(id=name, rgb=U.hx(o.fnv(refs[False].disparity_vis(img, supp)))))
    with open(U.VECTORS, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    ties = [r["id"] for r in out["matching"] if "tie_alternatives" in r]
    undefined = [r["id"] for r in out["matching"] if r["undefined"]]
    print("%d matching cases (ties: %s, undefined: %s), %d training, %d ramp -> %s"
          % (len(out["matching"]), ties, undefined, len(out["training"]), len(out["ramp"]), U.VECTORS))


if __name__ == "__main__":
    main()
