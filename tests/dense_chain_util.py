"""The dense chain as a whole -- match, refine, fill, search or aggregate, flip and the same again for the backward field,
clean, complete, score -- on scenes with known truth: chain_cpu() composes the restatements the stages' own tests trust
(refine_util, dense_util, search_util, aggregate_util, clean_util, inpaint_util, field_score_util; called, never copied, and
coupled by nothing but the arrays the C ABI passes between the stages), chain_gpu() queues the same chain as single *_device
calls over sentinel-filled outputs.  Both return the same dict of every intermediate, so that a test compares them name by
name.  conditions() says what the data of a chain reaches: the places the stages' synthetic generators avoid.

The scenes are the occlusion scenes of tools/dense_quality.py, scaled down: a foreground rectangle over a background, both of
opengpc_amd.synth._texture, with per-pixel truth, an ignore plane and an occlusion class.  C = 1: pairs (L, R) with
disparities 2 .. 4 behind and 7 .. 10 in front.  C = 2: three frames, the rectangle moving by (u_fg, v_fg) a frame over a
background moving by (u_bg, v_bg), all four non-zero and the layers different in both components."""
import functools

import numpy as np

import aggregate_util as au
import clean_util as cu
import dense_util as du
import field_score_util as fs
import inpaint_util as iu
import pyramid_util as pu
import refine_util as ru
import search_util as su
import track_util as tu

NONE = -2 ** 31
FILL = 0xA5
SHAPES = ((96, 64), (130, 67))
P = 2                                            # pairs, or three frames
RADIUS = 3                                       # of the refinement between match and fill
FOREST = "zero"
FILL_PRM = du.DEFAULTS
SEARCH_PRM = su.DEFAULTS                         # radius 2, range 1: the label bands of neighbours miss each other from 2R + 3 = 5 on
AGG_PRM = au.DEFAULTS[:6]                        # + paths
# The cleaner's defaults but for speckle_min (64): a parameter chosen for these small images, not a trick of the scenes, so
# that every scene has components below it and components above it (tests/test_dense_chain.py asserts both counts).
CLEAN_PRM = (256, 256, 24, 1)
# The completer's defaults but for its reach: radius 4 over 32 passes covers 128 pixels, more than these images are wide, and
# no hole would be left.  Radius 2 over 3 passes reaches 6 pixels: the occluded band is filled from its rim inwards in more
# than one pass and its middle stays a hole.
INPAINT_PRM = (2, 3, 512, 3)
SCORE_PRM = fs.DEFAULTS
SPEED_PRM = (fs.DEFAULTS[0], 768, 50, (1024,))   # C = 2 without classes: one speed bin boundary at 4 pixels, between the layers
SEEDS = {(1, 96, 64): 1, (1, 130, 67): 1, (2, 96, 64): 1, (2, 130, 67): 2}    # tuned until every condition holds
MIDDLES = ("search", "aggregate", None)           # None: the chain of inpaint_*_device, which has no middle stage
FIELDS = ("fill_fwd", "mid_fwd", "clean_out", "done_out")      # the four stage fields that are scored


def match_width(W):
    """The matcher takes widths that are a multiple of 16 only (the reference's own restriction; check_dims refuses the
    others), the dense stages take any.  So at 130 x 67 the records are matched on the left 128 columns of the images -- a
    record's coordinates are the same in the crop and in the image -- and every stage behind the match runs at 130 x 67."""
    return W - W % 16


def cap_of(W, H):
    return (W - 26) * (H - 26) + 1                # every record of a pair


def _crop(big, M, x, y, W, H):
    return big[M - y:M - y + H, M - x:M - x + W]


@functools.lru_cache(maxsize=None)
def scene(C, W, H, seed):
    """a dict, read-only: imgL, imgR [P, H, W] uint8 (C = 2: frames t and t + 1 of `frames` [P + 1, H, W]), u, v [P, H, W]
    float32 (v None with C = 1), ignore, cls [P, H, W] uint8 (cls 1: background the foreground hides in the other image),
    layers: per pair ((u_bg, v_bg), (u_fg, v_fg), [x0, y0, x1, y1] in the pair's first image)"""
    from opengpc_amd.synth import _texture
    rng = np.random.default_rng([seed, C, W, H])
    xs, ys = np.arange(W)[None, :], np.arange(H)[:, None]
    rect = lambda x, y, r: (x >= r[0]) & (x < r[2]) & (y >= r[1]) & (y < r[3])
    out = {}
    if C == 1:
        L, R, u, ign, cls, layers = [], [], [], [], [], []
        for k in range(P):
            d_bg, d_fg = int(rng.integers(2, 5)), int(rng.integers(7, 11))
            x0, y0 = int(rng.integers(W // 4, W // 3)), int(rng.integers(H // 5, H // 3))
            r = [x0, y0, x0 + int(rng.integers(W // 3, W // 2)), y0 + int(rng.integers(H // 3, H // 2))]
            fg_l, fg_r = rect(xs, ys, r), rect(xs + d_fg, ys, r)
            s = 100 * seed + k
            L.append(np.where(fg_l, _texture(W, H, 1000 + s, d_fg), _texture(W, H, s, d_bg)))
            R.append(np.where(fg_r, _texture(W, H, 1000 + s, 2 * d_fg), _texture(W, H, s, 2 * d_bg)))
            t = np.where(fg_l, d_fg, d_bg).astype(np.float32)
            u.append(t)
            ign.append(xs - t < 0)
            cls.append(~fg_l & rect(xs - d_bg + d_fg, ys, r))
            layers.append(((d_bg, 0), (d_fg, 0), r))
        out.update(imgL=np.stack(L), imgR=np.stack(R), u=np.stack(u), v=None)
    else:
        M = 40
        sgn = lambda: int(rng.choice([-1, 1]))
        bg = (sgn() * int(rng.integers(1, 3)), sgn() * int(rng.integers(1, 3)))
        fg = (-np.sign(bg[0]) * int(rng.integers(5, 8)), -np.sign(bg[1]) * int(rng.integers(4, 7)))
        fg = (int(fg[0]), int(fg[1]))
        x0, y0 = int(rng.integers(W // 3, W // 2)), int(rng.integers(H // 3, H // 2))
        r0 = [x0, y0, x0 + int(rng.integers(W // 3, W // 2)), y0 + int(rng.integers(H // 3, H // 2))]
        big_bg, big_fg = _texture(W + 2 * M, H + 2 * M, 100 * seed, 0), _texture(W + 2 * M, H + 2 * M, 1000 + 100 * seed, 0)
        at = lambda t: [r0[0] + t * fg[0], r0[1] + t * fg[1], r0[2] + t * fg[0], r0[3] + t * fg[1]]
        frames = [np.where(rect(xs, ys, at(t)), _crop(big_fg, M, t * fg[0], t * fg[1], W, H), _crop(big_bg, M, t * bg[0], t * bg[1], W, H))
                  for t in range(P + 1)]
        u, v, ign, cls, layers = [], [], [], [], []
        for t in range(P):
            here = rect(xs, ys, at(t))
            tu_, tv_ = np.where(here, fg[0], bg[0]), np.where(here, fg[1], bg[1])
            u.append(tu_.astype(np.float32))
            v.append(tv_.astype(np.float32))
            ign.append((xs + tu_ < 0) | (xs + tu_ >= W) | (ys + tv_ < 0) | (ys + tv_ >= H))
            cls.append(~here & rect(xs + bg[0], ys + bg[1], at(t + 1)))
            layers.append((bg, fg, at(t)))
        frames = np.ascontiguousarray(np.stack(frames)).astype(np.uint8)
        out.update(frames=frames, imgL=frames[:-1], imgR=frames[1:], u=np.stack(u), v=np.stack(v))
    out.update(ignore=np.stack(ign).astype(np.uint8), cls=np.stack(cls).astype(np.uint8), layers=tuple(map(str, layers)))
    for k in ("u", "v"):                              # no truth in the last three rows, as a data set's invalid pixels
        if out[k] is not None:
            out[k][:, H - 3:, :] = np.nan
    Wm = match_width(W)                               # what the matcher sees: the left Wm columns ("mL" is the frames with C = 2)
    out["mL"], out["mR"] = (out["frames"] if C == 2 else out["imgL"])[:, :, :Wm], out["imgR"][:, :, :Wm]
    for k in ("imgL", "imgR", "u", "v", "ignore", "cls", "frames", "mL", "mR"):
        if out.get(k) is not None:
            out[k] = np.ascontiguousarray(out[k])
            out[k].setflags(write=False)
    return out


def padded(lists, dtype, cap):
    """per-pair record lists -> ([P, cap] of dtype with FILL bytes behind the records, counts [P] int32)"""
    out = np.full((len(lists), cap, dtype.itemsize), FILL, np.uint8).view(dtype).reshape(len(lists), cap)
    for t, r in enumerate(lists):
        out[t, :len(r)] = np.ascontiguousarray(r).view(dtype)
    return out, np.array([len(r) for r in lists], np.int32)


@functools.lru_cache(maxsize=None)
def oracle_matches(C, W, H, seed):
    """the CPU oracle's records of the scene, as the match calls leave them in FILL-filled outputs: (rec [P, cap], cnt [P])"""
    from oracle.pyoracle import sparsematch_settings
    o, sc = pu.the_oracle(), scene(C, W, H, seed)
    rc, f = o.read_forest(pu.FORESTS[FOREST], match_width(W), H)
    assert rc == 0
    if C == 1:
        lists = [o.match_pair(sc["mL"][t], sc["mR"][t], f, sparsematch_settings(5, 128, 0, True, False, False))[0] for t in range(P)]
        return padded(lists, du.SUPPORT, cap_of(W, H))
    rec, cnt, _ = tu.oracle_sequence(o, sc["mL"], f, False, False)
    return padded([rec[t, :cnt[t]] for t in range(P)], du.CORR, cap_of(W, H))


# ---- the stages: each one restatement, over the arrays the stage before it left ----------------------------------------------

def stage_refine(rec, cnt, imgL, imgR):
    return ru.expected_arrays(rec, cnt, imgL, imgR, RADIUS, FILL)[0]


def stage_fill(rec, cnt, ref, W, H):
    return du.densify(rec, cnt, W, H, FILL_PRM, ref)


def stage_flip(rec, cnt, ref):
    """into sentinel-filled arrays or in place, the same bytes: the slots behind the counts stay as they are, and hold the
    sentinel in rec and ref already"""
    return cu.flip(rec, cnt, ref, rec, ref)


def stage_middle(middle, field, imgL, imgR, paths=15):
    """-> (out, cost, choice, stats) and, aggregated, agg"""
    if middle == "search":
        return su.search(field, imgL, imgR, SEARCH_PRM)
    return au.aggregate(field, imgL, imgR, AGG_PRM + (paths,))


def stage_clean(fwd, bwd, check):
    return cu.clean(fwd, bwd if check else None, CLEAN_PRM if check else (-1,) + CLEAN_PRM[1:])


def stage_complete(field, guide):
    return iu.inpaint(field, guide, INPAINT_PRM)


def stage_score(field, sc, speed=False):
    """-> (words [P, 64] int64, err [P, H, W] uint16)"""
    if speed:
        return fs.score(field, sc["u"], sc["v"], sc["ignore"], None, SPEED_PRM)
    return fs.score(field, sc["u"], sc["v"], sc["ignore"], sc["cls"], SCORE_PRM)


MID_NAMES = ("out", "cost", "choice", "stats", "agg")


def links(res, sc, C, middle, check, paths):
    """Every stage's restatement applied to the arrays that res holds of the stage before it: a list of (stage, name ->
    expected array).  res may be a dict that is being filled (chain_cpu: every link reads what the links before it wrote) or
    the read-back of a GPU chain (every link reads what the GPU left)."""
    H, W = sc["imgL"].shape[1:]
    out = []

    def link(stage, names, arrays):
        got = dict(zip(names, arrays))
        out.append((stage, got))
        for n, a in got.items():
            res.setdefault(n, a)

    mid = lambda d: ["mid_" + d if n == "out" else "mid_%s_%s" % (d, n) for n in MID_NAMES]
    link("refine", ["ref"], [stage_refine(res["rec"], res["cnt"], sc["imgL"], sc["imgR"])])
    link("fill", ["fill_fwd", "level"], stage_fill(res["rec"], res["cnt"], res["ref"], W, H))
    fwd, bwd = "fill_fwd", None
    if middle:
        link(middle, mid("fwd"), stage_middle(middle, res["fill_fwd"], sc["imgL"], sc["imgR"], paths))
        fwd = "mid_fwd"
    if check:
        link("flip", ["rec_bwd", "ref_bwd"], stage_flip(res["rec"], res["cnt"], res["ref"]))
        link("fill, backward", ["fill_bwd"], stage_fill(res["rec_bwd"], res["cnt"], res["ref_bwd"], W, H)[:1])
        bwd = "fill_bwd"
        if middle:
            link(middle + ", backward", mid("bwd"), stage_middle(middle, res["fill_bwd"], sc["imgR"], sc["imgL"], paths))
            bwd = "mid_bwd"
    link("clean", ["clean_out", "clean_state", "clean_label", "clean_stats"], stage_clean(res[fwd], res[bwd] if check else None, check))
    link("complete", ["done_out", "done_pass", "done_stats"], stage_complete(res["clean_out"], sc["imgL"]))
    for n in FIELDS:
        if n in res:
            link("score of " + n, ["score_" + n, "err_" + n], stage_score(res[n], sc))
            if C == 2:
                link("score by speed of " + n, ["speed_" + n], stage_score(res[n], sc, True)[:1])
    return out


@functools.lru_cache(maxsize=None)
def chain_cpu(C, W, H, middle="search", check=True, paths=15, seed=None):
    """the whole chain on the CPU from the oracle's matches: a dict name -> array of every intermediate, read-only, computed
    once per configuration.  middle: "search", "aggregate" or None; check: the backward direction and the cross-check."""
    seed = SEEDS[(C, W, H)] if seed is None else seed
    sc = scene(C, W, H, seed)
    rec, cnt = oracle_matches(C, W, H, seed)
    res = dict(rec=rec, cnt=cnt)
    links(res, sc, C, middle, check, paths)
    for a in res.values():
        a.setflags(write=False)
    return res


# ---- the same chain by single device calls -------------------------------------------------------------------------------------

def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))


def filled(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def settings(C):
    import opengpc_amd as g
    return g.Settings(5, 128, 0, C == 1, False, 1)


def params(middle, check, paths=15):
    """(Densify, Search or Aggregate or None, Clean, Inpaint) of the library"""
    import opengpc_amd as g
    mid = g.Search(*SEARCH_PRM) if middle == "search" else g.Aggregate(*(AGG_PRM + (paths,))) if middle else None
    return g.Densify(*FILL_PRM), mid, g.Clean(*(CLEAN_PRM if check else (-1,) + CLEAN_PRM[1:])), g.Inpaint(*INPAINT_PRM)


def score_prm(speed=False):
    import opengpc_amd as g
    return g.FieldScorePrm(*(SPEED_PRM if speed else SCORE_PRM))


def layout(C, W, H):
    """name -> (dtype, shape) of every array of a chain"""
    cap = cap_of(W, H)
    rec = du.CORR if C == 2 else du.SUPPORT
    s = dict(rec=(rec, (P, cap)), cnt=(np.int32, (P,)), ref=(du.REFINEMENT, (P, cap)), rec_bwd=(rec, (P, cap)),
             ref_bwd=(du.REFINEMENT, (P, cap)), level=(np.uint8, (P, H, W)), clean_state=(np.uint8, (P, H, W)),
             clean_label=(np.int32, (P, H, W)), clean_stats=(np.int32, (P, 4)), done_pass=(np.uint8, (P, H, W)), done_stats=(np.int32, (P, 2)))
    for n in ("fill_fwd", "fill_bwd", "mid_fwd", "mid_bwd", "clean_out", "done_out"):
        s[n] = (np.int32, (P, C, H, W))
    for d in ("fwd", "bwd"):
        s.update({"mid_%s_cost" % d: (np.uint16, (P, H, W)), "mid_%s_choice" % d: (np.uint8, (P, H, W)), "mid_%s_stats" % d: (np.int32, (P, 4)),
                  "mid_%s_agg" % d: (np.uint32, (P, H, W))})
    for n in FIELDS:
        s.update({"score_" + n: (np.int64, (P, 64)), "speed_" + n: (np.int64, (P, 64)), "err_" + n: (np.uint16, (P, H, W))})
    return s


def nbytes(C, W, H, name):
    dt, shape = layout(C, W, H)[name]
    return int(np.prod(shape)) * np.dtype(dt).itemsize


def typed(name, raw, C, W, H):
    """the bytes read back from a device buffer as the array chain_cpu gives under that name"""
    dt, shape = layout(C, W, H)[name]
    return np.ascontiguousarray(raw).view(np.uint8).reshape(-1).view(dt).reshape(shape)


def chain_calls(C, W, H, middle="search", check=True, paths=15, in_place=False, scores=True):
    """The chain as single *_device calls: (outputs: name -> the name of the buffer that holds it, in the order they are
    first written; calls: functions (ctx, p), one library call each, over the pointers p[name] of the outputs' buffers and
    of the inputs "L", "R" (C = 2: "L" is the frames, "R" is not read), their crops for the matcher "mL", "mR" (see
    match_width), "u", "v", "ign", "cls").  in_place: every stage that the
    header allows writes over its input (search, aggregate and complete: out == field; the flip: out == rec) -- then several
    names share a buffer, which holds what the LAST of them left."""
    cap, corr, Wm = cap_of(W, H), C == 2, match_width(W)
    s = settings(C)
    fill, mid, clean, inp = params(middle, check, paths)
    iL = lambda p: p["L"]
    iR = lambda p: p["L"] + W * H if corr else p["R"]
    outs, calls = {}, []

    def out(name, alias=None):
        outs[name] = outs[alias] if alias else name
        return name

    for n in ("rec", "cnt", "ref", "fill_fwd", "level"):
        out(n)
    if corr:
        calls.append(lambda c, p: c.match_sequence_device(p["mL"], Wm, H, P + 1, s, p["rec"], cap, p["cnt"]))
    else:
        calls.append(lambda c, p: c.match_batch_device(p["mL"], p["mR"], Wm, H, P, s, p["rec"], cap, p["cnt"]))
    calls.append(lambda c, p: c.refine_records_device(p["rec"], corr, cap, p["cnt"], iL(p), iR(p), W, H, P, RADIUS, p["ref"]))
    calls.append(lambda c, p: c.densify_records_device(p["rec"], corr, cap, p["cnt"], W, H, P, fill, p["fill_fwd"], p["level"], p["ref"]))

    def middle_stage(d, field, a, b):
        m = out("mid_" + d, field if in_place else None)
        q = {n: out("mid_%s_%s" % (d, n)) for n in MID_NAMES[1:] if n != "agg" or middle == "aggregate"}
        if middle == "search":
            calls.append(lambda c, p: c.search_fields_device(p[field], a(p), b(p), C, W, H, P, mid, p[m], p[q["cost"]], p[q["choice"]], p[q["stats"]]))
        else:
            calls.append(lambda c, p: c.aggregate_fields_device(p[field], a(p), b(p), C, W, H, P, mid, p[m], p[q["cost"]], p[q["choice"]],
                                                                p[q["stats"]], p[q["agg"]]))
        return m

    fwd = middle_stage("fwd", "fill_fwd", iL, iR) if middle else "fill_fwd"
    bwd = None
    if check:
        rb, fb = out("rec_bwd", "rec" if in_place else None), out("ref_bwd", "ref" if in_place else None)
        calls.append(lambda c, p: c.flip_records_device(p["rec"], corr, cap, p["cnt"], P, p[rb], p["ref"], p[fb]))
        out("fill_bwd")
        calls.append(lambda c, p: c.densify_records_device(p[rb], corr, cap, p["cnt"], W, H, P, fill, p["fill_bwd"], 0, p[fb]))
        bwd = middle_stage("bwd", "fill_bwd", iR, iL) if middle else "fill_bwd"
    for n in ("clean_out", "clean_state", "clean_label", "clean_stats"):
        out(n)
    calls.append(lambda c, p: c.clean_fields_device(p[fwd], C, W, H, P, clean, p["clean_out"], p[bwd] if check else 0, p["clean_state"],
                                                    p["clean_label"], p["clean_stats"]))
    out("done_out", "clean_out" if in_place else None), out("done_pass"), out("done_stats")
    calls.append(lambda c, p: c.inpaint_fields_device(p["clean_out"], iL(p), C, W, H, P, inp, p["done_out"], p["done_pass"], p["done_stats"]))
    if scores and not in_place:
        for n in FIELDS:
            if n not in outs:
                continue
            out("score_" + n), out("err_" + n)
            calls.append(lambda c, p, n=n: c.score_fields_device(p[n], C, W, H, P, p["u"], p["v"] if corr else 0, p["ign"], score_prm(),
                                                                 p["score_" + n], p["cls"], p["err_" + n]))
            if corr:
                out("speed_" + n)
                calls.append(lambda c, p, n=n: c.score_fields_device(p[n], C, W, H, P, p["u"], p["v"], p["ign"], score_prm(True), p["speed_" + n]))
    return outs, calls


def chain_gpu(ctx, C, W, H, middle="search", check=True, paths=15, seed=None, in_place=False, scores=True):
    """chain_calls() in a context whose forest is loaded for (match_width(W), H), every output buffer filled with the sentinel first and
    read back at the end: the dict of chain_cpu (in_place: see chain_calls)"""
    import torch
    seed = SEEDS[(C, W, H)] if seed is None else seed
    sc = scene(C, W, H, seed)
    outs, calls = chain_calls(C, W, H, middle, check, paths, in_place, scores)
    T = dict(L=dev(sc["frames"] if C == 2 else sc["imgL"]), R=dev(sc["imgR"]), u=dev(sc["u"]), ign=dev(sc["ignore"]), cls=dev(sc["cls"]))
    T["mL"], T["mR"] = (dev(sc["mL"]), dev(sc["mR"])) if match_width(W) != W else (T["L"], T["R"])
    if C == 2:
        T["v"] = dev(sc["v"])
    for name, buf in outs.items():
        if buf == name:
            T[name] = filled(nbytes(C, W, H, name))
    p = {n: t.data_ptr() for n, t in T.items()}
    p.update({n: p[b] for n, b in outs.items()})
    torch.cuda.synchronize()
    for call in calls:
        call(ctx, p)
    ctx.synchronize()
    back = {n: T[n].cpu().numpy() for n in set(outs.values())}
    return {n: typed(n, back[b], C, W, H) for n, b in outs.items()}


def same(got, want, what, names=None):
    """every array of want (or those in names) equals got's: exact, the failure naming the stage's array, the number of
    differing elements and the first of them"""
    for n in (names if names is not None else sorted(want)):
        g_, w = got[n], want[n]
        assert g_.dtype == w.dtype and g_.shape == w.shape, (what, n, g_.dtype, w.dtype, g_.shape, w.shape)
        if not np.array_equal(g_, w):
            bad = np.argwhere(g_ != w)
            raise AssertionError("%s: %s differs at %d of %d elements, the first at %s: %s, expected %s" % (
                what, n, len(bad), w.size, bad[0].tolist(), g_[tuple(bad[0])], w[tuple(bad[0])]))


# ---- what a chain's data reaches -------------------------------------------------------------------------------------------------

def q8_parts(field):
    """the Q8 part of every valued element of [P, C, H, W], per channel: |F| & 255 with the value's sign -> list of int64 arrays"""
    F = field.astype(np.int64)
    valued = F[:, 0] != NONE
    return [(np.sign(F[:, c]) * (np.abs(F[:, c]) & 255))[valued & (F[:, c] != NONE)] for c in range(F.shape[1])]


def base_steps(field, R):
    """the differences of the whole-pixel bases of adjacent live pixels of [P, C, H, W]: (horizontal, vertical) int64 arrays of
    the largest per-channel difference; live: valued with some target inside the image"""
    hs, vs = [], []
    for f in field:
        valued, r, bx, by = su.base(f)
        C, H, W = f.shape
        live = np.zeros((H, W), bool)
        for kx, ky in au.labels(C, R):
            live |= valued & (bx + kx >= 0) & (bx + kx < W) & (by + ky >= 0) & (by + ky < H)
        d = np.abs(r[:, :, 1:] - r[:, :, :-1]).max(0)
        hs.append(d[live[:, 1:] & live[:, :-1]])
        d = np.abs(r[:, 1:, :] - r[:, :-1, :]).max(0)
        vs.append(d[live[1:, :] & live[:-1, :]])
    return np.concatenate(hs), np.concatenate(vs)


def conditions(res, C, W, H, middle, check):
    """name -> bool of every condition the chain's data must meet to prove anything (tests/test_dense_chain.py lists them),
    from the arrays of one chain -- chain_cpu's or the GPU's own"""
    c = {}
    R = SEARCH_PRM[1]
    for d in ("fwd", "bwd") if check else ("fwd",):
        parts = q8_parts(res["fill_" + d])
        for ch, q in enumerate(parts):
            a = np.abs(q)
            c["fill_%s ch %d: a Q8 part in 101 .. 127" % (d, ch)] = bool(((a >= 101) & (a <= 127)).any())
            c["fill_%s ch %d: a Q8 part in 129 .. 155" % (d, ch)] = bool(((a >= 129) & (a <= 155)).any())
    if middle:
        outs = [res["mid_fwd"]] + ([res["mid_bwd"]] if check else [])
        F = np.concatenate([o.astype(np.int64).ravel() for o in outs])
        F = F[F != NONE]
        half = (np.abs(F) & 255) == 128
        c["middle: a kept value with a low byte of 128, positive"] = bool((half & (F > 0)).any())
        c["middle: a kept value with a low byte of 128, negative"] = bool((half & (F < 0)).any())
        st = res["mid_fwd_stats"].sum(0)
        c["middle: kept pixels"] = bool(st[0] > 0)
        c["middle: unmatched pixels (no target inside the image)"] = bool(st[2] > 0 or (check and res["mid_bwd_stats"].sum(0)[2] > 0))
    hs, vs = base_steps(res["fill_fwd"], R)
    if check:
        hb, vb = base_steps(res["fill_bwd"], R)
        hs, vs = np.concatenate([hs, hb]), np.concatenate([vs, vb])
    for name, s in (("horizontally", hs), ("vertically", vs)):
        c["prior: %s adjacent bases differ by more than 2R + 2" % name] = bool((s > 2 * R + 2).any())
    both = np.concatenate([hs, vs])
    c["prior: adjacent bases differ by exactly 2R + 1"] = bool((both == 2 * R + 1).any())
    c["prior: adjacent bases differ by exactly 2R + 2"] = bool((both == 2 * R + 2).any())
    st = res["clean_stats"].sum(0)
    c["clean: kept pixels"] = bool(st[0] > 0)
    if check:
        c["clean: pixels that failed the cross-check"] = bool(st[2] > 0)
    c["clean: pixels removed as speckles"] = bool(st[3] > 0)
    src = res["mid_fwd"] if middle else res["fill_fwd"]
    kept = res["clean_state"] == 0
    c["clean: the median changes a kept pixel"] = bool(((res["clean_out"] != src).any(1) & kept).any())
    pz = res["done_pass"]
    c["complete: holes filled in a pass after the first"] = bool(((pz > 1) & (pz < 255)).any())
    c["complete: holes left"] = bool((pz == 255).any())
    hole = res["clean_out"][:, 0] == NONE
    ys, xs = np.mgrid[0:H, 0:W]
    edge = ((xs % 32 == 0) | (xs % 32 == 31) | (ys % 32 == 0) | (ys % 32 == 31))[None]
    c["complete: a hole on a 32 x 32 tile edge"] = bool((hole & edge).any())
    for n in FIELDS:
        if "score_" + n not in res:
            continue
        w = res["score_" + n].sum(0)
        last = n in ("clean_out", "done_out")      # the fill and the middle stage leave (almost) no hole: asked of the cleaned fields
        c["score %s: judged, ignored and no-truth pixels" % n] = bool(w[fs.ALL] > 0 and w[1] > 0 and w[2] > 0)
        if last:
            c["score %s: holes" % n] = bool(w[3] > 0)
        c["score %s: both occlusion classes" % n] = bool(w[fs.BIN] > 0 and w[fs.BIN + fs.TALLY] > 0)
        if C == 2:
            v = res["speed_" + n].sum(0)
            c["score %s: two speed bins" % n] = bool(v[fs.BIN] > 0 and v[fs.BIN + fs.TALLY] > 0)
    return c
