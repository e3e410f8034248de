"""The rule of the scanline hole closing (include/gpc_hip.h, gpc_hip_gapfill_*) restated twice: gapfill_plain pixel by pixel
with Python loops and Python integers, straight from the definition of a run (walk left, right, up and down from the hole),
and gapfill_np with numpy (the position of the nearest valued pixel on either side by a running maximum / minimum of
indices, the ends gathered, everything in int64 / uint64).  Neither shares anything with the kernels' method (ballot masks
and a carried scalar along rows, banded column walks with a look-back, uint16 distance planes with two codes).  Also the
fields and guides the tests run on, by seed, and conditions(): what a set of cases reaches."""
import functools

import numpy as np

NONE = -2 ** 31
IMAX, IMIN1 = 2 ** 31 - 1, -2 ** 31 + 1
DEFAULTS = (64, 128, 0, 1)          # max_gap, discon_q8, select, border
CHUNK, BAND = 64, 64               # the kernels' row chunk and least band of rows: only conditions() knows of them


def band_of(max_gap):
    return max(BAND, max_gap)


def mean(S, N):
    """sgn(S) * ((2 |S| + N) div (2 N)) of Python integers"""
    q = (2 * abs(S) + N) // (2 * N)
    return -q if S < 0 else q


# ---- pixel by pixel ----------------------------------------------------------------------------------------------------------

def _axis_plain(F, G, C, W, H, x, y, dx, dy, prm):
    """the candidate of the axis (dx, dy) for the hole (x, y): None where the axis is not usable, else (n, kind, values)"""
    max_gap, discon, select, border = prm
    inside = lambda px, py: 0 <= px < W and 0 <= py < H
    da = 1
    while inside(x - da * dx, y - da * dy) and F[0][y - da * dy][x - da * dx] == NONE:
        da += 1
    db = 1
    while inside(x + db * dx, y + db * dy) and F[0][y + db * dy][x + db * dx] == NONE:
        db += 1
    ax, ay, bx, by = x - da * dx, y - da * dy, x + db * dx, y + db * dy
    va, vb = inside(ax, ay), inside(bx, by)
    n = da + db - 1
    if n > max_gap or not (va or vb) or (not (va and vb) and not border):
        return None
    if not (va and vb):
        ex, ey = (ax, ay) if va else (bx, by)
        return n, 3, [F[c][ey][ex] for c in range(C)]
    A, B = [F[c][ay][ax] for c in range(C)], [F[c][by][bx] for c in range(C)]
    if all(abs(a - b) <= discon for a, b in zip(A, B)):
        return n, 1, [mean(a * db + b * da, da + db) for a, b in zip(A, B)]
    ka, kb = (sum(a * a for a in A), da), (sum(b * b for b in B), db)
    if select == 1:
        ka, kb = (abs(G[y][x] - G[ay][ax]),) + ka, (abs(G[y][x] - G[by][bx]),) + kb
    return n, 2, B if kb < ka else A


def gapfill_plain(field, guide, prm=DEFAULTS):
    """one pair: field [C, H, W] int32, guide [H, W] uint8 or None -> out [C, H, W] int32, how [H, W] uint8, stats [4] int32"""
    C, H, W = field.shape
    F = [[[int(field[c, y, x]) for x in range(W)] for y in range(H)] for c in range(C)]
    G = [[int(guide[y, x]) for x in range(W)] for y in range(H)] if guide is not None else None
    out, how, stats = np.array(field, np.int32), np.zeros((H, W), np.uint8), [0, 0, 0, 0]
    for y in range(H):
        for x in range(W):
            if F[0][y][x] != NONE:
                continue
            h, v = _axis_plain(F, G, C, W, H, x, y, 1, 0, prm), _axis_plain(F, G, C, W, H, x, y, 0, 1, prm)
            if h is None and v is None:
                out[:, y, x], how[y, x] = NONE, 255
                stats[3] += 1
                continue
            vert = h is None or (v is not None and v[0] < h[0])
            n, kind, val = v if vert else h
            out[:, y, x], how[y, x] = val, kind + (3 if vert else 0)
            stats[kind - 1] += 1
    return out, how, np.array(stats, np.int32)


# ---- numpy -------------------------------------------------------------------------------------------------------------------

def _axis_np(F, G, prm):
    """along the last axis of F [P, C, H, W] int64 (G [P, H, W] int64 or None): a dict of [P, H, W] planes -- usable, n, da,
    db, kind -- and val [P, C, H, W], meaningful at the holes"""
    max_gap, discon, select, border = prm
    P, C, H, W = F.shape
    xs = np.arange(W, dtype=np.int64)
    valued = F[:, 0] != NONE
    pa = np.maximum.accumulate(np.where(valued, xs, -1), axis=2)                       # the nearest valued x at or left of x
    pb = np.minimum.accumulate(np.where(valued, xs, W)[..., ::-1], axis=2)[..., ::-1]  # at or right of x
    da, db = xs - pa, pb - xs
    va, vb = pa >= 0, pb < W
    n = da + db - 1
    usable = ~valued & (n <= max_gap) & ((va & vb) | ((va | vb) & bool(border)))
    ia, ib = np.clip(pa, 0, W - 1), np.clip(pb, 0, W - 1)
    A = np.take_along_axis(F, np.broadcast_to(ia[:, None], F.shape), 3)
    B = np.take_along_axis(F, np.broadcast_to(ib[:, None], F.shape), 3)
    cont = (np.abs(A - B) <= discon).all(1)
    S, N = A * db[:, None] + B * da[:, None], np.maximum(da + db, 1)[:, None]
    q = (2 * np.abs(S) + N) // (2 * N)
    interp = np.where(S < 0, -q, q)
    ma = (np.abs(A).astype(np.uint64) ** 2).sum(1, dtype=np.uint64)
    mb = (np.abs(B).astype(np.uint64) ** 2).sum(1, dtype=np.uint64)
    take_b = (mb < ma) | ((mb == ma) & (db < da))
    tie_m, tie_all, tie_g = (ma == mb), (ma == mb) & (da == db), np.zeros_like(valued)
    if select == 1:
        ga = np.abs(G - np.take_along_axis(G, ia, 2))
        gb = np.abs(G - np.take_along_axis(G, ib, 2))
        take_b = (gb < ga) | ((gb == ga) & take_b)
        tie_g = ga == gb
    closed = va & vb
    kind = np.where(~closed, 3, np.where(cont, 1, 2))
    val = np.where((closed & cont)[:, None], interp, np.where((closed & take_b)[:, None] | (~closed & vb)[:, None], B, A))
    return dict(usable=usable, n=n, da=da, db=db, kind=kind, val=val, va=va, vb=vb, pa=pa, pb=pb, S=S, N=N,
                maxdiff=np.abs(A - B).max(1), tie_m=tie_m, tie_all=tie_all, tie_g=tie_g, A=A, B=B)


def _both_np(field, guide, prm):
    F = np.asarray(field).astype(np.int64)
    G = np.asarray(guide).astype(np.int64) if guide is not None else None
    h = _axis_np(F, G, prm)
    v = _axis_np(F.swapaxes(2, 3), G.swapaxes(1, 2) if G is not None else None, prm)
    v = {k: (a.swapaxes(2, 3) if a.ndim == 4 else a.swapaxes(1, 2)) for k, a in v.items()}
    return F, h, v


def gapfill_np(field, guide, prm=DEFAULTS, want_info=False):
    """P pairs: field [P, C, H, W] int32, guide [P, H, W] uint8 or None -> out, how [P, H, W] uint8, stats [P, 4] int32"""
    F, h, v = _both_np(field, guide, prm)
    hole = F[:, 0] == NONE
    vert = v["usable"] & (~h["usable"] | (v["n"] < h["n"]))
    filled = hole & (h["usable"] | v["usable"])
    kind = np.where(vert, v["kind"], h["kind"])
    out = np.where(filled[:, None], np.where(vert[:, None], v["val"], h["val"]), np.where(hole[:, None], NONE, F))
    how = np.where(~hole, 0, np.where(filled, kind + 3 * vert, 255)).astype(np.uint8)
    stats = np.stack([(filled & (kind == k)).sum((1, 2)) for k in (1, 2, 3)] + [(hole & ~filled).sum((1, 2))], 1).astype(np.int32)
    res = out.astype(np.int32), how, stats
    return res + (dict(h=h, v=v, hole=hole, vert=vert, filled=filled, kind=kind),) if want_info else res


def gapfill(field, guide, prm=DEFAULTS):
    return gapfill_np(field, guide, prm)


# ---- cases -------------------------------------------------------------------------------------------------------------------

KINDS = ("random", "runs", "sparse")
WIDTHS, HEIGHTS = (1, 5, 63, 64, 65, 130, 257), (1, 3, 9, 67, 130)          # 67 straddles a band of 64 rows, 130 one of 100
PRMS = ((3, 256, 0, 1), (8, 255, 1, 0), (100, 512, 1, 1), (1, 0, 0, 0))


def sweep():
    """every width with every height, the kinds taking turns: (kind, W, H)"""
    return [(KINDS[(i + j) % len(KINDS)], W, H) for i, W in enumerate(WIDTHS) for j, H in enumerate(HEIGHTS)]


def values(rng, shape):
    """two surfaces about 2048 apart with a spread of a few hundred, both signs: neighbours agree within 256 about as often
    as not"""
    base = rng.choice(np.array([-2560, -512, 512, 2560], np.int64), shape)
    return (base + rng.integers(-200, 201, shape)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(kind, W, H, P, C, seed=0):
    """(field [P, C, H, W] int32, guide [P, H, W] uint8), read-only.  "random": holes pixel by pixel, a share that differs
    from pair to pair; "runs": rows of alternating valued and hole segments of 1 .. 12 pixels, so that runs of every length
    about a small max_gap occur, some rows of holes only; "sparse": almost all holes, so that runs span chunks and bands."""
    rng = np.random.default_rng([seed, KINDS.index(kind), W, H, P, C])
    f = values(rng, (P, C, H, W))
    hole = np.zeros((P, H, W), bool)
    for t in range(P):
        if kind == "random":
            hole[t] = rng.random((H, W)) < (0.3, 0.6, 0.85)[t % 3]
        elif kind == "sparse":
            hole[t] = rng.random((H, W)) < 0.985
        else:
            for y in range(H):
                x, on = 0, bool(rng.integers(0, 2))
                while x < W:
                    ln = int(rng.integers(1, 13))
                    hole[t, y, x:x + ln] = on
                    x, on = x + ln, not on
                if rng.random() < 0.1:
                    hole[t, y] = True
    f[:, 0][hole] = NONE
    if C == 2:
        f[:, 1][rng.random((P, H, W)) < 0.2] = NONE            # on holes and on valued pixels alike: a value in channel 1
    ext = rng.random((P, C, H, W)) < 0.02                       # the extremes of int32 as values
    ext[:, 0] &= ~hole
    f[ext] = rng.choice(np.array([IMAX, IMIN1], np.int64), int(ext.sum())).astype(np.int32)
    g = rng.integers(0, 4, (P, H, W)).astype(np.uint8) * 60     # few levels: guide ties are common
    f.setflags(write=False)
    g.setflags(write=False)
    return f, g


def _row(vals, C=1, ch1=None):
    """a field [1, C, 1, W] from a list of channel-0 values (None: a hole)"""
    f = np.zeros((1, C, 1, len(vals)), np.int32)
    f[0, 0, 0] = [NONE if v is None else v for v in vals]
    if C == 2:
        f[0, 1, 0] = ch1 if ch1 is not None else 0
    return f


@functools.lru_cache(maxsize=None)
def crafted():
    """single situations, each a (name, field, guide, prm): the ones a random field reaches too rarely to rely on"""
    N_, out = None, []
    g = lambda f, vals=None: (np.array(vals, np.uint8).reshape(f[:, 0].shape) if vals is not None else np.zeros(f[:, 0].shape, np.uint8))
    add = lambda name, f, prm, gv=None: out.append((name, f, g(f, gv), prm))
    for b in (0, 1):
        add("left border, border=%d" % b, _row([N_, N_, 300, 300]), (4, 256, 0, b))
        add("right border, border=%d" % b, _row([300, 300, N_, N_]), (4, 256, 0, b))
        add("upper border, border=%d" % b, _row([N_, N_, 300, 300]).swapaxes(2, 3).copy(), (4, 256, 0, b))
        add("lower border, border=%d" % b, _row([300, 300, N_, N_]).swapaxes(2, 3).copy(), (4, 256, 0, b))
    add("a run of max_gap and one of max_gap + 1", _row([100, N_, N_, N_, 200, N_, N_, N_, N_, 300]), (3, 256, 0, 1))
    cross = np.full((1, 1, 5, 5), 1000, np.int32)               # both axes closed with n = 3: horizontal wins, 1000 .. 1200
    cross[0, 0, 2, 1:4] = NONE
    cross[0, 0, 1:4, 2] = NONE
    cross[0, 0, 2, 0], cross[0, 0, 2, 4], cross[0, 0, 0, 2], cross[0, 0, 4, 2] = 1000, 1200, 5000, 5200
    add("equal lengths", cross, (8, 256, 0, 1))
    tall = np.full((1, 1, 3, 7), 700, np.int32)                 # horizontal n = 5, vertical n = 1
    tall[0, 0, 1, 1:6] = NONE
    tall[0, 0, 0], tall[0, 0, 2] = 4000, 4100
    add("the vertical run shorter", tall, (8, 256, 0, 1))
    add("ends apart by discon and by discon + 1", _row([0, N_, 256, N_, 513, N_, -100, N_, -356]), (4, 256, 0, 1))
    add("a negative half rounds away from zero", _row([-1, N_, -2, N_, 2, N_, 1, N_, -3, N_, N_, 0]), (4, 256, 0, 1))
    add("equal m: the nearer end, then A", _row([900, N_, N_, -900, N_, 900, N_, N_, N_, -900, N_, N_, 900]), (4, 16, 0, 1))
    add("a guide tie", _row([900, N_, N_, -900, N_, 100, N_, 2000, N_, 2000, N_, 100]), (4, 16, 1, 1),
        [10, 20, 25, 30, 50, 60, 50, 40, 50, 40, 70, 90])
    add("the extremes of int32 as ends", _row([IMAX, N_, IMAX, N_, IMIN1, N_, N_, IMAX, N_, IMIN1, N_, IMIN1]), (4, 1 << 24, 0, 1))
    add("the extremes, C = 2", _row([IMAX, N_, IMIN1, N_, IMAX, N_, 5], 2, [IMIN1, 7, IMIN1, 7, NONE, 7, NONE]), (4, 0, 0, 1))
    add("channel 1 of a valued pixel none, of a hole not", _row([100, N_, 150, N_, 5000], 2, [NONE, 77, NONE, 88, 3]), (4, 256, 0, 1))
    holes_row = np.full((1, 1, 3, 6), 500, np.int32)
    holes_row[0, 0, 1] = NONE
    add("a row of holes only", holes_row, (4, 256, 0, 1))
    add("a field of holes only", np.full((1, 2, 3, 5), NONE, np.int32), (4, 256, 0, 1))
    add("a field without holes", np.full((1, 2, 3, 5), 123, np.int32), (4, 256, 0, 1))
    wide = np.full((1, 1, 1, 140), NONE, np.int32)              # ends in chunks 0 and 1, then 1 and 2
    wide[0, 0, 0, [60, 70, 120, 135]] = [100, 200, 300, 5000]
    add("ends in different chunks", wide, (64, 256, 0, 1))
    high = wide.swapaxes(2, 3).copy()
    add("ends in different bands", high, (64, 256, 0, 1))
    add("ends in different bands of max_gap rows", high, (70, 256, 0, 0))
    for c in out:
        c[1].setflags(write=False)
        c[2].setflags(write=False)
    return tuple(out)


def conditions(cases):
    """what a set of (name, field, guide, prm) reaches: a dict of counts, every one of which a complete set has above zero"""
    keys = ["left border, border=0", "left border, border=1", "right border, border=0", "right border, border=1",
            "upper border, border=0", "upper border, border=1", "lower border, border=0", "lower border, border=1",
            "run == max_gap", "run == max_gap + 1", "equal lengths, horizontal wins", "vertical shorter", "diff == discon",
            "diff == discon + 1", "negative half", "positive half", "equal m by distance", "equal m and distance: A", "guide tie",
            "INT32_MAX end", "INT32_MIN + 1 end", "valued with F_1 none", "hole with F_1 a value", "row of holes", "field of holes",
            "field without holes", "ends in different chunks", "ends in different bands", "hole left", "C = 2", "select = 1"]
    c = dict.fromkeys(keys, 0)
    for name, field, guide, prm in cases:
        max_gap, discon, select, border = prm
        out, how, stats, info = gapfill_np(field, guide, prm, want_info=True)
        hole, h, v = info["hole"], info["h"], info["v"]
        P, C, H, W = field.shape
        for ax, a, names in (("h", h, ("left", "right")), ("v", v, ("upper", "lower"))):
            short = a["n"] <= max_gap
            c["%s border, border=%d" % (names[0], border)] += int((hole & ~a["va"] & a["vb"] & short).sum())
            c["%s border, border=%d" % (names[1], border)] += int((hole & a["va"] & ~a["vb"] & short).sum())
            closed = hole & a["va"] & a["vb"]
            c["run == max_gap"] += int((closed & (a["n"] == max_gap)).sum())
            c["run == max_gap + 1"] += int((closed & (a["n"] == max_gap + 1)).sum())
            won = info["filled"] & (info["vert"] == (ax == "v"))
            c["diff == discon"] += int((won & closed & (a["maxdiff"] == discon)).sum())
            c["diff == discon + 1"] += int((won & closed & (a["maxdiff"] == discon + 1)).sum())
            half = (2 * np.abs(a["S"])) % (2 * a["N"]) == a["N"]
            cont = (won & closed & (a["kind"] == 1))[:, None]
            c["negative half"] += int((cont & half & (a["S"] < 0)).sum())
            c["positive half"] += int((cont & half & (a["S"] > 0)).sum())
            dis = won & closed & (a["kind"] == 2)
            if select == 0:
                c["equal m by distance"] += int((dis & a["tie_m"] & (a["da"] != a["db"])).sum())
                c["equal m and distance: A"] += int((dis & a["tie_all"]).sum())
            else:
                c["guide tie"] += int((dis & a["tie_g"]).sum())
            ends = won[:, None] & ((a["va"] & a["vb"])[:, None])
            c["INT32_MAX end"] += int((ends & ((a["A"] == IMAX) | (a["B"] == IMAX))).sum())
            c["INT32_MIN + 1 end"] += int((ends & ((a["A"] == IMIN1) | (a["B"] == IMIN1))).sum())
            size = CHUNK if ax == "h" else band_of(max_gap)
            apart = won & closed & (np.maximum(a["pa"], 0) // size != np.minimum(a["pb"], (W if ax == "h" else H) - 1) // size)
            c["ends in different chunks" if ax == "h" else "ends in different bands"] += int(apart.sum())
        both = hole & h["usable"] & v["usable"]
        c["equal lengths, horizontal wins"] += int((both & (h["n"] == v["n"])).sum())
        c["vertical shorter"] += int((both & (v["n"] < h["n"])).sum())
        if C == 2:
            c["C = 2"] += 1
            c["valued with F_1 none"] += int((~hole & (field[:, 1] == NONE)).sum())
            c["hole with F_1 a value"] += int((hole & (field[:, 1] != NONE)).sum())
        c["row of holes"] += int((hole.all(2) & ~hole.all((1, 2))[:, None]).sum())
        c["field of holes"] += int(hole.all((1, 2)).sum())
        c["field without holes"] += int((~hole).all((1, 2)).sum())
        c["hole left"] += int(stats[:, 3].sum())
        c["select = 1"] += int(select == 1)
    return c


# ---- the property: an occlusion closes on the background ---------------------------------------------------------------------

def edge_scene(W=96, H=64, seed=1):
    """Built like dense_chain_util.scene with C = 1: a foreground rectangle (disparity 7 .. 10) over a background (2 .. 4).
    -> (truth [1, 1, H, W] int32 in 1/256 pixel, punched: the same with the occluded band and a margin of 2 pixels around it
    taken out, band [H, W] bool, guide [1, H, W] uint8: background and foreground 40 and 200)"""
    rng = np.random.default_rng([seed, 1, W, H])
    xs, ys = np.arange(W)[None, :], np.arange(H)[:, None]
    d_bg, d_fg = int(rng.integers(2, 5)), int(rng.integers(7, 11))
    x0, y0 = int(rng.integers(W // 4, W // 3)), int(rng.integers(H // 5, H // 3))
    r = [x0, y0, x0 + int(rng.integers(W // 3, W // 2)), y0 + int(rng.integers(H // 3, H // 2))]
    rect = lambda x, y: (x >= r[0]) & (x < r[2]) & (y >= r[1]) & (y < r[3])
    fg = rect(xs, ys)
    band = ~fg & rect(xs - d_bg + d_fg, ys)                     # background that the foreground hides in the other image
    truth = (256 * np.where(fg, d_fg, d_bg)).astype(np.int32)[None, None]
    grown = np.zeros_like(band)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            grown[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] |= band[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    punched = truth.copy()
    punched[0, 0][grown] = NONE
    guide = np.where(fg, 200, 40).astype(np.uint8)[None]
    return truth, punched, band, guide
