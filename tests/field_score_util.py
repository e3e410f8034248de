"""The rule of the dense field scorer (gpc_hip_score_fields*, include/gpc_hip.h, "score dense fields against ground
truth") restated with numpy, vectorised: score() gives the 64 int64 words of every pair's gpc_field_score and the error
plane.  score_plain() takes the rule pixel by pixel with Python integers (math.isqrt, round) and shares no line with it.
The inputs of the tests are made here once and shared: random_case(), crafted()."""
import functools
import math

import numpy as np

NONE = -2 ** 31
WORDS, TALLY, ALL, BIN = 64, 12, 4, 16          # words of gpc_field_score, of a tally; where `all` and bin 0 start
TRUTH_MAX, AXIS_MAX, E2_MAX = 32768.0, 65536, 2 ** 32
DEFAULTS = ((256, 768, 1280), 768, 50, ())       # thr_q8, out_abs_q8, out_rel_pm, speed_q8
SINTEL_SPEED = (2560, 10240)
SIZES = ((1, 1, 1), (5, 3, 1), (37, 29, 3), (64, 48, 1), (130, 70, 2), (512, 260, 2))


def isqrt(x):
    """floor(sqrt(x)) of int64 x <= 2^32: float64's root is correctly rounded and exact integers stay exact below 2^52"""
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    r -= (r * r > x)
    r += ((r + 1) * (r + 1) <= x)
    return r


def pixels(field, u, v, ignore):
    """per pixel of [P, C, H, W]: (category 0 ignored, 1 no truth, 2 hole, 3 judged; e2; e; m2), int64"""
    P, C, H, W = field.shape
    truth = [u] if C == 1 else [u, v]
    with np.errstate(invalid="ignore"):
        ok = np.ones((P, H, W), bool)
        for t in truth:
            ok &= np.abs(t.astype(np.float64)) <= TRUTH_MAX     # (false for NaN)
    e2, m2 = np.zeros((P, H, W), np.int64), np.zeros((P, H, W), np.int64)
    for c, t in enumerate(truth):
        tq = np.rint(256.0 * np.where(ok, t, 0).astype(np.float64)).astype(np.int64)   # the product is exact: ties go to even
        a = np.minimum(np.abs(field[:, c].astype(np.int64) - tq), AXIS_MAX)
        e2 += a * a
        m2 += tq * tq
    e2 = np.minimum(e2, E2_MAX)
    cat = np.full((P, H, W), 3, np.int64)
    cat[field[:, 0] == NONE] = 2
    cat[~ok] = 1
    if ignore is not None:
        cat[ignore != 0] = 0
    return cat, e2, isqrt(e2), m2


def score(field, u, v=None, ignore=None, cls=None, prm=DEFAULTS):
    """-> (words [P, 64] int64: the bytes of gpc_field_score, err [P, H, W] uint16)"""
    thr, out_abs, out_rel, speed = prm
    P, C, H, W = field.shape
    cat, e2, e, m2 = pixels(field, u, v, ignore)
    judged = cat == 3
    if cls is not None:
        bins = np.minimum(cls.astype(np.int64), 3)
    else:
        bins = np.zeros((P, H, W), np.int64)
        for s in speed:
            bins += m2 >= s * s
    outlier = (e2 > out_abs * out_abs) & (e2 * 10 ** 6 > m2 * (out_rel * out_rel))
    words = np.zeros((P, WORDS), np.int64)
    words[:, 0] = H * W
    for k in range(3):
        words[:, 1 + k] = (cat == k).sum(axis=(1, 2))
    for where, sel in [(ALL, judged)] + [(BIN + TALLY * b, judged & (bins == b)) for b in range(4)]:
        words[:, where] = sel.sum(axis=(1, 2))
        for k, t in enumerate(thr):
            words[:, where + 1 + k] = (sel & (e2 <= t * t)).sum(axis=(1, 2))
        words[:, where + 9] = (sel & outlier).sum(axis=(1, 2))
        words[:, where + 10] = np.where(sel, e, 0).sum(axis=(1, 2))
        words[:, where + 11] = np.where(sel, e2, 0).sum(axis=(1, 2))
    err = np.where(judged, np.minimum(e, 0xFFFE), 0xFFFF).astype(np.uint16)
    return words, err


def score_plain(field, u, v, ignore, cls, prm):
    """one pair [C, H, W], pixel by pixel in Python integers -> (words list of 64, err rows)"""
    thr, out_abs, out_rel, speed = prm
    C, H, W = field.shape
    words, err = [0] * WORDS, [[0] * W for _ in range(H)]
    words[0] = W * H
    for y in range(H):
        for x in range(W):
            err[y][x] = 0xFFFF
            if ignore is not None and int(ignore[y, x]) != 0:
                words[1] += 1
                continue
            truth = [float(u[y, x])] + ([float(v[y, x])] if C == 2 else [])
            if any(math.isnan(t) or math.isinf(t) or abs(t) > 32768.0 for t in truth):
                words[2] += 1
                continue
            if int(field[0, y, x]) == NONE:
                words[3] += 1
                continue
            t = [round(256.0 * g) for g in truth]                # Python's round: to nearest, ties to even
            a = [min(abs(int(field[c, y, x]) - t[c]), 65536) for c in range(C)]
            e2 = min(sum(q * q for q in a), 2 ** 32)
            e, m2 = math.isqrt(e2), sum(q * q for q in t)
            b = min(int(cls[y, x]), 3) if cls is not None else sum(1 for s in speed if m2 >= s * s)
            err[y][x] = min(e, 0xFFFE)
            for where in (ALL, BIN + TALLY * b):
                words[where] += 1
                for k, q in enumerate(thr):
                    words[where + 1 + k] += e2 <= q * q
                words[where + 9] += e2 > out_abs ** 2 and e2 * 10 ** 6 > m2 * out_rel ** 2
                words[where + 10] += e
                words[where + 11] += e2
    return words, err


@functools.lru_cache(maxsize=None)
def random_case(W, H, P, C, seed=0):
    """(field, u, v, ignore, cls), read-only: truth of a few pixels' magnitude, mostly on the 1/256 grid and sometimes off
    it; a field around it with errors from 1/256 pixel to beyond the clamp; holes, ignored pixels, pixels without truth,
    the ends of int32, classes 0 .. 5; v is None with C = 1"""
    rng = np.random.default_rng(1000 * seed + 7 * W + 3 * H + P + 100 * C)
    shape = (P, H, W)
    truth = []
    for c in range(C):
        t = (rng.integers(-30 * 256, 60 * 256, shape) / 256.0).astype(np.float32)
        off = rng.random(shape) < 0.3
        t[off] = (rng.standard_normal(off.sum()) * 20).astype(np.float32)
        half = rng.random(shape) < 0.1
        t[half] = ((rng.integers(-2000, 2000, half.sum()) + 0.5) / 256.0).astype(np.float32)
        bad = rng.random(shape) < 0.04
        t[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e9, 32768.5, -40000.0], np.float32), bad.sum())
        truth.append(t)
    field = np.zeros((P, C, H, W), np.int32)
    for c in range(C):
        base = np.rint(256.0 * np.nan_to_num(truth[c].astype(np.float64), nan=0, posinf=0, neginf=0).clip(-40000, 40000))
        scale = rng.choice(np.array([0, 2, 60, 300, 900, 3000, 40000, 200000]), shape)
        field[:, c] = (base + np.rint(rng.standard_normal(shape) * scale)).clip(-2 ** 31 + 1, 2 ** 31 - 1).astype(np.int64)
        ends = rng.random(shape) < 0.01
        field[:, c][ends] = rng.choice(np.array([2 ** 31 - 1, -2 ** 31 + 1, NONE if c else 0], np.int64), ends.sum())
    field[:, 0][rng.random(shape) < 0.12] = NONE
    ignore = (rng.random(shape) < 0.1).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    cls = rng.choice(np.array([0, 0, 0, 1, 1, 2, 3, 4, 5, 255], np.uint8), shape)
    out = [field, truth[0], truth[1] if C == 2 else None, ignore, cls]
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return tuple(out)


def two_squares(target):
    """(a, b), b <= a <= 65536, with a^2 + b^2 == target, or None"""
    b = np.arange(0, 65537, dtype=np.int64)
    rest = target - b * b
    b = b[rest >= b * b]
    rest = target - b * b
    a = isqrt(rest)
    hit = np.flatnonzero((a * a == rest) & (a <= 65536))
    return (int(a[hit[0]]), int(b[hit[0]])) if len(hit) else None


CRAFT_THR = (256, 768, 1280, 5, 65535, 0, 25, 1)
CRAFT_PRMS = ((CRAFT_THR, 768, 50, ()), (CRAFT_THR, 768, 0, ()), (CRAFT_THR, 0, 255, ()), (CRAFT_THR, 65535, 255, SINTEL_SPEED),
              ((), 768, 50, (0, 2560, 2560)), (DEFAULTS[0], 768, 50, SINTEL_SPEED))


@functools.lru_cache(maxsize=None)
def crafted(C):
    """one pair of one row, a pixel per case, read-only: (field [1, C, 1, n], u, v, ignore, cls, notes).  A pixel is given
    as (F_0, F_1, u, v, ignore, cls); with C = 1 the second axis is dropped, so a sum of two squares becomes its first."""
    px, notes = [], []

    def add(note, f0, f1=0, u=0.0, v=0.0, ign=0, c=0):
        px.append((f0, f1, u, v, ign, c))
        notes.append(note)

    def add_e2(note, target, u=0.0, v=0.0):
        ab = two_squares(target)
        if ab:
            add("%s: e2 = %d = %d^2 + %d^2" % (note, target, ab[0], ab[1]), ab[0] + int(round(256 * u)), -ab[1] + int(round(256 * v)), u, v)
        return ab is not None

    # the square root: e2 at k^2, k^2 - 1, k^2 + 1 for small k and for k near 65535, wherever two squares reach it
    reached = 0
    for k in list(range(0, 40)) + list(range(65500, 65537)):
        for d in (-1, 0, 1):
            if 0 <= k * k + d <= 2 ** 32:
                reached += add_e2("root, k = %d, %+d" % (k, d), k * k + d)
    assert reached > 120
    # 2^32 - 1 is 3 mod 4 and no sum of two squares: the largest sum below 2^32, then the clamp from every side
    a = np.arange(46341, 65536, dtype=np.int64)
    below = int((a * a + isqrt(2 ** 32 - 1 - a * a) ** 2).max())
    assert 2 ** 32 - 64 < below < 2 ** 32 and add_e2("the largest e2 below 2^32", below)
    add("e2 = 2^32 exactly", 65536, 0)
    add("e2 = 2^32 + 1, clamped", 65536, 1)
    add("both axes at the clamp", 65536, 65536)
    add("an axis beyond its clamp", 65537, 0)
    add("an axis far beyond its clamp", 10 ** 9, 3)
    # thresholds met exactly and missed by one
    for t in CRAFT_THR:
        for d in (-1, 0, 1):
            if t * t + d >= 0:
                add_e2("threshold %d, %+d" % (t, d), t * t + d)
    for t in CRAFT_THR:
        add("threshold %d along one axis" % t, t, 0)
        add("threshold %d + 1 along one axis" % t, -t - 1, 0)
    # truth: what is no truth, the bound itself, ties of the rounding on both parities
    big = float(np.nextafter(np.float32(32768), np.float32(np.inf)))
    for g in (np.nan, np.inf, -np.inf, 1e9, -1e9, big, -big):
        add("no truth: u = %r" % g, 5, 5, g, 0.0)
        add("no truth: v = %r" % g, 5, 5, 0.0, g)
    for g in (32768.0, -32768.0):
        add("truth at the bound %r" % g, int(256 * g) + 3, int(256 * g) - 4, g, g)
        add("truth at the bound, the field far away", 0, 0, g, -g)
    for m in (0, 1, 2, 3, 100, 101, -1, -2, -3, -100, -101):
        g = (m + 0.5) / 256.0
        for f in (m - 1, m, m + 1, m + 2):
            add("tie: 256 u = %s, F = %d" % (m + 0.5, f), f, f, g, g)
    # the order of the classification
    add("ignored over no truth", 7, 7, np.nan, np.nan, ign=1)
    add("ignored over a hole", NONE, 7, 1.0, 1.0, ign=255)
    add("ignored over a judged pixel", 256, 256, 1.0, 1.0, ign=2)
    add("no truth over a hole", NONE, NONE, np.inf, 0.0)
    add("a hole", NONE, NONE, 1.0, 1.0)
    add("a hole whatever F_1 holds", NONE, 12, 1.0, 1.0)
    # field values at the ends of int32
    for g in (0.0, 32768.0, -32768.0):
        add("F = INT32_MAX", 2 ** 31 - 1, 2 ** 31 - 1, g, g)
        add("F = INT32_MIN + 1", -2 ** 31 + 1, -2 ** 31 + 1, g, g)
        add("F_1 = NONE, F_0 valued", 300, NONE, g, g)
    # the outlier test (768 / 50): both inequalities at equality and one step either side; e2 * 400 == m2 at e = 1000, t = 20000
    for e in (767, 768, 769):
        add("outlier, absolute: e = %d, m2 = 0" % e, e, 0)
    for e, t in ((999, 20000), (1000, 20000), (1001, 20000), (1000, 19999), (1000, 20001)):
        add("outlier, relative: e = %d, t = %d" % (e, t), t + e, 0, t / 256.0, 0.0)
    for g in (32768.0, -32768.0):                          # the largest m2, for out_rel_pm 0 and 255
        for e in (1, 769, 2139095, 2139096, 65536):
            add("outlier, |truth| = 32768: e = %d" % e, int(256 * g) + min(e, 65536), int(256 * g), g, g)
    # speed bins: m2 == speed^2 exactly (10 px = 2560; 1536^2 + 2048^2 = 2560^2) and one step either side
    for t0, t1 in ((2559, 0), (2560, 0), (2561, 0), (1536, 2048), (1536, 2047), (10239, 0), (10240, 0), (6144, 8192), (-10240, 0), (0, 0)):
        add("speed: t = (%d, %d)" % (t0, t1), t0 + 100, t1, t0 / 256.0, t1 / 256.0)
    # classes
    for c in (0, 1, 2, 3, 4, 255):
        add("class %d" % c, 400, 10, 1.0, 0.0, c=c)
        add("class %d, a hole" % c, NONE, 0, 1.0, 0.0, c=c)
    n = len(px)
    field = np.zeros((1, C, 1, n), np.int32)
    u, v = np.zeros((1, 1, n), np.float32), np.zeros((1, 1, n), np.float32)
    ignore, cls = np.zeros((1, 1, n), np.uint8), np.zeros((1, 1, n), np.uint8)
    for i, (f0, f1, g0, g1, ign, c) in enumerate(px):
        field[0, 0, 0, i] = f0
        if C == 2:
            field[0, 1, 0, i] = f1
        u[0, 0, i], v[0, 0, i], ignore[0, 0, i], cls[0, 0, i] = g0, g1, ign, c
    out = (field, u, v if C == 2 else None, ignore, cls)
    for a_ in out:
        if a_ is not None:
            a_.setflags(write=False)
    return out + (tuple(notes),)


def accessors(words):
    """the figures the bindings' accessors derive from one pair's words, over all judged pixels: a dict of floats"""
    n = int(words[ALL])
    d = lambda a, b: float(a) / float(b) if b else float("nan")
    return dict(epe=d(int(words[ALL + 10]), 256 * n), rms=d(int(words[ALL + 11]), 65536 * n) ** 0.5,
                within=[d(int(words[ALL + 1 + k]), n) for k in range(8)], outlier_rate=d(int(words[ALL + 9]), n),
                density=d(n, n + int(words[3])))
