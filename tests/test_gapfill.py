"""CPU: the scanline hole closing (gpc_hip_gapfill_*) -- the declarations in header and binding, the refusals with a null
context, the numpy restatement (tests/gapfill_util.py) against the rule taken pixel by pixel with Python loops, the condition
that the shared cases of the GPU test contain every situation a kernel can get wrong, and the rule's property on an edge: an
occluded band closes on the background, where the completion's mean leaves it off.

All but the first two tests need no library: they compare one restatement of the rule with the other and say what the cases
reach.  They prove nothing about the kernels; their purpose is to give the byte equality of tests/test_gpu_gapfill.py its
meaning -- the GPU equals a restatement that equals the rule taken literally, on cases that hold every situation named."""
import ctypes as C
import os
import re

import numpy as np

import gapfill_util as gu
import inpaint_util as iu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpc_hip_gapfill_fields_device": 11, "gpc_hip_gapfill_fields": 11}
SMALL = ((1, 1), (5, 3), (63, 9), (65, 3), (9, 67))      # W, H: small enough for the Python loops


def lib():
    import opengpc_amd as g
    from opengpc_amd import build
    build.build()
    return g, g.load()


def test_entry_points_are_declared_and_bound():
    g, L = lib()
    raw = open(os.path.join(ROOT, "include", "gpc_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    body = re.search(r"typedef struct gpc_gapfill \{(.*?)\} gpc_gapfill;", header, re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", body) == ["max_gap", "discon_q8", "select", "border"] == [f[0] for f in g.Gapfill._fields_]
    assert C.sizeof(g.Gapfill) == 16
    d = g.Gapfill()
    assert (d.max_gap, d.discon_q8, d.select, d.border) == gu.DEFAULTS
    assert re.search(r"\} gpc_gapfill;\s*/\* 16 bytes\.\s+Documented defaults: %d, %d, %d, %d" % gu.DEFAULTS, raw)
    for name, nargs in NAMES.items():
        assert name in g.capi.SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == nargs == len(getattr(L, name).argtypes), name
    for m in ("gapfill_fields_device", "gapfill_fields"):
        assert callable(getattr(g.Context, m)), m
    assert "close holes along scanlines from the background side" in raw
    # no timing slot: the table is as it was
    assert not [n for n in (L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_slots())) if "gapfill" in n]


def test_refusals_with_a_null_context():
    g, L = lib()
    gf = C.byref(g.Gapfill())
    assert L.gpc_hip_gapfill_fields_device(None, 4096, 8, 1, 4, 4, 1, gf, 8192, None, None) == g.capi.E_INVALID
    assert L.gpc_hip_gapfill_fields(None, 4096, 8, 1, 4, 4, 1, gf, 8192, None, None) == g.capi.E_INVALID


def shared_cases():
    """the three-pair half of what tests/test_gpu_gapfill.py runs, as (name, field, guide, prm): what a part reaches, the whole
    reaches"""
    out = list(gu.crafted())
    for Cn in (1, 2):
        for kind, W, H in gu.sweep():
            f, g_ = gu.case(kind, W, H, 3, Cn)
            out += [((kind, W, H, 3, Cn), f, g_, prm) for prm in gu.PRMS]
    return out


def test_the_two_restatements_agree():
    cases = list(gu.crafted())
    for kind in gu.KINDS:
        for Cn in (1, 2):
            for W, H in SMALL:
                f, g_ = gu.case(kind, W, H, 2, Cn)
                cases += [((kind, W, H, Cn), f, g_, prm) for prm in gu.PRMS]
    for name, f, g_, prm in cases:
        out, how, stats = gu.gapfill_np(f, g_, prm)
        for t in range(len(f)):
            po, ph, ps = gu.gapfill_plain(f[t], g_[t], prm)
            assert np.array_equal(out[t], po) and np.array_equal(how[t], ph) and np.array_equal(stats[t], ps), (name, prm, t)
        # what the rule promises of every result
        hole = f[:, 0] == gu.NONE
        assert np.array_equal(out.transpose(0, 2, 3, 1)[~hole], f.transpose(0, 2, 3, 1)[~hole])
        assert ((how == 0) == ~hole).all() and ((out[:, 0] == gu.NONE) == (how == 255)).all()
        assert (out.transpose(0, 2, 3, 1)[how == 255] == gu.NONE).all()
        assert np.array_equal(stats.sum(1), hole.sum((1, 2)))
        if prm[2] == 0:                                          # without select = 1 the guide is not read
            assert all(np.array_equal(a, b) for a, b in zip(gu.gapfill_np(f, None, prm), (out, how, stats)))


def test_crafted_values():
    """a few results by hand, so that the two restatements are not wrong together"""
    N = gu.NONE
    row = lambda name: next(c for c in gu.crafted() if c[0] == name)
    _, f, g_, prm = row("a negative half rounds away from zero")
    out, how, _ = gu.gapfill_np(f, g_, prm)
    #  -1 _ -2 -> -1.5 -> -2;  -2 _ 2 -> 0;  2 _ 1 -> 1.5 -> 2;  1 _ -3 -> -1;  -3 _ _ 0: -2 and -1
    assert out[0, 0, 0].tolist() == [-1, -2, -2, 0, 2, 2, 1, -1, -3, -2, -1, 0] and set(how[0, 0, 1::2][:4]) == {1}
    _, f, g_, prm = row("a run of max_gap and one of max_gap + 1")
    out, how, stats = gu.gapfill_np(f, g_, prm)
    assert out[0, 0, 0].tolist() == [100, 125, 150, 175, 200, N, N, N, N, 300] and stats[0].tolist() == [3, 0, 0, 4]
    _, f, g_, prm = row("ends apart by discon and by discon + 1")
    assert gu.gapfill_np(f, g_, prm)[1][0, 0].tolist() == [0, 1, 0, 2, 0, 2, 0, 1, 0]
    _, f, g_, prm = row("equal m: the nearer end, then A")
    out, how, _ = gu.gapfill_np(f, g_, prm)
    assert out[0, 0, 0].tolist() == [900, 900, -900, -900, -900, 900, 900, 900, -900, -900, -900, 900, 900]
    _, f, g_, prm = row("equal lengths")
    out, how, _ = gu.gapfill_np(f, g_, prm)
    # the centre has n = 3 both ways and takes the row's 1000 .. 1200, not the column's 5000 .. 5200; its neighbours have n = 1 across
    assert how[0, 2].tolist() == [0, 4, 1, 4, 0] and out[0, 0, 2].tolist() == [1000, 1000, 1100, 1000, 1200] and how[0, 1, 2] == 1
    _, f, g_, prm = row("the vertical run shorter")
    out, how, _ = gu.gapfill_np(f, g_, prm)
    assert (how[0, 1, 1:6] == 4).all() and (out[0, 0, 1, 1:6] == 4050).all()
    for b in (0, 1):
        for side in ("left", "right", "upper", "lower"):
            _, f, g_, prm = row("%s border, border=%d" % (side, b))
            out, how, stats = gu.gapfill_np(f, g_, prm)
            assert stats[0].tolist() == ([0, 0, 2, 0] if b else [0, 0, 0, 2])
            assert set(how[f[:, 0] == N]) == ({3 if side in ("left", "right") else 6} if b else {255})


def test_the_shared_cases_hold_every_situation():
    cond = gu.conditions(shared_cases())
    assert all(v > 0 for v in cond.values()), {k: v for k, v in cond.items() if v == 0}
    # and the random kinds alone reach the common ones in bulk, at every size class
    bulk = gu.conditions([c for c in shared_cases() if c[0][0] in gu.KINDS])
    for k in ("run == max_gap", "run == max_gap + 1", "equal lengths, horizontal wins", "vertical shorter", "guide tie", "hole left",
              "ends in different chunks", "ends in different bands", "valued with F_1 none", "hole with F_1 a value", "INT32_MAX end"):
        assert bulk[k] >= 10, (k, bulk[k])


def test_an_occluded_band_closes_on_the_background():
    """With select 0 EVERY band pixel ends on its true value.  The completion at its defaults leaves the band off it, though
    not every pixel of it, and what is asserted is the part that follows from the construction alone: the band column next to
    the foreground, in the rows whose whole 9 x 9 window lies inside the rectangle's rows.  Whenever such a pixel is filled,
    its window holds the 18 valued foreground pixels of the two columns behind the punched margin, each with weight
    256 >> min(8, 160 >> 3) = 1 (the guide is 40 against 200), and 63 other pixels of weight at most 256 whose values, input
    or filled, are nowhere below the background's.  So its mean lies at least 18 * 768 / (63 * 256 + 18) = 0.86 of 1/256 pixel
    above the truth (the layers are at least 3 pixels apart) and rounds to at least 1 above it.  The two band columns farthest
    from the foreground are filled from background alone and come out exact, so "all of them off" would be false; the share
    that is off (0.56 .. 0.61 on these seeds) is printed, not asserted."""
    for seed in (1, 2, 3):
        truth, punched, band, guide = gu.edge_scene(seed=seed)
        # the construction alone: the band is background, lies left of the foreground, and is all punched out with its margin
        assert band.sum() > 50 and (truth[0, 0][band] == truth[0, 0].min()).all() and (punched[0, 0][band] == gu.NONE).all()
        assert (punched[0, 0] == gu.NONE).sum() > band.sum() and truth[0, 0].max() - truth[0, 0].min() >= 768
        out, how, stats = gu.gapfill_np(punched, None, gu.DEFAULTS)
        assert np.array_equal(out[0, 0][band], truth[0, 0][band]) and stats[0, 3] == 0
        assert (how[0][band] == 2).all()                         # each one a choice at a depth edge, along its row
        done = iu.inpaint(punched, guide, iu.DEFAULTS)[0]
        assert iu.DEFAULTS[:2] == (4, 3) and (done[0, 0][band] != gu.NONE).all()
        rows, x1 = np.nonzero(band.any(1))[0], np.nonzero(band.any(0))[0].max()        # the band's rows; its column next to the foreground
        assert truth[0, 0, rows[0], x1 + 1] == truth[0, 0].max() and (punched[0, 0, rows, x1 + 3:x1 + 5] == truth[0, 0].max()).all()
        near = done[0, 0, rows[4:-4], x1]
        assert len(near) > 8 and (near >= truth[0, 0].min() + 1).all(), near
        off = done[0, 0][band] != truth[0, 0][band]
        print("seed %d: %d band pixels, %.3f of them off the truth after the completion" % (seed, band.sum(), off.mean()))
