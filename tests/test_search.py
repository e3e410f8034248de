"""CPU: the local dense search (gpc_hip_search_*) -- the declarations in header and binding, the place of the timing slot, the
refusals with a null context and at every parameter bound, the numpy restatement (tests/search_util.py) against the rule
taken pixel by pixel with Python loops, its properties on constructed inputs, and the condition that the random case of the
GPU test visits every branch of the rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import refine_util as ru
import search_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpc_hip_search_fields_device": 13, "gpc_hip_search_batch_device": 20, "gpc_hip_search_sequence_device": 19,
         "gpc_hip_search_fields": 13}


def lib():
    import opengpc_amd as g
    from opengpc_amd import build
    build.build()
    return g, g.load()


def test_entry_points_are_declared_and_bound():
    g, L = lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpc_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct gpc_search \{(.*?)\} gpc_search;", header, re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", body) == ["radius", "range", "subpixel", "max_cost"] == [f[0] for f in g.Search._fields_]
    assert C.sizeof(g.Search) == 16
    d = g.Search()
    assert (d.radius, d.range, d.subpixel, d.max_cost) == su.DEFAULTS == (2, 1, 1, 0xFFFF)
    raw = open(os.path.join(ROOT, "include", "gpc_hip.h")).read()
    assert re.search(r"\} gpc_search;\s*/\* documented defaults: 2, 1, 1, 0xFFFF", raw)
    for name, nargs in NAMES.items():
        assert name in g.capi.SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == nargs == len(getattr(L, name).argtypes), name
    for m in ("search_fields_device", "search_batch_device", "search_sequence_device", "search_fields"):
        assert callable(getattr(g.Context, m)), m
    # the section stands between "clean" and "complete"
    assert raw.index("gpc_hip_clean_fields(") < raw.index("typedef struct gpc_search") < raw.index("typedef struct gpc_inpaint")


def test_timing_slot_sits_directly_before_k_refine():
    g, L = lib()
    kernels = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_slots())]
    assert len(set(kernels)) == len(kernels) and "" not in kernels
    at = kernels.index("k_search")
    assert at == 32 and kernels[at - 1] == "k_score_matchable" and kernels[at + 1] == "k_refine"
    assert L.gpc_hip_kernel_count() == 32 and L.gpc_hip_abi_version() == 1


def test_refusals_with_a_null_context():
    """without a context every call refuses before it touches anything"""
    g, L = lib()
    E = g.capi.E_INVALID
    sr, prm, fill, s = C.byref(g.Search()), C.byref(g.Clean()), C.byref(g.Densify()), C.byref(g.Settings.sparsematch())
    assert L.gpc_hip_search_fields_device(None, 4096, 8, 16, 1, 4, 4, 1, sr, 8192, None, None, None) == E
    assert L.gpc_hip_search_fields(None, 4096, 8, 16, 1, 4, 4, 1, sr, 8192, None, None, None) == E
    assert L.gpc_hip_search_batch_device(None, 8, 8, 96, 64, 1, s, 0, fill, sr, prm, 8, *([None] * 8)) == E
    assert L.gpc_hip_search_sequence_device(None, 8, 96, 64, 2, s, 0, fill, sr, prm, 8, *([None] * 8)) == E


def test_the_model_equals_the_rule_pixel_by_pixel():
    rng = np.random.default_rng(3)
    for C_ in (1, 2):
        for kind in su.KINDS:
            W, H = 33, 31
            f, L, R = su.case(kind, W, H, 1, C_)
            for prm in ((1, 0, 1, 0xFFFF), (2, 1, 1, 0xFFFF), (4, 2, 1, 9000), (3, 2, 0, 0xFFFF), (2, 1, 1, 0)):
                out, cost, choice, stats = su.search(f, L, R, prm)
                states = np.zeros(4, np.int64)
                picks = [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(40)] + [(0, 0), (W - 1, H - 1), (0, H - 1)]
                for x, y in picks:
                    o, c, k, s = su.search_plain(f[0], L[0], R[0], prm, x, y)
                    assert (out[0, :, y, x].tolist(), int(cost[0, y, x]), int(choice[0, y, x])) == (o, c, k), (C_, kind, prm, x, y)
                    states[s] += 1
                assert stats.sum() == W * H and (stats[0, 1] == (f[0, 0] == su.NONE).sum())
                assert ((out[0, 0] == su.NONE) == (out[0, -1] == su.NONE)).all()


@pytest.mark.parametrize("C_", [1, 2])
@pytest.mark.parametrize("R", [0, 1, 2])
def test_shifted_pair_returns_the_true_value(C_, R):
    """imgR is imgL moved by a known whole shift and the prior is off by up to R per axis: every pixel whose windows stay
    inside the image (and inside what imgL covers of imgR) finds the true target at cost 0.  Without the parabola the value
    is exactly 256 * true; with it the whole-pixel part is (a cost of 0 is a minimum, and the parabola moves it by at most
    half a pixel)."""
    W, H, P, radius = 40, 36, 2, 2
    L, Rr = su.images("shifted", W, H, P, C_)
    f = su.shifted_prior(W, H, C_, P, R)
    u, v = su.TRUE_SHIFT[C_]
    m = radius + 2 * R + 1 + max(abs(u), abs(v))               # the window, the prior's error, the search, the shift itself
    inner = np.zeros((H, W), bool)
    inner[m:H - m, m:W - m] = True
    assert inner.sum() > 100
    out, cost, choice, stats = su.search(f, L, Rr, (radius, R, 0, 0xFFFF))
    want = [256 * u, 256 * v][:C_]
    for c in range(C_):
        assert (out[:, c][:, inner] == want[c]).all()
    assert (cost[:, inner] == 0).all()
    out1, cost1, choice1, _ = su.search(f, L, Rr, (radius, R, 1, 0xFFFF))
    assert np.array_equal(cost1, cost) and np.array_equal(choice1, choice)
    for c in range(C_):
        assert (np.abs(out1[:, c][:, inner].astype(np.int64) - want[c]) <= 128).all()


@pytest.mark.parametrize("C_", [1, 2])
def test_constant_images_choose_the_centre(C_):
    """every cost is the same, so the prior wins wherever it is admissible, and no axis has a minimum: the value is the
    prior rounded to whole pixels"""
    W, H, P = 33, 31, 1
    f, L, R = su.case("constant", W, H, P, C_)
    for rng_ in (0, 1, 2):
        out, cost, choice, stats = su.search(f, L, R, (2, rng_, 1, 0xFFFF))
        valued, r, bx, by = su.base(f[0])
        centre = valued & (bx >= 0) & (bx < W) & (by >= 0) & (by < H)
        assert centre.sum() > 100
        assert (choice[0][centre] == (rng_ if C_ == 1 else rng_ * (2 * rng_ + 1) + rng_)).all()
        assert (cost[0][choice[0] != 255] == 25 * 7).all()
        for c in range(C_):
            assert (out[0, c][centre] == 256 * r[c][centre]).all()


@pytest.mark.parametrize("radius", [1, 2, 4])
def test_range_zero_equals_the_refinement_of_the_record(radius):
    """R = 0 with the parabola: an interior pixel's (cost, qx, qy) is what tests/refine_util.py gives the record with that
    whole-pixel target and the same radius"""
    W, H = 33, 31
    for C_ in (1, 2):
        f, L, R = su.case("random", W, H, 1, C_)
        out, cost, choice, stats = su.search(f, L, R, (radius, 0, 1, 0xFFFF))
        valued, r, bx, by = su.base(f[0])
        ys, xs = np.nonzero(valued)
        if C_ == 1:
            rec = np.zeros(len(xs), ru.SUPPORT)
            rec["x"], rec["y"], rec["d"] = xs, ys, r[0][ys, xs]
        else:
            rec = np.zeros(len(xs), ru.CORR)
            rec["src_x"], rec["src_y"], rec["tar_x"], rec["tar_y"] = xs, ys, bx[ys, xs], by[ys, xs]
        ref, _ = ru.refine_pair(rec, L[0], R[0], radius)
        ev = (ref["flags"] & ru.EVALUATED) != 0
        assert ev.sum() > 50
        ys, xs = ys[ev], xs[ev]
        assert np.array_equal(cost[0][ys, xs], ref["cost"][ev])
        q = out[0][:, ys, xs].astype(np.int64) - 256 * r[:, ys, xs]
        assert np.array_equal(q[0], (-1 if C_ == 1 else 1) * ref["dx_q8"][ev].astype(np.int64))
        if C_ == 2:
            assert np.array_equal(q[1], ref["dy_q8"][ev].astype(np.int64))


MAX_COST_FOR_STATS = {1: 3000, 2: 3000}


@pytest.mark.parametrize("C_", [1, 2])
def test_the_random_case_visits_every_branch(C_):
    """a condition, not a measurement: on the (70, 45, 3) random case of tests/test_gpu_search.py the model alone shows each
    of the four stats categories, a choice off the centre, a tie decided by the order, a pixel on the byte-wise border path,
    an axis with and one without a minimum -- the GPU equality cannot pass on inputs that leave a branch unvisited"""
    W, H, P = su.SIZES[-1]
    assert (W, H, P) == (70, 45, 3)
    f, L, R = su.case("random", W, H, P, C_)
    prm = (su.DEFAULTS[0], su.DEFAULTS[1], 1, MAX_COST_FOR_STATS[C_])
    stats, tot = np.zeros(4, np.int64), {}
    for t in range(P):
        info = {}
        stats += su.search_np(f[t], L[t], R[t], prm, info)[3]
        for k, v in info.items():
            tot[k] = tot.get(k, 0) + v
    assert (stats > 0).all(), stats
    assert all(tot[k] > 0 for k in ("off_centre", "ties", "border", "axis_min", "axis_none")), tot
    assert tot["border"] < stats.sum() - stats[1]          # and the fast path is visited too


def test_search_hpp_compiles(tmp_path):
    """include/gpc/search.hpp compiles against the library with a plain host compiler; the program runs no device code"""
    import subprocess
    lib()
    src, exe = str(tmp_path / "search_hpp_check.cpp"), str(tmp_path / "search_hpp_check")
    with open(src, "w") as f:
        f.write("#include <gpc/search.hpp>\n"
                "int main() {\n"
                "  gpc::dense::Field field;\n"
                "  ndb::Buffer<uint8_t> l, r;\n"
                "  if (false) { gpc::search::Result q = gpc::search::search(field, l, r, gpc::search::Params()); return q.stats[0]; }\n"
                "  const gpc_search c = gpc::search::Params().toC();\n"
                "  return c.radius == 2 && c.range == 1 && c.subpixel == 1 && c.max_cost == 0xFFFF ? 0 : 1;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-pthread"])
    assert subprocess.run([exe], timeout=60).returncode == 0
