"""CPU: the propagation of field values between neighbours (gpc_hip_propagate_*) -- the declarations in header and binding,
the refusals with a null context, the numpy restatement (tests/propagate_util.py) against the rule taken pixel by pixel with
Python loops, the condition that the shared cases of the GPU test contain every situation a kernel can get wrong, and the
rule's property on an edge: values from the right side of it replace the wrong ones."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import propagate_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpc_hip_propagate_fields_device": 13, "gpc_hip_propagate_fields": 13}
RADII, NEIGHBOURS = (1, 2, 4), (4, 8)        # with pu.SPANS and iterations 1 .. pu.MAX_N: what tests/test_gpu_propagate.py runs


def lib():
    import opengpc_amd as g
    from opengpc_amd import build
    build.build()
    return g, g.load()


def test_entry_points_are_declared_and_bound():
    g, L = lib()
    raw = open(os.path.join(ROOT, "include", "gpc_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    body = re.search(r"typedef struct gpc_propagate \{(.*?)\} gpc_propagate;", header, re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", body) == ["radius", "span", "iterations", "neighbours"] == [f[0] for f in g.Propagate._fields_]
    assert C.sizeof(g.Propagate) == 16
    d = g.Propagate()
    assert (d.radius, d.span, d.iterations, d.neighbours) == pu.DEFAULTS
    assert re.search(r"\} gpc_propagate;\s*/\* documented defaults: %d, %d, %d, %d" % pu.DEFAULTS, raw)
    for name, nargs in NAMES.items():
        assert name in g.capi.SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == nargs == len(getattr(L, name).argtypes), name
    for m in ("propagate_fields_device", "propagate_fields"):
        assert callable(getattr(g.Context, m)), m
    assert "propagate field values between neighbours" in raw
    # no timing slot: the table is as it was
    assert "k_propagate" not in [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_slots())]


def test_refusals_with_a_null_context():
    g, L = lib()
    pg = C.byref(g.Propagate())
    assert L.gpc_hip_propagate_fields_device(None, 4096, 8, 16, 1, 4, 4, 1, pg, 8192, None, None, None) == g.capi.E_INVALID
    assert L.gpc_hip_propagate_fields(None, 4096, 8, 16, 1, 4, 4, 1, pg, 8192, None, None, None) == g.capi.E_INVALID


@pytest.mark.parametrize("C_", [1, 2])
def test_the_model_equals_the_rule_pixel_by_pixel(C_):
    """every pixel of every iteration at the small sizes: the iteration's input is the model's own previous field"""
    for kind in pu.KINDS:
        for W, H, P in ((1, 1, 1), (7, 5, 1), (33, 31, 1)):
            f, L, R = pu.case(kind, W, H, P, C_)
            for radius, span, nb in ((1, 4, 8), (2, 1, 4), (4, 64, 8)):
                if (W, radius) == (33, 4):
                    continue                                                   # (the loops over 81-pixel windows: the 7 x 5 case has them)
                res = pu.run(f[0], L[0], R[0], radius, span, 2, nb)
                prev = f[0]
                for i, (out, cost, choice, stats) in enumerate(res):
                    states = np.zeros(4, np.int64)
                    for y in range(H):
                        for x in range(W):
                            o, c, k, s = pu.propagate_plain(prev, L[0], R[0], (radius, pu.stride(span, i), 1, nb), x, y)
                            assert (out[:, y, x].tolist(), int(cost[y, x]), int(choice[y, x])) == (o, c, k), (C_, kind, W, radius, span, nb, i, x, y)
                            states[s] += 1
                    assert states.tolist() == stats.tolist()
                    prev = out


SITUATIONS = ["won_by_%d" % j for j in range(1, 9)] + [
    "tie_own_wins", "tie_between_neighbours", "source_outside", "source_hole", "own_inadmissible_neighbour_admissible", "unmatched",
    "duplicate_of_own", "duplicate_of_neighbour", "travelled_further_than_a_stride", "moved_in_two_iterations",
    "tile_edge_winner_interior", "tile_edge_winner_clamped"]


@pytest.mark.parametrize("C_", [1, 2])
def test_the_shared_cases_contain_every_situation(C_):
    """a condition, not a measurement: across the cases tests/test_gpu_propagate.py runs, the model alone shows each situation
    of SITUATIONS at least once -- the GPU equality cannot pass on inputs that leave one unvisited.  (A tie counts only
    between candidates of different displacement; "further than a stride": the pixel holds the input value of a pixel more
    than the FIRST stride away, which no single iteration can bring.)"""
    tot = {}
    for kind in pu.KINDS:
        for W, H, P in pu.SIZES:
            for radius in RADII:
                for span in pu.SPANS:
                    for nb in NEIGHBOURS:
                        for k, v in pu.runs(kind, W, H, P, C_, radius, span, nb)[1].items():
                            tot[k] = tot.get(k, 0) + v
    print(C_, tot)
    missing = [k for k in SITUATIONS if tot.get(k, 0) == 0]
    assert not missing, (missing, tot)


@pytest.mark.parametrize("C_", [1, 2])
def test_on_an_edge_true_values_replace_wrong_ones(C_):
    """kind "edge", span 4, 4 iterations, 8 neighbours: of the band's pixels whose true target is inside the image and visible,
    at least as many end on their true whole-pixel value as started on it, and strictly more in every pair"""
    W, H, P = 70, 45, 3
    field, L, R, truth, visible = pu.edge_case(W, H, P, C_)
    out, _, _, stats = pu.propagate(field, L, R, (2, 4, 4, 8))
    band = pu.edge_band(W, H)
    on_truth = lambda F: (pu.su.whole(F.astype(np.int64)) == truth).all(1) & visible & band
    before, after = on_truth(field).sum((1, 2)), on_truth(out).sum((1, 2))
    print(C_, "band pixels counted", (visible & band).sum((1, 2)).tolist(), "before", before.tolist(), "after", after.tolist())
    assert (after >= before).all() and (after > before).all(), (before, after)
    assert (stats[:, :, 3].sum(1) > 0).all()


def test_propagate_hpp_compiles(tmp_path):
    """include/gpc/propagate.hpp compiles against the library with a plain host compiler; the program runs no device code"""
    import subprocess
    lib()
    src, exe = str(tmp_path / "propagate_hpp_check.cpp"), str(tmp_path / "propagate_hpp_check")
    with open(src, "w") as f:
        f.write("#include <gpc/propagate.hpp>\n"
                "int main() {\n"
                "  gpc::dense::Field field;\n"
                "  ndb::Buffer<uint8_t> l, r;\n"
                "  if (false) { gpc::propagate::Result q = gpc::propagate::propagate(field, l, r, gpc::propagate::Params()); return q.stats[0]; }\n"
                "  const gpc_propagate c = gpc::propagate::Params().toC();\n"
                "  return c.radius == 2 && c.span == 1 && c.iterations == 6 && c.neighbours == 8 ? 0 : 1;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-pthread"])
    assert subprocess.run([exe], timeout=60).returncode == 0
