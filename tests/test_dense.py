"""CPU: dense maps from sparse matches (gpc_hip_densify_*) -- the numpy restatement of the rule against the Python-loop one
on random small cases and on constructed ones, the declarations in header and binding, the new kernels' resources, and the
host-side checks driven by a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_util as du

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
NAMES = {"gpc_hip_densify_supports_device": 11, "gpc_hip_densify_correspondences_device": 11, "gpc_hip_densify_batch_device": 13,
         "gpc_hip_densify_sequence_device": 12, "gpc_hip_densify_supports": 11, "gpc_hip_densify_correspondences": 11}
KERNELS = ("k_dense_claim", "k_dense_pull", "k_dense_top", "k_dense_push")


@pytest.mark.parametrize("corr", [False, True])
def test_restatements_agree_on_random_cases(corr):
    rng = np.random.default_rng(5 + corr)
    for trial in range(12):
        W, H = int(rng.integers(1, 40)), int(rng.integers(1, 24))
        m = int(rng.integers(0, max(W * H // 3, 2)))
        cap = m + 3
        rec = du.random_records(rng, W, H, m, corr, cap)
        ref = du.random_refinements(rng, cap) if trial % 2 else None
        prm = (int(rng.choice([1, 2, 3, 15])), int(rng.choice([1, 2, 5, 1000])), int(trial % 3 != 0),
               int(rng.choice([0xFFFF, 1500])) if ref is not None else 0xFFFF)
        count = [m, m + 9, -2, 0][trial % 4] if trial > 7 else m
        value, level = du.densify_pair(rec, count, W, H, prm, ref)
        assert value.shape == (2 if corr else 1, H, W) and value.dtype == np.int32 and level.dtype == np.uint8
        for y in range(H):
            for x in range(W):
                v, l = du.brute_pixel(rec, count, W, H, x, y, prm, ref)
                assert tuple(int(q) for q in value[:, y, x]) == v and int(level[y, x]) == l, (trial, W, H, prm, x, y)
        assert ((level == 255) == (value[0] == du.NONE)).all()


def test_constructed_cases():
    s = lambda *r: np.array(list(r), du.SUPPORT).reshape(-1)
    # one record in a corner of 7x5: the top cell holds it, so every pixel takes its value
    for x, y in ((0, 0), (6, 0), (0, 4), (6, 4)):
        value, level = du.densify_pair(s((x, y, float(min(x, 2)))), 1, 7, 5)
        assert (value == 256 * min(x, 2)).all() and level[y, x] == 0 and level.max() <= du.lmax(7, 5) == 3
    # the lowest index wins
    value, _ = du.densify_pair(s((3, 3, 1.0), (3, 3, 2.0), (3, 3, 3.0)), 3, 7, 5)
    assert value[0, 3, 3] == 256
    # exact halves round away from zero, on both sides
    ref = np.zeros(2, du.REFINEMENT)
    ref["flags"], ref["dx_q8"] = 1, (1, 0)
    value, _ = du.densify_pair(s((0, 0, 0.0), (3, 0, 0.0)), 2, 4, 1, du.DEFAULTS, ref)
    assert value[0, 0].tolist() == [-1, -1, -1, 0]                # level 1, both cells: (-1 + 0) / 2 = -0.5 -> -1
    ref["dx_q8"] = (-1, 0)
    value, level = du.densify_pair(s((0, 0, 0.0), (3, 0, 0.0)), 2, 4, 1, (15, 2, 0, 0xFFFF), ref)
    assert value[0, 0].tolist() == [1, 1, 1, 0] and level[0].tolist() == [0, 2, 2, 0]
    # spread 0 against spread 1 at a grid edge; min_count nobody reaches; max_level 1
    rec = s((0, 0, 0.0))
    assert (du.densify_pair(rec, 1, 8, 1, (1, 1, 0, 0xFFFF))[1][0] == [0, 1, 255, 255, 255, 255, 255, 255]).all()
    assert (du.densify_pair(rec, 1, 8, 1, (1, 1, 1, 0xFFFF))[1][0] == [0, 1, 1, 1, 255, 255, 255, 255]).all()
    assert (du.densify_pair(rec, 1, 8, 1, (15, 2, 1, 0xFFFF))[1][0] == [0] + [255] * 7).all()
    # nothing participates: everything none
    value, level = du.densify_pair(s((9, 0, 0.0), (1, 0, 0.5), (1, 0, np.nan), (1, 0, 5.0)), 4, 8, 1)
    assert (value == du.NONE).all() and (level == 255).all()
    # a cost ceiling excludes the dearer record and the one that was not evaluated
    ref = np.zeros(3, du.REFINEMENT)
    ref["flags"], ref["cost"] = (1, 1, 0), (10, 11, 0xFFFF)
    rec = s((0, 0, 0.0), (1, 0, 1.0), (2, 0, 2.0))
    assert du.densify_pair(rec, 3, 4, 1, (15, 1, 1, 10), ref)[1][0].tolist() == [0, 1, 1, 1]
    assert du.densify_pair(rec, 3, 4, 1, (15, 1, 1, 0xFFFF), ref)[1][0].tolist() == [0, 0, 0, 1]


def test_entry_points_are_declared_and_bound():
    import opengpc_amd as g
    from opengpc_amd import build
    build.build()
    L = g.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpc_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+GPC_DENSE_NONE\s+\(-2147483647 - 1\)", header) and g.capi.DENSE_NONE == du.NONE
    body = re.search(r"typedef struct gpc_densify \{(.*?)\} gpc_densify;", header, re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", body) == ["max_level", "min_count", "spread", "max_cost"]
    assert C.sizeof(g.Densify) == 16
    d = g.Densify()
    assert (d.max_level, d.min_count, d.spread, d.max_cost) == du.DEFAULTS
    for name, nargs in NAMES.items():
        assert name in g.capi.SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == nargs == len(getattr(L, name).argtypes), name
    kernels = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_slots())]
    assert len(set(kernels)) == len(kernels) and "" not in kernels
    at = kernels.index("k_pyr_write")
    assert tuple(kernels[at + 1:at + 1 + len(KERNELS)]) == KERNELS and at >= L.gpc_hip_kernel_count() == 32
    for m in ("densify_records_device", "densify_batch_device", "densify_sequence_device", "densify_records"):
        assert callable(getattr(g.Context, m)), m
    # without a context every call refuses before it touches anything
    prm = C.byref(d)
    assert L.gpc_hip_densify_supports_device(None, 8, 1, 8, None, 4, 4, 1, prm, 8, None) == g.capi.E_INVALID
    assert L.gpc_hip_densify_correspondences(None, 8, 1, 8, None, 4, 4, 1, prm, 8, None) == g.capi.E_INVALID
    assert L.gpc_hip_densify_batch_device(None, 8, 8, 96, 64, 1, None, 0, prm, 8, None, None, None) == g.capi.E_INVALID
    assert L.gpc_hip_densify_sequence_device(None, 8, 96, 64, 2, None, 0, prm, 8, None, None, None) == g.capi.E_INVALID


def test_dense_kernels_use_no_scratch(capsys):
    """every k_dense_* instantiation: no scratch, no VGPR spills (gfx950 cross-compile, tools/kres.sh)"""
    env = dict(os.environ, KRES_OUT=os.path.join(ROOT, "tests", "cpp", "bin", "libgpc_kres_dense.so"))
    os.makedirs(os.path.dirname(env["KRES_OUT"]), exist_ok=True)
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), r"k_dense"], capture_output=True, text=True,
                         env=env, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"^(gpc::\S.*?)\s+sgpr\s+\d+\s+vgpr\s+(\d+)\s+spill s\s+\d+\s+v\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line)
        if m:
            rows[m.group(1).strip()] = tuple(int(v) for v in m.groups()[1:])
    assert sorted(rows) == ["gpc::k_dense_claim<false>", "gpc::k_dense_claim<true>", "gpc::k_dense_pull<false>",
                            "gpc::k_dense_pull<true>", "gpc::k_dense_push<1>", "gpc::k_dense_push<2>", "gpc::k_dense_top<1>",
                            "gpc::k_dense_top<2>"], out
    for name, (vgpr, vspill, scratch, occ) in sorted(rows.items()):
        print("%-28s vgpr %3d  occupancy %d waves/SIMD" % (name, vgpr, occ))
        assert vspill == 0 and scratch == 0, (name, rows[name])


def test_cpp_dense_header_compiles(tmp_path):
    """include/gpc/dense.hpp compiles against the library with a plain host compiler; the program only converts a field"""
    src, exe = str(tmp_path / "dense_hpp_check.cpp"), str(tmp_path / "dense_hpp_check")
    with open(src, "w") as f:
        f.write("#include <cmath>\n#include <gpc/dense.hpp>\n"
                "int main() {\n"
                "  if (false) gpc::dense::densify(std::vector<ndb::Support>(), 8, 8);\n"
                "  if (false) gpc::dense::densify(std::vector<ndb::Correspondence>(), 8, 8, gpc::dense::Params());\n"
                "  gpc::dense::Field f;\n  f.width = 2, f.height = 1, f.channels = 1;\n"
                "  f.value.emplace_back(2, 1);\n  f.value[0].data()[0] = 640, f.value[0].data()[1] = GPC_DENSE_NONE;\n"
                "  const std::vector<float> v = f.asFloat(0);\n"
                "  return v.size() == 2 && v[0] == 2.5f && std::isnan(v[1]) && !f.valid(1, 0) && f.valid(0, 0) ? 0 : 1;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-pthread"])
    assert subprocess.run([exe], timeout=60).returncode == 0


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm toolchain's clang++")
def test_host_checks_under_asan_ubsan(tmp_path):
    """opengpc_amd/csrc/dense_host.h driven by a stand-alone program: parameters, limits, Lmax, the pyramid's geometry and
    the workspace sizes"""
    exe = str(tmp_path / "dense_check")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "opengpc_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "dense_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.returncode, res.stdout, res.stderr)
