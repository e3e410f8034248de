"""CPU: completing cleaned dense fields, guided by the image (gpc_hip_inpaint_*) -- hand-written cases of the rule against
both restatements (tests/inpaint_util.py), the two restatements against each other on small random fields, the declarations
in header and binding, the refusals with a null context, the place of the timing slots, inpaint.hpp under a plain host
compiler, and the C++ restatement of gpc/inpaint.hpp against the model through a stand-alone program, built plainly and under
AddressSanitizer and UBSan and run as its own process."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import inpaint_util as iu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
N = iu.NONE
NAMES = {"gpc_hip_inpaint_fields_device": 11, "gpc_hip_inpaint_batch_device": 22, "gpc_hip_inpaint_sequence_device": 21,
         "gpc_hip_inpaint_fields": 11}
KERNELS = ("k_inpaint_begin", "k_inpaint_pass")


def both(field, guide, prm):
    """the two restatements of one pair given as nested lists [C][H][W] and [H][W]; they must agree; -> out, pass, stats as lists"""
    f = np.array(field, np.int64).astype(np.int32)
    g = np.array(guide, np.uint8)
    plain, fast = iu.inpaint_plain(f, g, prm), iu.inpaint_np(f, g, prm)
    for p, q in zip(plain, fast):
        assert p.dtype == q.dtype and np.array_equal(p, q), (p, q)
    return tuple(p.tolist() for p in plain)


def test_weight_and_mean():
    assert [iu.weight(d, 0) for d in (0, 1, 2, 7, 8, 9, 255)] == [256, 128, 64, 2, 1, 1, 1]
    assert [iu.weight(d, 3) for d in (0, 7, 8, 15, 16, 63, 64, 255)] == [256, 256, 128, 128, 64, 2, 1, 1]
    assert all(iu.weight(d, 8) == 256 for d in range(256))
    assert [iu.mean(s, 2) for s in (-3, 3, -1, 1, 0, 2, -2)] == [-2, 2, -1, 1, 0, 1, -1]
    assert [iu.mean(s, 3) for s in (4, 5, -4, -5, 1, 2)] == [1, 2, -1, -2, 0, 1]


def test_passes_read_the_previous_pass_only():
    # a strip valued at x = 0 only, r = 1, min_weight 1: one pixel per pass, pass numbers 1, 2, 3, the rest holes
    f = [[[7] + [N] * 9]]
    out, pz, stats = both(f, [[0] * 10], (1, 8, 1, 3))
    assert out == [[[7, 7, 7, 7] + [N] * 6]] and pz == [[0, 1, 2, 3] + [255] * 6] and stats == [3, 6]
    # r = 2: two pixels per pass
    out, pz, stats = both(f, [[0] * 10], (2, 8, 1, 2))
    assert pz == [[0, 1, 1, 2, 2] + [255] * 5] and stats == [4, 5]


def test_rounding_half_away_from_zero():
    g = [[5, 5, 5]]
    assert both([[[-1, N, -2]]], g, (1, 8, 1, 1))[0] == [[[-1, -2, -2]]]
    assert both([[[1, N, 2]]], g, (1, 8, 1, 1))[0] == [[[1, 2, 2]]]
    # three neighbours, no tie: (1 + 2 + 5) / 3 = 2.67 -> 3, (-1 - 2 - 4) / 3 = -2.33 -> -2
    assert both([[[1, 2, 5], [N, N, N]]], [[5] * 3] * 2, (1, 8, 1, 1))[0][0][1] == [2, 3, 4]
    assert both([[[-1, -2, -4], [N, N, N]]], [[5] * 3] * 2, (1, 8, 1, 1))[0][0][1][1] == -2


def test_threshold_is_inclusive():
    # a hole with n = 3 valued neighbours of weight 256 each: filled at min_weight 768, not at 769
    f, g = [[[4, N, 4], [N, 4, N]]], [[9] * 3] * 2
    assert both(f, g, (1, 3, 768, 1))[1][0][1] == 1 and both(f, g, (1, 3, 769, 1))[1][0][1] == 255


def test_guide_weights_and_edges():
    # the hole at x = 2 looks like the right side: left values weigh 1 each, right values 256
    f, g = [[[0, 0, N, 1000, 1000]]], [[0, 0, 200, 200, 200]]
    out, pz, stats = both(f, g, (2, 0, 1, 1))
    assert out[0][0][2] == iu.mean(2 * 256 * 1000, 2 * 256 + 2) == 996
    # unguided: the plain mean
    assert both(f, g, (2, 8, 1, 1))[0][0][0][2] == 500
    # a hole of the input whose channel 1 held a value comes back as none in both channels; channel 1 of a source may be INT32_MIN
    out, pz, stats = both([[[N, 3]], [[44, N]]], [[0, 0]], (1, 8, 512, 5))
    assert out == [[[N, 3]], [[N, N]]] and pz == [[255, 0]] and stats == [0, 1]
    out, _, _ = both([[[N, 3]], [[44, N]]], [[0, 0]], (1, 8, 256, 5))
    assert out == [[[3, 3]], [[N, N]]]


def test_extremes():
    M, m = iu.IMAX, iu.IMIN1
    for v in (M, m):
        f = np.full((1, 17, 17), v, np.int64)
        f[0, 8, 8] = N
        out, pz, stats = both(f, np.zeros((17, 17)), (8, 8, 1, 1))
        assert out[0][8][8] == v and stats == [1, 0]
    out, _, _ = both([[[M, N, m]]], [[0, 0, 0]], (1, 8, 1, 1))
    assert out == [[[M, 0, m]]]
    out, _, _ = both([[[M, N, M, m]]], [[0, 0, 0, 0]], (2, 8, 1, 1))
    assert out[0][0][1] == iu.mean(2 * M + m, 3)


def test_stopping_is_not_observable():
    # an island that can never reach min_weight: one source, min_weight 257
    f, g = [[[5, N, N]]], [[0, 0, 0]]
    assert both(f, g, (1, 8, 257, 254)) == ([[[5, N, N]]], [[0, 255, 255]], [0, 2])
    # complete after 2 passes: 254 passes give what 2 give
    assert both(f, g, (1, 8, 256, 254)) == both(f, g, (1, 8, 256, 2)) == ([[[5, 5, 5]]], [[0, 1, 2]], [2, 0])
    assert both([[[N, N]]], [[1, 2]], (1, 3, 1, 9)) == ([[[N, N]]], [[255, 255]], [0, 2])
    assert both([[[1, 2]]], [[1, 2]], (1, 3, 1, 9)) == ([[[1, 2]]], [[0, 0]], [0, 0])


@pytest.mark.parametrize("C_", [1, 2])
def test_restatements_agree_on_random_fields(C_):
    rng = np.random.default_rng(70 + C_)
    for trial in range(12):
        W, H = int(rng.integers(1, 30)), int(rng.integers(1, 24))
        f = iu.random_fields(W, H, C_, 2, float(rng.choice([0.1, 0.5, 0.95])), seed=trial)
        g = iu.guides(["random", "constant", "step"][trial % 3], W, H, 2, seed=trial)
        prm = (int(rng.integers(1, 9)), int(rng.choice([0, 3, 8])), int(rng.choice([1, 256, 512, 2000])), int(rng.choice([1, 3, 32])))
        for t in range(2):
            p, q = iu.inpaint_plain(f[t], g[t], prm), iu.inpaint_np(f[t], g[t], prm)
            for a, b in zip(p, q):
                assert a.dtype == b.dtype and np.array_equal(a, b), (trial, W, H, prm)
            out, pz, stats = p
            assert stats.sum() == (f[t, 0] == N).sum() and ((pz == 255) == (out[0] == N)).all()
            assert np.array_equal(out[:, pz == 0], f[t][:, pz == 0]) and (out[:, pz == 255] == N).all()


def test_entry_points_are_declared_and_bound():
    import opengpc_amd as g
    from opengpc_amd import build
    build.build()
    L = g.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpc_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct gpc_inpaint \{(.*?)\} gpc_inpaint;", header, re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", body) == ["radius", "range_shift", "min_weight", "passes"]
    assert C.sizeof(g.Inpaint) == 16
    d = g.Inpaint()
    assert (d.radius, d.range_shift, d.min_weight, d.passes) == iu.DEFAULTS
    for name, nargs in NAMES.items():
        assert name in g.capi.SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == nargs == len(getattr(L, name).argtypes), name
    for m in ("inpaint_fields_device", "inpaint_batch_device", "inpaint_sequence_device", "inpaint_fields"):
        assert callable(getattr(g.Context, m)), m


def test_timing_slots_sit_between_tf_commit_and_quad_sides():
    import opengpc_amd as g
    from opengpc_amd import build
    build.build()
    L = g.load()
    kernels = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_slots())]
    assert len(set(kernels)) == len(kernels) and "" not in kernels
    at = kernels.index("k_tf_commit")
    assert tuple(kernels[at + 1:at + 1 + len(KERNELS)]) == KERNELS and kernels[at + 1 + len(KERNELS)] == "k_quad_sides"
    assert L.gpc_hip_kernel_count() == 32


def test_refusals_with_a_null_context():
    """without a context every call refuses before it touches anything"""
    import opengpc_amd as g
    from opengpc_amd import build
    build.build()
    L = g.load()
    E = g.capi.E_INVALID
    ip, prm, fill, s = C.byref(g.Inpaint()), C.byref(g.Clean()), C.byref(g.Densify()), C.byref(g.Settings.sparsematch())
    assert L.gpc_hip_inpaint_fields_device(None, 8, 8, 1, 4, 4, 1, ip, 4096, None, None) == E
    assert L.gpc_hip_inpaint_fields(None, 8, 8, 1, 4, 4, 1, ip, 4096, None, None) == E
    assert L.gpc_hip_inpaint_batch_device(None, 8, 8, 96, 64, 1, s, 0, fill, prm, ip, 8, *([None] * 10)) == E
    assert L.gpc_hip_inpaint_sequence_device(None, 8, 96, 64, 2, s, 0, fill, prm, ip, 8, *([None] * 10)) == E


def test_cpp_inpaint_header_compiles(tmp_path):
    """include/gpc/inpaint.hpp compiles against the library with a plain host compiler; the program only runs the CPU rule"""
    src, exe = str(tmp_path / "inpaint_hpp_check.cpp"), str(tmp_path / "inpaint_hpp_check")
    with open(src, "w") as f:
        f.write("#include <gpc/inpaint.hpp>\n"
                "int main() {\n"
                "  gpc::dense::Field field;\n"
                "  ndb::Buffer<uint8_t> guide;\n"
                "  if (false) { gpc::inpaint::Result r = gpc::inpaint::inpaint(field, guide, gpc::inpaint::Params()); return r.stats[0]; }\n"
                "  const int32_t f[3] = {-1, GPC_DENSE_NONE, -2};\n"
                "  const uint8_t g[3] = {5, 5, 5};\n"
                "  int32_t out[3], stats[2];\n"
                "  uint8_t pass[3];\n"
                "  gpc::inpaint::Params p;\n"
                "  p.radius = 1, p.minWeight = 1, p.passes = 1;\n"
                "  gpc::inpaint::reference(f, g, 1, 3, 1, p, out, pass, stats);\n"
                "  const gpc_inpaint c = gpc::inpaint::Params().toC();\n"
                "  const bool ok = out[0] == -1 && out[1] == -2 && out[2] == -2 && pass[1] == 1 && stats[0] == 1 && stats[1] == 0 &&\n"
                "                  c.radius == 4 && c.range_shift == 3 && c.min_weight == 512 && c.passes == 32;\n"
                "  return ok ? 0 : 1;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-pthread"])
    assert subprocess.run([exe], timeout=60).returncode == 0


def cases():
    """(field [C, H, W], guide [H, W], prm) for the stand-alone program: random ones, and the extremes (every neighbour
    INT32_MAX, every neighbour INT32_MIN + 1, mixed, at r = 8 unguided), so that UBSan sees the 64-bit sums at their ends"""
    out = []
    rng = np.random.default_rng(5)
    for trial in range(8):
        W, H, C_ = int(rng.integers(1, 40)), int(rng.integers(1, 40)), 1 + trial % 2
        f = iu.random_fields(W, H, C_, 1, [0.1, 0.5, 0.95][trial % 3], seed=40 + trial)[0]
        g = iu.guides(["random", "constant", "step"][trial % 3], W, H, 1, seed=trial)[0]
        out.append((f, g, (int(rng.integers(1, 9)), int(rng.choice([0, 3, 8])), int(rng.choice([1, 512, 3000])), int(rng.choice([1, 4, 254])))))
    for v in (iu.IMAX, iu.IMIN1):
        f = np.full((2, 17, 17), v, np.int32)
        f[:, 8, 8] = N
        out.append((f, np.zeros((17, 17), np.uint8), (8, 8, 1, 1)))
    f = rng.choice(np.array([iu.IMAX, iu.IMIN1, N, 0], np.int64), (2, 20, 23)).astype(np.int32)
    out.append((f, iu.guides("random", 23, 20, 1)[0], (8, 8, 1, 4)))
    out.append((f, iu.guides("random", 23, 20, 1)[0], (8, 0, 300, 4)))
    return out


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm toolchain's clang++")
@pytest.mark.parametrize("sanitize", [False, True])
def test_cpp_restatement_agrees_with_the_model(tmp_path, sanitize):
    """gpc/inpaint.hpp's reference() and opengpc_amd/csrc/inpaint_host.h driven by tests/cpp/inpaint_check.cpp, a program of
    its own: built plainly and with -fsanitize=address,undefined, run as a process, its results equal to the model's bytes"""
    exe, cin, cout = str(tmp_path / "inpaint_check"), str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    flags = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call([CLANG, "-std=c++17", "-O1"] + flags + ["-I" + os.path.join(ROOT, "opengpc_amd", "csrc"),
                                                                   "-I" + os.path.join(ROOT, "include"), "-o", exe,
                                                                   os.path.join(ROOT, "tests", "cpp", "inpaint_check.cpp")])
    cs = cases()
    with open(cin, "wb") as f:
        f.write(np.array([len(cs)], np.int32).tobytes())
        for field, guide, prm in cs:
            Cn, H, W = field.shape
            f.write(np.array([Cn, W, H] + list(prm), np.int32).tobytes() + field.tobytes() + guide.tobytes())
    res = subprocess.run([exe, cin, cout], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.returncode, res.stdout, res.stderr)
    got = open(cout, "rb").read()
    want = b"".join(b"".join(a.tobytes() for a in iu.inpaint_np(field, guide, prm)) for field, guide, prm in cs)
    assert got == want
