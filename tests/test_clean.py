"""CPU: cleaning dense fields (gpc_hip_clean_*) -- hand-written cases of every rule against both restatements
(tests/clean_util.py), the two restatements against each other on small random fields, the reversed records, the
declarations in header and binding, the refusals with a null context, clean.hpp under a plain host compiler, the host-side
checks driven by a stand-alone program under AddressSanitizer and UBSan, and the conditions the GPU tests put on their own
inputs (every state occurs, a component runs through three tiles)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import clean_util as cu
import dense_util as du

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
N = cu.NONE
NAMES = {"gpc_hip_clean_fields_device": 12, "gpc_hip_flip_supports_device": 8, "gpc_hip_flip_correspondences_device": 8,
         "gpc_hip_clean_batch_device": 18, "gpc_hip_clean_sequence_device": 17, "gpc_hip_clean_fields": 12}
KERNELS = ("k_clean_flip", "k_clean_check", "k_clean_tile", "k_clean_border", "k_clean_flatten", "k_clean_sizes", "k_clean_apply")


def both(fwd, bwd, prm):
    """the two restatements of one pair given as nested lists [C][H][W]; they must agree; -> out, state, label, stats as lists"""
    f = np.array(fwd, np.int64).astype(np.int32)
    b = None if bwd is None else np.array(bwd, np.int64).astype(np.int32)
    plain, fast = cu.clean_plain(f, b, prm), cu.clean_np(f, b, prm)
    for p, q in zip(plain, fast):
        assert p.dtype == q.dtype and np.array_equal(p, q), (p, q)
    return tuple(p.tolist() for p in plain)


def test_check_fails_by_leaving_the_image():
    # one row of five, C = 1: the target is x - r.  256 at x = 0 points to x = -1; -512 at x = 4 to x = 6
    out, state, label, stats = both([[[256, 0, 0, 0, -512]]], [[[0, 0, 0, 0, 0]]], (0, 1 << 24, 0, 0))
    assert state == [[2, 0, 0, 0, 2]] and out == [[[N, 0, 0, 0, N]]] and label == [[-1, 1, 1, 1, -1]] and stats == [3, 0, 2, 0]
    # C = 2: the target is (x + r0, y + r1).  (0, 256) at the bottom row leaves downwards, (-256, 0) at x = 0 to the left
    f = [[[-256, 0], [0, 0]], [[0, 0], [0, 256]]]
    out, state, label, stats = both(f, [[[0, 0], [0, 0]], [[0, 0], [0, -256]]], (0, 1 << 24, 0, 0))
    assert state == [[2, 0], [0, 2]] and stats == [2, 0, 2, 0] and label == [[-1, 1], [2, -1]]   # (diagonal neighbours stay apart)
    assert out == [[[N, 0], [0, N]], [[N, 0], [0, N]]]


def test_check_fails_by_none_at_the_target():
    # x = 2 has d = 1 px -> target x = 1, where bwd has nothing; x = 3 (d = 1 px) -> x = 2, where bwd answers -256
    out, state, label, stats = both([[[0, 0, 256, 256]]], [[[0, N, -256, 0]]], (0, 0, 0, 0))
    assert state == [[0, 2, 2, 0]] and out == [[[0, N, N, 256]]] and label == [[0, -1, -1, 3]] and stats == [2, 0, 2, 0]
    # a pixel that has no value itself is state 1 whatever bwd holds
    out, state, label, stats = both([[[N, 0]]], [[[0, 0]]], (0, 0, 0, 0))
    assert state == [[1, 0]] and out == [[[N, 0]]] and label == [[-1, 1]] and stats == [1, 1, 0, 0]


def test_check_tolerance_is_inclusive():
    # F + G = 100 at x = 0 (passes at tol 100), 101 at x = 1 (one over), -100 and -101 at x = 2, 3
    f, g = [[[40, 40, -40, -40]]], [[[60, 61, -60, -61]]]
    out, state, label, stats = both(f, g, (100, 1 << 24, 0, 0))
    assert state == [[0, 2, 0, 2]] and out == [[[40, N, -40, N]]] and label == [[0, -1, 2, -1]] and stats == [2, 0, 2, 0]
    assert both(f, g, (101, 1 << 24, 0, 0))[1] == [[0, 0, 0, 0]] and both(f, g, (99, 1 << 24, 0, 0))[1] == [[2, 2, 2, 2]]
    # the check off: bwd is not needed at all
    assert both(f, None, (-1, 1 << 24, 0, 0))[1] == [[0, 0, 0, 0]]
    # C = 2: one channel over the tolerance is enough
    out, state, _, _ = both([[[10, 10]], [[10, 10]]], [[[0, 0]], [[0, 1]]], (10, 0, 0, 0))
    assert state == [[0, 2]] and out == [[[10, N]], [[10, N]]]


def test_rounding_of_the_shift_half_away_from_zero():
    assert [cu.rshift(v) for v in (127, 128, -127, -128, 383, 384, -383, -384, 0, cu.IMAX, cu.IMIN1)] == \
        [0, 1, 0, -1, 1, 2, -1, -2, 0, 1 << 23, -(1 << 23)]
    # a row of nine, every pixel tested alone at x = 4 with bwd marking which target it reached: G = -F only at the target
    for v, r in ((127, 0), (128, 1), (-127, 0), (-128, -1), (383, 1), (384, 2), (-383, -1), (-384, -2)):
        f = [[[N] * 9]]
        f[0][0][4] = v
        for t in range(9):
            g = [[[N] * 9]]
            g[0][0][t] = -v
            _, state, _, _ = both(f, g, (0, 0, 0, 0))
            assert (state[0][4] == 0) == (t == 4 - r), (v, r, t)
        # C = 2 moves the other way, in x and in y
        f2 = np.full((2, 9, 9), N, np.int64)
        f2[:, 4, 4] = (v, -v)
        for ty, tx in ((4 - r, 4 + r), (4 + r, 4 - r), (4, 4)):
            g2 = np.full((2, 9, 9), N, np.int64)
            g2[:, ty, tx] = (-v, v)
            _, state, _, _ = both(f2, g2, (0, 0, 0, 0))
            assert (state[4][4] == 0) == ((ty, tx) == (4 - r, 4 + r)), (v, r, ty, tx)


def test_component_connected_only_through_a_chain():
    # a ring round a hole: 0, 10, 20 .. 70 clockwise from the top-left corner, step 10 = speckle_diff; the ends 0 and 70
    # are neighbours and 70 apart, and belong together through the chain.  The centre differs from all by more.
    f = [[[0, 10, 20], [70, 500, 30], [60, 50, 40]]]
    out, state, label, stats = both(f, None, (-1, 10, 8, 0))
    assert label == [[0, 0, 0], [0, 4, 0], [0, 0, 0]] and state == [[0, 0, 0], [0, 3, 0], [0, 0, 0]] and stats == [8, 0, 0, 1]
    assert out == [[[0, 10, 20], [70, N, 30], [60, 50, 40]]]
    # one more pixel needed than the ring has: everything is a speckle, and the labels stay
    out, state, label, stats = both(f, None, (-1, 10, 9, 0))
    assert state == [[3] * 3] * 3 and label == [[0, 0, 0], [0, 4, 0], [0, 0, 0]] and stats == [0, 0, 0, 9] and out == [[[N] * 3] * 3]
    # a step of 11 cuts the chain in two places: 0 | 11 22 | 33 .. : three runs of a row
    out, state, label, stats = both([[[0, 11, 21, 32, 42]]], None, (-1, 10, 2, 0))
    assert label == [[0, 1, 1, 3, 3]] and state == [[3, 0, 0, 0, 0]]
    # speckle_min 0 and 1 remove nothing; the label is computed all the same
    for smin in (0, 1):
        _, state, label, _ = both(f, None, (-1, 10, smin, 0))
        assert state == [[0] * 3] * 3 and label == [[0, 0, 0], [0, 4, 0], [0, 0, 0]]
    # C = 2: both channels must be near
    _, _, label, _ = both([[[0, 0, 0]], [[0, 5, 11]]], None, (-1, 5, 0, 0))
    assert label == [[0, 0, 2]]


def test_lower_median_with_n_even():
    # 2 x 2, radius 1: every window is the whole image, n = 4, the lower median is element 1 of (1, 2, 3, 4)
    out, state, _, _ = both([[[4, 1], [3, 2]]], None, (-1, 1 << 24, 0, 1))
    assert out == [[[2, 2], [2, 2]]]
    # a pixel that is not kept gives no value to its neighbours and gets none: windows of 3 kept -> element 1 of (1, 3, 4)
    out, state, _, _ = both([[[4, 1], [3, N]]], None, (-1, 1 << 24, 0, 1))
    assert out == [[[3, 3], [3, N]]] and state == [[0, 0], [0, 1]]
    # a row of six, radius 2: windows clipped to the image; n = 3, 4, 5, 5, 4, 3
    out, _, _, _ = both([[[9, 1, 8, 2, 7, 3]]], None, (-1, 1 << 24, 0, 2))
    assert out == [[[8, 2, 7, 3, 3, 3]]]
    # radius 0 copies
    assert both([[[9, 1, 8, 2, 7, 3]]], None, (-1, 1 << 24, 0, 0))[0] == [[[9, 1, 8, 2, 7, 3]]]
    # the median reads fwd, never out, and skips speckles: the lone 1000 is removed, its neighbours ignore it
    out, state, _, _ = both([[[5, 6, 1000, 7, 8]]], None, (-1, 10, 2, 1))
    assert state == [[0, 0, 3, 0, 0]] and out == [[[5, 5, N, 7, 7]]]


def test_int32_extremes_side_by_side():
    M, m = cu.IMAX, cu.IMIN1
    # differences of 2^32 - 2 and sums of +-(2^32 - 2) in 64 bits: apart at any diff, failing at any tolerance
    out, state, label, stats = both([[[M, m, m, M]]], None, (-1, 1 << 24, 0, 0))
    assert label == [[0, 1, 1, 3]] and out == [[[M, m, m, M]]]
    out, state, label, stats = both([[[M, m, m, M]]], None, (-1, 1 << 24, 2, 1))
    assert state == [[3, 0, 0, 3]] and out == [[[N, m, m, N]]] and stats == [2, 0, 0, 2]
    # channel 1 may hold INT32_MIN as a value: it is no "none" there
    _, state, label, _ = both([[[0, 0]], [[N, M]]], None, (-1, 1 << 24, 0, 0))
    assert state == [[0, 0]] and label == [[0, 1]]
    # the check: the shifts are +-2^23 pixels, outside any image; with r = 0 the sums M + M and m + m do not wrap
    assert both([[[M, m]]], [[[0, 0]]], (1 << 24, 0, 0, 0))[1] == [[2, 2]]
    f, g = [[[0], [0]], [[M], [m]]], [[[0], [0]], [[M], [m]]]                        # r1 = +-2^23: outside
    assert both(f, g, (1 << 24, 0, 0, 0))[1] == [[2], [2]]
    # medians over both extremes: the windows are (M, 0), (M, 0, m) and (0, m)
    out, _, _, _ = both([[[M, 0, m]]], None, (-1, 1 << 24, 0, 1))
    assert out == [[[0, 0, m]]]


@pytest.mark.parametrize("C_", [1, 2])
def test_restatements_agree_on_random_fields(C_):
    rng = np.random.default_rng(90 + C_)
    for trial in range(10):
        W, H = int(rng.integers(1, 41)), int(rng.integers(1, 36))
        fwd, bwd = cu.random_fields(W, H, C_, 2, seed=int(rng.integers(1 << 30)))
        prm = (int(rng.choice([-1, 0, 256, 300])), int(rng.choice([0, 100, 256])), int(rng.choice([0, 1, 2, 5, 64])), trial % 3)
        for t in range(2):
            p, q = cu.clean_plain(fwd[t], bwd[t], prm), cu.clean_np(fwd[t], bwd[t], prm)
            for a, b in zip(p, q):
                assert a.dtype == b.dtype and np.array_equal(a, b), (trial, W, H, prm)
            assert p[3].sum() == W * H and ((p[1] == 0) == (p[0][0] != N)).all() and ((p[2] >= 0) == ((p[1] == 0) | (p[1] == 3))).all()


def test_constructed_fields_have_the_components_they_are_built_for():
    for name, (f0, ncomp) in cu.constructed(72, 40).items():
        f = f0[None].astype(np.int32)
        _, state, label, _ = cu.clean_np(f, None, (-1, 256, 0, 0))
        roots = np.unique(label[label >= 0])
        assert len(roots) == ncomp, (name, len(roots))
        assert np.array_equal(label, cu.clean_plain(f, None, (-1, 256, 0, 0))[2]), name
    big = cu.constructed()
    for name in ("serpentine", "spiral", "comb", "u"):
        on = big[name][0] != N
        assert on.sum() > 2000 or name == "u"
    assert (big["serpentine"][0] != N).any(axis=1).all()         # through every row of 200 x 90


def test_fields_of_the_gpu_tests_meet_their_conditions():
    """the random fields tests/test_gpu_clean.py runs on (same seeds): every state occurs at every size that has room for
    them, one pair has no value at all, and a component runs through three tiles wherever the image has three"""
    for W, H in cu.SIZES:
        for C_ in (1, 2):
            fwd, bwd = cu.random_fields(W, H, C_)
            assert fwd.shape == (3, C_, H, W) and (fwd[1] == N).all()
            out, state, label, stats = cu.clean(fwd, bwd, cu.DEFAULTS)
            assert stats[1].tolist() == [0, W * H, 0, 0]
            if W * H >= 33 * 17:
                assert (stats[0] > 0).all() and (stats[2] > 0).all(), (W, H, C_, stats.tolist())
            tiles = ((W + 31) // 32) * ((H + 31) // 32)
            if tiles >= 3:
                assert cu.spans_three_tiles(label[0]) and cu.spans_three_tiles(label[2]), (W, H, C_)
                assert cu.spans_three_tiles(cu.clean(fwd, None, (-1, 256, 64, 1))[2][0])


def test_flip_restatement():
    sup = np.array([[(5, 3, 2.0), (5, 3, -2.0), (5, 3, 0.5), (5, 3, np.nan), (5, 3, np.inf), (5, 3, 2.0 ** 24), (0, 0, -0.0),
                     (-2 ** 31, 1, 1.0), (9, 9, 9.0)]], du.SUPPORT)
    out, _ = cu.flip(sup, [8])
    assert out[0, :8].tolist() == [(3, 3, -2.0), (7, 3, 2.0), (-1, -1, 0.0), (-1, -1, 0.0), (-1, -1, 0.0), (-1, -1, 0.0), (0, 0, 0.0),
                                   (2 ** 31 - 1, 1, -1.0)]
    assert out[0, 8].tolist() == (0, 0, 0.0)                             # beyond the count: not touched
    assert np.signbit(out["d"][0, 1]) == False and np.signbit(out["d"][0, 6]) == False and np.signbit(out["d"][0, 0])
    back, _ = cu.flip(out, [8])
    assert back[0, :2].tobytes() == sup[0, :2].tobytes() and back[0, 6:8].tobytes() == sup[0, 6:8].tobytes()
    cor = np.array([[(1, 2, 3, 4), (-5, 6, 2 ** 31 - 1, -2 ** 31)]], du.CORR)
    ref = np.array([[(3, -4, 7, 1), (-32768, 32767, 0xFFFF, 6)]], du.REFINEMENT)
    out, fout = cu.flip(cor, [5], ref)
    assert out[0].tolist() == [(3, 4, 1, 2), (2 ** 31 - 1, -2 ** 31, -5, 6)]
    assert fout[0].tolist() == [(-3, 4, 7, 1), (-32768, -32767, 0xFFFF, 6)]
    # F + G = 0: the fields of a record and of its reverse cancel at the record's ends
    rec = np.array([(10, 4, 3.0)], du.SUPPORT)
    rref = np.array([(40, 0, 5, 1)], du.REFINEMENT)
    rev, rrev = cu.flip(rec[None], [1], rref[None])
    f, _ = du.densify_pair(rec, 1, 16, 8, du.DEFAULTS, rref)
    g, _ = du.densify_pair(rev[0], 1, 16, 8, du.DEFAULTS, rrev[0])
    assert f[0, 4, 10] == 256 * 3 - 40 and g[0, 4, 7] == -f[0, 4, 10]


def test_entry_points_are_declared_and_bound():
    import opengpc_amd as g
    from opengpc_amd import build
    build.build()
    L = g.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpc_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct gpc_clean \{(.*?)\} gpc_clean;", header, re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", body) == ["check_tol_q8", "speckle_diff_q8", "speckle_min", "median_radius"]
    assert C.sizeof(g.Clean) == 16
    d = g.Clean()
    assert (d.check_tol_q8, d.speckle_diff_q8, d.speckle_min, d.median_radius) == cu.DEFAULTS
    for name, nargs in NAMES.items():
        assert name in g.capi.SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == nargs == len(getattr(L, name).argtypes), name
    kernels = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_slots())]
    assert len(set(kernels)) == len(kernels) and "" not in kernels
    at = kernels.index("k_quad_write")
    assert tuple(kernels[at + 1:]) == KERNELS and L.gpc_hip_kernel_count() == 32
    for m in ("clean_fields_device", "flip_records_device", "clean_batch_device", "clean_sequence_device", "clean_fields"):
        assert callable(getattr(g.Context, m)), m


def test_refusals_with_a_null_context():
    """without a context every call refuses before it touches anything"""
    import opengpc_amd as g
    from opengpc_amd import build
    build.build()
    L = g.load()
    E = g.capi.E_INVALID
    prm, fill, s = C.byref(g.Clean()), C.byref(g.Densify()), C.byref(g.Settings.sparsematch())
    assert L.gpc_hip_clean_fields_device(None, 8, 8, 1, 4, 4, 1, prm, 4096, None, None, None) == E
    assert L.gpc_hip_clean_fields(None, 8, 8, 1, 4, 4, 1, prm, 4096, None, None, None) == E
    assert L.gpc_hip_flip_supports_device(None, 8, None, 4, 8, 1, 8, None) == E
    assert L.gpc_hip_flip_correspondences_device(None, 8, None, 4, 8, 1, 8, None) == E
    assert L.gpc_hip_clean_batch_device(None, 8, 8, 96, 64, 1, s, 0, fill, prm, 8, None, None, None, None, None, None, None) == E
    assert L.gpc_hip_clean_sequence_device(None, 8, 96, 64, 2, s, 0, fill, prm, 8, None, None, None, None, None, None, None) == E


def test_cpp_clean_header_compiles(tmp_path):
    """include/gpc/clean.hpp compiles against the library with a plain host compiler; the program only reverses records"""
    src, exe = str(tmp_path / "clean_hpp_check.cpp"), str(tmp_path / "clean_hpp_check")
    with open(src, "w") as f:
        f.write("#include <gpc/clean.hpp>\n"
                "int main() {\n"
                "  gpc::dense::Field fwd;\n"
                "  if (false) { gpc::clean::Result r = gpc::clean::clean(fwd, &fwd, gpc::clean::Params()); return r.stats[0]; }\n"
                "  if (false) gpc::clean::clean(fwd);\n"
                "  std::vector<ndb::Support> s = {ndb::Support(5, 3, 2.f), ndb::Support(5, 3, 0.5f)};\n"
                "  const std::vector<ndb::Support> r = gpc::clean::reversed(s);\n"
                "  std::vector<ndb::Correspondence> c = {ndb::Correspondence(ndb::Point(1, 2), ndb::Point(3, 4))};\n"
                "  const std::vector<ndb::Correspondence> q = gpc::clean::reversed(c);\n"
                "  const gpc_clean p = gpc::clean::Params().toC();\n"
                "  const bool ok = r[0].x == 3 && r[0].y == 3 && r[0].d == -2.f && r[1].x == -1 && r[1].y == -1 && q[0].srcPt.x == 3 &&\n"
                "                  q[0].tarPt.y == 2 && p.check_tol_q8 == 256 && p.speckle_min == 64 && gpc::clean::Speckle == 3;\n"
                "  return ok ? 0 : 1;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-pthread"])
    assert subprocess.run([exe], timeout=60).returncode == 0


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm toolchain's clang++")
def test_host_checks_under_asan_ubsan(tmp_path):
    """opengpc_amd/csrc/clean_host.h driven by a stand-alone program: parameters, limits, overlap, the tile geometry and
    the workspace sizes"""
    exe = str(tmp_path / "clean_check")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "opengpc_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "clean_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.returncode, res.stdout, res.stderr)
