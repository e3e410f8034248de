"""CPU: matching over an image pyramid (gpc_hip_pyramid_*) -- the numpy restatement of its two new steps checked on itself,
the figures the GPU cases rely on taken from the oracle alone, the declarations in header and binding, the new kernels'
resources, and the host-side checks driven by a stand-alone program under AddressSanitizer and UBSan."""
import os
import re
import subprocess

import numpy as np
import pytest

import pyramid_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
NAMES = {"gpc_hip_pyramid_levels": 5, "gpc_hip_pyramid_down_device": 6, "gpc_hip_pyramid_merge_supports_device": 12,
         "gpc_hip_pyramid_merge_correspondences_device": 12, "gpc_hip_pyramid_batch_device": 13,
         "gpc_hip_pyramid_sequence_device": 12, "gpc_hip_pyramid_batch": 13, "gpc_hip_pyramid_sequence": 12}
KERNELS = ("k_pyr_down", "k_pyr_keep", "k_pyr_scan", "k_pyr_write")


def test_rounding_at_every_class_of_the_sum():
    """sums = 0 .. 3 mod 4 round half up: (s + 2) >> 2"""
    for s, want in ((0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 1), (6, 2), (7, 2), (1017, 254), (1018, 255), (1020, 255)):
        a = min(s, 255)
        b = min(s - a, 255)
        c = min(s - a - b, 255)
        d = s - a - b - c
        img = np.array([[a, b], [c, d]], np.uint8)
        assert pu.down(img)[0, 0] == want == (s + 2) // 4, s
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (7, 12)).astype(np.uint8)          # odd height: the last row is dropped
    got = pu.down(img)
    assert got.shape == (3, 6)
    for y in range(3):
        for x in range(6):
            assert got[y, x] == (int(img[2 * y, 2 * x]) + int(img[2 * y, 2 * x + 1]) + int(img[2 * y + 1, 2 * x]) +
                                 int(img[2 * y + 1, 2 * x + 1]) + 2) >> 2
    assert (pu.down(np.full((4, 4), 255, np.uint8)) == 255).all()


def test_block_test_at_the_corners_and_just_outside():
    W, H = 64, 40
    for l in (1, 2, 3):
        n = 1 << l
        x, y = 3, 2                                                # the block [x n, x n + n) x [y n, y n + n)
        corners = [(x * n, y * n), (x * n + n - 1, y * n), (x * n, y * n + n - 1), (x * n + n - 1, y * n + n - 1)]
        outside = [(x * n - 1, y * n), (x * n + n, y * n), (x * n, y * n - 1), (x * n, y * n + n)]
        for (px, py), hit in [(c, True) for c in corners] + [(o, False) for o in outside]:
            occ = np.zeros((H, W), bool)
            occ[py, px] = True
            assert pu.block_hit(occ, x, y, l) == hit, (l, px, py)
            lv0 = np.array([(px, py, 1.0)], pu.SUPPORT)
            coarse = np.array([(x, y, 1.0)], pu.SUPPORT)
            levels = [lv0] + [np.zeros(0, pu.SUPPORT)] * (l - 1) + [coarse]
            merged, kept = pu.merge(levels, W, H)
            assert kept[0] == 1 and kept[-1] == (0 if hit else 1), (l, px, py)
            if not hit:
                assert tuple(merged[-1]) == (x << l, y << l, float(1 << l))


def test_merge_rules():
    W, H = 64, 40
    s = lambda *r: np.array(list(r), pu.SUPPORT).reshape(-1)
    # records of one level never suppress each other; a kept level-1 record suppresses level 2, a dropped one does not
    l0 = s((10, 10, 2.0))
    l1 = s((5, 5, 1.0), (5, 5, 3.0), (9, 9, 1.0))                # the first two: block [10, 12) x [10, 12), hit by level 0
    l2 = s((2, 2, 1.0), (4, 4, 1.0), (15, 9, 0.0))               # [8, 12)^2: hit by level 0; [16, 20)^2: by kept (18, 18); free
    merged, kept = pu.merge([l0, l1, l2], W, H)
    assert kept == [1, 1, 1]
    assert [tuple(r) for r in merged] == [(10, 10, 2.0), (18, 18, 2.0), (60, 36, 0.0)]
    merged, kept = pu.merge([np.zeros(0, pu.SUPPORT), s((9, 9, 1.0), (9, 9, 2.0)), s((4, 4, 1.0))], W, H)
    assert kept == [0, 2, 0] and [tuple(r) for r in merged] == [(18, 18, 2.0), (18, 18, 4.0)]
    c = np.array([(3, 4, 5, 6)], pu.CORR)
    assert tuple(pu.map_records(c, 2)[0]) == (12, 16, 20, 24)
    # outside its level's image: kept, marks nothing
    merged, kept = pu.merge([s((70, 3, 0.0)), s((32, 1, 0.0), (-1, 0, 0.0)), s((16, 0, 0.0))], W, H)
    assert kept == [1, 2, 1]


def test_level_geometry():
    assert pu.level_sizes(1024, 436, 3) == [(1024, 436), (512, 218), (256, 109)]
    assert pu.level_sizes(1920, 1080, 3)[2] == (480, 270)
    assert pu.level_sizes(192, 120, 3)[2] == (48, 30) and pu.level_sizes(192, 119, 3) is None
    assert pu.level_sizes(160, 100, 3) is None and pu.level_sizes(224, 200, 3) is None and pu.level_sizes(320, 161, 1) is not None
    assert pu.level_sizes(256, 102, 2)[1] == (128, 51) and pu.level_sizes(320, 162, 2)[1] == (160, 81)
    assert pu.level_sizes(384, 240, 4)[3] == (48, 30) and pu.level_sizes(384, 240, 0) is None and pu.level_sizes(384, 240, 5) is None
    import opengpc_amd as g
    for W, H, n in ((1024, 436, 3), (192, 120, 3), (192, 119, 3), (160, 100, 3), (224, 200, 3), (384, 240, 4), (384, 240, 5),
                    (384, 240, 0), (256, 102, 2), (16400, 64, 1)):
        st, ws, hs = g.capi.pyramid_levels(W, H, n)
        want = pu.level_sizes(W, H, n)
        assert (st == 0) == (want is not None), (W, H, n, st)
        if want:
            assert list(zip(ws.tolist(), hs.tolist())) == want


def test_fixture_figures_from_the_oracle(oracle):
    """synth_pair(256, 128, 0, 8), zero forest, sparsematch settings: what the GPU cases take for granted"""
    L, R = oracle.synth_pair(256, 128, 0, 8)
    merged, kept, raw, ncand = pu.expected_supports(L, R, "zero", 3)
    assert raw == [14991, 3133, 125]
    assert kept[0] == 14991 and kept[1] == 213 and len(merged) == sum(kept)
    assert (merged["d"] == 8.0).all()                               # every level carries d * 2^l = 8
    lv = np.repeat(np.arange(3), kept)
    assert ((merged["x"] & ((1 << lv) - 1)) == 0).all() and ((merged["y"] & ((1 << lv) - 1)) == 0).all()
    # a construction whose level 2 keeps records: the right half 4x enlarged
    L, R = pu.enlarged_pair()
    merged, kept, raw, _ = pu.expected_supports(L, R, "zero", 3)
    assert all(k > 0 for k in kept) and kept[1] < raw[1] and kept[2] < raw[2], (kept, raw)


def test_entry_points_are_declared_and_bound():
    import opengpc_amd as g
    from opengpc_amd import build
    build.build()
    L = g.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpc_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+GPC_MAX_PYRAMID_LEVELS\s+4\b", header)
    for name, nargs in NAMES.items():
        assert name in g.capi.SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == nargs == len(getattr(L, name).argtypes), name
    kernels = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_slots())]
    assert len(set(kernels)) == len(kernels) and "" not in kernels
    at = kernels.index("k_refine")
    assert tuple(kernels[at + 1:at + 1 + len(KERNELS)]) == KERNELS and at >= L.gpc_hip_kernel_count() == 32
    for m in ("pyramid_down_device", "pyramid_merge_device", "pyramid_batch_device", "pyramid_sequence_device", "pyramid_batch",
              "pyramid_sequence"):
        assert callable(getattr(g.Context, m)), m
    # without a context every call refuses before it touches anything
    assert L.gpc_hip_pyramid_down_device(None, 8, 32, 2, 1, 8) == g.capi.E_INVALID
    assert L.gpc_hip_pyramid_batch_device(None, 8, 8, 192, 120, 1, 3, None, 8, 1, 8, 8, None) == g.capi.E_INVALID
    assert L.gpc_hip_pyramid_sequence(None, 8, 192, 120, 2, 3, None, 8, 1, 8, 8, None) == g.capi.E_INVALID
    assert L.gpc_hip_pyramid_merge_supports_device(None, 8, 8, 8, 64, 40, 1, 2, 8, 1, 8, 8) == g.capi.E_INVALID


def test_pyramid_kernels_use_no_scratch(capsys):
    """every k_pyr_* instantiation: no scratch, no VGPR spills (gfx950 cross-compile, tools/kres.sh)"""
    env = dict(os.environ, KRES_OUT=os.path.join(ROOT, "tests", "cpp", "bin", "libgpc_kres_pyramid.so"))
    os.makedirs(os.path.dirname(env["KRES_OUT"]), exist_ok=True)
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), r"k_pyr_"], capture_output=True, text=True,
                         env=env, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"^(gpc::\S.*?)\s+sgpr\s+\d+\s+vgpr\s+(\d+)\s+spill s\s+\d+\s+v\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line)
        if m:
            rows[m.group(1).strip()] = tuple(int(v) for v in m.groups()[1:])
    assert sorted(rows) == ["gpc::k_pyr_down", "gpc::k_pyr_keep", "gpc::k_pyr_scan", "gpc::k_pyr_write<false>",
                            "gpc::k_pyr_write<true>"], out
    for name, (vgpr, vspill, scratch, occ) in sorted(rows.items()):
        print("%-26s vgpr %3d  occupancy %d waves/SIMD" % (name, vgpr, occ))
        assert vspill == 0 and scratch == 0, (name, rows[name])


def test_cpp_pyramid_header_compiles(tmp_path):
    """include/gpc/pyramid.hpp compiles against the library with a plain host compiler; the program only asks for a geometry"""
    src, exe = str(tmp_path / "pyramid_hpp_check.cpp"), str(tmp_path / "pyramid_hpp_check")
    with open(src, "w") as f:
        f.write("#include <gpc/pyramid.hpp>\n"
                "int main() {\n  int w[4], h[4];\n"
                "  if (false) gpc::pyramid::matchPair(*(ndb::Buffer<uint8_t>*)nullptr, *(ndb::Buffer<uint8_t>*)nullptr,\n"
                "                                     gpc::inference::Forest::FilterMask(std::vector<int32_t>(), 0, 0, 0), gpc::inference::InferenceSettings(), 3);\n"
                "  return gpc::pyramid::levels(1024, 436, 3, w, h) && w[2] == 256 && h[2] == 109 ? 0 : 1;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-pthread"])
    assert subprocess.run([exe], timeout=60).returncode == 0


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm toolchain's clang++")
def test_host_checks_under_asan_ubsan(tmp_path):
    """opengpc_amd/csrc/pyramid_host.h driven by a stand-alone program: geometry, per-level settings and capacity, the
    argument checks of the downsampling step and the merge"""
    exe = str(tmp_path / "pyramid_check")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "opengpc_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "pyramid_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.returncode, res.stdout, res.stderr)
