"""CPU: the scoring rules of gpc_hip_score_* (include/gpc_hip.h) as tests/score_util.py restates them, on cases small enough
to count by hand; the float32 inputs that tell a fused multiply-add from two roundings; the kernels' resources and their
ISA (no scratch, no vector spills, no fused multiply-add); the Python wrappers' argument checks against a fake library; and the
C++ API (include/gpc/evaluation.hpp, samples/evaluate) compiling and building Truth planes numpy agrees with."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import score_util as su
from score_util import write_flo, write_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SUPPORT = np.dtype([("x", "<i4"), ("y", "<i4"), ("d", "<f4")])
CORR = np.dtype([("sx", "<i4"), ("sy", "<i4"), ("tx", "<i4"), ("ty", "<i4")])


def one_support(d, g, thr, ignore=0):
    u = np.full((4, 16), g, F32)
    ign = np.full((4, 16), ignore, np.uint8)
    return su.score_records(np.array([(3, 2, d)], SUPPORT), 1, 8, u, None, ign, thr)


def test_threshold_edges_by_hand():
    s = one_support(7.0, 4.0, [3.0, 2.0])                     # e2 = 9 == 3^2 counts; 9 > 4 does not
    assert (s["n_records"], s["n_judged"], s["n_within"][:3], s["sum_e2_q8"]) == (1, 1, [1, 0, 0], 9 * 256)
    beyond = np.nextafter(F32(3.0), F32(4.0))                 # one ulp beyond the threshold
    s = one_support(float(beyond), 0.0, [3.0])
    assert s["n_judged"] == 1 and s["n_within"][0] == 0
    s = one_support(float(np.nextafter(F32(3.0), F32(0.0))), 0.0, [3.0])
    assert s["n_within"][0] == 1
    s = one_support(2.0, 2.0, [0.0])                          # threshold 0: exact hits only
    assert s["n_within"][0] == 1 and s["sum_e2_q8"] == 0
    assert one_support(2.5, 2.0, [0.0])["n_within"][0] == 0 and one_support(2.5, 2.0, [0.0])["sum_e2_q8"] == 64


@pytest.mark.parametrize("g", [np.nan, np.inf, -np.inf, 1e10, -1e10, 1e9, -1e9])
def test_unknown_truth_is_not_judged(g):
    s = one_support(1.0, g, [1.0])
    assert (s["n_records"], s["n_ignored"], s["n_no_truth"], s["n_judged"], s["sum_e2_q8"]) == (1, 0, 1, 0, 0)
    s = one_support(1.0, g, [1.0], ignore=7)                  # ignore takes precedence over no-truth
    assert (s["n_ignored"], s["n_no_truth"], s["n_judged"]) == (1, 0, 0)


def test_truth_just_below_1e9_is_judged_and_the_sum_is_clamped():
    g = float(np.nextafter(F32(1e9), F32(0.0)))
    s = one_support(0.0, g, [1000.0])
    assert s["n_judged"] == 1 and s["n_within"][0] == 0 and s["sum_e2_q8"] == 1048576 * 256
    s = one_support(1024.0, 0.0, [1024.0])                    # e2 == 2^20 exactly: the clamp's edge
    assert s["n_within"][0] == 1 and s["sum_e2_q8"] == 1048576 * 256


def test_records_whose_own_values_are_not_numbers():
    """d = NaN or +-inf on usable truth: e2 is NaN / inf; the record stays judged, is within no threshold (not even 1e9^2
    would hold a NaN) and adds the clamp, as fminf(e2, 2^20) gives it"""
    for d in (np.nan, np.inf, -np.inf):
        s = one_support(d, 2.0, [0.0, 1000.0])
        assert (s["n_judged"], s["n_no_truth"], s["n_within"][:2], s["sum_e2_q8"]) == (1, 0, [0, 0], 1048576 * 256)


def test_counts_cap_and_out_of_image_records():
    u = np.zeros((4, 16), F32)
    rec = np.array([(1, 1, 0.0), (16, 1, 0.0), (-1, 2, 0.0), (3, 4, 0.0), (2, 2, 0.5)], SUPPORT)
    s = su.score_records(rec, 9, 5, u, None, None, [0.0])     # count above cap: min(count, cap) records
    assert (s["n_records"], s["n_no_truth"], s["n_judged"], s["n_within"][0]) == (5, 3, 2, 1)
    assert su.score_records(rec, 2, 5, u, None, None, [0.0])["n_records"] == 2
    assert su.score_records(rec, 0, 5, u, None, None, [0.0]) == su.empty_score()


def test_correspondence_error_and_rounding():
    u, v = np.full((4, 16), 1.5, F32), np.full((4, 16), -2.0, F32)
    rec = np.array([(2, 1, 4, 0)], CORR)                      # ex = 2 - 1.5, ey = -1 + 2: e2 = 1.25
    s = su.score_records(rec, 1, 1, u, v, None, [1.0, 1.25 ** 0.5, 2.0])
    assert s["n_within"][:3] == [0, int(F32(1.25) <= F32(1.25 ** 0.5) * F32(1.25 ** 0.5)), 1] and s["sum_e2_q8"] == 320
    assert list(su.round_half_away(np.array([0.5, -0.5, 1.5, -1.5, 0.49999997, 2.4999998], F32))) == [1, -1, 2, -2, 0, 2]


def test_matchable_margin_edges():
    W, H = 64, 48
    candL = np.zeros((H, W), bool)
    candR = np.ones((H, W), bool)
    pts = [(13, 13), (50, 34), (20, 20), (30, 30), (40, 20)]
    for x, y in pts:
        candL[y, x] = True
    u, v = np.zeros((H, W), F32), np.zeros((H, W), F32)
    u[13, 13] = -0.5           # R(-0.5) = -1: x = 12, left of the margin
    u[34, 50] = 0.49           # stays on x = 50 = W - 14, the last column inside
    v[20, 20] = 14.5           # R = 15: y = 35 = H - 13, below the margin
    v[30, 30] = -17.0          # y = 13: the first row inside
    u[20, 40] = np.nan
    assert su.matchable(candL, candR, u, v, None) == (5, 2)
    ign = np.zeros((H, W), np.uint8)
    ign[34, 50] = 1
    assert su.matchable(candL, candR, u, v, ign) == (5, 1)
    candR[13, 30] = False      # the true target is not a candidate of the right image
    assert su.matchable(candL, candR, u, v, ign) == (5, 0)
    g = np.zeros((H, W), F32)  # stereo: (x - R(g), y)
    g[13, 13], g[34, 50], g[20, 20] = 0.5, 37.0, 7.4
    candR[:] = True
    assert su.matchable(candL, candR, g, None, None) == (5, 4)   # (13,13) -> x = 12 is out; 50 - 37 = 13 is the first column inside


def test_fma_sensitive_inputs():
    """fl(fl(ex*ex) + fl(ey*ey)) and fma(ex, ex, fl(ey*ey)) on different sides of the threshold: the restatement gives the
    two-rounding answer.  The GPU test feeds the same inputs to the kernel."""
    pairs, thr = su.fma_sensitive_corr()
    assert len(pairs) == 8
    t2 = F32(thr) * F32(thr)
    for ex, ey in pairs:
        two = F32(F32(ex * ex) + F32(ey * ey))
        fused = F32(float(ex) * float(ex) + float(F32(ey * ey)))
        assert (two <= t2) != (fused <= t2)
        u, v = np.full((2, 16), -ex, F32), np.full((2, 16), -ey, F32)
        s = su.score_records(np.array([(5, 1, 5, 1)], CORR), 1, 1, u, v, None, [thr])
        assert s["n_within"][0] == int(two <= t2)


# --------------------------------------------------------------------------- the kernels, compiled for gfx950
@pytest.fixture(scope="module")
def score_isa(tmp_path_factory):
    """k_score.h alone, every instantiation, as device assembly with the compiler's resource remarks"""
    d = tmp_path_factory.mktemp("k_score")
    src = d / "k_score_only.hip"
    src.write_text('#include "k_score.h"\n'
                   "template __global__ void gpc::k_score_records<false>(const gpc::ScRec<false>*, long, const int32_t*, int, int, const float*, const float*, const uint8_t*, gpc::ScoreThr, gpc::ScoreDev*);\n"
                   "template __global__ void gpc::k_score_records<true>(const gpc::ScRec<true>*, long, const int32_t*, int, int, const float*, const float*, const uint8_t*, gpc::ScoreThr, gpc::ScoreDev*);\n" +
                   "".join("template __global__ void gpc::k_score_matchable<%s, %s>(const uint8_t*, int, int, int, GpcDivW, const float*, const float*, const uint8_t*, gpc::ScoreDev*);\n" % (a, b)
                           for a in ("false", "true") for b in ("false", "true")))
    out = d / "k_score_only.s"
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                          "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "opengpc_amd", "csrc"),
                          "-o", str(out), str(src)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return out.read_text(), res.stderr


def test_kernel_resources(score_isa):
    asm, remarks = score_isa
    names = re.findall(r"Function Name: (\S+)", remarks)
    assert len(names) == 6 and all("k_score" in n for n in names)
    for key in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill", "SGPRs Spill"):
        vals = [int(v) for v in re.findall(key + r": (\d+)", remarks)]
        assert len(vals) == 6
        assert max(vals) == 0 or key.startswith("SGPRs"), (key, vals)     # no scratch, no vector spills
    assert max(int(v) for v in re.findall(r"SGPRs Spill: (\d+)", remarks)) <= 8
    assert min(int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", remarks)) >= 7
    assert "scratch_" not in asm


def test_kernels_are_not_contracted_and_use_integer_atomics_only(score_isa):
    asm, _ = score_isa
    ops = set(re.findall(r"^\s+(v_\w+|global_atomic\w+|flat_atomic\w+|ds_\w*add\w*)", asm, flags=re.M))
    fused = sorted(o for o in ops if re.match(r"v_(pk_)?(fma|fmac|mad|mac)\w*_f(16|32|64)", o))
    assert fused == [], fused
    assert "v_mul_f32" in " ".join(ops) or "v_mul_f32_e32" in ops
    atomics = sorted(o for o in ops if "atomic" in o)
    assert atomics and all(re.fullmatch(r"global_atomic_add_x2", a) for a in atomics), atomics


def test_kernel_resources_in_the_library():
    """tools/kres.sh on the library's own translation unit, as tests/test_kernel_resources.py holds the other kernels: every
    k_score_ instantiation without scratch and without vector spills, at most 8 scalars spilled to VGPR lanes, 7+ waves."""
    line = re.compile(r"^(gpc::\S.*?)\s+sgpr\s+(\d+)\s+vgpr\s+(\d+)\s+spill s\s+(\d+)\s+v\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)")
    env = dict(os.environ, KRES_OUT=os.path.join(ROOT, "tests", "cpp", "bin", "libgpc_kres_score.so"))
    os.makedirs(os.path.dirname(env["KRES_OUT"]), exist_ok=True)
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), "k_score_"], env=env, check=True, capture_output=True,
                         text=True, timeout=900).stdout
    rows = {m.group(1).strip(): tuple(map(int, m.groups()[1:])) for m in map(line.match, txt.splitlines()) if m}
    assert len(rows) == 6, txt[-2000:]
    for name, (sgpr, vgpr, sspill, vspill, scratch, occ) in rows.items():
        assert scratch == 0 and vspill == 0 and sspill <= 8 and occ >= 7 and vgpr <= 64, (name, rows[name])


def test_score_kernels_in_the_library_too():
    """the same through tools/kres.sh on the whole translation unit is held by test_kernel_resources.py's fixture for the
    other kernels; here: the library names the two kernels in its timing table"""
    from opengpc_amd import build
    build.build()
    import opengpc_amd as g
    L = g.load()
    names = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_count())]
    assert names[-2:] == ["k_score_records", "k_score_matchable"] and len(names) <= 32
    assert g.SCORE_DTYPE.itemsize == 120 and C.sizeof(g.capi.Truth) == 24
    assert L.gpc_hip_abi_version() == 1


# --------------------------------------------------------------------------- the Python wrappers
class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("gpc_hip_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


def _fake_context():
    import opengpc_amd as g
    ctx = g.Context.__new__(g.Context)
    ctx.L, ctx.h, ctx.device, ctx._pinned = _FakeLib(), C.c_void_p(1), 0, []
    return ctx


def test_wrappers_refuse_bad_arguments_before_the_library():
    import opengpc_amd as g
    ctx = _fake_context()
    s = g.Settings.sparsematch()
    P, H, W = 2, 48, 64
    L = np.zeros((P, H, W), np.uint8)
    u = np.zeros((P, H, W), F32)
    ign = np.zeros((P, H, W), np.uint8)
    bad_thr = ([], [1.0] * 9, [-1.0], [float("nan")], [1.0, float("inf")], [[1.0, 2.0]])
    for thr in bad_thr:
        for call in (lambda: ctx.score_batch(L, L, s, u, ign, thr),
                     lambda: ctx.score_sequence(L, s, u[:1], u[:1], None, thr),
                     lambda: ctx.score_supports_device(64, 8, 64, W, H, P, 64, 0, thr, 64),
                     lambda: ctx.score_correspondences_device(64, 8, 64, W, H, P, 64, 64, 0, thr, 64),
                     lambda: ctx.score_batch_device(64, 64, W, H, P, s, 64, 0, thr, 64),
                     lambda: ctx.score_sequence_device(64, W, H, P, s, 64, 64, 0, thr, 64)):
            with pytest.raises(ValueError):
                call()
    shapes = (lambda: ctx.score_batch(L, L[:1], s, u, ign, [1.0]),
              lambda: ctx.score_batch(L, L, s, u[:1], ign, [1.0]),
              lambda: ctx.score_batch(L, L, s, u, ign[:, :, :32], [1.0]),
              lambda: ctx.score_batch(L, L, s, u.astype(np.float64), ign, [1.0]),
              lambda: ctx.score_batch(L.astype(np.int32), L, s, u, ign, [1.0]),
              lambda: ctx.score_batch(L, L, s, None, ign, [1.0]),
              lambda: ctx.score_sequence(L, s, u, u, None, [1.0]),              # truth of N - 1 pairs, not N
              lambda: ctx.score_sequence(L, s, u[:1], None, None, [1.0]),       # correspondences need v
              lambda: ctx.score_sequence(L[:1], s, u[:0], u[:0], None, [1.0]),  # one frame
              lambda: ctx.score_supports_device(64, 8, 64, W, H, P, 0, 0, [1.0], 64),
              lambda: ctx.score_supports_device(64, 0, 64, W, H, P, 64, 0, [1.0], 64),
              lambda: ctx._score_records_device(ctx.L.gpc_hip_score_supports_device, 64, 8, 64, W, H, P, 64, 64, 0, [1.0], 64,
                                                False),                         # v given for supports
              lambda: ctx.score_correspondences_device(64, 8, 64, W, H, P, 64, 0, 0, [1.0], 64),
              lambda: ctx.score_sequence_device(64, W, H, 1, s, 64, 64, 0, [1.0], 64))
    for call in shapes:
        with pytest.raises(ValueError):
            call()
    sup = np.zeros((P, 8), g.SUPPORT_DTYPE)
    cor = np.zeros((P, 8), g.CORR_DTYPE)
    for call in (lambda: ctx.score_records(sup, [1, 2], u, u, None, [1.0]),          # v given for supports
                 lambda: ctx.score_records(cor, [1, 2], u, None, None, [1.0]),       # correspondences need v
                 lambda: ctx.score_records(sup, [1], u, None, None, [1.0]),          # one count for two pairs
                 lambda: ctx.score_records(sup, [1, 2], u[:1], None, None, [1.0]),
                 lambda: ctx.score_records(sup[0], [1], u[:1], None, None, [1.0]),   # not [P, cap]
                 lambda: ctx.score_records(np.zeros((P, 8, 3), np.int32), [1, 2], u, None, None, [1.0]),
                 lambda: ctx.score_records(sup, [1, 2], u, None, ign[:, :8], [1.0]),
                 lambda: ctx.score_records(sup, [1, 2], u, None, None, [])):
        with pytest.raises(ValueError):
            call()
    assert ctx.L.calls == []
    assert len(ctx.score_records(sup, [1, 2], u, None, ign, [1.0])) == P and len(ctx.score_records(cor, [8, 9], u, u, None, 2.0)) == P
    assert ctx.L.calls == ["gpc_hip_score_supports", "gpc_hip_score_correspondences"]
    del ctx.L.calls[:]
    # and good arguments reach the entry point they name
    assert ctx.score_batch(L, L, s, u, None, [1.0, 2.0]).dtype == g.SCORE_DTYPE
    assert len(ctx.score_sequence(L, s, u[:1], u[:1], ign[:1], 3.0)) == 1
    ctx.score_supports_device(64, 8, 64, W, H, P, 64, 0, [1.0], 64)
    ctx.score_correspondences_device(64, 8, 64, W, H, P, 64, 64, 64, [1.0], 64)
    ctx.score_batch_device(64, 64, W, H, P, s, 64, 0, [1.0], 64)
    ctx.score_sequence_device(64, W, H, 3, s, 64, 64, 0, [1.0], 64)
    assert ctx.L.calls == ["gpc_hip_score_batch", "gpc_hip_score_sequence", "gpc_hip_score_supports_device",
                           "gpc_hip_score_correspondences_device", "gpc_hip_score_batch_device", "gpc_hip_score_sequence_device"]


# --------------------------------------------------------------------------- the C++ API
def test_cpp_truth_planes_round_trip(tmp_path):
    """gpc::evaluation::Truth from a synthetic .flo + four masks, and from an RGB disparity map + two masks, holds the planes
    numpy expects (FNV-1a of the float / byte planes printed by tests/cpp/evaluation_check.cpp)."""
    from test_host_api import BIN, compile_cpp, run
    from opengpc_amd import build
    build.build()
    exe = compile_cpp(os.path.join(ROOT, "tests", "cpp", "evaluation_check.cpp"), os.path.join(BIN, "evaluation_check"))
    rng = np.random.default_rng(3)
    W, H = 64, 48
    t = str(tmp_path / "training")
    u = rng.normal(0, 4, (H, W)).astype(F32)
    v = rng.normal(0, 2, (H, W)).astype(F32)
    u[5, 7] = 1e10
    write_flo(os.path.join(t, "flow", "alley_1", "frame_0001.flo"), u, v)
    masks = [(rng.random((H, W)) < 0.1).astype(np.uint8) * 255 for _ in range(4)]
    for name, m in zip(("occlusions/alley_1/frame_0001", "occlusions/alley_1/frame_0002", "invalid/alley_1/frame_0001",
                        "invalid/alley_1/frame_0002"), masks):
        write_png(os.path.join(t, name + ".png"), m)
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    write_png(os.path.join(t, "disparities", "alley_1", "frame_0001.png"), rgb)
    write_png(os.path.join(t, "outofframe", "alley_1", "frame_0001.png"), masks[2])
    for d in ("clean", "final", "clean_left", "clean_right"):
        write_png(os.path.join(t, d, "alley_1", "frame_0001.png"), np.zeros((H, W), np.uint8))

    def fnv(a):
        h = 1469598103934665603
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return h

    out = run(exe, str(tmp_path) + "/")
    got = {l.split()[0]: l.split()[1:] for l in out.splitlines() if l.startswith(("FLOW", "STEREO", "SUBPIX", "SCORE"))}
    ign_flow = ((masks[0] | masks[1] | masks[2] | masks[3]) != 0).astype(np.uint8)
    assert got["FLOW"] == [str(W), str(H), str(fnv(u)), str(fnv(v)), str(fnv(ign_flow))]
    disp = (4 * rgb[..., 0].astype(np.int32) + rgb[..., 1] // 64).astype(F32)          # SintelStereo::decodeDisparity
    ign_st = ((masks[0] | masks[2]) != 0).astype(np.uint8)
    assert got["STEREO"] == [str(W), str(H), str(fnv(disp)), str(fnv(ign_st))]
    sub = (rgb[..., 0].astype(F32) * F32(4) + rgb[..., 1].astype(F32) / F32(64) + rgb[..., 2].astype(F32) / F32(16384))
    assert got["SUBPIX"] == [str(fnv(sub.astype(F32)))]
    assert got["SCORE"] == ["0.75", "0.5"]                                              # precision(0), recall(0) of 3 / 4 / 6


def test_evaluate_sample_builds():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "samples"), "evaluate"])
    exe = os.path.join(ROOT, "samples", "evaluate")
    assert os.access(exe, os.X_OK)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode != 0 and "usage" in (res.stdout + res.stderr).lower()
