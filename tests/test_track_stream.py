"""Track streams (gpc_hip_track_stream_*), host side: the new kernels' resources, the declarations in header and binding,
the C++ class, the refusals that need no GPU, and the stream's bookkeeping (pairs per push, frames or records, the 31-bit
bound on the ids) driven by a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
NAMES = ("gpc_hip_track_stream_create", "gpc_hip_track_stream_destroy", "gpc_hip_track_stream_reset",
         "gpc_hip_track_stream_push_device", "gpc_hip_track_stream_push", "gpc_hip_track_stream_push_records_device",
         "gpc_hip_track_stream_state", "gpc_hip_track_stream_table", "gpc_hip_track_stream_read_tracks")
KERNELS = ("k_trs_fill", "k_trs_scatter", "k_trs_link", "k_trs_settle", "k_trs_scan", "k_trs_walk", "k_trs_save", "k_trs_ncand")


def test_entry_points_are_exported_and_declared():
    import opengpc_amd as g
    import opengpc_amd.capi as capi
    L = g.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpc_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        # the binding passes as many arguments as the header declares
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(getattr(L, name).argtypes) == len(decl.split(",")), name
    assert re.search(r"typedef\s+struct\s+gpc_hip_track_stream\s+gpc_hip_track_stream\s*;", header)
    for m in ("push", "push_device", "push_records_device", "state", "table", "read_tracks", "reset", "close"):
        assert hasattr(g.TrackStream, m), m
    assert hasattr(g.Context, "track_stream")
    # gpc_track as the table holds it: the struct of the header and the binding's dtype
    fields = re.search(r"typedef struct gpc_track \{(.*?)\} gpc_track;", header, flags=re.S).group(1)
    assert tuple(re.findall(r"int32_t\s+(\w+)\s*;", fields)) == g.TRACK_DTYPE.names and g.TRACK_DTYPE.itemsize == 16
    # the new launches have timing slots of their own, behind the filter's and before the two of the scoring kernels (which
    # stay the last two, as tests/test_score.py holds them); every slot still fits the 32-bit timing mask
    names = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_count())]
    at = names.index("k_trs_fill")
    assert tuple(names[at:at + len(KERNELS)]) == KERNELS and names[at - 1] == "k_cons_write" and len(names) <= 32


def test_refusals_without_a_device():
    """Without a context every call refuses before it touches anything; without a GPU there is no context to make a stream
    on: gpc_hip_create fails with the library's no-device status."""
    import opengpc_amd as g
    import opengpc_amd.capi as capi
    L = g.load()
    s = g.Settings.sparsematch()
    h = C.c_void_p(0)
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    k, n = C.c_int(), C.c_int32()
    assert L.gpc_hip_track_stream_create(None, 96, 64, C.byref(s), 16, 4, C.byref(h)) == capi.E_INVALID and not h.value
    fake = C.c_void_p(p)   # (never dereferenced: a null context refuses first)
    assert L.gpc_hip_track_stream_push_device(None, fake, p, 1, p, p, None, p, p, C.byref(k)) == capi.E_INVALID
    assert L.gpc_hip_track_stream_push(None, fake, p, 1, p, p, None, p, p, C.byref(k), C.byref(n)) == capi.E_INVALID
    assert L.gpc_hip_track_stream_push_records_device(None, fake, p, p, 1, p, p) == capi.E_INVALID
    assert L.gpc_hip_track_stream_state(None, fake, None, None, C.byref(n)) == capi.E_INVALID
    assert L.gpc_hip_track_stream_read_tracks(None, fake, 0, 1, p, C.byref(n)) == capi.E_INVALID
    assert L.gpc_hip_track_stream_reset(None, fake) == capi.E_INVALID
    assert L.gpc_hip_track_stream_destroy(None, fake) == capi.E_INVALID
    assert L.gpc_hip_track_stream_table(None, C.byref(h), C.byref(h)) == capi.E_INVALID
    count = C.c_int(-1)
    L.gpc_hip_device_count(C.byref(count))
    if count.value <= 0:
        ctx = C.c_void_p()
        assert L.gpc_hip_create(0, C.byref(ctx)) == capi.E_NO_DEVICE and not ctx.value
        with pytest.raises(g.GpcError) as e:
            g.Context(0)
        assert e.value.status == capi.E_NO_DEVICE


def test_stream_kernels_use_no_scratch(capsys):
    """the k_trs_* kernels: no scratch, no VGPR spills (gfx950 cross-compile, tools/kres.sh); their occupancy is reported"""
    env = dict(os.environ, KRES_OUT=os.path.join(ROOT, "tests", "cpp", "bin", "libgpc_kres_track_stream.so"))
    os.makedirs(os.path.dirname(env["KRES_OUT"]), exist_ok=True)
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), r"k_trs_"], capture_output=True, text=True,
                         env=env, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"^(gpc::\S+)\s+sgpr\s+\d+\s+vgpr\s+(\d+)\s+spill s\s+\d+\s+v\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line)
        if m:
            rows[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    assert sorted(rows) == sorted("gpc::" + k for k in KERNELS), out   # every timing slot is a kernel of that name
    for name, (vgpr, vspill, scratch, occ) in sorted(rows.items()):
        print("%-22s vgpr %3d  occupancy %d waves/SIMD" % (name, vgpr, occ))
        assert vspill == 0 and scratch == 0, (name, rows[name])


def test_cpp_track_stream_compiles():
    """gpc::tracking::TrackStream (include/gpc/tracking.hpp): tests/cpp/track_stream_check.cpp compiles against the library;
    without arguments the program only says ok"""
    out = os.path.join(ROOT, "tests", "cpp", "bin", "track_stream_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "track_stream_check.cpp"), "-o", out,
                           "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"),
                           "-pthread"])
    res = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.returncode, res.stdout, res.stderr)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm toolchain's clang++")
def test_bookkeeping_under_asan_ubsan(tmp_path):
    """opengpc_amd/csrc/track_stream_host.h, the part of a stream that needs no HIP, driven by a stand-alone program: the
    argument checks, the id bound (refusal at 2^31 - 1, nothing changed, tightened by the true total), the per-push limits"""
    exe = str(tmp_path / "track_stream_book_check")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "opengpc_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "track_stream_book_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.returncode, res.stdout, res.stderr)
