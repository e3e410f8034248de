"""Frame sequences, host side: the two entry points are exported and declared, refusals that need no GPU, the C++ API
compiles, and the sequence kernels' resources match their pair-layout twins.  No GPU needed."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gpc_hip_match_sequence_device", "gpc_hip_match_sequence")


def test_entry_points_are_exported_and_declared():
    import opengpc_amd as g
    import opengpc_amd.capi as capi
    L = g.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpc_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert hasattr(g.Context, "match_sequence") and hasattr(g.Context, "match_sequence_device")


def test_refusals_without_a_context():
    import opengpc_amd as g
    L = g.load()
    s = g.Settings.sparsematch()
    buf = np.zeros(4 * 64 * 96, np.uint8)
    out = np.zeros(16, g.CORR_DTYPE)
    cnt = np.zeros(4, np.int32)
    for fn in (L.gpc_hip_match_sequence, L.gpc_hip_match_sequence_device):
        assert fn(None, buf.ctypes.data, 96, 64, 4, s, out.ctypes.data, 1, cnt.ctypes.data, None) == g.capi.E_INVALID


def test_cpp_api_compiles():
    """tests/cpp/sequence_check.cpp uses Forest::sequenceMatch."""
    out = os.path.join(ROOT, "tests", "cpp", "bin", "sequence_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sequence_check.cpp"), "-o", out,
                           "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-pthread"])
    assert os.path.exists(out)


def test_sequence_kernels_match_their_twins():
    """k_row_join_seq: no scratch, no VGPR spills and the occupancy of the k_row_join instantiation with the same
    parameters; k_seq_stats: no scratch (gfx950 cross-compile)."""
    env = dict(os.environ, KRES_OUT=os.path.join(ROOT, "tests", "cpp", "bin", "libgpc_kres_seq.so"))
    os.makedirs(os.path.dirname(env["KRES_OUT"]), exist_ok=True)
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), r"k_row_join<|k_row_join_seq|k_seq_stats"],
                         capture_output=True, text=True, env=env, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"^(gpc::\S.*?)\s+sgpr\s+\d+\s+vgpr\s+(\d+)\s+spill s\s+\d+\s+v\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line)
        if m:
            rows[m.group(1).strip()] = tuple(int(v) for v in m.groups()[1:])
    seq = {k: v for k, v in rows.items() if "k_row_join_seq<" in k}
    assert len(seq) == 22, sorted(rows)   # SPT 1 | 2 | 4 x NT 256 | 512 | 1024, (8 | 16, 1024); x WIDE
    for name, (vgpr, vspill, scratch, occ) in seq.items():
        twin = rows[name.replace("k_row_join_seq<", "k_row_join<")]
        assert vspill == 0 and scratch == 0, (name, seq[name])
        assert occ == twin[3], (name, seq[name], twin)
    st = rows["gpc::k_seq_stats"]
    assert st[1] == 0 and st[2] == 0
