"""Point tracks, host side: the plain restatement of the linking rule (tests/track_util.py) on hand-made cases with the
answers written out, the new kernels' resources, the C++ assembly of Track vectors, and the entry points' declarations
and refusals that need no GPU."""
import os
import re
import subprocess

import numpy as np

from track_util import corr_array, expected_arrays, restate, track_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gpc_hip_track_records_device", "gpc_hip_track_sequence_device", "gpc_hip_track_records", "gpc_hip_track_sequence")
W, H = 32, 24


def run(pairs, cap=None):
    rec, counts = corr_array(pairs, cap)
    return restate(rec, counts, W, H)


def test_chain_through_all_pairs():
    nxt, tid, rows, n = run([[(1, 1, 2, 2)], [(2, 2, 3, 3)], [(3, 3, 4, 4)]])
    assert nxt == [[0], [0], [-1]] and tid == [[0], [0], [0]] and rows == [(0, 0, 3, 0)] and n == 1


def test_chain_that_starts_late_and_one_that_ends_early():
    pairs = [[(1, 1, 2, 2), (9, 9, 8, 8)],             # record 1 finds nobody at (8, 8): ends early
             [(5, 5, 6, 6), (2, 2, 3, 3)],             # record 0 has no predecessor: starts late
             [(3, 3, 4, 4), (6, 6, 7, 7)]]
    nxt, tid, rows, n = run(pairs)
    assert nxt == [[1, -1], [1, 0], [-1, -1]]
    assert rows == [(0, 0, 3, 0), (0, 1, 1, 1), (1, 0, 2, 1)] and n == 3
    assert tid == [[0, 1], [2, 0], [0, 2]]
    rec, _ = corr_array(pairs)
    assert track_points(rec, nxt, rows) == [(0, [(1, 1), (2, 2), (3, 3), (4, 4)]), (0, [(9, 9), (8, 8)]),
                                            (1, [(5, 5), (6, 6), (7, 7)])]


def test_empty_middle_pair():
    nxt, tid, rows, n = run([[(1, 1, 2, 2)], [], [(2, 2, 3, 3)]])
    assert nxt == [[-1], [], [-1]] and tid == [[0], [], [1]] and rows == [(0, 0, 1, 0), (2, 0, 1, 0)] and n == 2


def test_duplicate_sources_in_the_next_pair():
    """two records of pair 1 start at (2, 2): the lower one is the candidate, the other is a head"""
    nxt, tid, rows, n = run([[(1, 1, 2, 2)], [(7, 7, 0, 0), (2, 2, 5, 5), (2, 2, 6, 6)]])
    assert nxt == [[1], [-1, -1, -1]] and tid == [[0], [1, 0, 2]]
    assert rows == [(0, 0, 2, 1), (1, 0, 1, 0), (1, 2, 1, 2)] and n == 3


def test_two_records_sharing_a_target():
    """records 0 and 2 of pair 0 both end at (4, 4): the lower one is continued, the other's track ends"""
    nxt, tid, rows, n = run([[(1, 1, 4, 4), (8, 8, 9, 9), (2, 2, 4, 4)], [(4, 4, 5, 5)]])
    assert nxt == [[0, -1, -1], [-1]] and tid == [[0, 1, 2], [0]]
    assert rows == [(0, 0, 2, 0), (0, 1, 1, 1), (0, 2, 1, 2)] and n == 3


def test_out_of_image_coordinates_never_link():
    pairs = [[(1, 1, 2, 2), (3, 3, W, 5), (-1, 4, 6, 6)],      # target outside; source outside
             [(2, 2, 3, -1), (W, 5, 7, 7), (6, 6, 8, 8), (2, 2, 9, 9)]]
    nxt, tid, rows, n = run(pairs)
    # pair 1's record 0 has its target outside, so it takes no part: (2, 2) is continued by record 3
    assert nxt == [[3, -1, -1], [-1, -1, -1, -1]]
    assert rows == [(0, 0, 2, 3), (0, 1, 1, 1), (0, 2, 1, 2), (1, 0, 1, 0), (1, 1, 1, 1), (1, 2, 1, 2)] and n == 6
    assert tid == [[0, 1, 2], [3, 4, 5, 0]]


def test_one_pair():
    nxt, tid, rows, n = run([[(1, 1, 2, 2), (2, 2, 3, 3)]])
    assert nxt == [[-1, -1]] and tid == [[0, 1]] and rows == [(0, 0, 1, 0), (0, 1, 1, 1)] and n == 2


def test_counts_beyond_cap_and_untouched_entries():
    """cap 1: only record 0 of each pair exists; expected_arrays leaves the fill value beyond it and beyond track_cap"""
    rec, counts = corr_array([[(1, 1, 2, 2), (5, 5, 6, 6)], [(2, 2, 3, 3), (6, 6, 7, 7)]], cap=1)
    assert list(counts) == [2, 2]
    a, b, tab, n = expected_arrays(rec, counts, W, H, -7, 4)
    assert a.tolist() == [[0], [-1]] and b.tolist() == [[0], [0]] and n == 1
    assert tab[0].tolist() == (0, 0, 2, 0) and tab[1].tolist() == (-7, -7, -7, -7)
    rec, counts = corr_array([[(1, 1, 2, 2)], [(2, 2, 3, 3), (6, 6, 7, 7)]])
    counts[1] = 1
    a, b, tab, n = expected_arrays(rec, counts, W, H, -7, 0)
    assert a.tolist() == [[0, -7], [-1, -7]] and b.tolist() == [[0, -7], [0, -7]] and n == 1 and len(tab) == 0


def test_entry_points_are_exported_and_declared():
    import ctypes as C
    import opengpc_amd as g
    import opengpc_amd.capi as capi
    L = g.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpc_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    for m in ("track_sequence", "track_sequence_device", "track_records", "track_records_device"):
        assert hasattr(g.Context, m), m
    assert g.TRACK_DTYPE.itemsize == 16 and g.TRACK_DTYPE.names == ("first_pair", "first_record", "length", "last_record")
    names = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_count())]
    for k in ("k_track_fill", "k_track_scatter", "k_track_link", "k_track_settle", "k_track_scan", "k_track_walk"):
        assert k in names, k
    # without a context every form refuses before it touches anything
    s = g.Settings.sparsematch()
    buf = np.zeros(16, g.CORR_DTYPE)
    i32 = np.zeros(16, np.int32)
    p = lambda a: a.ctypes.data
    for fn in (L.gpc_hip_track_records, L.gpc_hip_track_records_device):
        assert fn(None, p(buf), 4, p(i32), 96, 64, 2, p(i32), p(i32), p(buf), 4, p(i32)) == capi.E_INVALID
    img = np.zeros(3 * 64 * 96, np.uint8)
    for fn in (L.gpc_hip_track_sequence, L.gpc_hip_track_sequence_device):
        assert fn(None, p(img), 96, 64, 3, C.byref(s), p(buf), 4, p(i32), None, p(i32), p(i32), p(buf), 4, p(i32)) == capi.E_INVALID


def test_track_kernels_use_no_scratch():
    """the six k_track_* kernels: no scratch, no VGPR spills (gfx950 cross-compile, tools/kres.sh)"""
    env = dict(os.environ, KRES_OUT=os.path.join(ROOT, "tests", "cpp", "bin", "libgpc_kres_track.so"))
    os.makedirs(os.path.dirname(env["KRES_OUT"]), exist_ok=True)
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), r"k_track_"], capture_output=True, text=True,
                         env=env, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"^(gpc::\S+)\s+sgpr\s+\d+\s+vgpr\s+(\d+)\s+spill s\s+\d+\s+v\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line)
        if m:
            rows[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    assert sorted(rows) == ["gpc::k_track_fill", "gpc::k_track_link", "gpc::k_track_scan", "gpc::k_track_scatter",
                            "gpc::k_track_settle", "gpc::k_track_walk"], out
    for name, (vgpr, vspill, scratch, occ) in rows.items():
        assert vspill == 0 and scratch == 0, (name, rows[name])


def test_cpp_track_assembly():
    """tests/cpp/track_check.cpp: gpc::tracking::assemble on hand-made records and links, without a GPU; and
    tests/cpp/track_gpu_check.cpp (Forest::trackSequence, trackRecords) compiles."""
    cmd = lambda name: ["g++", "-std=c++17", "-O1", "-Wall", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", os.path.join(ROOT, "tests", "cpp", "bin", name),
                        "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"),
                        "-pthread"]
    os.makedirs(os.path.join(ROOT, "tests", "cpp", "bin"), exist_ok=True)
    subprocess.check_call(cmd("track_check"))
    res = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "track_check")], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.returncode, res.stdout, res.stderr)
    subprocess.check_call(cmd("track_gpu_check"))
