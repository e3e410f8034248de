"""Group mode, host side: gpc_hip_read_forest_groups / gpc_hip_parse_forest_groups against the oracle's readForest of
each group's own text, the packing rule, refusals, the C++ API and the new kernels' resources.  No GPU needed."""
import os
import re
import subprocess

import pytest

from forest_groups_util import PLANE_FIRST, TAU_RULES, TAU_VALUES, fern_split, forest_text, group_texts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORESTS = {k: os.path.join(ROOT, "forests", f) for k, f in
           (("zero", "defaultZeroForest.txt"), ("tau", "defaultTauForest.txt"), ("stress", "stress16x20Forest.txt"))}


def _same_as_oracle(oracle, group, text, W, H):
    rc, f = oracle.parse_forest_text(text, W, H)
    assert rc == 0
    n = f.num_tests
    assert group.num_tests == n and group.type == f.type and group.discarded == 0
    assert (group.width, group.height) == (W, H)
    assert list(group.mask[:2 * n]) == list(f.offs[:2 * n])
    assert list(group.tau[:n]) == list(f.tau[:n])


@pytest.mark.parametrize("name", ["zero", "tau", "stress"])
@pytest.mark.parametrize("W,H", [(96, 64), (1024, 436), (3840, 2160)])
def test_groups_of_committed_forests(oracle, name, W, H):
    import opengpc_amd as g
    st, groups = g.read_forest_groups(FORESTS[name], W, H)
    assert st == 0
    texts = group_texts(open(FORESTS[name]).read())
    assert len(groups) == len(texts) == (16 if name == "stress" else 1)
    for grp, text in zip(groups, texts):
        _same_as_oracle(oracle, grp, text, W, H)
    if name == "stress":
        assert [grp.num_tests for grp in groups] == [20] * 16
    else:  # one group of 30 tests: today's mask
        st1, fm = g.read_forest(FORESTS[name], W, H)
        assert st1 == 0 and groups[0].num_tests == fm.num_tests == 30 and groups[0].type == fm.type
        assert list(groups[0].mask) == list(fm.mask) and list(groups[0].tau) == list(fm.tau)


@pytest.mark.parametrize("sizes,want", [
    ([10, 10, 10, 10], [30, 10]),
    ([40], [32, 8]),
    ([5, 32], [5, 32]),
    ([20, 12], [32]),
    ([3, 70, 4], [3, 32, 32, 6, 4]),
    ([0, 7, 0, 25], [32]),
    ([32, 32], [32, 32]),
    ([32, 5, 1, 20, 7, 9], [32, 26, 16]),   # the unequal groups of test_gpu_forest_shapes.py
    ([40, 3], [32, 8, 3]),
])
def test_packing_rule(oracle, sizes, want):
    import opengpc_amd as g
    text = forest_text(sizes, seed=len(sizes))
    st, groups = g.parse_forest_groups(text, 640, 480)
    assert st == 0 and [grp.num_tests for grp in groups] == want
    texts = group_texts(text)
    assert len(texts) == len(groups)
    for grp, t in zip(groups, texts):
        _same_as_oracle(oracle, grp, t, 640, 480)


def test_type_is_per_group():
    import opengpc_amd as g
    text = forest_text([20], seed=1, tau=False).rstrip("\n").split("\n")
    tau = forest_text([20], seed=2, tau=True).split("\n")[2:]
    body = "2\n" + "\n".join(text[1:]) + "\n1 l 20\n" + "\n".join(tau)
    st, groups = g.parse_forest_groups(body, 96, 64)
    assert st == 0 and [grp.type for grp in groups] == [0, 1]


def test_refusals_and_io_errors():
    import ctypes as C
    import opengpc_amd as g
    L = g.load()
    st, groups = g.parse_forest_groups(forest_text([20] * 33), 96, 64)
    assert st == g.capi.E_UNSUPPORTED and groups == []
    st, groups = g.parse_forest_groups(forest_text([20] * 32), 96, 64)
    assert st == 0 and len(groups) == 32
    for bad in ("", "garbage", "2\n0 l 3\n0 1 2 3 4 0\n", "1\n0 l 2\n0 1 2 3 4 0\n1 1 2 3"):
        st_ref, _ = g.parse_forest(bad, 96, 64)
        st, groups = g.parse_forest_groups(bad, 96, 64)
        assert st == st_ref == g.capi.E_IO and groups == []
    st, groups = g.read_forest_groups("/nonexistent.txt", 96, 64)
    assert st == g.capi.E_IO and groups == []
    # a short array: the true count and the first `cap` groups
    arr = (g.FilterMask * 3)()
    n = C.c_int()
    st = L.gpc_hip_parse_forest_groups(forest_text([20] * 5).encode(), 96, 64, arr, 3, C.byref(n))
    assert st == g.capi.E_CAPACITY and n.value == 5 and arr[2].num_tests == 20
    assert L.gpc_hip_set_forest_groups(None, arr, 2) == g.capi.E_INVALID
    assert L.gpc_hip_hash_codes_groups(None, None, None, 96, 64, None) == g.capi.E_INVALID


def test_cpp_api_compiles():
    """tests/cpp/forest_groups_check.cpp uses Forest::readForestGroups and the group overloads."""
    out = os.path.join(ROOT, "tests", "cpp", "bin", "forest_groups_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "forest_groups_check.cpp"), "-o", out,
                           "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-pthread"])
    assert os.path.exists(out)


def test_new_kernels_use_no_scratch():
    """k_hash_groups and the k_group_union kernels: no scratch, no VGPR spills (gfx950 cross-compile)."""
    env = dict(os.environ, KRES_OUT=os.path.join(ROOT, "tests", "cpp", "bin", "libgpc_kres_groups.so"))
    os.makedirs(os.path.dirname(env["KRES_OUT"]), exist_ok=True)
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), "k_hash_groups|k_group_union"],
                         capture_output=True, text=True, env=env, check=True).stdout
    rows = [l for l in out.splitlines() if "gpc::" in l]
    assert len([r for r in rows if "k_hash_groups" in r]) == 12 and len([r for r in rows if "k_group_union" in r]) == 7
    for r in rows:
        m = re.search(r"spill s +\d+ v +(\d+) +scratch +(\d+)", r)
        assert m and m.group(1) == "0" and m.group(2) == "0", r


def test_forest_text_rules():
    """forest_text as test_gpu_forest_shapes.py uses it: where the rules put the zeros, the values, the ferns' scales, the split
    and -128 on the last test that is kept"""
    for T in (1, 9, 26, 33):
        for rule in TAU_RULES:
            tok = forest_text(fern_split(T, "each"), seed=T, tau=rule, scales="sml").split()
            taus = [int(tok[1 + 9 * i + 8]) for i in range(T)]
            zero = {"zero": lambda s: True, "nonzero": lambda s: False, "plane_first": lambda s: s not in PLANE_FIRST,
                    "plane_rest": lambda s: s in PLANE_FIRST, "alternating": lambda s: s % 2 == 1}[rule]
            assert all((t == 0) == zero(s) and (t == 0 or t in TAU_VALUES) for s, t in enumerate(taus)), (T, rule)
            assert [tok[1 + 9 * i + 1] for i in range(T)] == ["sml"[i % 3] for i in range(T)]
    assert fern_split(9, 1) == [9] and fern_split(9, 2) == [5, 4] and fern_split(3, "each") == [1, 1, 1]
    # the texts the generator gave before it knew rules and scales, literally
    assert forest_text([2, 1], seed=2) == "2\n0 l 2\n0 9 -6 -11 -5 -4\n1 8 -1 -11 -4 4\n1 l 1\n0 8 6 13 -8 16\n"
    assert forest_text([2], seed=3, tau=False) == "1\n0 l 2\n0 8 -11 -9 -7 0\n1 -9 8 10 2 0\n"
    assert forest_text([20, 20], tau="alternating", m128_last=True).split("\n")[1 + 1 + 20 + 12].split()[-1] == "-128"
