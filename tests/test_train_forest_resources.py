"""CPU (hipcc cross-compiles without a GPU): the forest-training kernels (k_tf_*, opengpc_amd/csrc/k_train_forest.h) use no
scratch memory and spill no vector register, by the compiler's own resource report (tools/kres.sh), as
tests/test_refine_resources.py holds for the refinement kernels; their timing slots stand behind the existing ones; the
new entry point is declared, exported and bound."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^(gpc::\S.*?)\s+sgpr\s+(\d+)\s+vgpr\s+(\d+)\s+spill s\s+(\d+)\s+v\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)\s+lds\s+(\d+)")
KERNELS = ("k_tf_begin", "k_tf_eval", "k_tf_tot", "k_tf_commit")


@pytest.fixture(scope="module")
def kres(tmp_path_factory):
    out = tmp_path_factory.mktemp("kres") / "libgpc_kres.so"
    env = dict(os.environ, KRES_OUT=str(out))
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), "k_tf_"], env=env, check=True, capture_output=True,
                         text=True, timeout=900).stdout
    rows = {}
    for line in txt.splitlines():
        m = LINE.match(line)
        if m:
            rows[m.group(1).strip()] = dict(zip(("sgpr", "vgpr", "sspill", "vspill", "scratch", "occ", "lds"), map(int, m.groups()[1:])))
    return rows


def test_no_scratch_and_no_vgpr_spills(kres):
    assert sorted(kres) == sorted("gpc::" + k for k in KERNELS), sorted(kres)
    for name, r in kres.items():
        assert r["scratch"] == 0 and r["vspill"] == 0, (name, r)


def test_the_evaluation_keeps_eight_waves_per_simd(kres):
    """the weighted evaluation streams bytes like k_ts_eval_level: at most 64 vector registers, and only the two
    64-entry difference arrays in LDS"""
    r = kres["gpc::k_tf_eval"]
    assert r["occ"] == 8 and r["vgpr"] <= 64 and r["lds"] == 2 * 64 * 4, r


def test_abi_and_timing_slots():
    import ctypes as C
    from opengpc_amd import build
    build.build()
    import opengpc_amd as g
    L = g.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpc_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+gpc_hip_train_forest\s*\(([^)]*)\)", header).group(1)
    assert "gpc_hip_train_forest" in g.capi.SYMBOLS and hasattr(L, "gpc_hip_train_forest")
    assert len(decl.split(",")) == 14 == len(L.gpc_hip_train_forest.argtypes)
    assert callable(g.capi.TrainSet.train_forest)
    kernels = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_slots())]
    assert len(set(kernels)) == len(kernels) and "" not in kernels
    at = kernels.index("k_dense_push")
    assert tuple(kernels[at + 1:at + 1 + len(KERNELS)]) == KERNELS and at >= L.gpc_hip_kernel_count() == 32
    assert kernels.index("k_train_eval") < 32
    # without a context the call refuses before it touches anything
    assert L.gpc_hip_train_forest(None, None, 1, 1, None, 1, 0, 1, 0, C.c_double(0.5), None, 0, None, None) == g.capi.E_INVALID
