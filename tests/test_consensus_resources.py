"""CPU (hipcc cross-compiles without a GPU): the consensus kernels (k_cons_*, opengpc_amd/csrc/k_consensus.h) use no scratch
memory and spill no vector register, by the compiler's own resource report (tools/kres.sh), as tests/test_kernel_resources.py
holds for the matching kernels."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^(gpc::\S.*?)\s+sgpr\s+(\d+)\s+vgpr\s+(\d+)\s+spill s\s+(\d+)\s+v\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)\s+lds\s+(\d+)")


@pytest.fixture(scope="module")
def kres(tmp_path_factory):
    out = tmp_path_factory.mktemp("kres") / "libgpc_kres.so"
    env = dict(os.environ, KRES_OUT=str(out))
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), "k_cons_"], env=env, check=True, capture_output=True,
                         text=True, timeout=900).stdout
    rows = {}
    for line in txt.splitlines():
        m = LINE.match(line)
        if m:
            rows[m.group(1).strip()] = dict(zip(("sgpr", "vgpr", "sspill", "vspill", "scratch", "occ", "lds"), map(int, m.groups()[1:])))
    return rows


def test_no_scratch_and_no_vgpr_spills(kres):
    for kernel in ("k_cons_cells<", "k_cons_scan<", "k_cons_scatter<", "k_cons_count", "k_cons_blocks", "k_cons_write<"):
        assert any(kernel in name for name in kres), (kernel, sorted(kres))
    assert len(kres) >= 10       # both record types of the three typed kernels, both forms of the scan
    for name, r in kres.items():
        assert r["scratch"] == 0 and r["vspill"] == 0, (name, r)


def test_the_class_table_leaves_room_for_eight_waves_per_simd(kres):
    """16 KiB of LDS per workgroup of k_cons_count: more workgroups fit a CU (160 KiB) than its wave slots take"""
    r = kres["gpc::k_cons_count"]
    assert r["lds"] <= 17 * 1024 and r["occ"] == 8, r
