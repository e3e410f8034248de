"""CPU (hipcc cross-compiles without a GPU): the completion kernels (k_inpaint_*, opengpc_amd/csrc/k_inpaint.h) use no scratch
memory and spill no vector register, by the compiler's own resource report (tools/kres.sh), as
tests/test_clean_resources.py holds for the cleaning kernels."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^(gpc::\S.*?)\s+sgpr\s+(\d+)\s+vgpr\s+(\d+)\s+spill s\s+(\d+)\s+v\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)\s+lds\s+(\d+)")
KERNELS = ["k_inpaint_%s<%d>" % (k, c) for k in ("begin", "pass") for c in (1, 2)]


@pytest.fixture(scope="module")
def kres(tmp_path_factory):
    out = tmp_path_factory.mktemp("kres") / "libgpc_kres.so"
    env = dict(os.environ, KRES_OUT=str(out))
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), "k_inpaint_"], env=env, check=True, capture_output=True,
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
    # the staged tile of C = 2 at the largest radius: values, guide and flags, the hole list -- about 25 KiB, six workgroups a CU
    assert kres["gpc::k_inpaint_pass<2>"]["lds"] <= 26 * 1024
