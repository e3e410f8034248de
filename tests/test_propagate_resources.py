"""CPU (hipcc cross-compiles without a GPU): every instantiation of the propagation kernel (k_propagate,
opengpc_amd/csrc/k_propagate.h) uses no scratch memory and spills no vector register, and its LDS is what DESIGN.md states,
by the compiler's own resource report (tools/kres.sh), as tests/test_search_resources.py holds for the search kernel."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^(gpc::\S.*?)\s+sgpr\s+(\d+)\s+vgpr\s+(\d+)\s+spill s\s+(\d+)\s+v\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)\s+lds\s+(\d+)")
KERNELS = ["k_propagate<%d, %d, %d>" % (c, r, nb) for c in (1, 2) for r in (1, 2, 3, 4) for nb in (4, 8)]
# the staged tile is that of k_search -- (8 + 2 * 4) rows of 44 bytes, whatever the radius -- plus the
# workgroup's four counts: 16 * 44 + 16 bytes
LDS_BYTES = 16 * 44 + 16


@pytest.fixture(scope="module")
def kres(tmp_path_factory):
    out = tmp_path_factory.mktemp("kres") / "libgpc_kres.so"
    env = dict(os.environ, KRES_OUT=str(out))
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), "k_propagate<"], env=env, check=True, capture_output=True,
                         text=True, timeout=900).stdout
    rows = {}
    for line in txt.splitlines():
        m = LINE.match(line)
        if m:
            rows[m.group(1).strip()] = dict(zip(("sgpr", "vgpr", "sspill", "vspill", "scratch", "occ", "lds"), map(int, m.groups()[1:])))
    return rows


def test_no_scratch_no_vgpr_spills_and_the_stated_lds(kres):
    assert sorted(kres) == sorted("gpc::" + k for k in KERNELS), sorted(kres)
    for name, r in kres.items():
        assert r["scratch"] == 0 and r["vspill"] == 0, (name, r)
        assert r["lds"] <= LDS_BYTES == 720, (name, r)
