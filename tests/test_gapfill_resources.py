"""CPU (hipcc cross-compiles without a GPU): every kernel of the scanline hole closing (opengpc_amd/csrc/k_gapfill.h) uses no
scratch memory and spills no vector register, and its LDS is what DESIGN.md states, by the compiler's own resource report
(tools/kres.sh), as tests/test_propagate_resources.py holds for the propagation kernel."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^(gpc::\S.*?)\s+sgpr\s+(\d+)\s+vgpr\s+(\d+)\s+spill s\s+(\d+)\s+v\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)\s+lds\s+(\d+)")
CHOOSE = ["k_gapfill_choose<%d, %d>" % (c, s) for c in (1, 2) for s in (0, 1)]
# the scans use no LDS; the choice holds the workgroup's four counts
LDS_BYTES = {"k_gapfill_rows": 0, "k_gapfill_cols": 0, **{k: 16 for k in CHOOSE}}


@pytest.fixture(scope="module")
def kres(tmp_path_factory):
    out = tmp_path_factory.mktemp("kres") / "libgpc_kres.so"
    env = dict(os.environ, KRES_OUT=str(out))
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), "k_gapfill_"], env=env, check=True, capture_output=True,
                         text=True, timeout=900).stdout
    rows = {}
    for line in txt.splitlines():
        m = LINE.match(line)
        if m:
            rows[m.group(1).strip()] = dict(zip(("sgpr", "vgpr", "sspill", "vspill", "scratch", "occ", "lds"), map(int, m.groups()[1:])))
    return rows


def test_no_scratch_no_vgpr_spills_and_the_stated_lds(kres):
    assert sorted(kres) == sorted("gpc::" + k for k in LDS_BYTES), sorted(kres)
    for name, r in kres.items():
        assert r["scratch"] == 0 and r["vspill"] == 0, (name, r)
        assert r["lds"] == LDS_BYTES[name[len("gpc::"):]], (name, r)
