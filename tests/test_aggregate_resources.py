"""CPU (hipcc cross-compiles without a GPU): every instantiation of the aggregation's kernels (opengpc_amd/csrc/k_aggregate.h)
uses no scratch memory and spills no vector register, and its LDS is what DESIGN.md 4.20 states, by the compiler's own
resource report (tools/kres.sh), as tests/test_search_resources.py holds for the search kernel."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^(gpc::\S.*?)\s+sgpr\s+(\d+)\s+vgpr\s+(\d+)\s+spill s\s+(\d+)\s+v\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)\s+lds\s+(\d+)")
CG = [(c, g) for c in (1, 2) for g in (0, 1, 2)]


def labels(c, g):
    return (2 * g + 1) ** c


def cells(c, g):
    return (2 * g + 3) ** c


def chunk(k):
    return 8 if k > 9 else 16 if k > 5 else 32


# DESIGN.md 4.20.  k_agg_cost: k_search's staged tile, 16 rows of 44 bytes.  k_agg_path_v: the gather slots, one dword per cell
# and lane.  k_agg_path_h: the slots, the staged chunk (labels x 64 rows x (chunk + 2) halfwords) and its bases (channels x 64
# rows x (chunk + 1) dwords).  k_agg_choose: the workgroup's four counts.
LDS = {"k_agg_cost<%d, %d, %d>" % (c, r, g): 16 * 44 for c, g in CG for r in (1, 2, 3, 4)}
LDS.update({"k_agg_path_v<%d, %d>" % (c, g): 256 * cells(c, g) for c, g in CG})
LDS.update({"k_agg_path_h<%d, %d>" % (c, g): 256 * cells(c, g) + labels(c, g) * 64 * (chunk(labels(c, g)) + 2) * 2 +
            c * 64 * (chunk(labels(c, g)) + 1) * 4 for c, g in CG})
LDS.update({"k_agg_choose<%d, %d>" % (c, g): 16 for c, g in CG})


@pytest.fixture(scope="module")
def kres(tmp_path_factory):
    out = tmp_path_factory.mktemp("kres") / "libgpc_kres.so"
    env = dict(os.environ, KRES_OUT=str(out))
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), "k_agg_"], env=env, check=True, capture_output=True,
                         text=True, timeout=900).stdout
    rows = {}
    for line in txt.splitlines():
        m = LINE.match(line)
        if m:
            rows[m.group(1).strip()] = dict(zip(("sgpr", "vgpr", "sspill", "vspill", "scratch", "occ", "lds"), map(int, m.groups()[1:])))
    return rows


def test_no_scratch_no_vgpr_spills_and_the_stated_lds(kres):
    assert sorted(kres) == sorted("gpc::" + k for k in LDS), sorted(kres)
    assert LDS["k_agg_path_h<2, 2>"] == 49152 and LDS["k_agg_path_h<2, 1>"] == 35840 and LDS["k_agg_path_v<2, 2>"] == 12544
    for name, r in kres.items():
        assert r["scratch"] == 0 and r["vspill"] == 0, (name, r)
        assert r["lds"] == LDS[name[len("gpc::"):]], (name, r)
