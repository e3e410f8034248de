"""CPU (hipcc cross-compiles without a GPU): the refinement kernels (k_refine<CORR, R>, opengpc_amd/csrc/k_refine.h) use no
scratch memory and spill no vector register in any instantiation, by the compiler's own resource report (tools/kres.sh), as
tests/test_consensus_resources.py holds for the consensus kernels."""
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
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), "k_refine"], env=env, check=True, capture_output=True,
                         text=True, timeout=900).stdout
    rows = {}
    for line in txt.splitlines():
        m = LINE.match(line)
        if m:
            rows[m.group(1).strip()] = dict(zip(("sgpr", "vgpr", "sspill", "vspill", "scratch", "occ", "lds"), map(int, m.groups()[1:])))
    return rows


def test_no_scratch_and_no_vgpr_spills(kres):
    for corr in ("false", "true"):
        for r in range(1, 7):
            assert any("k_refine<%s, %d>" % (corr, r) in name for name in kres), (corr, r, sorted(kres))
    assert len(kres) == 12       # both record types, radius 1 .. 6
    for name, r in kres.items():
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["lds"] == 0, (name, r)


def test_the_common_radii_keep_eight_waves_per_simd(kres):
    """radius 1 .. 3 fit 64 vector registers; the largest window (radius 6, correspondences: 13 source rows held while 15
    target rows pass) still leaves three waves per SIMD"""
    for name, r in kres.items():
        radius = int(name.split(",")[1].strip(" >"))
        assert r["occ"] >= (8 if radius <= 3 else 3), (name, r)
