"""C++ training API (include/gpc/{Feature,Fern,training}.hpp): host-only pieces on CPU, the scoring
through the C ABI on the GPU, checked against the oracle with the hyperplanes the run actually drew.
Parity unpinned for this row (see tests/test_training.py)."""
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import SPLIT_DTYPE
from test_host_api import BIN, ROOT, compile_cpp, linked_libs, run
from test_training import make_triplets, stats_equal

# the reference's own samples/train.cpp, compiled by build() (oracle/Makefile, target `ref`)
REF_TRAIN_ON_AMD = os.path.join(ROOT, "oracle", "_ref", "ref_train_on_amd_headers")


@pytest.fixture(scope="module")
def train_bin():
    from opengpc_amd import build
    build.build()
    return compile_cpp(os.path.join(ROOT, "tests", "cpp", "train_api_check.cpp"), os.path.join(BIN, "train_api_check"))


def test_sample_hyperplane_stays_in_its_window(train_bin):
    """Feature::sampleHyperplane (Feature.hpp:131-176): i != j, offsets inside the 7x7 / 17x17 / 27x27
    centre, i = (ix+13) + 27*(iy+13) at every scale, tau in [-15, 15]."""
    for scale, half in ((2, 3), (1, 8), (0, 13)):
        out = run(train_bin, "sample", str(scale), "300", "42")
        rows = [list(map(int, l.split()[1:])) for l in out.splitlines() if l.startswith("HP")]
        assert len(rows) == 300
        for i, j, ix, iy, jx, jy, tau in rows:
            assert i != j and max(abs(ix), abs(iy), abs(jx), abs(jy)) <= half and -15 <= tau <= 15
            assert i == (ix + 13) + 27 * (iy + 13) and j == (jx + 13) + 27 * (jy + 13)
        assert run(train_bin, "sample", str(scale), "300", "42") == out  # seeded -> reproducible


def test_patch_extraction_and_file_round_trip(train_bin, tmp_path):
    out = run(train_bin, "patch", str(tmp_path / "t.bin"))
    # patch(0,0) = pixel(20-13, 18-13); feature(1) = patch(0,1) = pixel(7, 6); feature(27) = patch(1,0) = pixel(8, 5)
    px = lambda x, y: (7 * x + 13 * y) & 255
    assert "PATCH %d %d %d" % (px(7, 5), px(7, 6), px(8, 5)) in out
    assert "ROUNDTRIP 1 1" in out
    assert os.path.getsize(str(tmp_path / "t.bin")) == 3 * 729


@pytest.mark.skipif(not os.path.exists(REF_TRAIN_ON_AMD), reason="oracle/_ref not built (no reference tree)")
def test_reference_train_sample_compiles_against_these_headers():
    """The reference's own samples/train.cpp, compiled where it lies against include/gpc/training.hpp."""
    assert os.access(REF_TRAIN_ON_AMD, os.X_OK)
    assert "libgpc_hip.so" in linked_libs(REF_TRAIN_ON_AMD)


@pytest.mark.gpu
@pytest.mark.parametrize("only,taulo,tauhi,scale", [(1, 0, 1, 0), (0, -3, 3, 1), (1, -2, 2, 2)])
def test_cpp_fern_api_matches_oracle(train_bin, tmp_path, oracle, only, taulo, tauhi, scale):
    n, depth, nres, w1, seed = 3000, 4, 6, 0.5, 11
    t = make_triplets(n, 77)
    path = str(tmp_path / "triplets.bin")
    t.tofile(path)
    dump = str(tmp_path / "cand.txt")
    env = dict(os.environ, GPC_TRAIN_DUMP_CANDIDATES=dump)
    out = subprocess.run([train_bin, "api", path, str(seed), str(depth), str(nres), str(taulo), str(tauhi), str(only),
                          str(w1), str(scale)], check=True, capture_output=True, text=True, env=env).stdout
    lines = {l.split()[0]: l.split()[1:] for l in out.splitlines() if l and l.split()[0] in ("EVAL", "MARKS", "PARAMS", "MARKS2")}
    # evalSplit / markSplitSamples on the fixed parameter list
    params = np.zeros(3, SPLIT_DTYPE)
    params["i"], params["j"], params["tau"] = [5, 364, 700], [33, 365, 2], [0, 2, -3]
    marks = np.array([(1 if k % 3 == 0 else 0) | (2 if k % 5 == 0 else 0) for k in range(n)], np.uint8)
    s = oracle.eval_split(t, marks, params, 2, w1)
    ev = lines["EVAL"]
    assert [int(v) for v in ev[:4]] == [s["tp"], s["fp"], s["fn"], s["tot"]]
    assert [float(v) for v in ev[4:]] == [s["prec"], s["rec"], s["hmean"], s["convcomb"]]
    oracle.mark_split_samples(t, marks, params, 2)
    assert np.array_equal(np.array(lines["MARKS"], np.uint8), marks)
    # train(): the oracle with the hyperplanes this run drew
    ij = np.loadtxt(dump, dtype=np.int32).reshape(-1, 2)
    assert len(ij) == depth * nres
    cand = np.zeros(len(ij), SPLIT_DTYPE)
    cand["i"], cand["j"] = ij[:, 0], ij[:, 1]
    fp, st = oracle.train_fern(t, marks, depth, cand, nres, taulo, tauhi, bool(only), w1)
    got = np.array(lines["PARAMS"], np.int32).reshape(depth, 7)
    assert np.array_equal(got[:, 0], fp["i"]) and np.array_equal(got[:, 1], fp["j"]) and np.array_equal(got[:, 2], fp["tau"])
    assert np.array_equal(got[:, 3], fp["i"] % 27 - 13) and np.array_equal(got[:, 4], fp["i"] // 27 - 13)
    assert np.array_equal(np.array(lines["MARKS2"], np.uint8), marks)
    # the table train() prints carries the oracle's per-level statistics
    table = [l.split() for l in out.splitlines() if l.split() and l.split()[0].isdigit() and len(l.split()) == 12]
    assert len(table) == depth
    for level, row in enumerate(table):
        assert [int(row[4]), int(row[5]), int(row[6]), int(row[7])] == [st[level]["tot"], st[level]["tp"], st[level]["fp"], st[level]["fn"]]


@pytest.mark.gpu
def test_cpp_forest_train_and_export(train_bin, tmp_path, oracle):
    """Forest::trainAndExport writes a forest the inference side reads back (Forest::readForest)."""
    t = make_triplets(2000, 5)
    path, fpath = str(tmp_path / "triplets.bin"), str(tmp_path / "forest.txt")
    t.tofile(path)
    out = run(train_bin, "forest", path, fpath)
    assert "Fern(3/3) num samples:1400" in out and "Exporting forest" in out
    assert "ERR: No extracted training set found at given path" in out and "MISSING 0" in out
    rc, f = oracle.read_forest(fpath, 1024, 436)
    assert rc == 0 and f.num_tests == 9 and f.type == 0
    text = open(fpath).read().split()
    assert text[0] == "3" and text[1:4] == ["0", "s", "3"]
