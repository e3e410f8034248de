"""CPU: the host-only legs of bench.py -- the cpu_baseline object of the contract and the core count it
reports, the options of a plain run.  GPU: a plain run's line and what --dump-outputs writes."""
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_cpu_baseline_object(forest_paths):
    import bench
    assert 1 <= bench.host_cores() <= 16
    args = types.SimpleNamespace(forest=forest_paths["zero"], cpu_seconds=1.0)
    cb = bench.cpu_baseline(args, 256, 96)
    assert set(["value", "unit", "cores", "kind", "sample"]) <= set(cb)
    assert cb["unit"] == "Mpix/s" and cb["cores"] == 1 and cb["kind"] in ("port", "reference") and cb["value"] > 0
    if cb.get("all_cores"):
        assert cb["all_cores"]["cores"] == bench.host_cores() and cb["all_cores"]["value"] > 0


def test_default_workload_is_baseline_config():
    import bench
    old = sys.argv
    sys.argv = ["bench.py"]
    try:
        a = bench.parse_args()
    finally:
        sys.argv = old
    assert (a.gpus, a.width, a.height, a.batch) == (1, 1024, 436, 256)
    assert os.path.basename(a.forest) == "defaultZeroForest.txt" and a.steps > 0 and a.warmup >= 0


def test_plain_run_defaults_time_exactly_the_steps():
    """A plain run times ONE window of --steps steps; the side legs wait for --full; no dump unless asked."""
    import bench
    old = sys.argv
    sys.argv = ["bench.py", "--steps", "7"]
    try:
        a = bench.parse_args()
    finally:
        sys.argv = old
    assert a.steps == 7 and a.windows == 1 and a.full is False and a.dump_outputs is None


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(tmp_path, oracle, forest_paths):
    """A plain run prints the headline only, and --dump-outputs writes what its last step computed: float arrays whose
    sampled supports are the oracle's, bit for bit (x, y, d are exact in float32)."""
    import json
    import subprocess
    import numpy as np
    from oracle.pyoracle import sparsematch_settings
    from opengpc_amd.synth import synth_batch
    W, H, B = 256, 96, 16
    d = str(tmp_path / "out")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                          "--batch", str(B), "--width", str(W), "--height", str(H), "--dump-outputs", d],
                         check=True, capture_output=True, text=True, timeout=600).stdout
    line = json.loads(out.strip().splitlines()[-1])
    assert line["steps"] == 4 and line["windows"]["count"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Mpix/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["verified_vs_oracle"] is None
    got = {n: np.load(os.path.join(d, n + ".npy")) for n in
           ("counts", "candidates", "sample_pairs", "sample_offsets", "sample_supports")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["counts"].shape == (B,) and got["candidates"].shape == (B, 2)
    L, R = synth_batch(W, H, list(range(B)))
    rc, f = oracle.read_forest(forest_paths["zero"], W, H)
    offs = got["sample_offsets"].astype(np.int64)
    pairs = got["sample_pairs"].astype(np.int64)
    assert len(pairs) == min(B, 12) and len(offs) == len(pairs) + 1
    for k, j in enumerate(pairs):
        want, nl, nr = oracle.match_pair(L[j], R[j], f, sparsematch_settings())
        assert int(got["counts"][j]) == len(want) and tuple(got["candidates"][j]) == (nl, nr)
        sup = got["sample_supports"][offs[k]:offs[k + 1]]
        assert np.array_equal(sup[:, 0], want["x"]) and np.array_equal(sup[:, 1], want["y"])
        assert np.array_equal(sup[:, 2], want["d"])
