"""C++ host API (include/gpc/*.hpp): host-only logic on CPU, whole path on GPU through the
sparsematch sample -- including the reference's OWN samples/sparsematch.cpp compiled unchanged
against these headers (when the reference tree is present)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "bin")
LIBDIR = os.path.join(ROOT, "opengpc_amd")
# the reference's own samples/sparsematch.cpp, unchanged, compiled against include/gpc/*.hpp by build()
# (oracle/Makefile, target `ref`: where the reference tree is present; the binary travels with oracle/_ref)
REF_ON_AMD = os.path.join(ROOT, "oracle", "_ref", "ref_sparsematch_on_amd_headers")


def compile_cpp(src, out, sse=True, opt="-O1"):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # -D_INTRINSICS_SSE is the reference's default build option (samples/CMakeLists.txt:13-17)
    subprocess.check_call(["g++", "-std=c++17", opt] + (["-D_INTRINSICS_SSE"] if sse else []) +
                          ["-I" + os.path.join(ROOT, "include"), "-o", out, src,
                           "-L" + LIBDIR, "-lgpc_hip", "-lz", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.fixture(scope="module")
def check_bin():
    from opengpc_amd import build
    build.build()
    return compile_cpp(os.path.join(ROOT, "tests", "cpp", "host_api_check.cpp"), os.path.join(BIN, "host_api_check"))


def run(*args, cwd=None):
    return subprocess.run(list(args), check=True, capture_output=True, text=True, cwd=cwd).stdout


def test_settings_and_pods(check_bin):
    out = run(check_bin, "settings")
    assert "DEFAULT 10 128 1 0 0 1" in out          # inference.hpp:74-89
    assert "BUILT 5 64 0 1 0 1" in out              # numThreads clamps to hardware_concurrency
    assert "SIZES 24 12 16" in out                  # Descriptor / Support / Correspondence layouts
    assert "Error opening forest file" in out and "MISSING 0 0 96 64" in out


def test_failed_call_leaves_a_status_and_defined_outputs(check_bin, forest_paths):
    """The reference's API returns by value and has no error channel: a failed call returns an empty result, which is
    also what "no matches" looks like.  gpc::inference::lastStatus() / lastError() tell them apart, and matchPair's
    candidate counts are defined on every path out (a device index that does not exist: fails here and on a GPU box)."""
    env = dict(os.environ, GPC_HIP_DEVICE="9999")
    out = subprocess.run([check_bin, "nodevice", forest_paths["zero"]], check=True, capture_output=True, text=True, env=env).stdout
    assert "BEFORE 0 []" in out
    after = [l for l in out.splitlines() if l.startswith("AFTER")][0].split(" ", 5)
    assert after[1:4] == ["0", "0", "0"] and int(after[4]) != 0 and "gpc_hip_create failed" in after[5]
    assert "CLEARED 0 []" in out


def test_forest_reader_matches_oracle(check_bin, oracle, forest_paths):
    for name, path in forest_paths.items():
        out = run(check_bin, "forest", path, "1024", "436")
        assert "number of ferns:6" in out
        vals = out.split("FOREST")[1].split()
        rc, f = oracle.read_forest(path, 1024, 436)
        assert int(vals[0]) == 60 and int(vals[2]) == f.type
        assert int(vals[1]) == (30 if f.type else 0)    # tau stays empty for a zero forest
        assert [int(v) for v in vals[3:]] == list(f.offs[:60])


def test_png_read(check_bin, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    cases = {
        "gray": (rng.integers(0, 256, (37, 50), dtype=np.uint8), "L"),
        "rgb": (rng.integers(0, 256, (20, 64, 3), dtype=np.uint8), "RGB"),
        "rgba": (rng.integers(0, 256, (8, 16, 4), dtype=np.uint8), "RGBA"),
    }
    for name, (arr, mode) in cases.items():
        p = str(tmp_path / (name + ".png"))
        Image.fromarray(arr, mode).save(p)
        raw = str(tmp_path / (name + ".raw"))
        out = run(check_bin, "read", p, raw)
        rc, cols, rows, w, h = map(int, out.split("RESULT")[1].split())
        H, W = arr.shape[:2]
        assert (rows, w, h, cols) == (H, W, H, (W + 15) // 16 * 16)
        buf = np.fromfile(raw, np.uint8).reshape(rows, cols)
        if name == "rgba":
            assert rc == 1 and "other than gray or 3 channel" in out   # buffer.hpp:309-313
            continue
        assert rc == 0
        want = arr if name == "gray" else (arr.astype(np.int32).sum(2) // 3).astype(np.uint8)
        assert np.array_equal(buf[:, :W], want) and not buf[:, W:].any()
    out = run(check_bin, "read", str(tmp_path / "missing.png"), str(tmp_path / "x.raw"))
    assert "could not be opened for reading" in out and "RESULT 1" in out
    notpng = tmp_path / "not.png"
    notpng.write_bytes(b"hello world, not a png")
    out = run(check_bin, "read", str(notpng), str(tmp_path / "y.raw"))
    assert "is not recognized as a PNG file" in out and "RESULT 1" in out


def test_png_write_and_visualisation(check_bin, tmp_path):
    from PIL import Image
    p = str(tmp_path / "g.png")
    run(check_bin, "write_gray", "50", "21", p)
    g = np.array(Image.open(p))
    y, x = np.mgrid[0:21, 0:50]
    assert g.shape == (21, 50) and np.array_equal(g, ((x * 3 + y * 7) & 0xFF).astype(np.uint8))
    p = str(tmp_path / "c.png")
    run(check_bin, "write_rgb", "33", "9", p)
    c = np.array(Image.open(p))
    y, x = np.mgrid[0:9, 0:33]
    assert np.array_equal(c, np.stack([x & 0xFF, y & 0xFF, (x ^ y) & 0xFF], -1).astype(np.uint8))
    p = str(tmp_path / "v.png")
    run(check_bin, "vis", "64", "48", p)
    v = np.array(Image.open(p)).astype(np.int32)
    y, x = np.mgrid[0:48, 0:64]
    off = x != y
    assert np.all(v[off] == ((x + y) & 0xFF)[off][:, None])          # untouched pixels stay gray
    assert tuple(v[0, 0]) == (0, 0, 255) and v[40, 40, 0] > v[2, 2, 0]  # ramp starts blue, reddens


def kitti_ramp(d):
    """numpy float32 restatement of the colour ramp of ndb::getDisparityVisualization (reference
    lib/gpc/buffer.hpp:958-1010), operation by operation in float32 with no fused multiply-add (a reference
    binary built with -march=core-avx2 may contract `w * a + (1 - w) * b` and differ in a last bit; the
    restatement pins this repository's header to the source's unfused arithmetic).  d: float array -> uint8 [n][3]."""
    f = np.float32
    ramp = np.array([[0, 0, 1, 185], [1, 0, 0, 114], [1, 0, 1, 174], [0, 1, 0, 114], [0, 1, 1, 185], [1, 1, 0, 114],
                     [1, 1, 1, 0], [0, 0, 0, 114]], np.float32)
    total = f(0)
    for i in range(8):                       # :964-967
        total = f(total + ramp[i, 3])
    weights, cumsum = np.zeros(8, np.float32), np.zeros(8, np.float32)
    for i in range(7):                       # :972-975
        weights[i] = f(total / ramp[i, 3])
        cumsum[i + 1] = f(cumsum[i] + f(ramp[i, 3] / total))
    out = np.zeros((len(d), 3), np.uint8)
    for k, disp in enumerate(np.asarray(d, np.float32)):
        value = max(f(0), min(f(0.8), f(f(disp - f(0)) / f(f(128) - f(0)))))   # :985-988
        b = 7
        for j in range(7):                   # :991-995
            if value < cumsum[j + 1]:
                b = j
                break
        w = f(f(1) - f(f(value - cumsum[b]) * weights[b]))                      # :999
        for ch in range(3):                  # :1000-1008: float -> uint8 truncates
            out[k, ch] = int(f(f(f(w * ramp[b, ch]) + f(f(f(1) - w) * ramp[b + 1, ch])) * f(255)))
    return out


def test_disparity_colour_ramp_over_every_disparity(check_bin, tmp_path):
    """disparityColor (include/gpc/buffer.hpp) == the restatement for every half-integer disparity from -4 to 260:
    all 129 integer disparities the default dispHigh admits, the clamp at 0.8 (d >= 102.4) and negative values."""
    p = str(tmp_path / "ramp.raw")
    run(check_bin, "ramp", p)
    got = np.fromfile(p, np.uint8).reshape(-1, 3)
    d = 0.5 * np.arange(-8, 521, dtype=np.float32)
    assert len(got) == len(d) == 529
    want = kitti_ramp(d)
    assert np.array_equal(got, want), np.flatnonzero(np.any(got != want, axis=1))[:10]
    assert tuple(got[8]) == (0, 0, 255) and len({tuple(c) for c in got[8:8 + 2 * 129:2]}) > 90   # d = 0 is blue; the ramp moves


def test_clear_boundary(check_bin, tmp_path, oracle):
    raw = str(tmp_path / "cb.raw")
    out = run(check_bin, "clear", "48", "20", raw)
    buf = np.fromfile(raw, np.uint8).reshape(20, 48)
    want = np.full((20, 48), 255, np.uint8)
    oracle.clear_boundary(want)
    assert np.array_equal(buf, want)


def linked_libs(exe):
    out = subprocess.run(["readelf", "-d", exe], check=True, capture_output=True, text=True).stdout
    return re.findall(r"\(NEEDED\)\s+Shared library: \[([^]]+)\]", out)


@pytest.mark.skipif(not os.path.exists(REF_ON_AMD), reason="oracle/_ref not built (no reference tree)")
def test_reference_sample_compiles_unchanged_against_these_headers():
    """Drop-in at source level: the reference's samples/sparsematch.cpp, untouched, builds
    against include/gpc/*.hpp (at the reference's own -O3, samples/CMakeLists.txt:17) and links
    this library.  build() compiles it into oracle/_ref (derived from reference source)."""
    assert os.access(REF_ON_AMD, os.X_OK)
    assert "libgpc_hip.so" in linked_libs(REF_ON_AMD)


def write_pair(tmp_path, W, H, s, D):
    from PIL import Image
    from opengpc_amd.synth import synth_pair
    L, R = synth_pair(W, H, s, D)
    lp, rp = str(tmp_path / "left.png"), str(tmp_path / "right.png")
    Image.fromarray(L, "L").save(lp)
    Image.fromarray(np.stack([R, R, R], -1), "RGB").save(rp)   # RGB input takes the (r+g+b)/3 path
    return L, R, lp, rp


LINE = re.compile(r"#candidatesL:(\d+), #candidatesR:(\d+), tMatch: [\d.e+-]+ ms, num matches:(\d+)")


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
def test_sparsematch_sample(tmp_path, golden, forest_paths, fused):
    from PIL import Image
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "samples")])
    c = golden["cases"][1]
    L, R, lp, rp = write_pair(tmp_path, c["W"], c["H"], c["s"], c["D"])
    args = [os.path.join(ROOT, "samples", "sparsematch"), forest_paths["zero"], lp, rp] + (["--fused"] if fused else [])
    out = run(*args, cwd=str(tmp_path))
    m = LINE.search(out)
    assert m, out
    assert [int(m.group(1)), int(m.group(2))] == c["n_cand"]
    assert int(m.group(3)) == c["zero"]["epipolar"]["n"]
    vis = np.array(Image.open(str(tmp_path / "disparity.png")))
    assert vis.shape == (c["H"], c["W"], 3)
    # every pixel of disparity.png: the gray left image with each support painted, in output order, in its ramp colour
    # (getDisparityVisualization + writePNGRGB, buffer.hpp:949-1014, 395-474); supports from the oracle
    from oracle.pyoracle import Oracle, sparsematch_settings
    o = Oracle()
    rc, f = o.read_forest(forest_paths["zero"], c["W"], c["H"])
    supp, nl, nr = o.match_pair(L, R, f, sparsematch_settings())
    want = np.repeat(L[:, :, None], 3, axis=2)
    ds = np.unique(supp["d"])
    lut = dict(zip(ds.tolist(), kitti_ramp(ds)))
    for s_ in supp:
        want[s_["y"], s_["x"]] = lut[float(s_["d"])]
    assert np.array_equal(vis, want)
    changed = np.any(vis != L[:, :, None], axis=2)
    assert 0 < changed.sum() <= c["zero"]["epipolar"]["n"]


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_ON_AMD), reason="reference sample build not present")
def test_reference_sample_runs_on_the_hip_path(tmp_path, golden, forest_paths):
    c = golden["cases"][1]
    L, R, lp, rp = write_pair(tmp_path, c["W"], c["H"], c["s"], c["D"])
    out = run(REF_ON_AMD, forest_paths["tau"], lp, rp, cwd=str(tmp_path))
    m = LINE.search(out)
    assert m, out
    assert [int(m.group(1)), int(m.group(2)), int(m.group(3))] == c["n_cand"] + [c["tau"]["epipolar"]["n"]]
    assert os.path.exists(str(tmp_path / "disparity.png"))


TIMES = re.compile(r"tPreprocess: ([\d.e+-]+) ms.*tMatch: ([\d.e+-]+) ms")


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_ON_AMD), reason="reference sample build not present")
def test_reference_sample_one_shot_is_fast(tmp_path, golden, forest_paths):
    """BASELINE configs[0]/[1] literally: the reference's unchanged sample, ONE process, ONE pair.  Its clock starts after
    readForest (samples/sparsematch.cpp:42-45), which is where this build makes the device context, loads the code
    objects and reserves the workspaces -- so the printed tPreprocess + tMatch is the work, not the start-up
    (round 4 printed 222 + 20 ms here; the CPU reference prints 9.5 + 35 ms)."""
    c = golden["cases"][1]
    L, R, lp, rp = write_pair(tmp_path, c["W"], c["H"], c["s"], c["D"])
    sums = []
    for _ in range(3):                 # three fresh processes; the median is asserted (a shared box can hiccup once)
        out = run(REF_ON_AMD, forest_paths["zero"], lp, rp, cwd=str(tmp_path))
        m, t = LINE.search(out), TIMES.search(out)
        assert m and t, out
        assert [int(m.group(1)), int(m.group(2)), int(m.group(3))] == c["n_cand"] + [c["zero"]["epipolar"]["n"]]
        sums.append(float(t.group(1)) + float(t.group(2)))
    assert sorted(sums)[1] < 5.0, sums


@pytest.mark.gpu
@pytest.mark.parametrize("epipolar,hashtable", [(1, 0), (0, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize("sse", [True, False], ids=["sse_build", "naive_build"])
def test_cpp_forest_api_matches_oracle(check_bin, tmp_path, oracle, forest_paths, epipolar, hashtable, sse):
    """gpc::inference::Forest::{preprocessImage, stereoMatch, rectifiedMatch, matchPair} through the C++
    headers on the GPU; built with and without -D_INTRINSICS_SSE like the reference's two build modes."""
    from oracle.pyoracle import CORR_DTYPE, SUPPORT_DTYPE, sparsematch_settings
    binp = check_bin if sse else compile_cpp(os.path.join(ROOT, "tests", "cpp", "host_api_check.cpp"),
                                             os.path.join(BIN, "host_api_check_naive"), sse=False)
    W, H = 272, 61
    L, R, lp, rp = write_pair(tmp_path, W, H, 3, 9)
    outp = str(tmp_path / "api.bin")
    run(binp, "api", forest_paths["tau"], lp, rp, str(epipolar), str(hashtable), outp)
    raw = np.fromfile(outp, np.uint8)
    pos = 0

    def take(dtype):
        nonlocal pos
        n = int(raw[pos:pos + 4].view(np.int32)[0])
        pos += 4
        a = raw[pos:pos + n * dtype.itemsize].view(dtype)
        pos += n * dtype.itemsize
        return a
    corr, supp, fused = take(CORR_DTYPE), take(SUPPORT_DTYPE), take(SUPPORT_DTYPE)
    nl, nr = raw[pos:pos + 8].view(np.int32)
    rc, f = oracle.read_forest(forest_paths["tau"], W, H)
    s = sparsematch_settings(5, 64, 1, bool(epipolar), bool(hashtable), not sse)
    want, wl, wr = oracle.match_pair(L, R, f, s)
    assert (nl, nr) == (wl, wr)
    assert np.array_equal(supp, want) and np.array_equal(fused, want)
    # stereoMatch = the same correspondences before the disparity filter
    pre = (oracle.preprocess if sse else oracle.preprocess_naive)
    pl, pr = pre(L, 5), pre(R, 5)
    if sse:
        cl, cr = oracle.hash(pl[0], pl[1], f), oracle.hash(pr[0], pr[1], f)
    else:
        cl, cr = oracle.hash_naive(pl[0], pl[2], f), oracle.hash_naive(pr[0], pr[2], f)
    sl, sr = oracle.descriptors(cl, pl[2], W, bool(epipolar)), oracle.descriptors(cr, pr[2], W, bool(epipolar))
    fn = oracle.hash_correspondences if hashtable else oracle.find_correspondences
    wc = fn(sl, pl[2], sr, pr[2], W)
    assert np.array_equal(corr, wc)
