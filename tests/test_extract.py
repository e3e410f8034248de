"""Training-set extraction (the reference's extract sample): the Sintel datasources of include/gpc/Sintel*.hpp on the CPU,
gpc_hip_extract_triplets / gpc_hip_train_set_read on the GPU, and the extract -> train -> sparsematch pipeline.

No test reads a Sintel subset: a mini-Sintel tree (both layouts, 1024 x 436, value-noise frames of opengpc_amd.synth, known
flow / disparity bands, occlusion and invalid masks with nonzero regions) is written into tmp_path with numpy + zlib."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from test_host_api import BIN, LIBDIR, ROOT, compile_cpp, linked_libs, run

W0, H0 = 1024, 436
LO, HI = 20, 40


# --------------------------------------------------------------------------- mini-Sintel tree
def write_png(path, a):
    a = np.ascontiguousarray(a, np.uint8)
    h, w = a.shape[:2]
    ctype, ch = (2, 3) if a.ndim == 3 else (0, 1)
    raw = b"".join(b"\x00" + a[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 1)) + chunk(b"IEND", b""))


def write_flo(path, u, v):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    h, w = u.shape
    uv = np.stack([u, v], -1).astype("<f4")
    with open(path, "wb") as f:
        f.write(np.array([202021.25], "<f4").tobytes() + np.array([w, h], "<i4").tobytes() + uv.tobytes())


def flow_field():
    """four bands of constant flow: |round(u, v)| = 0, 3, sqrt(37), >= 15"""
    u = np.zeros((H0, W0), np.float32)
    v = np.zeros((H0, W0), np.float32)
    u[:, 256:512], v[:, 256:512] = 3.4, 0.2
    u[:, 512:768], v[:, 512:768] = -6.0, 0.6
    u[:, 768:], v[:, 768:] = -40.0, -2.0
    return u, v


def disparity():
    """bands d = 0, 5, 301 (4 r + g / 64)"""
    d = np.zeros((H0, W0), np.int32)
    d[:, 400:800] = 5
    d[:, 800:] = 301
    rgb = np.zeros((H0, W0, 3), np.uint8)
    rgb[..., 0] = d // 4
    rgb[..., 1] = (d % 4) * 64 + 7   # + 7: the low bits of g do not count
    rgb[..., 2] = 99
    return d, rgb


def mask(k, y0, x0):
    m = np.zeros((H0, W0), np.uint8)
    m[y0 + 10 * k:y0 + 10 * k + 60, x0 + 20 * k:x0 + 20 * k + 120] = 255
    return m


def make_tree(root):
    """alley_1 and alley_2 (scene indices 0, 1) of 4 frames each; sleeping_2 (index 20) is never visited.  alley_2 lacks
    invalid/frame_0003.png (flow frame 2 needs it) and disparities/frame_0002.png (stereo frame 2)."""
    from opengpc_amd.synth import synth_pair
    u, v = flow_field()
    d, rgb = disparity()
    t = os.path.join(root, "training")
    for d_ in ("final",):
        os.makedirs(os.path.join(t, d_), exist_ok=True)
    for si, scene in enumerate(("alley_1", "alley_2", "sleeping_2")):
        for k in range(1, 5):
            name = "frame_%04d" % k
            L, R = synth_pair(W0, H0, 10 * si + k, 9)
            write_png(os.path.join(t, "clean", scene, name + ".png"), np.stack([L, L, R], -1))   # RGB: gray = (r+g+b)/3
            write_png(os.path.join(t, "clean_left", scene, name + ".png"), L)
            write_png(os.path.join(t, "clean_right", scene, name + ".png"), R)
            write_png(os.path.join(t, "occlusions", scene, name + ".png"), mask(k, 100, 300))
            write_png(os.path.join(t, "invalid", scene, name + ".png"), mask(k, 250, 600))
            write_png(os.path.join(t, "outofframe", scene, name + ".png"), mask(k, 250, 600))
            write_png(os.path.join(t, "disparities", scene, name + ".png"), rgb)
            if k < 4:
                write_flo(os.path.join(t, "flow", scene, name + ".flo"), u, v)
    os.remove(os.path.join(t, "invalid", "alley_2", "frame_0003.png"))
    os.remove(os.path.join(t, "disparities", "alley_2", "frame_0002.png"))
    return root


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_tree(str(tmp_path_factory.mktemp("sintel")))


@pytest.fixture(scope="module")
def check_bin():
    from opengpc_amd import build
    build.build()
    return compile_cpp(os.path.join(ROOT, "tests", "cpp", "extract_check.cpp"), os.path.join(BIN, "extract_check"))


def points(check_bin, tree, kind, per, seed, lo=LO, hi=HI):
    out = run(check_bin, "points", tree, kind, str(per), str(lo), str(hi), str(seed))
    frames, pts = [], []
    for line in out.splitlines():
        if line.startswith("F "):
            frames.append(line.split()[1])
        elif line.startswith("P "):
            pts.append(list(map(int, line.split()[1:])) + [len(frames) - 1])
    return frames, np.array(pts, np.int64).reshape(-1, 7)


def safe(x, y):  # SintelOpticalFlow.hpp:269-274 at 1024 x 436
    return (x > 20) & (y > 20) & (x < W0 - 21) & (y < H0 - 21)


def tagged(out, tag):
    """the words of the output line that starts with `tag` (the datasources also print their own messages)"""
    return [l.split() for l in out.splitlines() if l.startswith(tag + " ")][0]


FRAME_ID = {"alley_1/frame_0001": ("alley_1", 1), "alley_1/frame_0002": ("alley_1", 2), "alley_2/frame_0001": ("alley_2", 1)}


# --------------------------------------------------------------------------- CPU
def reference_tree():
    m = re.search(r"^REF \?= (\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M)
    return m.group(1) if m else None


@pytest.mark.skipif(not (reference_tree() and os.path.exists(os.path.join(reference_tree() or "", "samples", "extract.cpp"))),
                    reason="reference tree not present")
def test_reference_extract_sample_compiles_against_these_headers(tmp_path):
    """The reference's own samples/extract.cpp, unchanged, builds against include/gpc/training.hpp and links this library."""
    from opengpc_amd import build
    build.build()
    exe = str(tmp_path / "ref_extract")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D_INTRINSICS_SSE", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(reference_tree(), "samples", "extract.cpp"), "-L" + LIBDIR, "-lgpc_hip", "-lz",
                           "-lpthread", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    assert "libgpc_hip.so" in linked_libs(exe)


def reference_functions(tmp):
    """the reference's isSafePatchCenter and its two getGroundTruthMatches, copied unchanged into tmp as the include files
    tests/cpp/ref_sampler_check.cpp expects"""
    lib = os.path.join(reference_tree(), "lib", "gpc")
    flow = open(os.path.join(lib, "SintelOpticalFlow.hpp")).read()
    stereo = open(os.path.join(lib, "SintelStereo.hpp")).read()
    safe_fn = re.search(r"  inline bool isSafePatchCenter\(.*?\n  \}\n", flow, re.S).group(0)
    body = lambda t: re.search(r"  int getGroundTruthMatches\(.*?\}// getGroundTruthMatches", t, re.S).group(0) + "\n"
    for name, text in (("ref_safe.inc", safe_fn), ("ref_flow_fn.inc", body(flow)), ("ref_stereo_fn.inc", body(stereo))):
        with open(os.path.join(tmp, name), "w") as f:
            f.write(text)


@pytest.mark.skipif(not (reference_tree() and os.path.exists(os.path.join(reference_tree() or "", "lib", "gpc", "SintelStereo.hpp"))),
                    reason="reference tree not present")
@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_samplers_draw_what_the_reference_code_draws(tmp_path, opt):
    """The reference's own getGroundTruthMatches (SintelOpticalFlow.hpp:478-558, SintelStereo.hpp:390-463), compiled
    unchanged by the same g++ with std::random_device returning a fixed seed, and this library's samplers given
    std::mt19937(that seed): the same keypoint lists on 40 random flow fields, disparity maps and masks -- the draw order
    (left to right in `randOffset(rng) * signum(rng)`) included."""
    from opengpc_amd import build
    build.build()
    reference_functions(str(tmp_path))
    exe = str(tmp_path / "ref_sampler_check")
    subprocess.check_call(["g++", "-std=c++17", opt, "-w", "-I" + str(tmp_path), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "ref_sampler_check.cpp"), "-L" + LIBDIR, "-lgpc_hip", "-lz",
                           "-lpthread", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    m = re.search(r"SAME 40 (\d+)", out)
    assert m and int(m.group(1)) == 40 * 2 * 300, out


def test_flo_round_trip(check_bin, tmp_path):
    rng = np.random.default_rng(3)
    h, w = 37, 53
    u = rng.normal(0, 9, (h, w)).astype(np.float32)
    v = rng.normal(0, 9, (h, w)).astype(np.float32)
    write_flo(str(tmp_path / "training" / "flow" / "alley_1" / "frame_0007.flo"), u, v)
    for x, y in ((0, 0), (52, 36), (17, 5), (3, 30)):
        got = tagged(run(check_bin, "flo", str(tmp_path), "alley_1", "7", str(x), str(y)), "FLO")
        assert got[:3] == ["FLO", str(w), str(h)]
        assert np.float32(float(got[3])) == u[y, x] and np.float32(float(got[4])) == v[y, x]
    assert "FLO missing" in run(check_bin, "flo", str(tmp_path), "alley_1", "8", "0", "0")


def test_rgb_disparity_decode(check_bin, tmp_path):
    img = np.zeros((20, 40, 3), np.uint8)
    cases = [(1, 2, (0, 0, 5)), (3, 4, (1, 63, 0)), (5, 6, (1, 64, 0)), (7, 8, (75, 200, 1)), (39, 19, (255, 255, 255))]
    for x, y, c in cases:
        img[y, x] = c
    write_png(str(tmp_path / "training" / "disparities" / "alley_1" / "frame_0003.png"), img)
    for x, y, (r, g, b) in cases:
        got = tagged(run(check_bin, "disp", str(tmp_path), "alley_1", "3", str(x), str(y)), "DISP")
        assert got == ["DISP", str(4 * r + g // 64), str(r), str(g), str(b)]


@pytest.mark.parametrize("kind", ["flow", "stereo"])
def test_scene_walk(check_bin, tree, kind):
    """Scenes 0 .. 19 of the name list only (sleeping_2 is number 20), frames 1 .. n-2 of each, a frame whose files do not
    all open skipped (SintelOpticalFlow.hpp:126-157, SintelStereo.hpp:120-151)."""
    frames, pts = points(check_bin, tree, kind, 10, 1)
    assert frames == ["alley_1/frame_0001", "alley_1/frame_0002", "alley_2/frame_0001"]
    assert len(pts) == 30


def load_masks(tree, kind, scene, k):
    from PIL import Image
    t = os.path.join(tree, "training")
    rd = lambda d, i: np.asarray(Image.open(os.path.join(t, d, scene, "frame_%04d.png" % i)))
    if kind == "flow":
        return [rd("occlusions", k), rd("occlusions", k + 1), rd("invalid", k), rd("invalid", k + 1)]
    return [rd("occlusions", k), rd("outofframe", k)]


@pytest.mark.parametrize("kind", ["flow", "stereo"])
def test_sampler_invariants(check_bin, tree, kind):
    frames, P = points(check_bin, tree, kind, 1500, 5)
    rx, ry, px, py, nx, ny, f = P.T
    assert safe(rx, ry).all() and safe(px, py).all() and safe(nx, ny).all()
    u, v = flow_field()
    d, _ = disparity()
    for fi, name in enumerate(frames):
        sel = f == fi
        for m in load_masks(tree, kind, *FRAME_ID[name]):        # every mask read at the SOURCE point
            assert (m[ry[sel], rx[sel]] == 0).all()
    if kind == "flow":
        assert (px == rx + np.round(u[ry, rx]).astype(np.int64)).all() and (py == ry + np.round(v[ry, rx]).astype(np.int64)).all()
        ox, oy = nx - px, ny - py
        for o in (ox, oy):                                      # sig() is never 0
            assert ((np.abs(o) >= LO) & (np.abs(o) <= HI)).all()
    else:
        assert (py == ry).all() and (px == rx - d[ry, rx]).all()
        ox, oy = nx - px, ny - py
        for o in (ox, oy):                                      # raw signum: 0 or +-[lo, hi]
            assert ((o == 0) | ((np.abs(o) >= LO) & (np.abs(o) <= HI))).all()
            assert 0.2 < np.mean(o == 0) < 0.45                 # P(0) = 1/3, less the redraws of unsafe negatives
        both = np.mean((ox == 0) & (oy == 0))
        assert 0.04 < both < 0.2                                # about one in nine negatives sits on the positive


def expected_band_shares(kind, tree, frames, per):
    """P(a kept point lies in each band) from the valid pixels of each band times its acceptance rate"""
    u, v = flow_field()
    d, _ = disparity()
    ys, xs = np.mgrid[0:H0, 0:W0]
    if kind == "flow":
        ru, rv = np.round(u).astype(np.int64), np.round(v).astype(np.int64)
        ok_geo = safe(xs, ys) & safe(xs + ru, ys + rv)
        dist = np.sqrt(ru.astype(np.float64) ** 2 + rv ** 2)
        acc = 1 - (15 - np.minimum(dist, 15.)) / 15 * 0.5       # SintelOpticalFlow.hpp:516-519, 529
        edges = [0, 256, 512, 768, W0]
    else:
        ok_geo = safe(xs, ys) & safe(xs - d, ys)
        acc = 1 - (15 - np.minimum(np.abs(d), 15)) // 15 * 0.5  # SintelStereo.hpp:427: integer division
        edges = [0, 400, 800, W0]
    counts, want = np.zeros(len(edges) - 1), np.zeros(len(edges) - 1)
    for name in frames:
        ok = ok_geo.copy()
        for m in load_masks(tree, kind, *FRAME_ID[name]):
            ok &= m == 0
        w = np.array([(ok[:, a:b] * acc[:, a:b]).sum() for a, b in zip(edges, edges[1:])])
        want += per * w / w.sum()
    return edges, want


@pytest.mark.parametrize("kind", ["flow", "stereo"])
def test_acceptance_rates(check_bin, tree, kind):
    """Flow: accepted with probability 1 - (15 - min(|round(u, v)|, 15)) / 15 * 0.5 (continuous); stereo: 0.5 at d == 0,
    1 elsewhere.  The share of points per band of constant flow / disparity, against binomial tolerances."""
    per = 6000
    frames, P = points(check_bin, tree, kind, per, 9)
    edges, want = expected_band_shares(kind, tree, frames, per)
    n = len(P)
    got = np.histogram(P[:, 0], bins=edges)[0]
    p = want / want.sum()
    sigma = np.sqrt(n * p * (1 - p))
    assert (np.abs(got - want) < 5 * sigma).all(), (got, want, sigma)
    # and the rates are not all 1: with equal acceptance the d == 0 band would hold a larger share
    if kind == "stereo":
        assert got[0] < 0.8 * n * 380 / 982


@pytest.mark.parametrize("kind", ["flow", "stereo"])
def test_same_seed_same_points(check_bin, tree, kind):
    a = run(check_bin, "points", tree, kind, "200", "20", "40", "77")
    assert a == run(check_bin, "points", tree, kind, "200", "20", "40", "77")
    assert a != run(check_bin, "points", tree, kind, "200", "20", "40", "78")


def test_draw_cap_ends_a_frame_without_valid_pixels(check_bin):
    out = subprocess.run([check_bin, "cap"], capture_output=True, text=True, timeout=120).stdout
    assert "CAP 0 0" in out and out.count("draw cap") == 2


def test_extraction_kernels_use_no_scratch(tmp_path):
    """k_extract_gather and k_ts_read (k_extract.h): no scratch, no spilled VGPRs (compiler resource report)."""
    env = dict(os.environ, KRES_OUT=str(tmp_path / "libgpc_kres.so"))
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), "k_extract_gather|k_ts_read"], env=env, check=True,
                         capture_output=True, text=True, timeout=900).stdout
    rows = [l for l in txt.splitlines() if l.startswith("gpc::")]
    assert len(rows) == 2, txt
    for l in rows:
        m = re.search(r"spill s\s+(\d+) v\s+(\d+)\s+scratch\s+(\d+)", l)
        assert m and int(m.group(2)) == 0 and int(m.group(3)) == 0, l


# --------------------------------------------------------------------------- GPU
def frames_and_points(W, H, nframes, per, seed):
    from opengpc_amd.synth import synth_pair
    rng = np.random.default_rng(seed)
    L = np.empty((nframes, H, W), np.uint8)
    R = np.empty_like(L)
    pts, first = [], [0]
    edge = np.array([20, 21, W - 21, W - 20]), np.array([20, 21, H - 21, H - 20])
    for f in range(nframes):
        L[f], R[f] = synth_pair(W, H, 3 * f + seed, 7 + f)
        L[f, ::17] = rng.integers(0, 256, (len(range(0, H, 17)), W))   # some detail the box filter must get right
        p = np.stack([rng.integers(0, W, per), rng.integers(0, H, per), rng.integers(14, W - 14, per),
                      rng.integers(14, H - 14, per), rng.integers(21, W - 21, per), rng.integers(21, H - 21, per)], 1)
        # the keep rule's edges: x / y = 20 (dropped), 21, w-21 (kept), w-20 (dropped) on every point of the triplet
        for k in range(min(per, 48)):
            j = k % 3
            p[k, 2 * j] = edge[0][k % 4]
            p[k, 2 * j + 1] = edge[1][(k // 4) % 4]
        pts.append(p)
        first.append(first[-1] + per)
    return L, R, np.concatenate(pts).astype(np.int32), np.array(first, np.int32)


def restate(oracle, L, R, pts, first, naive, order=None):
    """numpy: Feature::extractAllTriplets on oracle.preprocess(..)[0] (naive: preprocess_naive), the keep rule, slicing"""
    pre = oracle.preprocess_naive if naive else oracle.preprocess
    nf, H, W = L.shape
    out = []
    inside = lambda x, y: (x > 20) & (y > 20) & (x < W - 20) & (y < H - 20)
    for f in range(nf):
        sL, sR = pre(L[f], 10)[0], pre(R[f], 10)[0]
        for rx, ry, px, py, nx, ny in pts[first[f]:first[f + 1]]:
            if not (inside(rx, ry) and inside(px, py) and inside(nx, ny)):
                continue
            cut = lambda s, x, y: s[y - 13:y + 14, x - 13:x + 14].T.reshape(729)   # byte 27 ix + iy = pixel(x+ix-13, y+iy-13)
            out.append(np.stack([cut(sL, rx, ry), cut(sR, px, py), cut(sR, nx, ny)]))
    out = np.array(out, np.uint8).reshape(-1, 3, 729)
    if order is not None:
        res = np.empty_like(out)
        res[order] = out
        out = res
    return out


@pytest.fixture(scope="module")
def gctx():
    import opengpc_amd as g
    ctx = g.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1024, 436), (640, 480), (1920, 1080)])
@pytest.mark.parametrize("naive", [False, True])
def test_extract_is_bit_exact_against_numpy(gctx, oracle, W, H, naive):
    import torch
    L, R, pts, first = frames_and_points(W, H, 3, 300, W + H + naive)
    gctx.set_arithmetic(naive)
    try:
        want = restate(oracle, L, R, pts, first, naive)
        n = len(want)
        assert 0 < n < len(pts)
        ts = gctx.extract_triplets(L, R, pts, first)
        assert ts.n == n and np.array_equal(ts.read(), want)
        assert np.array_equal(ts.read(n - 5, 5), want[n - 5:]) and ts.read(n, 0).shape == (0, 3, 729)
        assert (ts.marks() == 0).all()
        ts.close()
        order = np.random.default_rng(1).permutation(n).astype(np.int32)
        dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
        ts = gctx.extract_triplets(dL, dR, pts, first, order)   # device pointers, with a permutation
        assert ts.n == n and np.array_equal(ts.read(), restate(oracle, L, R, pts, first, naive, order))
        ts.close()
    finally:
        gctx.set_arithmetic(False)


@pytest.mark.gpu
def test_extract_multi_chunk(oracle, monkeypatch):
    """GPC_HIP_EXTRACT_FRAMES=2: seven frames in four chunks, with and without a permutation, from host and device memory"""
    import opengpc_amd as g
    import torch
    monkeypatch.setenv("GPC_HIP_EXTRACT_FRAMES", "2")
    ctx = g.Context(0)
    try:
        L, R, pts, first = frames_and_points(640, 480, 7, 203, 4)
        pts[first[3]:first[4], 0] = 3          # frame 3 keeps nothing (its chunk still runs for frame 2)
        want = restate(oracle, L, R, pts, first, False)
        n = len(want)
        order = np.random.default_rng(2).permutation(n).astype(np.int32)
        for o in (None, order):
            for src in ((L, R), (torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())):
                ts = ctx.extract_triplets(src[0], src[1], pts, first, o)
                exp = want if o is None else restate(oracle, L, R, pts, first, False, o)
                assert ts.n == n and np.array_equal(ts.read(), exp)
                ts.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_same_bytes_as_feature_extract_all_triplets(gctx, check_bin, tmp_path):
    """the read-back equals what the existing Feature::extractAllTriplets cuts for the same frames and points"""
    L, R, pts, first = frames_and_points(1024, 436, 3, 400, 8)
    for name, a in (("L", L), ("R", R), ("P", pts), ("F", first)):
        a.tofile(str(tmp_path / name))
    out = run(check_bin, "host", *(str(tmp_path / n) for n in ("L", "R", "P")), "1024", "436", "3", str(tmp_path / "F"),
              str(tmp_path / "host.bin"))
    host = np.fromfile(str(tmp_path / "host.bin"), np.uint8).reshape(-1, 3, 729)
    ts = gctx.extract_triplets(L, R, pts, first)
    assert "HOST %d" % ts.n in out and np.array_equal(ts.read(), host)
    ts.close()


@pytest.mark.gpu
def test_training_on_the_extracted_set(gctx):
    """gpc_hip_train_fern on the extracted set == on train_set_create(read-back)"""
    from test_training import make_cands
    L, R, pts, first = frames_and_points(1024, 436, 2, 1500, 12)
    n = len(restate_count(pts, 1024, 436))
    ext = gctx.extract_triplets(L, R, pts, first, np.random.default_rng(5).permutation(n))
    up = gctx.train_set(ext.read())
    cand = make_cands(6 * 8, 3)
    for taulo, tauhi in ((0, 1), (-5, 5)):
        a = ext.train_fern(6, cand, 8, taulo, tauhi, 1, 0.5)
        b = up.train_fern(6, cand, 8, taulo, tauhi, 1, 0.5)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ext.close()
    up.close()


@pytest.mark.gpu
def test_extract_errors(gctx):
    import opengpc_amd as g
    L, R, pts, first = frames_and_points(640, 480, 1, 50, 1)
    with pytest.raises(g.GpcError) as e:                  # width % 16
        gctx.extract_triplets(L[:, :, :632 + 4], R[:, :, :636], pts, first)
    assert e.value.status == g.capi.E_INVALID
    n = len(restate_count(pts, 640, 480))
    for bad in (np.zeros(n, np.int32), np.arange(1, n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)[::-1] - 1):
        with pytest.raises(g.GpcError) as e:              # not a permutation
            gctx.extract_triplets(L, R, pts, first, bad)
        assert e.value.status == g.capi.E_INVALID
    Lib = gctx.L
    h, k = C.c_void_p(), C.c_int()
    ff = np.ascontiguousarray(first)
    for args in ((None, L.ctypes.data), (L.ctypes.data, None)):   # null frames
        st = Lib.gpc_hip_extract_triplets(gctx.h, args[0], args[1], 640, 480, 1, pts.ctypes.data, ff.ctypes.data, None,
                                          C.byref(h), C.byref(k))
        assert st == g.capi.E_INVALID
    st = Lib.gpc_hip_extract_triplets(gctx.h, L.ctypes.data, R.ctypes.data, 640, 480, 1, None, ff.ctypes.data, None,
                                      C.byref(h), C.byref(k))
    assert st == g.capi.E_INVALID                          # null points
    far = pts.copy()
    far[:, 0] = 5                                          # nothing kept
    st = Lib.gpc_hip_extract_triplets(gctx.h, L.ctypes.data, R.ctypes.data, 640, 480, 1, far.ctypes.data, ff.ctypes.data, None,
                                      C.byref(h), C.byref(k))
    assert st == 0 and k.value == 0 and not h.value
    assert gctx.extract_triplets(L, R, far, first) is None


def restate_count(pts, W, H):
    x, y = pts[:, 0::2], pts[:, 1::2]
    return np.nonzero(((x > 20) & (y > 20) & (x < W - 20) & (y < H - 20)).all(1))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["flow", "stereo"])
def test_extract_train_sparsematch_pipeline(check_bin, tree, tmp_path, kind):
    """samples/extract (seeded) -> a .bin equal to the seeded extractTrainingSet read-back -> samples/train -> a forest
    gpc_hip_read_forest parses -> samples/sparsematch runs with it on a synthetic pair"""
    import opengpc_amd as g
    from PIL import Image
    from opengpc_amd.synth import synth_pair
    sdir = os.path.join(ROOT, "samples")
    out_bin = str(tmp_path / "set.bin")
    log = run(os.path.join(sdir, "extract"), tree, out_bin, kind, "300", "20", "40", "31")
    n = 3 * 300
    assert os.path.getsize(out_bin) == 3 * 729 * n, log
    run(check_bin, "extract", tree, kind, "300", "20", "40", "31", str(tmp_path / "dev.bin"))
    assert open(out_bin, "rb").read() == open(str(tmp_path / "dev.bin"), "rb").read()
    forest = str(tmp_path / "forest.txt")
    run(os.path.join(sdir, "train"), out_bin, forest, "tau", "1", "4", "4")
    st, fm = g.read_forest(forest, 640, 480)
    assert st == 0 and fm.num_tests == 12 and fm.type == 1
    L, R = synth_pair(640, 480, 2, 12)
    Image.fromarray(L, "L").save(str(tmp_path / "l.png"))
    Image.fromarray(R, "L").save(str(tmp_path / "r.png"))
    out = run(os.path.join(sdir, "sparsematch"), forest, str(tmp_path / "l.png"), str(tmp_path / "r.png"), cwd=str(tmp_path))
    m = re.search(r"#candidatesL:(\d+), #candidatesR:(\d+), tMatch: [\d.e+-]+ ms, num matches:(\d+)", out)
    assert m and int(m.group(1)) > 0 and "failed" not in out, out
    assert os.path.exists(str(tmp_path / "disparity.png"))


# --------------------------------------------------------------------------- the Python wrapper's argument checks (CPU)
class _FakeLib:
    """records which extraction entry point the wrapper calls; every call keeps nothing"""
    def __init__(self):
        self.calls = []

    def _entry(self, name):
        def fn(*args):
            self.calls.append(name)
            args[-1]._obj.value = 0
            return 0
        return fn

    def __getattr__(self, name):
        if name.startswith("gpc_hip_extract_triplets"):
            return self._entry(name)
        raise AttributeError(name)


def _fake_context():
    import opengpc_amd as g
    ctx = g.Context.__new__(g.Context)
    ctx.L, ctx.h, ctx.device, ctx._pinned = _FakeLib(), C.c_void_p(1), 0, []
    return ctx


def test_wrapper_routes_host_frames_and_refuses_bad_arguments():
    """Context.extract_triplets: numpy arrays and CPU tensors go to the HOST entry point (never to the _device one, whose
    kernels would fault on a host address); frames that are not uint8, points that do not match frame_first and an order
    of the wrong length raise ValueError before the library is called."""
    import torch
    ctx = _fake_context()
    L, R, pts, first = frames_and_points(640, 480, 2, 80, 1)
    n_kept = len(restate_count(pts, 640, 480))
    assert 0 < n_kept < len(pts)
    assert ctx.extract_triplets(L, R, pts, first) is None
    assert ctx.extract_triplets(torch.from_numpy(L), torch.from_numpy(R), pts, first, np.arange(n_kept)) is None
    assert ctx.L.calls == ["gpc_hip_extract_triplets"] * 2
    bad = [
        (L.astype(np.int64), R.astype(np.int64), pts, first, None),                                   # not uint8
        (torch.from_numpy(L).float(), torch.from_numpy(R).float(), pts, first, None),                 # not uint8 (tensor)
        (torch.from_numpy(L), R, pts, first, None),                                                   # tensor + array
        (L, R, pts[:-1], first, None),                                                                # frame_first past the points
        (L, R, pts, first[:-1], None),                                                                # frame_first too short
        (L, R, pts, first, np.arange(n_kept - 1)),                                                    # order too short
        (L, R, pts, first, np.arange(n_kept + 1)),                                                    # order too long
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ctx.extract_triplets(*args)
    assert ctx.L.calls == ["gpc_hip_extract_triplets"] * 2


@pytest.mark.gpu
def test_device_entry_refuses_what_is_not_on_the_device(gctx):
    """CUDA tensors of another dtype are refused by the wrapper; the C _device entry point refuses host memory (pageable
    and page-locked) with GPC_E_INVALID before it launches anything."""
    import torch
    import opengpc_amd as g
    L, R, pts, first = frames_and_points(640, 480, 1, 40, 2)
    with pytest.raises(ValueError):
        gctx.extract_triplets(torch.from_numpy(L).cuda().long(), torch.from_numpy(R).cuda().long(), pts, first)
    with pytest.raises(ValueError):
        gctx.extract_triplets(torch.from_numpy(L).cuda()[:, :, ::2], torch.from_numpy(R).cuda()[:, :, ::2], pts, first)
    pinned = gctx.pinned_empty(L.shape, np.uint8)
    pinned[...] = L
    ff = np.ascontiguousarray(first)
    h, k = C.c_void_p(), C.c_int()
    for src in (L, pinned):
        st = gctx.L.gpc_hip_extract_triplets_device(gctx.h, src.ctypes.data, src.ctypes.data, 640, 480, 1, pts.ctypes.data,
                                                     ff.ctypes.data, None, C.byref(h), C.byref(k))
        assert st == g.capi.E_INVALID and not h.value
    dL = torch.from_numpy(L).cuda()
    st = gctx.L.gpc_hip_extract_triplets_device(gctx.h, dL.data_ptr(), L.ctypes.data, 640, 480, 1, pts.ctypes.data,
                                                 ff.ctypes.data, None, C.byref(h), C.byref(k))
    assert st == g.capi.E_INVALID and not h.value
    ts = gctx.extract_triplets(L, R, pts, first)           # the context is fine afterwards
    assert ts is not None and ts.n == len(restate_count(pts, 640, 480))
    ts.close()
