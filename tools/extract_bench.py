"""Times training-set extraction (gpc_hip_extract_triplets) against the host path it replaces, for N synthetic 1024x436
frame pairs x K triplets each, and prints one JSON line (best of --reps, milliseconds):
  device_from_host_ms   frames in host memory: upload + smooth + gather into the device set
  device_from_hbm_ms    frames already in HBM: smooth + gather
  host_*                Feature::extractAllTriplets frame by frame (one ndb::Buffer per patch) and the packing +
                        gpc_hip_train_set_create that every scoring call of the reference-style API starts with
usage: python tools/extract_bench.py [--pairs N] [--triplets K] [--reps R]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--triplets", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from opengpc_amd import build
    build.build()
    lib = os.path.join(ROOT, "opengpc_amd")
    exe = os.path.join(ROOT, "tools", "bin_extract_bench")
    subprocess.check_call(["hipcc", "-std=c++17", "-O2", "-D_INTRINSICS_SSE", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tools", "src", "extract_bench.cpp"), "-L" + lib, "-lgpc_hip", "-lz", "-lpthread",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe, str(a.pairs), str(a.triplets), str(a.reps)], check=True, capture_output=True, text=True).stdout
    res = {}
    for line in out.splitlines():
        if line.startswith("RESULT "):
            _, k, v = line.split()
            res[k] = float(v) if "." in v else int(v)
    res["bytes_per_triplet"] = 3 * 729
    print(json.dumps(res))


if __name__ == "__main__":
    main()
