"""CPU, host code only: the bootstraps gpc::training::Forest draws for its device overload (include/gpc/training.hpp).
After Forest::seed(s) they are std::mt19937(s) through std::uniform_int_distribution<int>(0, perFern - 1), taken
nferns * perFern times in fern order, and GPC_TRAIN_DUMP_DRAWS receives them.  Checked by a stand-alone program
(tests/cpp/train_forest_draws_check.cpp), built once plainly and once under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

from test_host_api import BIN, LIBDIR, ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "train_forest_draws_check.cpp")
CASES = [(7, 3, 1400), (0, 6, 20000), (123456789, 1, 1), (5, 2, 2)]


def compile_check(out, sanitize):
    from opengpc_amd import build
    build.build()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    flags = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D_INTRINSICS_SSE"] + flags +
                          ["-I" + os.path.join(ROOT, "include"), "-o", out, SRC, "-L" + LIBDIR, "-lgpc_hip", "-lz", "-lpthread",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def draws_bin(request):
    return compile_check(os.path.join(BIN, "train_forest_draws_check_" + request.param), request.param != "plain")


@pytest.mark.parametrize("seed,nferns,per_fern", CASES)
def test_seeded_draws_are_the_reference_generator(draws_bin, tmp_path, seed, nferns, per_fern):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([draws_bin, str(seed), str(nferns), str(per_fern), str(tmp_path / "draws.txt")], capture_output=True,
                       text=True, env=env)
    assert r.returncode == 0 and "DRAWS OK %d" % (nferns * per_fern) in r.stdout, (r.stdout, r.stderr[-2000:])
