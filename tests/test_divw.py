"""CPU only: the host-made multiply-high divisors (make_divw: pixel indices, consensus cells, the fused join's ticket split)
and the fused join's shard split (join_shards_auto, make_join_split) of opengpc_amd/csrc/gpc_device.h, by a stand-alone
host program that includes that header as it stands (tests/cpp/divw_check.cpp says what it walks), under
AddressSanitizer + UndefinedBehaviorSanitizer.  Nothing is loaded into Python and no device is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "divw_check.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm toolchain's clang++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("divw") / "divw_check")
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "opengpc_amd", "csrc"), "-o", out, SRC, "-lpthread"])
    return out


def run(exe, cmd):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, cmd], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_make_divw_divides_every_dividend_below_2_31(exe):
    out = run(exe, "divw")
    assert "OK divw 132138 divisors" in out and "OK divw 2^31 - 1 and random dividends" in out


def test_join_shards_contract_for_every_batch_size(exe):
    assert "OK shards 4096 batch sizes" in run(exe, "shards")
