"""CPU: opengpc_amd/csrc/gapfill_host.h -- the argument checks, the overlap arithmetic, the bands of the column scan and the
workspace size of gpc_hip_gapfill_*, the host code reachable without a GPU -- driven by tests/cpp/gapfill_check.cpp, a
program of its own with its own main: built plainly and with -fsanitize=address,undefined, and run as a process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm toolchain's clang++")
@pytest.mark.parametrize("sanitize", [False, True])
def test_gapfill_host_checks(tmp_path, sanitize):
    exe = str(tmp_path / "gapfill_check")
    flags = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-Wall"] + flags + ["-I" + os.path.join(ROOT, "opengpc_amd", "csrc"), "-o", exe,
                                                                           os.path.join(ROOT, "tests", "cpp", "gapfill_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.returncode, res.stdout, res.stderr)
