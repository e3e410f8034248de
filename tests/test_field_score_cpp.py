"""tests/cpp/field_score_check.cpp, a program of its own with its own main.  CPU: opengpc_amd/csrc/field_score_host.h -- the
argument checks, the squared parameters, the launch geometry, the host's integer square root -- built plainly and with
-fsanitize=address,undefined, and run as a process.  GPU: the same program built against the library scores a case through
gpc::evaluation::scoreField (include/gpc/dense_evaluation.hpp) and compares with the numbers the Python model
(tests/field_score_util.py) wrote into a file."""
import os
import subprocess

import numpy as np
import pytest

import field_score_util as fu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "field_score_check.cpp")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm toolchain's clang++")
@pytest.mark.parametrize("sanitize", [False, True])
def test_field_score_host_checks(tmp_path, sanitize):
    exe = str(tmp_path / "field_score_check")
    flags = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-Wall"] + flags + ["-I" + os.path.join(ROOT, "opengpc_amd", "csrc"), "-o", exe, SRC])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.returncode, res.stdout, res.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("Cn, with_cls, prm", [(1, False, fu.DEFAULTS), (2, True, (fu.CRAFT_THR, 300, 255, ())),
                                              (2, False, (fu.DEFAULTS[0], 768, 50, fu.SINTEL_SPEED))])
def test_score_field_equals_the_model(tmp_path, Cn, with_cls, prm):
    from opengpc_amd import build
    build.build()
    W, H = 37, 29
    field, u, v, ignore, cls = [None if a is None else a[1] for a in fu.random_case(W, H, 3, Cn)]
    words, err = fu.score(field[None], u[None], None if v is None else v[None], ignore[None], cls[None] if with_cls else None, prm)
    thr, speed = list(prm[0]) + [0] * (8 - len(prm[0])), list(prm[3]) + [0] * (3 - len(prm[3]))
    head = np.array([W, H, Cn, int(with_cls), len(prm[0])] + thr + [prm[1], prm[2], len(prm[3])] + speed, np.int32)
    assert len(head) == 19
    data = str(tmp_path / "case.bin")
    with open(data, "wb") as f:
        for a in (head, field, u, v, ignore, cls, words[0], err[0]):
            if a is not None:
                f.write(np.ascontiguousarray(a).tobytes())
    exe = str(tmp_path / "field_score_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D_INTRINSICS_SSE", "-DFIELD_SCORE_WITH_LIBRARY",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "opengpc_amd", "csrc"), SRC, "-o", exe,
                           "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"),
                           "-pthread"])
    res = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    # (the refusal the program provokes on purpose is reported on stdout by gpc::inference, ahead of the verdict)
    assert res.returncode == 0 and res.stdout.split("\n")[-2:] == ["ok", ""], (res.returncode, res.stdout, res.stderr)
