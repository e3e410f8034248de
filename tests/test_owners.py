"""Who frees what: the owner types of opengpc_amd/csrc/owners.h driven by a stand-alone program with a recording
backend under AddressSanitizer and UBSan, and a source check that the host code releases nothing by hand."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "opengpc_amd", "csrc")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm toolchain's clang++")
def test_owners_under_asan_ubsan(tmp_path):
    """exactly one release per allocation through destruction, moves, self-move, std::swap, reset and failed allocations,
    for the block and the handle owner; allocations equal releases at exit (and the leak checker agrees)"""
    exe = str(tmp_path / "owners_check")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I" + CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "owners_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.returncode, res.stdout, res.stderr)


def test_owners_header_is_host_only():
    text = open(os.path.join(CSRC, "owners.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", text)


def test_nothing_is_released_by_hand():
    """hipFree, hipHostFree, hipStreamDestroy and hipEventDestroy are called by the owners' HIP backends (the structs DevMem,
    PinnedMem, StreamApi, EventApi) and by gpc_hip_host_free, which frees what the caller owns -- nowhere else in
    opengpc_amd/csrc, whichever file holds them (owners.h names the calls in prose only: no hit there)"""
    texts = {f: open(os.path.join(CSRC, f), errors="replace").read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))}
    allowed = {"hipFree(": "DevMem", "hipHostFree(": "PinnedMem", "hipStreamDestroy(": "StreamApi", "hipEventDestroy(": "EventApi"}
    # the bodies each call may stand in, per file: from the opening line of the struct / function to the first line that is
    # just a brace
    def bodies(text, opening):
        out = []
        for m in re.finditer(r"^" + re.escape(opening), text, flags=re.M):
            out.append((m.start(), m.start() + re.search(r"^\};?$", text[m.start():], flags=re.M).end()))
        return out
    for call, backend in allowed.items():
        found = 0
        for f, text in texts.items():
            spans = bodies(text, "struct %s {" % backend)
            if call == "hipHostFree(":
                spans += bodies(text, "int gpc_hip_host_free(")
            for m in re.finditer(r"\b" + re.escape(call), text):
                h = m.start()
                assert any(a <= h < b for a, b in spans), "%s at %s:%d" % (call, f, text.count("\n", 0, h) + 1)
                found += 1
        assert found, call
