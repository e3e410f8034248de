"""CPU: the dense field scorer (gpc_hip_score_fields*) -- the numpy restatement of the rule (tests/field_score_util.py)
against the rule taken pixel by pixel with Python integers, the structs of the header against the ctypes structures, the
documented defaults, the entry points in header and binding, the refusals with a null context, the block's place in the
header, the timing-slot table left as it was, and the accessors."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import field_score_util as fu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gpc_hip_score_fields_device": 11, "gpc_hip_score_fields": 11}
# opengpc_amd/csrc/gpc_hip.hip, kKernelNames of the parent commit: 62 names, "k_preprocess" .. "k_clean_apply"
PARENT_SLOTS = 62


def lib():
    import opengpc_amd as g
    from opengpc_amd import build
    build.build()
    return g, g.load()


def raw_header():
    return open(os.path.join(ROOT, "include", "gpc_hip.h")).read()


@pytest.mark.parametrize("C_", [1, 2])
@pytest.mark.parametrize("shape", [(5, 3), (9, 7)])
def test_the_model_equals_the_rule_pixel_by_pixel(shape, C_):
    W, H = shape
    field, u, v, ignore, cls = fu.random_case(W, H, 2, C_)
    prms = (fu.DEFAULTS, (fu.CRAFT_THR, 300, 255, fu.SINTEL_SPEED), ((), 0, 0, (0, 5000, 5000)))
    for prm in prms:
        for with_ign in (True, False):
            for with_cls in (True, False):
                ign_, cls_ = ignore if with_ign else None, cls if with_cls else None
                words, err = fu.score(field, u, v, ign_, cls_, prm)
                for t in range(2):
                    w, e = fu.score_plain(field[t], u[t], None if v is None else v[t], None if ign_ is None else ign_[t],
                                          None if cls_ is None else cls_[t], prm)
                    assert words[t].tolist() == w, (prm, with_ign, with_cls, t)
                    assert err[t].tolist() == e


@pytest.mark.parametrize("C_", [1, 2])
def test_the_model_on_the_crafted_pixels(C_):
    """every crafted pixel through both statements of the rule, under every parameter set the GPU test uses; and the
    crafted row does hold what it is meant to: all four categories, a clamped error, every bin, both outcomes of the
    outlier test"""
    field, u, v, ignore, cls, notes = fu.crafted(C_)
    assert field.shape[3] == len(notes) > 250
    for prm in fu.CRAFT_PRMS:
        for cls_ in (None, cls):
            words, err = fu.score(field, u, v, ignore, cls_, prm)
            w, e = fu.score_plain(field[0], u[0], None if v is None else v[0], ignore[0], None if cls_ is None else cls_[0], prm)
            assert words[0].tolist() == w and err[0].tolist() == e, prm
    words, err = fu.score(field, u, v, ignore, cls, fu.CRAFT_PRMS[0])
    assert (words[0, :4] > 0).all() and words[0, fu.ALL] > 0 and (err == 0xFFFE).any() and (err == 0).any()
    assert all(words[0, fu.BIN + fu.TALLY * b] > 0 for b in range(4))
    assert 0 < words[0, fu.ALL + 9] < words[0, fu.ALL]
    words, _ = fu.score(field, u, v, ignore, None, fu.CRAFT_PRMS[-1])
    assert all(words[0, fu.BIN + fu.TALLY * b] > 0 for b in range(3)) and words[0, fu.BIN + fu.TALLY * 3] == 0


def test_identities_of_the_header_on_the_model():
    for C_ in (1, 2):
        field, u, v, ignore, cls = fu.random_case(37, 29, 3, C_)
        for cls_, prm in ((cls, fu.DEFAULTS), (None, (fu.DEFAULTS[0], 768, 50, fu.SINTEL_SPEED)), (None, fu.DEFAULTS)):
            words, _ = fu.score(field, u, v, ignore, cls_, prm)
            assert (words[:, 0] == 37 * 29).all() and (words[:, 0] == words[:, 1:4].sum(axis=1) + words[:, fu.ALL]).all()
            bins = words[:, fu.BIN:].reshape(3, 4, fu.TALLY)
            assert np.array_equal(bins.sum(axis=1), words[:, fu.ALL:fu.BIN])
            assert (words[:, 1:4] > 0).all() and (words[:, fu.ALL] > 0).all()


def struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    return [(t, n, int(k) if k else 1) for t, n, k in re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?;", body)]


def test_structs_defaults_and_entry_points():
    g, L = lib()
    raw = raw_header()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    width = {"int32_t": 4, "int64_t": 8, "gpc_field_tally": 96}
    for name, cls_, size in (("gpc_field_score_prm", g.FieldScorePrm, 64), ("gpc_field_tally", g.FieldTally, 96),
                             ("gpc_field_score", g.FieldScore, 512)):
        fields = struct_fields(header, name)
        assert [f[1] for f in fields] == [f[0] for f in cls_._fields_], name
        assert sum(width[t] * k for t, _, k in fields) == size == C.sizeof(cls_), name
        for (t, n, k), (_, ct) in zip(fields, cls_._fields_):
            assert C.sizeof(ct) == width[t] * k and getattr(cls_, n).size == width[t] * k, (name, n)
    assert [f[1] for f in struct_fields(header, "gpc_field_score_prm")] == ["n_thr", "thr_q8", "out_abs_q8", "out_rel_pm", "n_speed",
                                                                            "speed_q8", "reserved"]
    assert [f[1] for f in struct_fields(header, "gpc_field_tally")] == ["n_judged", "n_within", "n_outlier", "sum_e_q8", "sum_e2_q16"]
    assert [f[1] for f in struct_fields(header, "gpc_field_score")] == ["n_pixels", "n_ignored", "n_no_truth", "n_hole", "all", "bin"]
    assert g.FieldScore.all.offset == 8 * fu.ALL and g.FieldScore.bin.offset == 8 * fu.BIN
    d = g.FieldScorePrm()
    assert (tuple(d.thr_q8[:d.n_thr]), d.out_abs_q8, d.out_rel_pm, tuple(d.speed_q8[:d.n_speed])) == fu.DEFAULTS
    assert (d.n_thr, d.n_speed, d.reserved, tuple(d.thr_q8[3:]), tuple(d.speed_q8)) == (3, 0, 0, (0,) * 5, (0,) * 3)
    assert re.search(r"\} gpc_field_score_prm;\s*/\* documented defaults: n_thr 3, thr_q8 \{256, 768, 1280\}, out 768 / 50, n_speed 0", raw)
    for name, nargs in NAMES.items():
        assert name in g.capi.SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == nargs == len(getattr(L, name).argtypes), name
    for m in ("score_fields_device", "score_fields"):
        assert callable(getattr(g.Context, m)), m
    # the block stands behind "complete" and before "measurement"
    assert (raw.index("gpc_hip_inpaint_fields(") < raw.index("/* ---- score dense fields against ground truth") <
            raw.index("typedef struct gpc_field_score_prm") < raw.index("gpc_hip_score_fields(") < raw.index("/* ---- measurement"))


def test_the_timing_slot_table_is_as_the_parent_left_it():
    """the kernel has no slot: 32 addressed by the mask, 62 in all, k_search at 32 and k_clean_apply the last"""
    g, L = lib()
    assert L.gpc_hip_kernel_count() == 32 and L.gpc_hip_kernel_slots() == PARENT_SLOTS and L.gpc_hip_abi_version() == 1
    kernels = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_slots())]
    assert kernels[0] == "k_preprocess" and kernels[32] == "k_search" and kernels[-1] == "k_clean_apply"
    assert not any("field" in k for k in kernels)


def test_refusals_with_a_null_context():
    """without a context every call refuses before it touches anything"""
    g, L = lib()
    prm, tr = C.byref(g.FieldScorePrm()), C.byref(g.capi.Truth(4096, None, None))
    assert L.gpc_hip_score_fields_device(None, 4096, 1, 4, 4, 1, tr, prm, None, 8192, None) == g.capi.E_INVALID
    assert L.gpc_hip_score_fields(None, 4096, 1, 4, 4, 1, tr, prm, None, 8192, None) == g.capi.E_INVALID


def test_accessors():
    g, _ = lib()
    field, u, v, ignore, cls = fu.random_case(37, 29, 3, 2)
    words, _ = fu.score(field, u, v, ignore, cls, fu.DEFAULTS)
    s = g.FieldScore.from_buffer_copy(words[1].tobytes())
    want = fu.accessors(words[1])
    assert (s.epe(), s.rms(), s.outlier_rate(), s.density()) == (want["epe"], want["rms"], want["outlier_rate"], want["density"])
    assert [s.within(k) for k in range(3)] == want["within"][:3]
    assert s.n_pixels == 37 * 29 and sum(s.tally(b).n_judged for b in range(4)) == s.all.n_judged
    assert math.isclose(sum(s.density(b) for b in range(4)), s.density()) and 0 < s.density() < 1
    assert s.epe(1) == s.bin[1].sum_e_q8 / (256 * s.bin[1].n_judged) and s.rms() >= s.epe() > 0
    empty = g.FieldScore()
    assert all(math.isnan(x) for x in (empty.epe(), empty.rms(), empty.within(0), empty.outlier_rate(), empty.density()))


def test_dense_evaluation_hpp_compiles(tmp_path):
    """include/gpc/dense_evaluation.hpp compiles against the library with a plain host compiler; the program runs no device code"""
    import subprocess
    lib()
    src, exe = str(tmp_path / "dense_evaluation_check.cpp"), str(tmp_path / "dense_evaluation_check")
    with open(src, "w") as f:
        f.write("#include <gpc/dense_evaluation.hpp>\n"
                "int main() {\n"
                "  gpc::dense::Field field;\n"
                "  gpc::evaluation::Truth truth;\n"
                "  if (false) { gpc::evaluation::FieldScore q = gpc::evaluation::scoreField(field, truth); return (int)q.counts.n_pixels; }\n"
                "  const gpc_field_score_prm c = gpc::evaluation::FieldParams().toC();\n"
                "  return c.n_thr == 3 && c.thr_q8[0] == 256 && c.thr_q8[1] == 768 && c.thr_q8[2] == 1280 && c.out_abs_q8 == 768 &&\n"
                "         c.out_rel_pm == 50 && c.n_speed == 0 && c.reserved == 0 ? 0 : 1;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D_INTRINSICS_SSE", "-I", os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L", os.path.join(ROOT, "opengpc_amd"), "-lgpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "opengpc_amd"), "-pthread"])
    assert subprocess.run([exe], timeout=60).returncode == 0
