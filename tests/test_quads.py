"""CPU: the plain restatement of the quad rule (tests/quad_util.py) on hand-written cases -- each reason a circle is
rejected, one at a time, the settle rule, the tolerance at exactly tol and at tol + 1 -- and what the Python layer
declares for gpc_hip_quads_* (symbols, QUAD_DTYPE, kernel slots)."""
import ctypes as C

import numpy as np
import pytest

import quad_util as qu

W, H = 32, 20
# one circle that closes: a = (10, 5), d = 3 -> b = (7, 5); a' = (12, 6), b' = (8, 6), d' = 4 -> c' = (8, 6)
S0, S1 = (10, 5, 3.0), (12, 6, 4.0)
FL, FR = (10, 5, 12, 6), (7, 5, 8, 6)
QUAD = (10, 5, 3, 2, 1, 4, 0, 0)


def run(s0, s1, fl, fr, tol=0, nsup=None, nfl=None, nfr=None):
    sup, ns = qu.sup_array([s0, s1])
    cap_f = max(len(fl), len(fr), 1)
    a, na = qu.corr_array([fl], cap_f)
    b, nb = qu.corr_array([fr], cap_f)
    return qu.restate(sup, ns if nsup is None else nsup, a, na if nfl is None else nfl, b, nb if nfr is None else nfr, W, H, tol)[0]


def test_the_circle_closes():
    assert run([S0], [S1], [FL], [FR]) == [QUAD]
    assert qu.QUAD.itemsize == 32 and qu.SUP.itemsize == 12 and qu.CORR.itemsize == 16


@pytest.mark.parametrize("what, s0, s1, fl, fr", [
    ("support outside the image (x)", [(W, 5, 3.0)], [S1], [(W, 5, 12, 6)], [FR]),
    ("support outside the image (y)", [(10, -1, 3.0)], [S1], [(10, -1, 12, 6)], [FR]),
    ("d is NaN", [(10, 5, float("nan"))], [S1], [FL], [FR]),
    ("d is infinite", [(10, 5, float("inf"))], [S1], [FL], [FR]),
    ("d is not integral", [(10, 5, 3.5)], [S1], [FL], [(6, 5, 8, 6), (7, 5, 8, 6)]),
    ("|d| above 16384", [(10, 5, 16385.0)], [S1], [FL], [FR]),
    ("right pixel left of the row", [(10, 5, 11.0)], [S1], [FL], [(-1, 5, 8, 6), FR]),
    ("right pixel right of the row", [(10, 5, -22.0)], [S1], [FL], [(32, 5, 8, 6), FR]),
    ("no left flow from a", [S0], [S1], [(11, 5, 12, 6)], [FR]),
    ("no right flow from b", [S0], [S1], [FL], [(8, 5, 8, 6)]),
    ("left flow record with its target outside", [S0], [S1], [(10, 5, 12, H)], [FR]),
    ("right flow record with its source outside", [S0], [S1], [FL], [(7, -5, 8, 6)]),
    ("no support at a'", [S0], [(13, 6, 4.0)], [FL], [FR]),
    ("the support at a' takes no part", [S0], [(12, 6, 4.25)], [FL], [FR]),
    ("c' misses b' in x", [S0], [(12, 6, 5.0)], [FL], [FR]),
    ("c' misses b' in y", [S0], [S1], [FL], [(7, 5, 8, 7)]),
])
def test_each_rejection(what, s0, s1, fl, fr):
    assert run(s0, s1, fl, fr) == [], what


def test_counts_clip_and_negative_counts():
    assert run([S0], [S1], [FL], [FR], nsup=np.array([0, 1], np.int32)) == []
    assert run([S0], [S1], [FL], [FR], nsup=np.array([1, -3], np.int32)) == []
    assert run([S0], [S1], [FL], [FR], nfl=np.array([-1], np.int32)) == []
    assert run([S0], [S1], [FL], [FR], nfr=np.array([0], np.int32)) == []
    assert run([S0], [S1], [FL], [FR], nsup=np.array([7, 9], np.int32), nfl=np.array([5], np.int32)) == [QUAD]   # clipped to cap


def test_lowest_index_is_the_lookup():
    # two supports of the same left pixel: only the lower one is a start, and it is the one whose disparity counts
    assert run([(10, 5, 2.0), S0], [S1], [FL], [FR, (8, 5, 8, 6)]) == [(10, 5, 2, 2, 1, 4, 0, 0)]
    assert run([(10, 5, 2.0), S0], [S1], [FL], [FR]) == []              # ... even where the higher one would close
    # two flow records of the same source: the lower one is followed
    assert run([S0], [S1], [(10, 5, 1, 1), FL], [FR]) == []
    assert run([S0], [S1], [FL, (10, 5, 1, 1)], [FR]) == [QUAD]
    # two supports at a': the lower one gives d'
    assert run([S0], [(12, 6, 9.0), S1], [FL], [FR]) == []
    assert run([S0], [S1, (12, 6, 9.0)], [FL], [FR]) == [QUAD]


def test_settle_lowest_start_keeps_the_quad():
    # starts 0 and 2 both close on support 0 of frame 1 (start 1 closes on nothing): the lower start keeps its quad
    s0 = [(20, 8, 3.0), (3, 3, 1.0), S0]
    fl = [(20, 8, 12, 6), FL]
    fr = [(17, 8, 8, 6), FR]
    assert run(s0, [S1], fl, fr) == [(20, 8, 3, -8, -2, 4, 0, 0)]
    assert run(list(reversed(s0)), [S1], fl, fr) == [QUAD]
    # starts that close on nothing do not contend: the only start that closes keeps its quad, whatever its index
    assert run([(3, 3, 1.0), (3, 4, 1.0), S0], [S1], fl, fr) == [(10, 5, 3, 2, 1, 4, 2, 0)]


def test_quads_chain_over_steps():
    sup, ns = qu.sup_array([[S0], [(1, 1, 0.0), S1], [(14, 7, 5.0)]])
    fl, nfl = qu.corr_array([[FL], [(12, 6, 14, 7)]])
    fr, nfr = qu.corr_array([[FR], [(8, 6, 9, 7)]])
    got = qu.restate(sup, ns, fl, nfl, fr, nfr, W, H, 0)
    assert got == [[(10, 5, 3, 2, 1, 4, 0, 1)], [(12, 6, 4, 2, 1, 5, 1, 0)]]
    assert got[0][0][7] == got[1][0][6]


@pytest.mark.parametrize("tol", [0, 1, 3])
def test_tolerance_at_tol_and_one_beyond(tol):
    for sx in (-1, 1):
        assert run([S0], [S1], [FL], [(7, 5, 8 + sx * tol, 6)], tol) == [QUAD]
        assert run([S0], [S1], [FL], [(7, 5, 8 + sx * (tol + 1), 6)], tol) == []
        assert run([S0], [S1], [FL], [(7, 5, 8, 6 + sx * tol)], tol) == [QUAD]
        assert run([S0], [S1], [FL], [(7, 5, 8, 6 + sx * (tol + 1))], tol) == []
        assert run([S0], [S1], [FL], [(7, 5, 8 + sx * tol, 6 - sx * tol)], tol) == [QUAD]


def test_expected_arrays_leave_the_fill_behind_the_valid_quads():
    sup, ns = qu.sup_array([[S0, (20, 8, 3.0)], [S1, (22, 9, 4.0)]])
    fl, nfl = qu.corr_array([[FL, (20, 8, 22, 9)]])
    fr, nfr = qu.corr_array([[FR, (17, 8, 18, 9)]])
    for cap, rows in ((0, 0), (1, 1), (2, 2), (5, 2)):
        tab, n = qu.expected_arrays(sup, ns, fl, nfl, fr, nfr, W, H, 0, -7, cap)
        assert list(n) == [2] and tab.shape == (1, max(cap, 1))
        flat = tab.view(np.int32).reshape(-1, 8)
        assert [tuple(r) for r in flat[:rows]] == [QUAD, (20, 8, 3, 2, 1, 4, 1, 1)][:rows] and (flat[rows:] == -7).all()


def test_stereo_frames_have_the_disparity_they_claim():
    L, R = qu.stereo_frames_of(96, 64, 3, 4, 5, dy=4)
    assert L.shape == R.shape == (3, 64, 96) and L.dtype == np.uint8
    for t in range(3):
        assert np.array_equal(L[t][:, 5:], R[t][:, :-5]) and not np.array_equal(L[t], R[t])
    assert not np.array_equal(L[0], L[1])


def test_python_layer_declares_the_quad_calls():
    import opengpc_amd as g
    from opengpc_amd import build
    build.build()
    L = g.load()
    assert g.QUAD_DTYPE == qu.QUAD and g.QUAD_DTYPE.itemsize == 32
    for name in ("gpc_hip_quads_records_device", "gpc_hip_match_stereo_sequence_device", "gpc_hip_quads_sequence_device",
                 "gpc_hip_quads_records", "gpc_hip_quads_sequence"):
        assert name in g.capi.SYMBOLS and hasattr(L, name)
    for m in ("quads_records", "quads_records_device", "match_stereo_sequence_device", "quads_sequence", "quads_sequence_device"):
        assert callable(getattr(g.Context, m))
    L.gpc_hip_kernel_name.restype = C.c_char_p
    names = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_slots())]
    at = names.index("k_quad_sides")
    assert names[at:at + 7] == ["k_quad_sides", "k_quad_fill", "k_quad_scatter", "k_quad_close", "k_quad_settle", "k_quad_scan",
                                "k_quad_write"] and at >= L.gpc_hip_kernel_count() == 32
    # refused before anything touches a device: no context
    assert L.gpc_hip_quads_records(None, None, 1, None, None, None, 1, None, None, 32, 20, 2, 0, None, 0, None) == g.capi.E_INVALID
