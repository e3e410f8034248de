"""CPU: the scanline aggregation's two restatements (tests/aggregate_util.py) agree on small cases; the two identities of the
rule hold against search_util.search; a path value stays below 2^16 at p2 = 32767 on a worst-case pair; the crafted scene
does what tests/test_gpu_aggregate.py claims of it; the bindings' struct and defaults; the slot table is as it was."""
import ctypes as C
import os

import numpy as np
import pytest

import aggregate_util as au
import search_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("Cn", [1, 2])
@pytest.mark.parametrize("R", [0, 1, 2])
def test_the_two_restatements_agree(Cn, R):
    """numpy across a scanline front against one pixel at a time, the minimum over all pairs taken literally"""
    for W, H in ((1, 1), (1, 6), (6, 1), (2, 2), (9, 7), (13, 5)):
        field, L, Rr = au.stepped_case(W, H, 1, Cn, R)
        for radius, subpixel, max_cost, p1, p2, paths in ((1, 1, 0xFFFF, 5, 40, 15), (2, 0, 900, 3, 3, 1), (1, 1, 0xFFFF, 0, 32767, 2),
                                                          (1, 1, 0xFFFF, 7, 9, 4), (1, 0, 0xFFFF, 1, 100, 8), (1, 1, 2000, 4, 4, 0)):
            prm = (radius, R, subpixel, max_cost, p1, p2, paths)
            out, cost, choice, stats, agg = au.aggregate(field, L, Rr, prm)
            p_out, p_cost, p_choice, p_state, p_agg = au.aggregate_plain(field[0], L[0], Rr[0], prm)
            what = (Cn, R, W, H, prm)
            assert np.array_equal(out[0], p_out) and np.array_equal(cost[0], p_cost) and np.array_equal(choice[0], p_choice), what
            assert np.array_equal(agg[0], p_agg), what
            assert stats[0].tolist() == [int((p_state == k).sum()) for k in range(4)], what


def test_the_stepped_prior_steps_as_it_says():
    """neighbouring bases differ by 0, 1, R, 2R, 2R + 1 and more, in both directions; holes, targets outside, the extremes"""
    for Cn in (1, 2):
        field = au.stepped_case(70, 45, 3, Cn, 2)[0]
        valued, r, bx, by = su.base(field[0])
        both = valued[:, 1:] & valued[:, :-1]
        dxs = set(np.abs(r[0][:, 1:] - r[0][:, :-1])[both].tolist())
        both = valued[1:] & valued[:-1]
        dys = set(np.abs(r[Cn - 1][1:] - r[Cn - 1][:-1])[both].tolist())
        for d in (dxs, dys):
            assert {0, 1, 2, 4, 5, 6, 9} <= d, sorted(d)
        assert (~valued).any() and (valued & ((bx < 0) | (bx >= 70))).any()
        assert (field == su.IMAX).any() and (field == su.IMIN1).any()


@pytest.mark.parametrize("Cn", [1, 2])
def test_identities_against_the_search(Cn):
    """paths = 0 (any p1, p2) and p1 = p2 = 0 (any paths): out, cost, choice and stats are the search's"""
    for kind in su.KINDS:
        for W, H, P in su.SIZES[:4]:
            field, L, R = su.case(kind, W, H, P, Cn)
            for radius, rng_, subpixel, max_cost in ((2, 1, 1, 0xFFFF), (1, 2, 1, 3000), (4, 0, 0, 0xFFFF)):
                want = su.expected(kind, W, H, P, Cn, (radius, rng_, subpixel, max_cost))
                for p1, p2, paths in ((8, 32, 0), (0, 32767, 0), (0, 0, 15), (0, 0, 1), (0, 0, 6)):
                    got = au.expected_search_case(kind, W, H, P, Cn, (radius, rng_, subpixel, max_cost, p1, p2, paths))
                    for g_, w in zip(got[:4], want):
                        assert g_.dtype == w.dtype and np.array_equal(g_, w), (kind, W, H, Cn, radius, rng_, p1, p2, paths)
                    matched = want[1] != 0xFFFF
                    dirs = bin(paths).count("1") or 1
                    assert np.array_equal(got[4][matched], dirs * want[1][matched].astype(np.uint32)) and (got[4][~matched] == au.NO_AGG).all()


def test_a_path_value_stays_below_two_to_the_sixteen():
    """black against white at radius 4: every cost is 81 * 255 = 20655; a checkered prior makes every neighbour's band miss
    this pixel's, so every step adds p2 = 32767: L = 53422 on every path, the sum of four below 2^18"""
    W, H = 12, 9
    L, R = np.zeros((1, H, W), np.uint8), np.full((1, H, W), 255, np.uint8)
    ys, xs = np.mgrid[0:H, 0:W]
    for Cn in (1, 2):
        field = np.zeros((1, Cn, H, W), np.int32)
        off = 4 * ((xs + ys) % 2) * np.where(xs < W // 2, 1, -1)             # the target's offset: every target inside
        field[0, 0] = 256 * (-off if Cn == 1 else off)
        info = {}
        out, cost, choice, stats, agg = au.aggregate(field, L, R, (4, 1, 1, 0xFFFF, 32767, 32767, 15), info)
        assert info["max_L"] == 20655 + 32767 < 2 ** 16
        assert (cost == 20655).all() and agg.max() == 4 * (20655 + 32767) < 2 ** 18
        assert agg[0, 0, 0] == 2 * 20655 + 2 * (20655 + 32767)              # a corner: two of its four paths start there


def test_the_crafted_scene():
    """the hand-written winners of tests/test_gpu_aggregate.py, on the CPU first: the search keeps the prior where the costs
    tie, the aggregated choice follows the neighbours"""
    field, L, R = au.scene()
    prm = au.SCENE_PRM
    grid = su.cost_grid(field[0], L[0], R[0], prm[0], prm[1])
    c = grid[0][1:4]                                                          # [kx + 1][y][x]: the three labels' costs
    assert (c[:, :, 7:11] == 0).all()                                         # all three tie at 0 in the band's middle
    assert (c[:2, :, 11] == 0).all() and (c[2, :, 11] > 0).all()              # and the first two in column 11
    assert (c[0][:, 2:20] == 0).all() and (c[1][:, 2:7] > 0).all() and (c[1][:, 12:19] > 0).all()
    s_choice = su.search(field, L, R, prm[:4])[2]
    a_choice = au.aggregate(field, L, R, prm)[2]
    assert (s_choice[0] == np.array(au.SEARCH_WINNERS, np.uint8)).all() and (a_choice[0] == np.array(au.AGGREGATE_WINNERS, np.uint8)).all()


def test_bindings_struct_and_defaults():
    import opengpc_amd as g
    a = g.Aggregate()
    assert C.sizeof(g.Aggregate) == 28
    assert (a.radius, a.range, a.subpixel, a.max_cost, a.p1, a.p2, a.paths) == au.DEFAULTS
    s = g.Search()
    assert (a.radius, a.range, a.subpixel, a.max_cost) == (s.radius, s.range, s.subpixel, s.max_cost)
    b = g.Aggregate(1, 2, 0, 100, 3, 4, 5)
    assert (b.radius, b.range, b.subpixel, b.max_cost, b.p1, b.p2, b.paths) == (1, 2, 0, 100, 3, 4, 5)
    for name in ("gpc_hip_aggregate_fields_device", "gpc_hip_aggregate_batch_device", "gpc_hip_aggregate_sequence_device",
                 "gpc_hip_aggregate_fields"):
        assert name in g.capi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "gpc_hip.h")).read()
    for name in ("gpc_hip_aggregate_fields_device", "gpc_hip_aggregate_fields", "typedef struct gpc_aggregate"):
        assert name in header


def test_the_slot_table_is_unchanged():
    """the new kernels launch outside the timing slots: 32 kernels, 62 slots, as before"""
    import opengpc_amd as g
    L = g.capi.load()
    assert L.gpc_hip_kernel_count() == 32 and L.gpc_hip_kernel_slots() == 62
    names = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_slots())]
    assert not any("agg" in n for n in names) and "k_search" in names
    for name in ("gpc_hip_aggregate_fields_device", "gpc_hip_aggregate_fields"):
        assert hasattr(L, name)
