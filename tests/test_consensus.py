"""CPU: the grid motion consensus rule (gpc_hip_consensus_*) as tests/consensus_util.py restates it -- the numpy form equals
the all-pairs form, the inequality is strict at an exact tie, the shifted grids only add bits, alpha 0 keeps what takes
part -- and its declarations in the Python binding."""
import ctypes as C

import numpy as np

import consensus_util as cu


def random_records(rng, W, H, m, corr):
    """clustered motion plus outliers, some records outside the image, supports with d that is no whole number"""
    if corr:
        r = np.zeros(m, cu.CORR)
        r["src_x"], r["src_y"] = rng.integers(-2, W + 2, m), rng.integers(-2, H + 2, m)
        coherent = rng.random(m) < 0.6
        r["tar_x"] = np.where(coherent, r["src_x"] + 9, rng.integers(-2, W + 2, m))
        r["tar_y"] = np.where(coherent, r["src_y"] - 5, rng.integers(-2, H + 2, m))
    else:
        r = np.zeros(m, cu.SUPPORT)
        r["x"], r["y"] = rng.integers(-2, W + 2, m), rng.integers(-2, H + 2, m)
        coherent = rng.random(m) < 0.6
        r["d"] = np.where(coherent, 7.0, rng.integers(-W, W, m)).astype(np.float32)
        r["d"][rng.integers(0, m, 4)] = (0.5, np.nan, np.inf, -np.inf)
    return r


def test_numpy_form_equals_all_pairs_form():
    rng = np.random.default_rng(3)
    for W, H, cell, m in ((72, 50, 8, 300), (16, 16, 16, 40), (40, 16, 16, 60), (33, 47, 6, 200), (64, 64, 4, 250)):
        for corr in (True, False):
            for alpha in ((6, 1), (3, 2), (0, 1), (1, 1)):
                r = random_records(rng, W, H, m, corr)
                prm = cu.Params(cell, 4, *alpha)
                fast, slow = cu.keep_of_pair(r, W, H, prm), cu.brute_keep(r, W, H, prm)
                assert np.array_equal(fast, slow), (W, H, cell, corr, alpha)
                if alpha == (1, 1):
                    assert 0 < np.count_nonzero(fast) < m


def coherent_block(n):
    """n records whose sources lie in the interior cell (2, 2) of a 5x5 grid of 16-pixel cells, all moving by (+16, 0)"""
    r = np.zeros(n, cu.CORR)
    r["src_x"], r["src_y"] = 32 + np.arange(n), 40
    r["tar_x"], r["tar_y"] = r["src_x"] + 16, 40
    return r


def test_the_inequality_is_strict_at_a_tie():
    prm = cu.Params(16, 1, 6, 1)
    ok, S, T, k = cu.brute_counts(coherent_block(4), 80, 80, prm, 0)
    assert all(ok) and S == [4] * 4 and T == [4] * 4 and k == [9] * 4      # 16 * 9 == 36 * 4: a tie
    assert not cu.keep_of_pair(coherent_block(4), 80, 80, prm).any()
    assert not cu.brute_keep(coherent_block(4), 80, 80, prm).any()
    assert (cu.keep_of_pair(coherent_block(5), 80, 80, prm) == 1).all()     # 25 * 9 > 36 * 5
    assert (cu.brute_keep(coherent_block(5), 80, 80, prm) == 1).all()


def test_bit_0_of_four_grids_is_the_single_grid():
    rng = np.random.default_rng(8)
    seen = set()
    for corr in (True, False):
        r = random_records(rng, 72, 50, 400, corr)
        one = cu.keep_of_pair(r, 72, 50, cu.Params(8, 1, 2, 1))
        four = cu.keep_of_pair(r, 72, 50, cu.Params(8, 4, 2, 1))
        assert np.array_equal(four & 1, one) and one.max() <= 1
        seen |= set(four.tolist())
    assert len(seen) > 4 and max(seen) > 1          # the shifted grids decide differently for some records


def test_alpha_zero_keeps_what_takes_part():
    rng = np.random.default_rng(9)
    for corr in (True, False):
        r = random_records(rng, 72, 50, 300, corr)
        ok = cu.ends(r, 72, 50)[0]
        assert 0 < ok.sum() < len(r)
        assert np.array_equal(cu.keep_of_pair(r, 72, 50, cu.Params(8, 1, 0, 1)), ok.astype(np.uint8))
        assert np.array_equal(cu.keep_of_pair(r, 72, 50, cu.Params(8, 4, 0, 7)), ok.astype(np.uint8) * 15)


def test_binding_declares_the_struct_and_the_entry_points():
    import opengpc_amd as g
    assert C.sizeof(g.Consensus) == 16
    d = g.Consensus()
    assert (d.cell, d.shifts, d.alpha_num, d.alpha_den) == (16, 4, 6, 1)
    assert [f[0] for f in g.Consensus._fields_] == ["cell", "shifts", "alpha_num", "alpha_den"]
    names = ["gpc_hip_consensus_supports_device", "gpc_hip_consensus_correspondences_device", "gpc_hip_consensus_batch_device",
             "gpc_hip_consensus_sequence_device", "gpc_hip_consensus_supports", "gpc_hip_consensus_correspondences"]
    from opengpc_amd import build
    build.build()
    L = g.load()
    for n in names:
        assert n in g.capi.SYMBOLS and getattr(L, n).argtypes is not None, n
    assert len(L.gpc_hip_consensus_supports_device.argtypes) == 13 and len(L.gpc_hip_consensus_batch_device.argtypes) == 13
    kernels = [L.gpc_hip_kernel_name(i).decode() for i in range(L.gpc_hip_kernel_count())]
    for k in ("k_cons_cells", "k_cons_scan", "k_cons_scatter", "k_cons_count", "k_cons_blocks", "k_cons_write"):
        assert k in kernels
    assert cu.CORR == g.CORR_DTYPE and cu.SUPPORT == g.SUPPORT_DTYPE
