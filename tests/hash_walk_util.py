"""Inputs, launch-plan arithmetic and runners of the tile-walk tests (test_gpu_hash_walk.py, test_hash_walk_inputs.py).

k_hash (k_hash_body.h) walks `tpw` vertically adjacent tiles of TY rows per workgroup.  The shapes here give that walk two to
five tiles with a ragged last one under both tile heights, and three inputs per shape place the texture so that the walk's
accumulators are fed by one end of it only:

  a  texture everywhere;
  b  texture in rows 0 .. 39 only (77 below): the candidates end inside the first tile, whichever its height;
  c  texture from row max(55, H - 46) on only (77 above): no candidate in the first tile, the last tile holds the last ones.

Under the SSE arithmetic rows H - 15 and H - 14 are candidates that are never hashed (gpcFilterSegment(13, height - 15)): their
code is 0, a whole row of them shares one key, and the sort matcher drops a key that occurs twice on the left.  Row H - 14
is a tile of its own at H = 91 and H = 155 with 32-row tiles, and a join that stops short of it (a wrong LASTROW) loses
nothing unless the row holds a support.  So inputs a and c of the SSE arithmetic are flattened in their last 15 rows but for
a few columns: the left image keeps its texture left of column 10 -- the one candidate of row H - 14 is x = 13 (a Sobel
decision shows at two pixels, x = 12 falls to the margin) -- and the right image in columns 20 .. 22, which gives the
candidates x = 22 and 23.  Two equal keys at the very end of the sorted targets match a unique source key (the reference's
lower bound never looks at the last target and skips the uniqueness test one before it, inference.hpp:243-249), so the
pair has exactly one support in row H - 14.  The SSE=OFF arithmetic hashes row H - 14 like any other and needs none of this.

conditions() asserts on the oracle's result alone what keeps a degenerate input from passing."""
import numpy as np

from devicewide_util import FILL32, R, compare, expected, filled, supp_words

HT_X = 256
SHAPES = tuple((W, H) for H in (91, 122, 155) for W in (96, 272))
TPWS = (1, 2, 3, 4, 5, 64)
KINDS = ("a", "b", "c")
FLAT = 77
B_END = 40            # input b: the first constant row
THR = 5
# (seed, disparity) of the two pairs of every input, found on the CPU so that conditions() holds for every forest the tests use
PAIRS = ((1, 9), (4, 13))


def c_start(H):
    return max(55, H - 46)


# ------------------------------------------------------------------------------------------------------------ launch plan
def tiles(H, ty):
    return -(-(H - 2 * R) // ty)


def tile_rows(H, ty):
    """[first row, end row) of every tile: the candidate rows 13 .. H - 14 in steps of ty"""
    return [(R + k * ty, min(R + (k + 1) * ty, H - R)) for k in range(tiles(H, ty))]


def split(ntiles, tpw):
    """tiles of each workgroup of a column"""
    tpw = min(tpw, ntiles)
    return [min(tpw, ntiles - k) for k in range(0, ntiles, tpw)]


def plan(W, H, nimg, ty, tpw, cus):
    """what gpc_hip_hash_plan reports for a launch with `tpw` forced: restated from the shape alone"""
    per_col = len(split(tiles(H, ty), tpw))
    nwg = -(-W // HT_X) * per_col * nimg
    return (ty, min(tpw, tiles(H, ty)), per_col, max(nwg - 2 * cus, 0))


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ----------------------------------------------------------------------------------------------------------------- inputs
def walk_pair(W, H, kind, seed, D, naive=False):
    from opengpc_amd.synth import synth_pair
    L, Rr = (a.copy() for a in synth_pair(W, H, seed, D))
    for img in (L, Rr):
        if kind == "b":
            img[B_END:] = FLAT
        if kind == "c":
            img[:c_start(H)] = FLAT
    if kind != "b" and not naive:
        L[H - 15:, 10:] = FLAT
        Rr[H - 15:, :20] = FLAT
        Rr[H - 15:, 23:] = FLAT
    return L, Rr


def walk_pairs(W, H, kind, naive=False):
    return [walk_pair(W, H, kind, s, D, naive) for s, D in PAIRS]


def cand_rows(case, i):
    """candidate rows of the left and the right image of pair i"""
    return [m // case.W for _, m in case.hashed[i]]


def conditions(case, kind, supports, what):
    """supports: per pair the oracle's records.  Raises unless the input does what its kind is for."""
    H = case.H
    for i, w in enumerate(supports):
        sy = np.asarray(w["y"])
        rows = cand_rows(case, i)
        assert len(sy) > 0, "%s, pair %d: no supports" % (what, i)
        if kind == "a":
            for ty in (32, 40):
                for y0, y1 in tile_rows(H, ty):
                    assert all(((r >= y0) & (r < y1)).any() for r in rows), "%s, pair %d: no candidate in rows %d .. %d" % (what, i, y0, y1 - 1)
                    assert ((sy >= y0) & (sy < y1)).any(), "%s, pair %d: no support in rows %d .. %d" % (what, i, y0, y1 - 1)
        if kind == "b":
            assert all(r.max() < R + 32 for r in rows), "%s, pair %d: a candidate below the first tile" % (what, i)
        if kind == "c":
            assert (sy == H - R - 1).any(), "%s, pair %d: no support in row %d" % (what, i, H - R - 1)
            assert all(r.min() >= R + 40 for r in rows), "%s, pair %d: a candidate in the first tile" % (what, i)
            assert all(r.max() == H - R - 1 for r in rows), "%s, pair %d: no candidate in row %d" % (what, i, H - R - 1)


# ---------------------------------------------------------------------------------------------------------------- runners
def launch_batch(ctx, c, settings, cap):
    """gpc_hip_match_batch_device on filled outputs: the raw words of (records [B + 1, cap, 3], counts [B + 1],
    candidate counts [B + 1, 2]) -- a spare pair's worth behind the batch"""
    import torch
    dev = torch.device("cuda", 0)
    B = c.B
    d_L, d_R = torch.from_numpy(c.L).to(dev), torch.from_numpy(c.R).to(dev)
    d_out, d_cnt, d_nc = filled((B + 1) * cap * 12, dev), filled((B + 1) * 4, dev), filled((B + 1) * 8, dev)
    torch.cuda.synchronize(dev)  # (the library's stream does not wait for torch's)
    ctx.match_batch_device(d_L.data_ptr(), d_R.data_ptr(), c.W, c.H, B, settings, d_out.data_ptr(), cap, d_cnt.data_ptr(), d_nc.data_ptr())
    ctx.synchronize()
    return (d_out.cpu().numpy().view(np.uint32).reshape(B + 1, cap, 3), d_cnt.cpu().numpy().view(np.int32),
            d_nc.cpu().numpy().view(np.int32).reshape(B + 1, 2))


def check_batch(got, wants, what):
    """wants: per pair (records, candidates left, candidates right).  Counts, candidate counts, every record, and the fill
    in every slot behind min(count, cap)."""
    out, cnt, nc = got
    B = len(wants)
    for i, (w, nl, nr) in enumerate(wants):
        assert tuple(nc[i]) == (nl, nr), "%s: pair %d: candidates %s, the oracle's %s" % (what, i, tuple(nc[i]), (nl, nr))
        assert cnt[i] == len(w), "%s: pair %d counts %d supports, the oracle %d" % (what, i, cnt[i], len(w))
    assert cnt[B:].view(np.uint32) == FILL32 and (nc[B:].view(np.uint32) == FILL32).all(), what + ": a count behind the batch's was written"
    words = [supp_words(w[0]) for w in wants]
    compare(out, expected(words, out.shape[1]), words, what)


def same_across(results, what):
    """results: {tpw: tuple of arrays}.  Every tpw's bytes against the first's: the walk must not show in the results."""
    keys = list(results)
    for k in keys[1:]:
        for a, b in zip(results[keys[0]], results[k]):
            assert np.array_equal(a, b), "%s: differs between tpw %s and %s (%d words)" % (what, keys[0], k, int((np.asarray(a) != np.asarray(b)).sum()))
