"""The dense chain on the CPU (tests/dense_chain_util.py): the scenes meet the conditions under which the GPU comparisons of
tests/test_gpu_dense_chain.py prove something -- the chain's own data reaches the places the stages' synthetic generators
avoid -- and chain_cpu is a pure function of the scene.  The scene seeds (dense_chain_util.SEEDS) were tuned until every
condition holds; the conditions were not."""
import numpy as np
import pytest

import dense_chain_util as dc
import search_util as su

CONFIGS = [(C, W, H) for C in (1, 2) for W, H in dc.SHAPES]


@pytest.mark.parametrize("C,W,H", CONFIGS)
def test_scenes(C, W, H):
    """deterministic by seed; two layers that differ in every component the field has, none of them zero; truth, ignored
    pixels, pixels without truth and both occlusion classes"""
    a = dc.scene(C, W, H, dc.SEEDS[(C, W, H)])
    b = dc.scene.__wrapped__(C, W, H, dc.SEEDS[(C, W, H)])
    other = dc.scene(C, W, H, dc.SEEDS[(C, W, H)] + 1)
    for k in ("imgL", "imgR", "u", "v", "ignore", "cls"):
        if a[k] is not None:
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") and a[k].shape == (dc.P, H, W), k
    assert not np.array_equal(a["imgL"], other["imgL"])
    for t in range(dc.P):
        for truth in (a["u"][t], a["v"][t]) if C == 2 else (a["u"][t],):
            vals = np.unique(truth[np.isfinite(truth)])
            assert len(vals) == 2 and (vals != 0).all(), vals
            if C == 1:
                assert 2 <= vals[0] <= 4 and 7 <= vals[1] <= 10, vals
        assert np.isnan(a["u"][t]).any() and a["ignore"][t].any() and (a["cls"][t] == 1).any() and (a["cls"][t] == 0).any()
    if C == 2:
        assert np.array_equal(a["frames"][:-1], a["imgL"]) and np.array_equal(a["frames"][1:], a["imgR"])


@pytest.mark.parametrize("middle", ["search", "aggregate"])
@pytest.mark.parametrize("C,W,H", CONFIGS)
def test_the_chain_reaches_what_the_generators_avoid(C, W, H, middle):
    """Every condition of dense_chain_util.conditions() on chain_cpu's arrays, the cross-check on:
    the fill writes Q8 parts in 101 .. 127 and in 129 .. 155 in every channel (where sr_whole and the cleaner's rounding turn);
    search and aggregate write kept values whose low byte is exactly 128, of both signs -- the rule allows it for a kept pixel:
    q = (256 |n| + a) div (2 a) with n = c_m - c_p and a = c_m + c_p - 2 c_0 reaches 128 when |n| = a, that is when the
    winner's cost ties with ONE neighbour's (c_0 = c_p < c_m), which the tie-break order of the candidates permits;
    adjacent live pixels of the prior differ in their whole-pixel base by exactly 2R + 1, by exactly 2R + 2 and by more
    (horizontally and vertically: the clamp of the label shift), some pixels have no target inside the image;
    the cleaner, with dense_chain_util.CLEAN_PRM = (256, 256, 24, 1) -- the defaults but for speckle_min, 64 by default --
    keeps pixels, fails pixels at the cross-check, removes speckles, and its median changes a kept value;
    the completer, with INPAINT_PRM = (2, 3, 512, 3), fills holes in a pass after the first, leaves holes, and meets a hole on
    the edge of a 32 x 32 tile;
    the scorer sees judged, ignored and no-truth pixels and both occlusion classes in all four stage fields, holes in the
    cleaned and the completed field (the fill at max_level 15 leaves none, and the middle stage only where no target lies
    inside the image), and with C = 2 two speed bins."""
    res = dc.chain_cpu(C, W, H, middle, True)
    cond = dc.conditions(res, C, W, H, middle, True)
    assert len(cond) >= 25
    missing = [k for k, v in cond.items() if not v]
    assert not missing, missing
    for n in ("clean_out", "done_out"):
        assert "score %s: holes" % n in cond
    st = res["clean_stats"].sum(0)
    print("clean: kept, holes, failed check, speckles", st.tolist(), "complete: filled, left", res["done_stats"].sum(0).tolist())


@pytest.mark.parametrize("C,W,H", CONFIGS)
def test_the_middle_stage_matters(C, W, H):
    """some pixel's winner under the aggregation is not the search's, and the two chains differ behind the cleaner: a test
    that passes with one middle stage says nothing about the other"""
    s, a = dc.chain_cpu(C, W, H, "search", True), dc.chain_cpu(C, W, H, "aggregate", True)
    for n in ("rec", "ref", "fill_fwd", "fill_bwd", "level"):
        assert np.array_equal(s[n], a[n]), n                                 # the same prior
    both = (s["mid_fwd_choice"] != 255) & (a["mid_fwd_choice"] != 255)
    assert (both & (s["mid_fwd_choice"] != a["mid_fwd_choice"])).any()
    assert not np.array_equal(s["clean_out"], a["clean_out"]) and not np.array_equal(s["done_out"], a["done_out"])
    one = dc.chain_cpu(C, W, H, "aggregate", True, 4)                        # a single direction is not all four
    assert not np.array_equal(one["mid_fwd"], a["mid_fwd"])


@pytest.mark.parametrize("C,W,H", CONFIGS)
def test_without_the_backward_direction_and_without_a_middle_stage(C, W, H):
    """the other chains the GPU tests run: the cross-check off (no backward arrays at all, no pixel fails the check), and no
    middle stage (the chain of inpaint_batch_device and inpaint_sequence_device)"""
    off = dc.chain_cpu(C, W, H, "search", False)
    assert not [n for n in off if "bwd" in n] and (off["clean_stats"][:, 2] == 0).all() and (off["clean_stats"][:, 0] > 0).all()
    on = dc.chain_cpu(C, W, H, "search", True)
    assert np.array_equal(off["mid_fwd"], on["mid_fwd"]) and not np.array_equal(off["clean_out"], on["clean_out"])
    bare = dc.chain_cpu(C, W, H, None, True)
    assert not [n for n in bare if n.startswith("mid_")] and np.array_equal(bare["fill_fwd"], on["fill_fwd"])
    cond = dc.conditions(bare, C, W, H, None, True)
    assert not [k for k, v in cond.items() if not v and k.startswith(("clean", "complete"))], cond


@pytest.mark.parametrize("C,W,H", CONFIGS[1:3])
def test_chain_cpu_is_a_pure_function(C, W, H):
    """two calls give equal arrays, and the inputs are as they were"""
    seed = dc.SEEDS[(C, W, H)]
    sc = dc.scene(C, W, H, seed)
    before = {k: np.array(v) for k, v in sc.items() if isinstance(v, np.ndarray)}
    rec, cnt = (np.array(a) for a in dc.oracle_matches(C, W, H, seed))
    first = dc.chain_cpu.__wrapped__(C, W, H, "aggregate", True, 15, seed)
    second = dc.chain_cpu.__wrapped__(C, W, H, "aggregate", True, 15, seed)
    assert sorted(first) == sorted(second) and len(first) > 30
    dc.same(first, second, "the second call")
    for k, v in before.items():
        assert np.array_equal(v, sc[k], equal_nan=v.dtype.kind == "f"), k
    again = dc.oracle_matches(C, W, H, seed)
    assert np.array_equal(rec.view(np.uint8), again[0].view(np.uint8)) and np.array_equal(cnt, again[1])
    assert (cnt > 50).all() and (cnt < dc.cap_of(W, H)).all()


def test_links_read_what_they_are_given():
    """links() over a dict that already holds a stage's output checks the NEXT stage against that output: a wrong fill is
    reported by the fill's link, and every later link follows the wrong fill instead of repeating the complaint"""
    C, W, H = 1, 96, 64
    sc = dc.scene(C, W, H, dc.SEEDS[(C, W, H)])
    good = dc.chain_cpu(C, W, H, "search", True)
    got = {n: np.array(a) for n, a in good.items()}
    got["fill_fwd"][0, 0, 5, 5] += 256 * 3
    wrong = [stage for stage, want in dc.links(got, sc, C, "search", True, 15) if any(not np.array_equal(got[n], want[n]) for n in want)]
    assert wrong[0] == "fill" and "search" in wrong and "fill, backward" not in wrong and "flip" not in wrong
    assert su.NONE == dc.NONE
