"""The dense chain on the GPU, held to the CPU restatements as a whole (tests/dense_chain_util.py): every stage against its
rule on the field the stage before it actually produced; the whole chain from the images alone against chain_cpu, which
starts from the CPU oracle's matches; the conditions of tests/test_dense_chain.py again on the GPU's own arrays; the composite
entry points against the CPU, not against another GPU run; the chain in place; the scores of the four stage fields; one
context revisited with other shapes, channel counts and middle stages; the chain on a borrowed stream without a wait between
the stages.  Every comparison is exact: the rules are made of integers."""
import numpy as np
import pytest

import dense_chain_util as dc
import pyramid_util as pu
import stream_order_util as so

pytestmark = pytest.mark.gpu

CONFIGS = [(C, W, H) for C in (1, 2) for W, H in dc.SHAPES]
# the middle stage, the cross-check, paths: the aggregation in all four directions and in one
CHAINS = [("search", True, 15), ("search", False, 15), ("aggregate", True, 15), ("aggregate", False, 15), ("aggregate", True, 2)]


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def run(c, C, W, H, middle, check, paths=15, **kw):
    c.load_forest(pu.FORESTS[dc.FOREST], dc.match_width(W), H)
    return dc.chain_gpu(c, C, W, H, middle, check, paths, **kw)


@pytest.mark.parametrize("middle,check,paths", CHAINS)
@pytest.mark.parametrize("C,W,H", CONFIGS)
def test_every_stage_follows_its_rule_on_what_the_stage_before_it_left(ctx, C, W, H, middle, check, paths):
    """for every stage k the GPU's outputs equal restatement k of the GPU's read-back outputs of stage k - 1, the first link
    being the refinement and the fill of the GPU's own match records: a failure names the one stage at fault"""
    got = run(ctx, C, W, H, middle, check, paths)
    sc = dc.scene(C, W, H, dc.SEEDS[(C, W, H)])
    seen = set()
    for stage, want in dc.links(dict(got), sc, C, middle, check, paths):
        dc.same(got, want, "%s of (C %d, %d x %d, %s, check %s, paths %d)" % (stage, C, W, H, middle, check, paths))
        seen |= set(want)
    assert seen | {"rec", "cnt"} == set(got)


@pytest.mark.parametrize("middle,check,paths", CHAINS + [(None, True, 15)])
@pytest.mark.parametrize("C,W,H", CONFIGS)
def test_from_the_images_alone(ctx, C, W, H, middle, check, paths):
    """every intermediate of the GPU chain equals chain_cpu's, which started from the oracle's matches.  The fill is compared
    too: the device writes its records in the oracle's order (tests/test_gpu_sequence.py, tests/test_gpu_parity.py hold it to
    that), and the records are compared here first."""
    got, want = run(ctx, C, W, H, middle, check, paths), dc.chain_cpu(C, W, H, middle, check, paths)
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    first = ["cnt", "rec", "ref", "fill_fwd", "level"]
    dc.same(got, want, "from the images (C %d, %d x %d, %s, check %s, paths %d)" % (C, W, H, middle, check, paths),
            first + sorted(set(want) - set(first)))


@pytest.mark.parametrize("middle", ["search", "aggregate"])
@pytest.mark.parametrize("C,W,H", CONFIGS)
def test_the_conditions_hold_on_the_arrays_of_the_gpu(ctx, C, W, H, middle):
    """tests/test_dense_chain.py's conditions, on what the GPU produced: a change in the matcher cannot silently empty a case"""
    got = run(ctx, C, W, H, middle, True)
    cond = dc.conditions(got, C, W, H, middle, True)
    assert len(cond) >= 25 and not [k for k, v in cond.items() if not v], [k for k, v in cond.items() if not v]
    other = run(ctx, C, W, H, "aggregate" if middle == "search" else "search", True, scores=False)
    both = (got["mid_fwd_choice"] != 255) & (other["mid_fwd_choice"] != 255)
    assert (both & (got["mid_fwd_choice"] != other["mid_fwd_choice"])).any() and not np.array_equal(got["clean_out"], other["clean_out"])


def composite(c, form, C, W, H, check):
    """one composite call with every output it offers -> name (as chain_cpu names it) -> array"""
    import torch
    fill, mid, clean, inp = dc.params(form if form != "inpaint" else None, check)
    sc = dc.scene(C, W, H, dc.SEEDS[(C, W, H)])
    names = dict(out="clean_out", state="clean_state", label="clean_label", stats="clean_stats", level="level", counts="cnt")
    if form == "inpaint":
        names.update(fwd="fill_fwd", done="done_out", pas="done_pass", fill_stats="done_stats")
    else:
        names.update(fwd="mid_fwd", cost="mid_fwd_cost")
    B = {k: dc.filled(dc.nbytes(C, W, H, n)) for k, n in names.items()}
    p = {k: t.data_ptr() for k, t in B.items()}
    d_L = dc.dev(sc["frames"] if C == 2 else sc["imgL"])
    d_R = dc.dev(sc["imgR"])
    img = (d_L.data_ptr(), W, H, dc.P + 1) if C == 2 else (d_L.data_ptr(), d_R.data_ptr(), W, H, dc.P)
    s = dc.settings(C)
    torch.cuda.synchronize()
    if form == "inpaint":
        fn = c.inpaint_sequence_device if C == 2 else c.inpaint_batch_device
        fn(*img, s, fill, clean, inp, p["done"], p["pas"], p["fill_stats"], p["out"], p["state"], p["label"], p["stats"], p["fwd"], p["level"],
           dc.RADIUS, p["counts"])
    else:
        fn = getattr(c, "%s_%s_device" % (form, "sequence" if C == 2 else "batch"))
        fn(*img, s, fill, mid, clean, p["out"], p["state"], p["label"], p["stats"], p["fwd"], p["level"], dc.RADIUS, p["counts"], 0, p["cost"])
    c.synchronize()
    return {n: dc.typed(n, B[k].cpu().numpy(), C, W, H) for k, n in names.items()}


@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("form", ["search", "aggregate", "inpaint"])
@pytest.mark.parametrize("C,W,H", [(1,) + dc.SHAPES[0], (2,) + dc.SHAPES[0]])
def test_composite_entry_points_against_the_cpu(ctx, C, W, H, form, check):
    """search_, aggregate_ and inpaint_batch_device (C = 1) and _sequence_device (C = 2, the frames of pair t being t and
    t + 1): out, state, label, stats, fwd, level, cost, counts -- and the completer's out, pass and stats -- equal chain_cpu's
    arrays.  A convention that the composite and the single calls share, such as the sign of a flipped disparity or which
    image guides which direction, cannot hide here: the other side is the CPU.  At 96 x 64 only: the composites match at the
    size they fill at, and the matcher refuses a width that is no multiple of 16 (test_composites_refuse_130_columns)."""
    ctx.load_forest(pu.FORESTS[dc.FOREST], W, H)
    got = composite(ctx, form, C, W, H, check)
    want = dc.chain_cpu(C, W, H, form if form != "inpaint" else None, check)
    dc.same(got, want, "%s_%s_device (%d x %d, check %s)" % (form, "sequence" if C == 2 else "batch", W, H, check), sorted(got))


def test_composites_refuse_130_columns(ctx):
    """why test_composite_entry_points_against_the_cpu has one shape: GPC_E_INVALID for a width of 130, and not a byte written"""
    import opengpc_amd as g
    W, H = dc.SHAPES[1]
    fill, mid, clean, inp = dc.params("search", True)
    ctx.load_forest(pu.FORESTS[dc.FOREST], dc.match_width(W), H)
    d_img, d_out = dc.filled(3 * W * H), dc.filled(dc.nbytes(2, W, H, "clean_out"))
    for call in (lambda: ctx.search_batch_device(d_img.data_ptr(), d_img.data_ptr() + W * H, W, H, dc.P, dc.settings(1), fill, mid, clean, d_out.data_ptr()),
                 lambda: ctx.search_sequence_device(d_img.data_ptr(), W, H, dc.P + 1, dc.settings(2), fill, mid, clean, d_out.data_ptr())):
        with pytest.raises(g.GpcError) as e:
            call()
        assert e.value.status == g.capi.E_INVALID
    ctx.synchronize()
    assert bool((d_out == dc.FILL).all())


@pytest.mark.parametrize("middle", ["search", "aggregate"])
@pytest.mark.parametrize("C,W,H", CONFIGS)
def test_in_place(ctx, C, W, H, middle):
    """search or aggregate, the flip and the completion writing over their inputs (the cleaner may not): the same bytes at the
    end, and in every buffer that is not written over"""
    got, want = run(ctx, C, W, H, middle, True, in_place=True), dc.chain_cpu(C, W, H, middle, True)
    names = ["cnt", "level", "mid_fwd", "mid_bwd", "rec_bwd", "ref_bwd", "clean_state", "clean_label", "clean_stats", "done_out", "done_pass",
             "done_stats"] + [n for n in want if n.startswith(("mid_fwd_", "mid_bwd_"))]
    dc.same(got, want, "in place (C %d, %d x %d, %s)" % (C, W, H, middle), names)
    assert np.array_equal(got["fill_fwd"], want["mid_fwd"]) and np.array_equal(got["clean_out"], want["done_out"])     # written over


@pytest.mark.parametrize("C,W,H", CONFIGS)
def test_scores_of_the_four_stage_fields(ctx, C, W, H):
    """score_fields_device over the filled, the searched, the cleaned and the completed field equals field_score_util on the
    field read back: classes and (C = 2, without classes) speed bins, the error plane included"""
    got = run(ctx, C, W, H, "aggregate", True)
    sc = dc.scene(C, W, H, dc.SEEDS[(C, W, H)])
    for n in dc.FIELDS:
        words, err = dc.stage_score(got[n], sc)
        dc.same(got, {"score_" + n: words, "err_" + n: err}, "scores of %s (C %d, %d x %d)" % (n, C, W, H))
        assert words[:, dc.fs.BIN].min() > 0 and words[:, dc.fs.BIN + dc.fs.TALLY].min() > 0 and (err != 0xFFFF).any() and (err == 0xFFFF).any()
        if C == 2:
            dc.same(got, {"speed_" + n: dc.stage_score(got[n], sc, True)[0]}, "scores by speed of %s (%d x %d)" % (n, W, H))


@pytest.mark.parametrize("budget", [None, "1"])
@pytest.mark.parametrize("first", [(1, "aggregate"), (2, "search")])
def test_one_context_revisited(monkeypatch, first, budget):
    """one context: the 130 x 67 chain, the 96 x 64 chain, the 130 x 67 chain with the other channel count and the other
    middle stage, then the first again -- after the stages have sized their per-context blocks for a larger shape, a smaller
    one, and another layout.  Every run equals chain_cpu, that is what a fresh context gives.  budget: GPC_HIP_AGG_GROUP_BYTES
    (read when the context is made) small enough that the aggregation works a pair at a time."""
    import opengpc_amd as g
    if budget is None:
        monkeypatch.delenv("GPC_HIP_AGG_GROUP_BYTES", raising=False)
    else:
        monkeypatch.setenv("GPC_HIP_AGG_GROUP_BYTES", budget)
    C, middle = first
    other = (3 - C, "search" if middle == "aggregate" else "aggregate")
    c = g.Context(0)
    try:
        for k, (Cn, mid, (W, H)) in enumerate(((C, middle, dc.SHAPES[1]), (C, middle, dc.SHAPES[0]), other + (dc.SHAPES[1],),
                                               (C, middle, dc.SHAPES[1]))):
            got = run(c, Cn, W, H, mid, True, scores=False)
            dc.same(got, dc.chain_cpu(Cn, W, H, mid, True), "visit %d (C %d, %d x %d, %s, budget %s)" % (k, Cn, W, H, mid, budget), sorted(got))
    finally:
        c.close()


def test_on_a_borrowed_stream_without_a_wait_between_the_stages():
    """the single-call chain (C = 1, 96 x 64, search, the cross-check on) through stream_order_util.run: the images arrive
    behind a delay on a stream set with set_stream, the calls are queued back to back with no wait between them, the outputs
    are copied away in stream order and everything is overwritten behind that copy; a warm-up run on another scene has left
    every per-context block holding valid but wrong state.  The bytes equal chain_cpu's."""
    import torch
    import opengpc_amd as g
    C, W, H = 1, so.W, so.H
    assert (W, H) == dc.SHAPES[0] and so.FILL == dc.FILL
    seed = dc.SEEDS[(C, W, H)]
    sc, warm = dc.scene(C, W, H, seed), dc.scene(C, W, H, seed + 1)
    want = dc.chain_cpu(C, W, H, "search", True)
    outs, calls = dc.chain_calls(C, W, H, "search", True)
    zeros = lambda a: np.zeros_like(a)
    inputs = {k: (sc[n], zeros(sc[n]), warm[n]) for k, n in (("L", "imgL"), ("R", "imgR"), ("ign", "ignore"), ("cls", "cls"))}
    plain = lambda call: lambda c, p: call(c, dict(p, mL=p["L"], mR=p["R"]))      # 96 is a multiple of 16: the matcher reads the images themselves
    inputs["u"] = (sc["u"], zeros(sc["u"]), warm["u"] + np.float32(1))
    spec = so.Spec("the dense chain, call by call", inputs, {n: dc.nbytes(C, W, H, n) for n in outs}, {n: want[n] for n in outs},
                   [plain(call) for call in calls], forest=dc.FOREST)
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    c = g.Context(0)
    try:
        c.set_stream(st.cuda_stream)
        so.run(c, st, [spec])
    finally:
        st.synchronize()
        c.set_stream(None)
        c.close()
