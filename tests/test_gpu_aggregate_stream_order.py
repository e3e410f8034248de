"""Stream ordering of the gpc_hip_aggregate_*_device entry points on a stream borrowed from torch, through the harness of
tests/stream_order_util.py (run) as tests/test_gpu_search_stream_order.py uses it: warm-up on other data, the real inputs
behind a delay on the stream, the outputs copied away on the stream with no host wait, bytes compared with the CPU models.
aggregate_fields_device (alone, in place, and two calls back to back -- the second reuses the first's workspace),
aggregate_batch_device and aggregate_sequence_device; the expected bytes of the match forms are the models' chain: the
oracle's records, refine_util, dense_util, aggregate_util, clean_util."""
import numpy as np
import pytest

import aggregate_util as au
import clean_util as cu
import dense_util as du
import refine_util as ru
import search_util as su
import stream_order_util as so

pytestmark = pytest.mark.gpu

W, H, B, P = so.W, so.H, so.B, so.P
PRM = (2, 1, 1, 3000, 8, 32, 15)


@pytest.fixture(scope="module")
def borrowed():
    import torch
    import opengpc_amd as g
    c = g.Context(0)
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    c.set_stream(st.cuda_stream)
    yield c, st
    st.synchronize()
    c.set_stream(None)
    c.close()


def aggregate_fields(in_place):
    def make(ctx, k):
        import opengpc_amd as g
        field, pf = su.random_fields(W, H, 1, 3, seed=40 + k), su.random_fields(W, H, 1, 3, seed=40 + so.PLACEHOLDER)
        (L, R), (pL, pR) = su.images("random", W, H, 3, 1, seed=k), su.images("random", W, H, 3, 1, seed=so.PLACEHOLDER)
        out, cost, choice, stats, agg = au.aggregate(field, L, R, PRM)
        assert (stats[:, :3] > 0).all() and stats[:, 3].sum() > 0
        n = len(field)
        return so.Spec("aggregate_fields_device(%s)" % ("in place" if in_place else "apart"), dict(field=(field, pf), L=(L, pL), R=(R, pR)),
                       dict(out="field" if in_place else n * H * W * 4, cost=n * H * W * 2, choice=n * H * W, stats=n * 16, agg=n * H * W * 4),
                       dict(out=out, cost=cost, choice=choice, stats=stats, agg=agg),
                       [lambda c, p: c.aggregate_fields_device(p["field"], p["L"], p["R"], 1, W, H, n, g.Aggregate(*PRM), p["out"],
                                                               p["cost"], p["choice"], p["stats"], p["agg"])])
    return make


def chain(rec, cnt, imgL, imgR, corr):
    """the models' chain behind the match forms: refine, fill, aggregate; flip, fill, aggregate with the images exchanged; clean"""
    ref, _ = ru.expected_arrays(rec, cnt, imgL, imgR, so.RADIUS, 0)
    for t, m in enumerate(ru.m_of(cnt, so.CAP)):
        ref[t, m:] = np.zeros(1, ru.REFINEMENT)[0]
    fwd, level = du.densify(rec, cnt, W, H, du.DEFAULTS, ref)
    fwd, cost = au.aggregate(fwd, imgL, imgR, au.DEFAULTS)[:2]
    r_rec, r_ref = cu.flip(rec, cnt, ref, rec, ref)
    bwd, _ = du.densify(r_rec, cnt, W, H, du.DEFAULTS, r_ref)
    bwd = au.aggregate(bwd, imgR, imgL, au.DEFAULTS)[0]
    out, state, label, stats = cu.clean(fwd, bwd, cu.DEFAULTS)
    assert (stats[:, 0] > 0).all()
    return dict(out=out, state=state, label=label, stats=stats, fwd=fwd, level=level, cost=cost)


def sizes(n, Cn):
    return dict(out=n * Cn * H * W * 4, state=n * H * W, label=n * H * W * 4, stats=n * 16, fwd=n * Cn * H * W * 4, level=n * H * W,
                cost=n * H * W * 2, cnt=n * 4)


def aggregate_batch(ctx, k):
    import opengpc_amd as g
    (rec, cnt), (L, R) = so.sup_in(k), so.pairs(k)
    want = dict(chain(rec, cnt, L, R, False), cnt=cnt, nc=so.match("pairs", k)[1])
    return so.Spec("aggregate_batch_device", so.image_inputs(k), dict(sizes(B, 1), nc=B * 8), want,
                   [lambda c, p: c.aggregate_batch_device(p["L"], p["R"], W, H, B, so.settings(), g.Densify(), g.Aggregate(), g.Clean(), p["out"],
                                                          p["state"], p["label"], p["stats"], p["fwd"], p["level"], so.RADIUS, p["cnt"], p["nc"],
                                                       p["cost"])], forest="zero")


def aggregate_sequence(ctx, k):
    import opengpc_amd as g
    (rec, cnt), F = so.corr_in(k), so.frames(k)
    want = dict(chain(rec, cnt, F[:-1], F[1:], True), cnt=cnt, nc=so.flow("frames", k)[1])
    return so.Spec("aggregate_sequence_device", so.image_inputs(k, "frames"), dict(sizes(P, 2), nc=so.N * 4), want,
                   [lambda c, p: c.aggregate_sequence_device(p["F"], W, H, so.N, so.settings(), g.Densify(), g.Aggregate(), g.Clean(), p["out"],
                                                             p["state"], p["label"], p["stats"], p["fwd"], p["level"], so.RADIUS, p["cnt"],
                                                          p["nc"], p["cost"])], forest="zero")


def test_aggregate_fields(borrowed):
    ctx, st = borrowed
    so.run(ctx, st, [aggregate_fields(False)(ctx, 0)])


def test_aggregate_fields_in_place(borrowed):
    ctx, st = borrowed
    so.run(ctx, st, [aggregate_fields(True)(ctx, 0)])


def test_aggregate_fields_back_to_back(borrowed):
    """two calls with different inputs and outputs behind one delay, no wait in between"""
    ctx, st = borrowed
    so.run(ctx, st, [aggregate_fields(False)(ctx, 0), aggregate_fields(False)(ctx, 1)])


def test_aggregate_batch(borrowed):
    ctx, st = borrowed
    so.run(ctx, st, [aggregate_batch(ctx, 0)])


def test_aggregate_sequence(borrowed):
    ctx, st = borrowed
    so.run(ctx, st, [aggregate_sequence(ctx, 0)])
