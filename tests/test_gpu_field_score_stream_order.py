"""Stream ordering of gpc_hip_score_fields_device on a stream borrowed from torch, through the harness of
tests/stream_order_util.py (run) as tests/test_gpu_search_stream_order.py uses it: warm-up on other data, the real inputs
behind a delay on the stream, the outputs copied away on the stream with no host wait, bytes compared with the model
(tests/field_score_util.py).  Alone, and two calls back to back into different score arrays."""
import pytest

import field_score_util as fu
import stream_order_util as so

pytestmark = pytest.mark.gpu

W, H, P = so.W, so.H, 3
PRM = (fu.DEFAULTS[0], 768, 50, fu.SINTEL_SPEED)


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


def score_fields(ctx, k):
    import opengpc_amd as g
    field, u, v, ignore, cls = fu.random_case(W, H, P, 2, seed=40 + k)
    pf, pu, pv, pi, pc = fu.random_case(W, H, P, 2, seed=40 + so.PLACEHOLDER)
    words, err = fu.score(field, u, v, ignore, cls, PRM)
    assert (words[:, :4] > 0).all() and (words[:, fu.BIN::fu.TALLY] > 0).all()
    return so.Spec("score_fields_device", dict(field=(field, pf), u=(u, pu), v=(v, pv), ign=(ignore, pi), cls=(cls, pc)),
                   dict(scores=P * 512, err=P * H * W * 2), dict(scores=words, err=err),
                   [lambda c, p: c.score_fields_device(p["field"], 2, W, H, P, p["u"], p["v"], p["ign"], g.FieldScorePrm(*PRM[:3], PRM[3]),
                                                       p["scores"], p["cls"], p["err"])])


def test_score_fields(borrowed):
    ctx, st = borrowed
    so.run(ctx, st, [score_fields(ctx, 0)])


def test_score_fields_back_to_back(borrowed):
    """two calls with different inputs and outputs behind one delay, no wait in between"""
    ctx, st = borrowed
    so.run(ctx, st, [score_fields(ctx, 0), score_fields(ctx, 1)])
