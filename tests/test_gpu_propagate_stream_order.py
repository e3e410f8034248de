"""Stream ordering of gpc_hip_propagate_fields_device on a stream borrowed from torch, through the harness of
tests/stream_order_util.py (run) as tests/test_gpu_search_stream_order.py uses it: warm-up on other data (so the workspace of
the ping-pong holds valid but wrong fields), the real inputs behind a delay on the stream, the outputs copied away on the
stream with no host wait, bytes compared with the CPU model.  The device form apart, in place (an odd N: the copy of the
field goes first), and two calls back to back."""
import numpy as np
import pytest

import propagate_util as pu
import search_util as su
import stream_order_util as so

pytestmark = pytest.mark.gpu

W, H = so.W, so.H
PRM = (2, 4, 3, 8)


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


def propagate_fields(in_place):
    def make(ctx, k):
        import opengpc_amd as g
        field, pf = su.random_fields(W, H, 1, 3, seed=40 + k), su.random_fields(W, H, 1, 3, seed=40 + so.PLACEHOLDER)
        (L, R), (pL, pR) = su.images("random", W, H, 3, 1, seed=k), su.images("random", W, H, 3, 1, seed=so.PLACEHOLDER)
        out, cost, choice, stats = pu.propagate(field, L, R, PRM)
        assert (stats[:, :, [0, 1, 3]] > 0).all()                             # every iteration of every pair moves pixels
        n = len(field)
        return so.Spec("propagate_fields_device(%s)" % ("in place" if in_place else "apart"), dict(field=(field, pf), L=(L, pL), R=(R, pR)),
                       dict(out="field" if in_place else n * H * W * 4, cost=n * H * W * 2, choice=n * H * W, stats=n * PRM[2] * 16),
                       dict(out=out, cost=cost, choice=choice, stats=stats),
                       [lambda c, p: c.propagate_fields_device(p["field"], p["L"], p["R"], 1, W, H, n, g.Propagate(*PRM), p["out"], p["cost"],
                                                               p["choice"], p["stats"])])
    return make


def test_propagate_fields(borrowed):
    ctx, st = borrowed
    so.run(ctx, st, [propagate_fields(False)(ctx, 0)])


def test_propagate_fields_in_place(borrowed):
    ctx, st = borrowed
    so.run(ctx, st, [propagate_fields(True)(ctx, 0)])


def test_propagate_fields_back_to_back(borrowed):
    """two calls with different inputs and outputs behind one delay, no wait in between: the second one's iterations reuse
    the workspace the first one's are still reading"""
    ctx, st = borrowed
    so.run(ctx, st, [propagate_fields(False)(ctx, 0), propagate_fields(False)(ctx, 1)])
