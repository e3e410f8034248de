"""Stream ordering of gpc_hip_gapfill_fields_device on a stream borrowed from torch, through the harness of
tests/stream_order_util.py (run) as tests/test_gpu_propagate_stream_order.py uses it: warm-up on other data (so the distance
planes of the workspace hold valid but wrong distances), the real inputs behind a delay on the stream, the outputs copied
away on the stream with no host wait, bytes compared with the CPU model.  The device form apart, in place, and two calls back
to back."""
import pytest

import gapfill_util as gu
import stream_order_util as so

pytestmark = pytest.mark.gpu

W, H = so.W, so.H
PRM = (8, 255, 1, 1)


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


def gapfill_fields(in_place):
    def make(ctx, k):
        import opengpc_amd as g
        (field, guide), (pf, pg) = gu.case("runs", W, H, 3, 1, seed=40 + k), gu.case("runs", W, H, 3, 1, seed=40 + so.PLACEHOLDER)
        out, how, stats = gu.gapfill(field, guide, PRM)
        assert (stats > 0).all()                                              # every pair fills holes of every kind and leaves some
        n = len(field)
        return so.Spec("gapfill_fields_device(%s)" % ("in place" if in_place else "apart"), dict(field=(field, pf), guide=(guide, pg)),
                       dict(out="field" if in_place else n * H * W * 4, how=n * H * W, stats=n * 16), dict(out=out, how=how, stats=stats),
                       [lambda c, p: c.gapfill_fields_device(p["field"], p["guide"], 1, W, H, n, g.Gapfill(*PRM), p["out"], p["how"],
                                                             p["stats"])])
    return make


def test_gapfill_fields(borrowed):
    ctx, st = borrowed
    so.run(ctx, st, [gapfill_fields(False)(ctx, 0)])


def test_gapfill_fields_in_place(borrowed):
    ctx, st = borrowed
    so.run(ctx, st, [gapfill_fields(True)(ctx, 0)])


def test_gapfill_fields_back_to_back(borrowed):
    """two calls with different inputs and outputs behind one delay, no wait in between: the second one's scans write the
    distance planes the first one's choice is still reading"""
    ctx, st = borrowed
    so.run(ctx, st, [gapfill_fields(False)(ctx, 0), gapfill_fields(False)(ctx, 1)])
