"""Stream ordering of the gpc_hip_inpaint_*_device entry points on a stream borrowed from torch, through the harness of
tests/stream_order_util.py (run) as tests/test_gpu_stream_order.py uses it: warm-up on other data, the real inputs behind a
delay on the stream, the outputs copied away on the stream with no host wait, bytes compared with the CPU models.  The
harness takes new forms as Spec objects, so it is used as it is.  inpaint_fields_device (alone, and two calls back to back,
which share the pass plane and the control words of the context) and inpaint_batch_device; the sequence form runs the same
host code behind clean_match and has no CPU model of its cleaned field in the harness, so it is left to
tests/test_gpu_inpaint.py."""
import numpy as np
import pytest

import inpaint_util as iu
import stream_order_util as so

pytestmark = pytest.mark.gpu

W, H, B = so.W, so.H, so.B


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


def inpaint_fields(ctx, k):
    import opengpc_amd as g
    field, pf = so.fields(k)[0], so.fields(so.PLACEHOLDER)[0]            # [3, 1, H, W]: random values and holes
    guide, pg = iu.guides("random", W, H, 3, seed=k), iu.guides("random", W, H, 3, seed=so.PLACEHOLDER)
    out, pz, stats = iu.inpaint(field, guide, iu.DEFAULTS)
    assert (stats[:, 0] > 0).any()
    n = len(field)
    return so.Spec("inpaint_fields_device", dict(field=(field, pf), guide=(guide, pg)), dict(out=n * H * W * 4, pz=n * H * W, stats=n * 8),
                   dict(out=out, pz=pz, stats=stats),
                   [lambda c, p: c.inpaint_fields_device(p["field"], p["guide"], 1, W, H, n, g.Inpaint(), p["out"], p["pz"], p["stats"])])


def inpaint_batch(ctx, k):
    import opengpc_amd as g
    base = so.clean_batch(ctx, k)                                          # the cleaned field and everything before it, from the CPU models
    cleaned = np.ascontiguousarray(base.want["out"]).view(np.int32).reshape(B, 1, H, W)
    out, pz, stats = iu.inpaint(cleaned, so.pairs(k)[0], iu.DEFAULTS)
    assert ((cleaned[:, 0] == iu.NONE).sum((1, 2)) > 0).all() and (stats[:, 0] > 0).all()
    sizes = dict(base.outputs, cleaned=B * H * W * 4, pz=B * H * W, fstats=B * 8)
    want = dict(base.want, out=out, cleaned=cleaned, pz=pz, fstats=stats)
    return so.Spec("inpaint_batch_device", base.inputs, sizes, want,
                   [lambda c, p: c.inpaint_batch_device(p["L"], p["R"], W, H, B, so.settings(), g.Densify(), g.Clean(), g.Inpaint(), p["out"],
                                                        p["pz"], p["fstats"], p["cleaned"], p["state"], p["label"], p["stats"], p["fwd"],
                                                        p["level"], so.RADIUS, p["cnt"], p["nc"])], forest="zero")


def test_inpaint_fields(borrowed):
    ctx, st = borrowed
    so.run(ctx, st, [inpaint_fields(ctx, 0)])


def test_inpaint_fields_back_to_back(borrowed):
    """two calls with different inputs and outputs behind one delay, no wait in between: the pass plane and the control words
    are handed from one call to the next in stream order"""
    ctx, st = borrowed
    so.run(ctx, st, [inpaint_fields(ctx, 0), inpaint_fields(ctx, 1)])


def test_inpaint_batch(borrowed):
    ctx, st = borrowed
    so.run(ctx, st, [inpaint_batch(ctx, 0)])
