"""Stream ordering of every *_device entry point on a stream borrowed from torch (gpc_hip_set_stream), as include/gpc_hip.h
promises it: the call only queues work on the context's stream (the device-wide matchers wait once on the host inside the
call), reads what that stream has produced when the call is made, and its outputs may be read behind any wait on the stream.

Every case (tests/stream_order_util.py: run) warms up on another data set of the same shape, so that every workspace of the
context holds valid but wrong state, starts with valid but wrong data in every device input, queues a delay and then
the real inputs on the stream, calls the entry point while the delay still runs, copies the outputs away on the stream with
no host wait, overwrites inputs and outputs behind that copy, waits for the torch stream alone and compares the copies with
the CPU models (oracle.pyoracle, the *_util.py restatements), byte for byte.  A launch on another stream, a blocking copy,
a count read on the host too early, an input read by a later call or a workspace reused before the call in flight has
finished with it all show as a wrong byte or a failed premise.  The premises are asserted in every case: the stream is
still busy immediately before the call, and -- for the entry points documented to only queue work -- immediately after it.

Not covered, on purpose: switching streams while work is in flight (the header says the caller waits for the old stream
first), and the record forms on the context's own stream behind an event of another stream: the Python wrapper has no call
that makes the own stream wait on an event."""
import pytest

import stream_order_util as so

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("name", sorted(so.RECORD_FORMS))
def test_record_form(borrowed, name):
    """the record forms: pure functions of device arrays, documented to only queue work"""
    ctx, st = borrowed
    so.run(ctx, st, [so.RECORD_FORMS[name](ctx, 0)])


@pytest.mark.parametrize("name", sorted(so.IMAGE_FORMS))
def test_image_form(borrowed, name):
    """the image forms with the zero forest, the three matcher modes of match_batch_device with the tau forest as well; the
    device-wide matchers (epipolar_mode = 0 or use_hashtable = 1) wait on the host inside the call and are held to the first
    premise only"""
    ctx, st = borrowed
    so.run(ctx, st, [so.IMAGE_FORMS[name](ctx, 0)])


@pytest.mark.parametrize("name", sorted(so.RECORD_FORMS) + ["match_batch_epipolar"])
def test_back_to_back(borrowed, name):
    """two calls with different inputs and different outputs, queued one behind the other behind one delay with no wait in
    between: the workspaces they share are handed from one call to the next in stream order"""
    ctx, st = borrowed
    make = so.RECORD_FORMS.get(name) or so.IMAGE_FORMS[name]
    so.run(ctx, st, [make(ctx, 0), make(ctx, 1)])
