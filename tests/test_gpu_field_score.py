"""The dense field scorer on the GPU (gpc_hip_score_fields*): every byte of gpc_field_score and of the error plane EQUALS
the restatement of the rule (tests/field_score_util.py), for C = 1 and 2 -- the scores start out filled with a sentinel
(the call clears them) and so does the error plane (every element must be written) -- at 1 x 1, 5 x 3, 37 x 29 with three
pairs (an odd plane misaligns pairs 1 and 2), 64 x 48, 130 x 70 and 512 x 260 with two pairs (several workgroups feed one
pair); device form and host form, with and without the error plane, the class plane, the ignore mask and speed bins; every
plane offset by one element so that the element-wise path runs on even planes too; the crafted pixels of
field_score_util.crafted under every parameter set; the refusals; the identities; one end-to-end case over
search_batch_device with the fields kept on the device."""
import ctypes as C

import numpy as np
import pytest

import field_score_util as fu

pytestmark = pytest.mark.gpu

FILL = 0xA5
SPEED_PRM = (fu.DEFAULTS[0], 768, 50, fu.SINTEL_SPEED)


@pytest.fixture(scope="module")
def ctx():
    import opengpc_amd as g
    c = g.Context(0)
    yield c
    c.close()


def P_(prm):
    import opengpc_amd as g
    return g.FieldScorePrm(prm[0], prm[1], prm[2], prm[3])


def dev(a, lead=0):
    """a copy on the device behind `lead` spare elements: (the tensor that owns it, the pointer of the first element)"""
    import torch
    if a is None:
        return None, 0
    flat = np.concatenate([np.zeros(lead, a.dtype), np.ascontiguousarray(a).reshape(-1)])
    t = torch.from_numpy(flat.view(np.uint8).copy()).to(torch.device("cuda", 0))
    return t, t.data_ptr() + lead * a.dtype.itemsize


def score_device(ctx, case, prm, with_ign=True, with_cls=False, with_err=True, lead=0):
    """the device form: (words [P, 64], err [P, H, W] or None) read back from sentinel-filled arrays"""
    import torch
    field, u, v, ignore, cls = case
    P, Cn, H, W = field.shape
    keep = [dev(field, lead), dev(u, lead), dev(v, lead), dev(ignore if with_ign else None, lead), dev(cls if with_cls else None, lead)]
    d_scores = torch.full((P * 512,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
    d_err = torch.full(((P * H * W + lead) * 2,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.score_fields_device(keep[0][1], Cn, W, H, P, keep[1][1], keep[2][1], keep[3][1], P_(prm), d_scores.data_ptr(), keep[4][1],
                            d_err.data_ptr() + 2 * lead if with_err else 0)
    ctx.synchronize()
    err = d_err.cpu().numpy().view(np.uint16)
    assert (err[:lead] == FILL * 257).all()
    if not with_err:
        assert (err == FILL * 257).all()
    return d_scores.cpu().numpy().view(np.int64).reshape(P, 64), err[lead:].reshape(P, H, W) if with_err else None


def score_host(ctx, case, prm, with_ign=True, with_cls=False, with_err=True):
    field, u, v, ignore, cls = case
    scores, err = ctx.score_fields(field, u, v, ignore if with_ign else None, P_(prm), cls if with_cls else None, want_err=with_err)
    return np.frombuffer(bytes(scores), np.int64).reshape(len(field), 64), err


def same(got, want, what):
    for n, g_, w in zip(("scores", "err"), got, want):
        if g_ is None:
            continue
        assert g_.dtype == w.dtype and g_.shape == w.shape, (what, n)
        if not np.array_equal(g_, w):
            bad = np.argwhere(g_ != w)
            raise AssertionError("%s: %s differs at %d of %d elements, the first at %s: %s, expected %s" % (
                what, n, len(bad), w.size, bad[0].tolist(), g_[tuple(bad[0])], w[tuple(bad[0])]))


def model(case, prm, with_ign=True, with_cls=False):
    field, u, v, ignore, cls = case
    return fu.score(field, u, v, ignore if with_ign else None, cls if with_cls else None, prm)


@pytest.mark.parametrize("size", fu.SIZES)
@pytest.mark.parametrize("Cn", [1, 2])
def test_every_byte_equals_the_rule(ctx, Cn, size):
    W, H, P = size
    case = fu.random_case(W, H, P, Cn)
    for prm, with_cls in ((fu.DEFAULTS, False), (fu.DEFAULTS, True), (SPEED_PRM, False), (fu.CRAFT_PRMS[3], True)):
        want = model(case, prm, True, with_cls)
        for with_err in (True, False):
            same(score_device(ctx, case, prm, True, with_cls, with_err), want, ("device", size, Cn, prm, with_cls, with_err))
            same(score_host(ctx, case, prm, True, with_cls, with_err), want, ("host", size, Cn, prm, with_cls, with_err))
    same(score_device(ctx, case, fu.DEFAULTS, with_ign=False), model(case, fu.DEFAULTS, False), ("no ignore mask", size, Cn))
    same(score_host(ctx, case, fu.DEFAULTS, with_ign=False), model(case, fu.DEFAULTS, False), ("host, no ignore mask", size, Cn))


@pytest.mark.parametrize("size", [(5, 3, 1), (37, 29, 3), (64, 48, 1), (130, 70, 2)])
@pytest.mark.parametrize("Cn", [1, 2])
def test_planes_offset_by_one_element(ctx, Cn, size):
    """every pointer one element (three for good measure) behind an allocation's start: no plane lies on a 16-byte boundary,
    on even planes too, and the bytes are the same"""
    W, H, P = size
    case = fu.random_case(W, H, P, Cn)
    for lead in (1, 3):
        for prm, with_cls in ((fu.DEFAULTS, False), (SPEED_PRM, False), (fu.DEFAULTS, True)):
            same(score_device(ctx, case, prm, True, with_cls, True, lead), model(case, prm, True, with_cls), ("lead", lead, size, Cn, with_cls))


def test_planes_of_differing_phase(ctx):
    """only the truth plane is offset: the field goes by vector loads and the truth element by element within one slot"""
    import torch
    for Cn in (1, 2):
        field, u, v, ignore, cls = fu.random_case(64, 48, 1, Cn)
        want = fu.score(field, u, v, ignore, cls, fu.DEFAULTS)
        f, tu, tv, ti, tc = dev(field), dev(u, 1), dev(v, 2 if v is not None else 0), dev(ignore, 3), dev(cls, 1)
        d_scores = torch.full((512,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
        d_err = torch.full((64 * 48 + 1, 2), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
        ctx.score_fields_device(f[1], Cn, 64, 48, 1, tu[1], tv[1], ti[1], P_(fu.DEFAULTS), d_scores.data_ptr(), tc[1], d_err.data_ptr() + 2)
        ctx.synchronize()
        got = d_scores.cpu().numpy().view(np.int64).reshape(1, 64), d_err.cpu().numpy().view(np.uint16).reshape(-1)[1:].reshape(1, 48, 64)
        same(got, want, ("differing phase", Cn))


@pytest.mark.parametrize("Cn", [1, 2])
def test_crafted_pixels(ctx, Cn):
    """the square root at and beside squares up to 2^32, the clamps, thresholds met exactly, truth that is none, at the bound
    and on a rounding tie, the order of the classification, the ends of int32, both outlier inequalities at equality and a
    step either side, speed bounds met exactly, classes 3, 4 and 255; the pixel is named where a byte differs"""
    field, u, v, ignore, cls, notes = fu.crafted(Cn)
    case = (field, u, v, ignore, cls)
    for prm in fu.CRAFT_PRMS:
        for with_cls in (False, True):
            want = model(case, prm, True, with_cls)
            for lead in (0, 1):
                got = score_device(ctx, case, prm, True, with_cls, True, lead)
                bad = np.flatnonzero(got[1][0, 0] != want[1][0, 0])
                assert len(bad) == 0, (prm, with_cls, lead, [(notes[i], int(got[1][0, 0, i]), int(want[1][0, 0, i])) for i in bad[:5]])
                same(got, want, ("crafted", Cn, prm, with_cls, lead))
            same(score_host(ctx, case, prm, True, with_cls), want, ("crafted, host", Cn, prm, with_cls))
    # pixel by pixel, so that a wrong count names its pixel: every crafted pixel alone as a 1 x 1 field
    prm = fu.CRAFT_PRMS[3]
    for i in range(0, len(notes), 7):
        one = tuple(None if a is None else np.ascontiguousarray(a[..., i:i + 1]) for a in case)
        same(score_device(ctx, one, prm, True, True), model(one, prm, True, True), ("alone", notes[i]))


def test_identities_on_random_inputs(ctx):
    for Cn in (1, 2):
        case = fu.random_case(130, 70, 2, Cn, seed=5)
        for prm, with_cls in ((fu.DEFAULTS, True), (SPEED_PRM, False), (fu.DEFAULTS, False)):
            words, _ = score_device(ctx, case, prm, True, with_cls)
            assert (words[:, 0] == 130 * 70).all() and (words[:, 0] == words[:, 1:4].sum(axis=1) + words[:, fu.ALL]).all()
            assert np.array_equal(words[:, fu.BIN:].reshape(2, 4, fu.TALLY).sum(axis=1), words[:, fu.ALL:fu.BIN])
            assert (words[:, fu.ALL] > 0).all()


def test_no_leak_between_pairs_and_inputs_untouched(ctx):
    case = fu.random_case(37, 29, 3, 2)
    whole = score_device(ctx, case, SPEED_PRM)
    for t in range(3):
        one = tuple(None if a is None else a[t:t + 1] for a in case)
        got = score_device(ctx, one, SPEED_PRM)
        assert np.array_equal(got[0], whole[0][t:t + 1]) and np.array_equal(got[1], whole[1][t:t + 1])
    d = [dev(a) for a in case]
    import torch
    d_scores = torch.zeros(3 * 512, dtype=torch.uint8, device=torch.device("cuda", 0))
    ctx.score_fields_device(d[0][1], 2, 37, 29, 3, d[1][1], d[2][1], d[3][1], P_(fu.DEFAULTS), d_scores.data_ptr(), d[4][1], 0)
    ctx.synchronize()
    for (t, _), a in zip(d, case):
        assert np.array_equal(t.cpu().numpy(), np.ascontiguousarray(a).view(np.uint8).reshape(-1))


def test_refusals(ctx):
    """every refusal of the rule with a live context; nothing is written"""
    import torch
    import opengpc_amd as g
    L, E, U = ctx.L, g.capi.E_INVALID, g.capi.E_UNSUPPORTED
    case = fu.random_case(5, 3, 1, 2)
    (tf, f), (tu, u), (tv, v), (ti, i), (tc, c) = [dev(a) for a in case]
    d_scores = torch.full((512,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
    s = d_scores.data_ptr()
    ok = g.FieldScorePrm()

    def call(fn=L.gpc_hip_score_fields_device, field=f, Cn=2, W=5, H=3, P=1, tr=(u, v, i), prm=ok, cls=c, scores=s, err=None, h=ctx.h):
        t = None if tr is None else C.byref(g.capi.Truth(*[p or None for p in tr]))
        return fn(h, C.c_void_p(field or None), Cn, W, H, P, t, None if prm is None else C.byref(prm), C.c_void_p(cls or None),
                  C.c_void_p(scores or None), err)

    assert call() == 0
    ctx.synchronize()
    d_scores.fill_(FILL)
    torch.cuda.synchronize()
    host = [np.ascontiguousarray(a) for a in case]
    h_scores = np.full(512, FILL, np.uint8)
    hp = [a.ctypes.data for a in host]
    for fn, kw in ((L.gpc_hip_score_fields_device, {}),
                   (L.gpc_hip_score_fields, dict(field=hp[0], tr=(hp[1], hp[2], hp[3]), cls=hp[4], scores=h_scores.ctypes.data))):
        tr = kw.get("tr", (u, v, i))
        bad = g.FieldScorePrm
        for what, st, a in (
                ("null field", E, dict(field=0)), ("null truth", E, dict(tr=None)), ("null u", E, dict(tr=(0, tr[1], tr[2]))),
                ("null prm", E, dict(prm=None)), ("null scores", E, dict(scores=0)), ("three channels", E, dict(Cn=3)),
                ("no channel", E, dict(Cn=0)), ("v missing with C = 2", E, dict(tr=(tr[0], 0, tr[2]))),
                ("v given with C = 1", E, dict(Cn=1)), ("width 0", E, dict(W=0)), ("height -1", E, dict(H=-1)), ("no pair", E, dict(P=0)),
                ("width beyond the limit", U, dict(W=32769, H=1)), ("height beyond the limit", U, dict(W=1, H=32769)),
                ("too many pairs", U, dict(P=65536)),
                ("n_thr 9", E, dict(prm=bad(n_thr=9))), ("n_thr -1", E, dict(prm=bad(n_thr=-1))),
                ("threshold beyond 65535", E, dict(prm=bad((256, 65536)))), ("threshold below 0", E, dict(prm=bad((-1,)))),
                ("out_abs beyond 65535", E, dict(prm=bad(out_abs_q8=65536))), ("out_abs below 0", E, dict(prm=bad(out_abs_q8=-1))),
                ("out_rel beyond 255", E, dict(prm=bad(out_rel_pm=256))), ("out_rel below 0", E, dict(prm=bad(out_rel_pm=-1))),
                ("n_speed 4", E, dict(prm=bad(n_speed=4))), ("n_speed -1", E, dict(prm=bad(n_speed=-1))),
                ("speed beyond 2^23", E, dict(prm=bad(speed_q8=(2 ** 23 + 1,)))), ("speed below 0", E, dict(prm=bad(speed_q8=(-1,)))),
                ("speeds descending", E, dict(prm=bad(speed_q8=(10, 9)))), ("reserved set", E, dict(prm=bad(reserved=1)))):
            assert call(fn, **dict(kw, **a)) == st, (fn.__name__, what)
        # what is allowed: the bounds themselves, equal speeds, entries out of range beyond those in use
        for what, a in (("bounds", bad((0, 65535), 65535, 255, (0, 2 ** 23, 2 ** 23))), ("nothing in use", bad((), 0, 0, ())),
                        ("unused entries", bad((256, -5, 10 ** 6), n_thr=1, speed_q8=(7, -1), n_speed=1))):
            assert call(fn, **dict(kw, prm=a)) == 0, (fn.__name__, what)
            ctx.synchronize()
        d_scores.fill_(FILL)
        h_scores[:] = FILL
        torch.cuda.synchronize()
        assert call(fn, **dict(kw, P=0)) == E
        ctx.synchronize()
        assert (d_scores.cpu().numpy() == FILL).all() and (h_scores == FILL).all()
    assert L.gpc_hip_score_fields_device(None, C.c_void_p(f), 2, 5, 3, 1, C.byref(g.capi.Truth(u, v, i)), C.byref(ok), None, C.c_void_p(s), None) == E


def test_a_searched_field_kept_on_the_device(ctx):
    """end to end: search_batch_device on synthetic pairs of constant disparity, forward field and cleaned field left on the
    device and scored there against the constant truth; the scores equal the model's over the bytes copied back"""
    import os
    import torch
    import opengpc_amd as g
    from opengpc_amd import synth
    W, H, B, disp = 96, 64, 2, 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ctx.load_forest(os.path.join(root, "forests", "defaultZeroForest.txt"), W, H)
    pairs = [synth.synth_pair(W, H, 10 + t, disp) for t in range(B)]
    L, R = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    d_L, d_R = dev(L), dev(R)
    cuda = torch.device("cuda", 0)
    d_out, d_fwd = torch.zeros((B, 1, H, W), dtype=torch.int32, device=cuda), torch.zeros((B, 1, H, W), dtype=torch.int32, device=cuda)
    u = np.full((B, H, W), float(disp), np.float32)
    ignore = np.zeros((B, H, W), np.uint8)
    ignore[:, :, :disp] = 1                                  # the columns whose true target lies outside the right image
    d_u, d_i = dev(u), dev(ignore)
    d_scores = torch.full((2, B, 512), FILL, dtype=torch.uint8, device=cuda)
    d_err = torch.full((B, H, W, 2), FILL, dtype=torch.uint8, device=cuda)
    ctx.search_batch_device(d_L[1], d_R[1], W, H, B, g.Settings(5, 128, 0, True, False, 1), g.Densify(), g.Search(), g.Clean(),
                            d_out.data_ptr(), d_fwd=d_fwd.data_ptr())
    ctx.score_fields_device(d_fwd.data_ptr(), 1, W, H, B, d_u[1], 0, d_i[1], g.FieldScorePrm(), d_scores[0].data_ptr(), 0, d_err.data_ptr())
    ctx.score_fields_device(d_out.data_ptr(), 1, W, H, B, d_u[1], 0, d_i[1], g.FieldScorePrm(), d_scores[1].data_ptr())
    ctx.synchronize()
    words = d_scores.cpu().numpy().view(np.int64).reshape(2, B, 64)
    for k, d_f in enumerate((d_fwd, d_out)):
        want, err = fu.score(d_f.cpu().numpy(), u, None, ignore, None, fu.DEFAULTS)
        assert np.array_equal(words[k], want)
        if k == 0:
            assert np.array_equal(d_err.cpu().numpy().view(np.uint16).reshape(B, H, W), err)
        assert (want[:, fu.ALL] > 1000).all() and (want[:, fu.ALL + 1] > 0).all()      # something was judged, and within a pixel
