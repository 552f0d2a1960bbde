"""The lookahead convolution through the C ABI (``ms_lookahead_forward``, ``ms_lookahead_window_forward``) with explicit
element strides, in both output layouts and with and without the clamp, against the float64 reference and the two input
families of tests/lookahead_cases.py (tests/test_lookahead_cpu.py proves those): the 256-frame blocks of the time-contiguous
kernel, the 256-lane blocks, 16-tap chunks and 16- / 32-frame tiles of the feature-contiguous one, windows of a stream, and
where a non-finite input frame may show.  The only criteria are exact equality and the derived gaussian bound.  Every y lies
between sentinel guards that must survive.  Needs a real MI355X: -m gpu."""
import numpy as np
import pytest
import torch

import lookahead_cases as C
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64                          # guard elements on either side of y
SENTINEL = -7.25e33


def act_args(act):
    return (_lib.ACT_NONE, 0.0, 0.0) if act is None else (_lib.ACT_CLAMP, act[0], act[1])


def put(x, kind, wide=False):
    """x [N, F, T] on the device as the kernel's input: (view, (xs_n, xs_f, xs_t)).  ``tcontig``: [N, F, T] as it is.
    ``fcontig``: the RNN's [T, N, F], or with ``wide`` the first F columns of a [T, N, 2 F] buffer whose other columns are
    NaN (a read outside the view poisons the result)."""
    N, F, T = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if kind == "tcontig":
        return xd, (F * T, T, 1)
    fw = 2 * F if wide else F
    buf = torch.full((T, N, fw), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :, :F] = xd.permute(2, 0, 1)
    view = buf[:, :, :F]
    assert N * fw != 1, "a time stride of 1 would select the time-contiguous kernel"
    return view, (fw, 1, N * fw)


def lookahead(lib, xv, xs, wd, N, F, T_in, T_out, ctx, layout, act, window, what, expect_ok=True):
    """One call; the result as numpy [N, F, T_out] whatever the layout (None if the call was refused, y then untouched)."""
    count = N * F * T_out
    buf = torch.full((count + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    y = buf[GUARD:GUARD + count]
    ys = (F * T_out, T_out, 1) if layout == "nft" else (T_out * F, 1, F)
    a, lo, hi = act_args(act)
    if window:
        rc = lib.ms_lookahead_window_forward(_lib.ptr(xv, strided=True), _lib.ptr(wd), _lib.ptr(y), N, F, T_in, T_out, ctx, *xs, *ys,
                                             a, lo, hi, _lib.stream_ptr())
    else:
        assert T_out == T_in
        rc = lib.ms_lookahead_forward(_lib.ptr(xv, strided=True), _lib.ptr(wd), _lib.ptr(y), N, F, T_in, ctx, *xs, *ys, a, lo, hi,
                                      _lib.stream_ptr())
    host = buf.cpu().numpy()
    if not expect_ok:
        assert rc != _lib.MS_OK, what
        assert np.all(host == np.float32(SENTINEL)), (what, "a refused call wrote")
        return None
    _lib.check(rc, "ms_lookahead")
    assert np.all(host[:GUARD] == np.float32(SENTINEL)) and np.all(host[-GUARD:] == np.float32(SENTINEL)), (what, "guards")
    got = host[GUARD:-GUARD]
    assert not np.any(got == np.float32(SENTINEL)), (what, "an output was not written")
    return got.reshape(N, F, T_out).copy() if layout == "nft" else got.reshape(N, T_out, F).transpose(0, 2, 1).copy()


def run_case(lib, kind, N, F, T, ctx, wide=False):
    for fam in C.FAMILIES:
        x, w = C.make(fam, N, F, T, ctx)
        xv, xs = put(x, kind, wide)
        wd = torch.from_numpy(w).cuda()
        for layout in C.LAYOUTS:
            for act in C.ACTS:
                what = (kind, fam, N, F, T, ctx, wide, layout, act)
                got = lookahead(lib, xv, xs, wd, N, F, T, T, ctx, layout, act, False, what)
                C.check(fam, got, x, w, T, act, what)


@pytest.mark.parametrize("N,F,T,ctx", C.tcontig_cases())
def test_time_contiguous_input(lib, N, F, T, ctx):
    run_case(lib, "tcontig", N, F, T, ctx)


@pytest.mark.parametrize("N,F,T,ctx,wide", C.fcontig_cases())
def test_feature_contiguous_input(lib, N, F, T, ctx, wide):
    run_case(lib, "fcontig", N, F, T, ctx, wide)


@pytest.mark.parametrize("kind,N,F", [("tcontig", 2, 3), ("fcontig", 2, 257)])
@pytest.mark.parametrize("T_in,ctx", sorted({(t_in, ctx) for t_in, _, ctx in C.window_cases()}))
def test_window_of_a_stream(lib, kind, N, F, T_in, ctx):
    """y has room for exactly T_out frames.  The first 16 frames of a T_out = 16 call (the 16-frame tile of the
    feature-contiguous kernel) equal those of the T_out = T_in call (its 32-frame tile) bit for bit: per output the
    products arrive in the same order."""
    t_outs = [t_out for t_in, t_out, c in C.window_cases() if (t_in, c) == (T_in, ctx)]
    assert 16 in t_outs and T_in in t_outs and T_in > 16
    for fam in C.FAMILIES:
        x, w = C.make(fam, N, F, T_in, ctx)
        xv, xs = put(x, kind, wide=True)
        wd = torch.from_numpy(w).cuda()
        for layout in C.LAYOUTS:
            for act in C.ACTS:
                got = {}
                for T_out in t_outs:
                    what = (kind, fam, N, F, T_in, T_out, ctx, layout, act)
                    got[T_out] = lookahead(lib, xv, xs, wd, N, F, T_in, T_out, ctx, layout, act, True, what)
                    C.check(fam, got[T_out], x, w, T_out, act, what)
                for T_out in t_outs:
                    assert np.array_equal(got[T_out].view(np.uint32), got[T_in][:, :, :T_out].view(np.uint32)), \
                        (kind, fam, T_in, T_out, ctx, layout, act, "a window's frames differ from the whole call's")


def test_a_context_that_does_not_fit_is_refused(lib):
    """Time-contiguous input stages 256 + 2 ctx floats per workgroup: ctx = 8100 does not fit, nothing is written."""
    N, F, T, ctx = 1, 2, 10, 8100
    x, w = C.make("gauss", N, F, T, ctx)
    xv, xs = put(x, "tcontig")
    lookahead(lib, xv, xs, torch.from_numpy(w).cuda(), N, F, T, T, ctx, "nft", None, False, "ctx 8100", expect_ok=False)


@pytest.mark.parametrize("kind", ["tcontig", "fcontig"])
@pytest.mark.parametrize("ctx", C.ISOLATION_CTX)
def test_a_non_finite_frame_reaches_the_outputs_that_read_it_and_no_other(lib, kind, ctx):
    """An Inf, then a NaN, at x[n0, f0, t0]: the outputs (n0, f0, t0 - ctx + 1 .. t0) are non-finite (the weights are not
    zero), every other output has the finite run's value -- as in the definition (pad + conv1d), where a tap that the context
    does not have multiplies nothing."""
    N, F, T = 2, 5, 70
    x, w = C.make("gauss", N, F, T, ctx)
    assert np.all(w != 0)
    wd = torch.from_numpy(w).cuda()
    n0, f0 = 1, 2
    for layout in C.LAYOUTS:
        xv, xs = put(x, kind)
        finite = lookahead(lib, xv, xs, wd, N, F, T, T, ctx, layout, None, False, (kind, ctx, layout, "finite"))
        C.check("gauss", finite, x, w, T, None, (kind, ctx, layout, "finite"))
        for t0 in (40, 5, T - 1):
            for value in (np.inf, np.nan):
                xb = x.copy()
                xb[n0, f0, t0] = value
                xv, xs = put(xb, kind)
                what = (kind, ctx, layout, t0, value)
                got = lookahead(lib, xv, xs, wd, N, F, T, T, ctx, layout, None, False, what)
                reads = np.zeros((N, F, T), dtype=bool)
                reads[n0, f0, max(0, t0 - ctx + 1):t0 + 1] = True
                assert not np.isfinite(got[reads]).any(), (what, "an output that reads the frame is finite")
                bad = ~reads & ~(got == finite)
                assert not bad.any(), (what, "outputs that do not read the frame changed", np.argwhere(bad)[:6].tolist())


@pytest.mark.parametrize("kind", ["tcontig", "fcontig"])
@pytest.mark.parametrize("ctx", C.ISOLATION_CTX)
def test_a_non_finite_frame_survives_the_clamp(lib, kind, ctx):
    """The same poisoned frame under the clamp (lo, hi), as torch.clamp and F.hardtanh define it: an output that reads a NaN
    is NaN, not ``lo``; an output that reads an Inf is what np.clip makes of the unclamped run's value there (NaN -> NaN,
    +Inf -> hi, -Inf -> lo); every other output keeps the clamped finite run's bits."""
    N, F, T = 2, 5, 70
    act = C.ACTS[1]
    lo, hi = np.float32(act[0]), np.float32(act[1])
    x, w = C.make("gauss", N, F, T, ctx)
    assert np.all(w != 0)
    wd = torch.from_numpy(w).cuda()
    n0, f0 = 1, 2
    for layout in C.LAYOUTS:
        xv, xs = put(x, kind)
        finite = lookahead(lib, xv, xs, wd, N, F, T, T, ctx, layout, act, False, (kind, ctx, layout, "finite, clamped"))
        C.check("gauss", finite, x, w, T, act, (kind, ctx, layout, "finite, clamped"))
        for t0 in (40, 5, T - 1):
            for value in (np.inf, -np.inf, np.nan):
                xb = x.copy()
                xb[n0, f0, t0] = value
                xv, xs = put(xb, kind)
                what = (kind, ctx, layout, t0, value)
                raw = lookahead(lib, xv, xs, wd, N, F, T, T, ctx, layout, None, False, what + ("unclamped",))
                got = lookahead(lib, xv, xs, wd, N, F, T, T, ctx, layout, act, False, what + ("clamped",))
                reads = np.zeros((N, F, T), dtype=bool)
                reads[n0, f0, max(0, t0 - ctx + 1):t0 + 1] = True
                assert not np.isfinite(raw[reads]).any(), (what, "an unclamped output that reads the frame is finite")
                want = np.clip(raw[reads], lo, hi)
                assert want.dtype == np.float32
                if np.isnan(value):
                    assert np.isnan(want).all()
                same = (np.isnan(got[reads]) & np.isnan(want)) | (got[reads].view(np.uint32) == want.view(np.uint32))
                assert same.all(), (what, "the clamp did not keep what np.clip keeps", got[reads][~same][:6].tolist(),
                                    want[~same][:6].tolist())
                bad = ~reads & ~(got.view(np.uint32) == finite.view(np.uint32))
                assert not bad.any(), (what, "outputs that do not read the frame changed", np.argwhere(bad)[:6].tolist())
