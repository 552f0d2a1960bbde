"""The convolution and lookahead backward on the device through the C ABI (``ms_maskconv_backward_data``,
``ms_maskconv_backward_weight``, ``ms_lookahead_backward``) against tests/conv_backward_cases.py: every case in the exact family
(``array_equal``) and in the gaussian one (the derived bound).  Outputs sit between sentinel guards, workspaces are filled with
0xFF bytes, two runs must give the same bits.  Then what a gradient must NOT do: read x past a length (poison there changes no
bit), spread a non-finite x or dy beyond the elements whose sums contain it, or launch anything on bad arguments."""
import numpy as np
import pytest
import torch

import conv_backward_cases as B
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 64          # floats on either side of an output (keeps the output 256-byte aligned)
CASES = B.cases()
BY_TAG = {c.tag: c for c in CASES}
LCASES = B.lookahead_cases()
SMALL = [c for c in CASES if not c.tag.startswith("g_k")]


def dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype).cuda().contiguous()      # (a copy: the draws are read-only)


class Guarded:
    """An output of ``shape`` with GUARD sentinels before and after it, itself pre-filled with the sentinel."""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n]

    def get(self, written=True):
        a = self.buf.cpu().numpy()
        assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + self.n:] == SENTINEL).all(), "a guard was overwritten"
        out = a[GUARD:GUARD + self.n].reshape(self.shape).copy()
        if written:
            assert not (out == SENTINEL).any(), "an output element was not written"
        else:
            assert (out == SENTINEL).all(), "an output was written by a refused call"
        return out


def workspace(nbytes):
    return torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device="cuda")


def run_conv(c, family, x=None, dy=None, expect=None, short_ws=False, null=(), **over):
    """(dx, dw, db | None) from the two entry points on a case's draw (x / dy replaced if given).  ``null``: tensor arguments
    passed as NULL; ``over``: geometry integers replaced by name.  ``expect``: the two calls' error names (0 = MS_OK)."""
    lib = _lib.load()
    x0, w, _, y, dy0 = B.make(c, family)
    act = B.clamp_of(c, family)
    a, lo, hi = (_lib.ACT_NONE, 0.0, 0.0) if act is None else (_lib.ACT_CLAMP, act[0], act[1])
    t = dict(x=dev(x0 if x is None else x), w=dev(w), y=dev(y), dy=dev(dy0 if dy is None else dy),
             lens=dev(c.lens, torch.int32))
    dx, dw = Guarded(c.N, c.Cin, c.Fin, c.Tin), Guarded(c.Cout, c.Cin, c.KF, c.KT)
    db = Guarded(c.Cout) if c.bias else None
    g = dict(N=c.N, Cin=c.Cin, Fin=c.Fin, Tin=c.Tin, Cout=c.Cout, Fout=c.Fout, Tout=c.Tout, KF=c.KF, KT=c.KT, SF=c.SF, ST=c.ST,
             DF=c.DF, DT=c.DT, pad_f=c.pad_f, pad_t=c.pad_t, act=a)
    for key in null:
        t[key] = None
    assert set(over) <= set(g)
    g.update(over)
    geom = tuple(g.values()) + (lo, hi)
    nbytes = lib.ms_maskconv_backward_workspace_bytes(c.N, c.Cin, c.Cout, c.Fout, c.Tout, c.KF, c.KT)
    assert nbytes >= B.slices(c) * c.Cout * (c.Cin * c.KF * c.KT + 1) * 4
    ws = workspace(nbytes)
    rc_d = lib.ms_maskconv_backward_data(_lib.ptr(t["w"]), _lib.ptr(t["y"]), _lib.ptr(t["dy"]), _lib.ptr(t["lens"]), _lib.ptr(dx.t),
                                         *geom, _lib.stream_ptr())
    rc_w = lib.ms_maskconv_backward_weight(_lib.ptr(t["x"]), _lib.ptr(t["y"]), _lib.ptr(t["dy"]), _lib.ptr(t["lens"]), _lib.ptr(dw.t),
                                           _lib.ptr(None if db is None else db.t), *geom, _lib.ptr(ws),
                                           nbytes - 256 if short_ws else nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    if expect is not None:
        assert [_lib.ERR_NAMES.get(rc, rc) for rc in (rc_d, rc_w)] == list(expect), (rc_d, rc_w)
        for out, rc in ((dx, rc_d), (dw, rc_w), (db, rc_w)):
            if out is not None and rc != 0:
                out.get(written=False)
        return None
    _lib.check(rc_d, "ms_maskconv_backward_data")
    _lib.check(rc_w, "ms_maskconv_backward_weight")
    return dx.get(), dw.get(), None if db is None else db.get()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("family", B.FAMILIES)
@pytest.mark.parametrize("c", CASES, ids=[c.tag for c in CASES])
def test_case(c, family):
    got = run_conv(c, family)
    B.check(c, family, got, c.tag)
    dx = got[0]
    for n, ln in enumerate(B.eff_lens(c)):      # masked frames: +0.0
        assert not dx[n, :, :, ln:].view(np.uint32).any()
    assert not dx[:, :, B.unread_positions(c)].view(np.uint32).any()      # ... and positions that no window reads
    again = run_conv(c, family)
    assert all(a is None or same_bits(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("tag", ["a_cin3_cout5", "b_conv1_cin1_cout32", "c_conv2_33_34", "d_s3_d2_nopad", "e_conv1d_cin40_cout7"])
def test_poison_past_the_lengths_changes_no_bit(tag):
    c = BY_TAG[tag]
    clean = run_conv(c, "gauss")
    x = B.make(c, "gauss")[0].copy()
    L = B.eff_lens(c)
    assert min(L) < c.Tin
    for n in range(c.N):
        x[n, :, :, L[n]:] = np.nan
        x[n, :, ::2, L[n]:] = np.inf
    got = run_conv(c, "gauss", x=x)
    assert all(same_bits(a, b) for a, b in zip(got, clean))


@pytest.mark.parametrize("poison", B.X.POISONS)
@pytest.mark.parametrize("tag", ["a_cin3_cout5", "c_conv2_33_34", "d_s3_d2_nopad"])
def test_non_finite_live_x_reaches_exactly_its_readers(tag, poison):
    c = BY_TAG[tag]
    clean = run_conv(c, "gauss")
    x = B.make(c, "gauss")[0].copy()
    # utterance 0 is full; a position that some window reads
    read = np.argwhere(~B.unread_positions(c))
    fi, ti = (int(v) for v in read[len(read) // 2])
    ci = c.Cin - 1
    x[0, ci, fi, ti] = poison
    mask = B.x_readers(c, 0, ci, fi, ti)
    assert mask.any() and not mask.all()
    dx, dw, db = run_conv(c, "gauss", x=x)
    assert not np.isfinite(dw[mask]).any()
    assert same_bits(dw[~mask], clean[1][~mask]) and same_bits(dx, clean[0]) and same_bits(db, clean[2])


@pytest.mark.parametrize("tag", ["a_cin3_cout5", "c_conv2_33_34", "d_s3_d2_nopad", "f_no_clamp"])
def test_nan_in_a_live_dy_element(tag):
    c = BY_TAG[tag]
    clean = run_conv(c, "gauss")
    _, _, _, y, dy = B.make(c, "gauss")
    act = B.clamp_of(c, "gauss")
    inside = np.ones(y.shape, dtype=bool) if act is None else (y > act[0]) & (y < act[1])
    # an element of the FULL utterance that the gate passes, away from the first output row and frame
    cand = [p for p in np.argwhere(inside[0]) if p[0] == c.Cout - 1]
    co0, fo0, to0 = (int(v) for v in cand[len(cand) // 2])
    dy = dy.copy()
    dy[0, co0, fo0, to0] = np.nan
    mx, mw = B.dy_window(c, 0, fo0, to0)
    assert mx.any() and not mx.all() and mw.any()
    dx, dw, db = run_conv(c, "gauss", dy=dy)
    assert np.isnan(dx[mx]).all() and same_bits(dx[~mx], clean[0][~mx])
    assert np.isnan(db[co0]) and np.isnan(dw[co0][mw]).all()
    rows = np.arange(c.Cout) != co0
    assert same_bits(dw[rows], clean[1][rows]) and same_bits(db[rows], clean[2][rows])


def test_bad_arguments_launch_nothing():
    c = BY_TAG["a_cin3_cout5"]
    inv = "MS_ERR_INVALID"
    run_conv(c, "gauss", expect=(inv, inv), null=("dy",))
    run_conv(c, "gauss", expect=(inv, inv), null=("y",))       # the case has a clamp: the gate needs the saved output
    run_conv(c, "gauss", expect=(inv, 0), null=("w",))
    run_conv(c, "gauss", expect=(0, inv), null=("x",))
    for key in ("N", "Cin", "Fin", "Tin", "Cout", "Fout", "Tout", "KF", "KT", "SF", "ST", "DF", "DT"):
        run_conv(c, "gauss", expect=(inv, inv), **{key: 0})
    run_conv(c, "gauss", expect=(inv, inv), pad_t=-1)
    run_conv(c, "gauss", expect=(inv, inv), act=7)
    run_conv(c, "gauss", expect=(inv, inv), Tout=c.Tout + 40)      # output frames that start past the input
    run_conv(c, "gauss", expect=(0, "MS_ERR_WORKSPACE"), short_ws=True)


# ----------------------------------------------------------------------------- lookahead
def run_lookahead(c, family, expect=None, **over):
    lib = _lib.load()
    x, w, y, dy = B.lookahead_make(c, family)
    act = B.LCLAMP[family] if c.act else None
    a, lo, hi = (_lib.ACT_NONE, 0.0, 0.0) if act is None else (_lib.ACT_CLAMP, act[0], act[1])
    N, F, T = x.shape
    if c.layout == "nft":
        xs, ys = (F * T, T, 1), (F * T, T, 1)
        lay_x = lay_y = lambda v: v                                   # noqa: E731
        dx = Guarded(N, F, T)
        back = lambda v: v                                            # noqa: E731
    else:
        xs, ys = (F, 1, N * F), (T * F, 1, F)
        lay_x = lambda v: v.transpose(2, 0, 1)                        # noqa: E731  [T, N, F]
        lay_y = lambda v: v.transpose(0, 2, 1)                        # noqa: E731  [N, T, F]
        dx = Guarded(T, N, F)
        back = lambda v: v.transpose(1, 2, 0)                         # noqa: E731
    dw = Guarded(F, c.ctx)
    t = dict(x=dev(lay_x(x)), w=dev(w), y=dev(lay_y(y)), dy=dev(lay_y(dy)))
    g = dict(N=N, F=F, T=T, ctx=c.ctx)
    act_arg = over.pop("act", a)
    for key, v in over.items():
        (t if key in t else g)[key] = v
    rc = lib.ms_lookahead_backward(_lib.ptr(t["x"]), _lib.ptr(t["w"]), _lib.ptr(t["y"]), _lib.ptr(t["dy"]), _lib.ptr(dx.t),
                                   _lib.ptr(dw.t), g["N"], g["F"], g["T"], g["ctx"], *xs, *ys, act_arg, lo, hi, _lib.stream_ptr())
    torch.cuda.synchronize()
    if expect is not None:
        assert _lib.ERR_NAMES.get(rc, rc) == expect
        dx.get(written=False)
        dw.get(written=False)
        return None
    _lib.check(rc, "ms_lookahead_backward")
    return np.ascontiguousarray(back(dx.get())), dw.get()


@pytest.mark.parametrize("family", B.FAMILIES)
@pytest.mark.parametrize("c", LCASES, ids=[c.tag for c in LCASES])
def test_lookahead_case(c, family):
    got = run_lookahead(c, family)
    B.lookahead_check(c, family, got, c.tag)
    again = run_lookahead(c, family)
    assert all(same_bits(a, b) for a, b in zip(got, again))


def test_lookahead_bad_arguments_launch_nothing():
    c = LCASES[0]
    for over in (dict(w=None), dict(dy=None), dict(y=None), dict(N=0), dict(F=0), dict(T=0), dict(ctx=0), dict(act=7)):
        run_lookahead(c, "gauss", expect="MS_ERR_INVALID", **over)
