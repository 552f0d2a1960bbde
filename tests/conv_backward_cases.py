"""Cases, input families and the float64 restatement of the convolution and lookahead BACKWARD entry points of
include/ms_hotpath.h: ``ms_maskconv_backward_data``, ``ms_maskconv_backward_weight``, ``ms_lookahead_backward``.  numpy only;
imports nothing of the package.  tests/test_conv_backward_cpu.py pins the restatement to torch float64 autograd and proves what
is promised here, tests/test_conv_backward_gpu.py runs the cases through the C ABI.

The operation (include/ms_hotpath.h).  Forward, groups == 1: y = act(b[co] + sum w[co,ci,kf,kt] xm[n, ci, fo SF - pad_f + kf DF,
to ST - pad_t + kt DT]), xm = x with frames t >= min(lens[n], Tin) and everything outside the input read as 0.  Backward from
x, the saved OUTPUT y, w, lens and dy: g = dy where there is no clamp or lo < y < hi strictly, +0 elsewhere;
dx[n,ci,fi,ti] = sum w[co,ci,kf,kt] g[n,co,fo,to] over the windows that read (fi, ti), +0 in masked frames and where no window
reads; dw[co,ci,kf,kt] = sum_{n,fo,to} g xm; db[co] = sum g.

Input families.
``dense``  g and w integers in [-7, 7] \\ {0}, x integers in [-15, 15], bias integers in [-20, 20]; y is the forward's own
           output under the clamp [-50, 120], which cuts some of it on either side and leaves some strictly inside.  Cap:
           sum |g| |x| < 2^24 and sum |w| |g| < 2^24 (``abs_sums`` evaluates them on absolute values), under which every sum is
           exact in float32 in any order: the device is compared with ``array_equal``.
``gauss``  N(0, 1) float32, clamp [-1, 2]: |got - ref| <= (terms + 2) 2^-24 sum |a| |b| with terms the reduction length --
           Cout KF KT for dx, N Fout Tout plus the number of slices for dw and db (one rounding per product and per partial
           sum; Higham, Accuracy and Stability, section 3.1: the bound of tests/conv_exact_cases.py).  Derived, not measured.

The kernel's constants (csrc/conv_backward.hip): ``SLICE`` = CBW_SLICE, the k = (n, fo, to) elements per slice of the weight
gradient; a tile is 32 channels x 128 columns."""
import functools
from collections import namedtuple

import numpy as np

import conv_exact_cases as X

U = 2.0 ** -24
CAP = 2 ** 24
SLICE = 8192           # csrc/conv_backward.hip: CBW_SLICE
FAMILIES = ("dense", "gauss")
CLAMP = {"dense": (-50.0, 120.0), "gauss": (-1.0, 2.0)}
LCLAMP = {"dense": (-20.0, 30.0), "gauss": (-0.5, 0.8)}      # the lookahead cases' (a context of 1 is one product)

Case = namedtuple("Case", "tag N Cin Fin Tin Cout Fout Tout KF KT SF ST DF DT pad_f pad_t lens bias act")


def mk(tag, N, Cin, Fin, Tin, Cout, KF, KT, SF=1, ST=1, DF=1, DT=1, same=True, lens="ragged", bias=True, act=True):
    c = X.mk("bwd", tag, N, Cin, Fin, Cout, KF, KT, Tin=Tin, SF=SF, ST=ST, DF=DF, DT=DT, same=same, lens=None)
    if isinstance(lens, str):
        # one full utterance, one of length 1, the rest in between
        lens = ([Tin, 1] + [max(1, Tin // 2 + 1)] * N)[:N] if N > 1 else [max(1, Tin - 7)]
    return Case(tag, N, Cin, Fin, Tin, Cout, c.Fout, c.Tout, KF, KT, SF, ST, DF, DT, c.pad_f, c.pad_t,
                None if lens is None else tuple(lens), bias, act)


def eff_lens(c):
    return [c.Tin if c.lens is None else min(max(int(v), 0), c.Tin) for v in (c.lens or [0] * c.N)]


def slices(c):
    return X.cdiv(c.N * c.Fout * c.Tout, SLICE)


def clamp_of(c, family):
    return CLAMP[family] if c.act else None


# ----------------------------------------------------------------------------- the restatement
def gate(dy, y, act):
    dy = np.asarray(dy, dtype=np.float64)
    if act is None:
        return dy
    y = np.asarray(y, dtype=np.float64)
    return np.where((y > act[0]) & (y < act[1]), dy, 0.0)


def forward(c, x, w, b, act):
    return X.reference(x, c.lens, w, b if c.bias else None, (c.SF, c.ST), (c.DF, c.DT), (c.pad_f, c.pad_t), 1, act,
                       (c.Fout, c.Tout))


def backward(c, x, w, g):
    """(dx, dw, db) float64 from the GATED gradient g, by the index arithmetic above."""
    x, w, g = (np.asarray(a, dtype=np.float64) for a in (x, w, g))
    L = eff_lens(c)
    xm = x.copy()
    for n in range(c.N):
        xm[n, :, :, L[n]:] = 0.0
    hf = (c.Fout - 1) * c.SF + (c.KF - 1) * c.DF + 1
    ht = (c.Tout - 1) * c.ST + (c.KT - 1) * c.DT + 1
    shape = (c.N, c.Cin, max(hf, c.pad_f + c.Fin), max(ht, c.pad_t + c.Tin))
    xp, dxp = np.zeros(shape), np.zeros(shape)
    xp[:, :, c.pad_f:c.pad_f + c.Fin, c.pad_t:c.pad_t + c.Tin] = xm
    dw = np.zeros((c.Cout, c.Cin, c.KF, c.KT))
    for kf in range(c.KF):
        for kt in range(c.KT):
            sl = (slice(None), slice(None), slice(kf * c.DF, kf * c.DF + (c.Fout - 1) * c.SF + 1, c.SF),
                  slice(kt * c.DT, kt * c.DT + (c.Tout - 1) * c.ST + 1, c.ST))
            dw[:, :, kf, kt] = np.tensordot(g, xp[sl], axes=([0, 2, 3], [0, 2, 3]))
            dxp[sl] += np.tensordot(w[:, :, kf, kt], g, axes=([0], [1])).transpose(1, 0, 2, 3)
    dx = dxp[:, :, c.pad_f:c.pad_f + c.Fin, c.pad_t:c.pad_t + c.Tin].copy()
    for n in range(c.N):
        dx[n, :, :, L[n]:] = 0.0
    return dx, dw, g.sum(axis=(0, 2, 3))


def abs_sums(c, x, w, g):
    """sum |w| |g| per dx element, sum |g| |x| per dw element, sum |g| per db element: the caps and the bounds' scales."""
    return backward(c, np.abs(x), np.abs(w), np.abs(g))


def x_readers(c, n, ci, fi, ti):
    """Boolean [Cout, Cin, KF, KT]: the dw elements whose sum reads input position (n, ci, fi, ti); none for a masked frame."""
    m = np.zeros((c.Cout, c.Cin, c.KF, c.KT), dtype=bool)
    if not (0 <= ti < eff_lens(c)[n] and 0 <= fi < c.Fin):
        return m
    for kf in range(c.KF):
        for kt in range(c.KT):
            nf, nt = fi + c.pad_f - kf * c.DF, ti + c.pad_t - kt * c.DT
            if nf >= 0 and nt >= 0 and nf % c.SF == 0 and nt % c.ST == 0 and nf // c.SF < c.Fout and nt // c.ST < c.Tout:
                m[:, ci, kf, kt] = True
    return m


def dy_window(c, n, fo, to):
    """(Boolean [N, Cin, Fin, Tin], Boolean [Cin, KF, KT]): the live input positions of the window of output (n, :, fo, to) and
    the taps that pair it with one."""
    mx = np.zeros((c.N, c.Cin, c.Fin, c.Tin), dtype=bool)
    mw = np.zeros((c.Cin, c.KF, c.KT), dtype=bool)
    for kf in range(c.KF):
        for kt in range(c.KT):
            fi, ti = fo * c.SF - c.pad_f + kf * c.DF, to * c.ST - c.pad_t + kt * c.DT
            if 0 <= fi < c.Fin and 0 <= ti < eff_lens(c)[n]:
                mx[n, :, fi, ti] = True
                mw[:, kf, kt] = True
    return mx, mw


# ----------------------------------------------------------------------------- families
def _nonzero(rng, lim, shape):
    return rng.integers(1, lim + 1, size=shape) * (rng.integers(0, 2, size=shape) * 2 - 1)


@functools.lru_cache(maxsize=None)
def make(c, family):
    """(x, w, b, y, dy) float32; y is the forward's output on (x, w, b) under the family's clamp (none: unclamped)."""
    rng = np.random.default_rng([7, FAMILIES.index(family), c.N, c.Cin, c.Fin, c.Tin, c.Cout, c.KF, c.KT])
    xs, ws, ys = (c.N, c.Cin, c.Fin, c.Tin), (c.Cout, c.Cin, c.KF, c.KT), (c.N, c.Cout, c.Fout, c.Tout)
    if family == "gauss":
        x, w, b, dy = (rng.standard_normal(s) for s in (xs, ws, c.Cout, ys))
    else:
        x, w, b, dy = rng.integers(-15, 16, size=xs), _nonzero(rng, 7, ws), rng.integers(-20, 21, size=c.Cout), _nonzero(rng, 7, ys)
    x, w, b, dy = (a.astype(np.float32) for a in (x, w, b, dy))
    y = forward(c, x, w, b, clamp_of(c, family)).astype(np.float32)
    for a in (x, w, b, y, dy):
        a.setflags(write=False)
    return x, w, b, y, dy


@functools.lru_cache(maxsize=None)
def want(c, family):
    """(dx, dw, db) float64 of a case's draw, computed once; callers must not write to them."""
    x, w, _, y, dy = make(c, family)
    out = backward(c, x, w, gate(dy, y, clamp_of(c, family)))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scales(c, family):
    x, w, _, y, dy = make(c, family)
    return abs_sums(c, x, w, gate(dy, y, clamp_of(c, family)))


def terms(c):
    """Reduction lengths of (dx, dw, db); the weight gradient's include one addition per slice."""
    k = c.N * c.Fout * c.Tout + slices(c)
    return c.Cout * c.KF * c.KT, k, k


def check(c, family, got, what):
    """got = (dx, dw, db or None) float32 arrays from the device."""
    for name, g, ref, scale, n in zip(("dx", "dw", "db"), got, want(c, family), scales(c, family), terms(c)):
        if g is None:
            continue
        assert g.shape == ref.shape and g.dtype == np.float32, (what, name, g.shape, ref.shape)
        if family == "dense":
            bad = ~(g.astype(np.float64) == ref)
            assert not bad.any(), (what, name, int(bad.sum()), "of", bad.size, "wrong; first at", np.argwhere(bad)[:4].tolist(),
                                   g[bad][:4].tolist(), ref[bad][:4].tolist())
        else:
            err, bound = np.abs(g.astype(np.float64) - ref), (n + 2) * U * scale
            bad = ~(err <= bound)
            assert not bad.any(), (what, name, "worst error / bound", float(np.nanmax(err / np.maximum(bound, 1e-300))),
                                   np.argwhere(bad)[:4].tolist())


# ----------------------------------------------------------------------------- the case list
def cases():
    out = [
        # (a) channel counts off every tile
        mk("a_cin3_cout5", 3, 3, 7, 9, 5, 3, 3, SF=2, ST=2),
        mk("a_lens_null", 3, 3, 7, 9, 5, 3, 3, SF=2, ST=2, lens=None),
        # (b) a miniature conv1
        mk("b_conv1_cin1_cout32", 3, 1, 9, 14, 32, 5, 3, SF=2, ST=2),
        # (c) a miniature conv2 on whole tiles and one past them
        mk("c_conv2_32_32", 3, 32, 5, 6, 32, 3, 3, SF=2),
        mk("c_conv2_33_34", 3, 33, 5, 6, 34, 3, 3, SF=2),
        # (d) stride 3, dilation 2, no padding: input positions that no window reads
        mk("d_s3_d2_nopad", 3, 2, 11, 14, 3, 3, 4, SF=3, ST=3, DF=2, DT=2, same=False),
        # (e) the conv1d form
        mk("e_conv1d_cin40_cout7", 3, 40, 1, 21, 7, 1, 5, ST=2),
        # (f) no bias
        mk("f_bias_null", 3, 3, 7, 9, 5, 3, 3, SF=2, ST=2, bias=False),
        mk("f_no_clamp", 3, 3, 7, 9, 5, 3, 3, SF=2, ST=2, act=False),
    ]
    # (g) reduction lengths N Fout Tout around one and two slices (N = 1: 8191 is prime)
    for k in (SLICE - 1, SLICE, SLICE + 1, 2 * SLICE - 1, 2 * SLICE, 2 * SLICE + 1):
        out.append(mk(f"g_k{k}", 1, 2, 1, k, 3, 1, 3))
    return out


def unread_positions(c):
    """Boolean [Fin, Tin]: input positions that no window reads."""
    m = np.ones((c.Fin, c.Tin), dtype=bool)
    fs = [fo * c.SF - c.pad_f + kf * c.DF for fo in range(c.Fout) for kf in range(c.KF)]
    ts = [to * c.ST - c.pad_t + kt * c.DT for to in range(c.Tout) for kt in range(c.KT)]
    fs = sorted({f for f in fs if 0 <= f < c.Fin})
    ts = sorted({t for t in ts if 0 <= t < c.Tin})
    m[np.ix_(fs, ts)] = False
    return m


# ----------------------------------------------------------------------------- lookahead
LCase = namedtuple("LCase", "tag N F T ctx layout act")


def lookahead_cases():
    """(h) contexts 1, 3 and 17 at T below, at and above the context, in both layouts: "nft" (x and y [N, F, T]) and "ds2"
    (x [T, N, F], the recurrent stack's output; y [N, T, F], what the fully connected stack reads)."""
    out = []
    for ctx in (1, 3, 17):
        for T in sorted({max(1, ctx - 1), ctx, ctx + 1, ctx + 20}):
            for layout in ("nft", "ds2"):
                out.append(LCase(f"ctx{ctx}_t{T}_{layout}", 3, 67, T, ctx, layout, True))
    out.append(LCase("ctx3_t9_nft_no_clamp", 3, 67, 9, 3, "nft", False))
    return out


def lookahead_forward(x, w, act):
    """x [N, F, T], w [F, ctx] -> y [N, F, T] float64."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    T, ctx = x.shape[2], w.shape[1]
    z = np.zeros(x.shape)
    for k in range(min(ctx, T)):
        z[:, :, :T - k] += w[None, :, k, None] * x[:, :, k:]
    return z if act is None else np.clip(z, act[0], act[1])


def lookahead_backward(x, w, g):
    """(dx [N, F, T], dw [F, ctx]) float64 from the gated gradient."""
    x, w, g = (np.asarray(a, dtype=np.float64) for a in (x, w, g))
    T, ctx = x.shape[2], w.shape[1]
    dx, dw = np.zeros(x.shape), np.zeros(w.shape)
    for k in range(min(ctx, T)):
        dx[:, :, k:] += w[None, :, k, None] * g[:, :, :T - k]
        dw[:, k] = (g[:, :, :T - k] * x[:, :, k:]).sum(axis=(0, 2))
    return dx, dw


@functools.lru_cache(maxsize=None)
def lookahead_make(c, family):
    """(x, w, y, dy) float32 in [N, F, T] order."""
    rng = np.random.default_rng([11, FAMILIES.index(family), c.N, c.F, c.T, c.ctx])
    xs, ws = (c.N, c.F, c.T), (c.F, c.ctx)
    if family == "gauss":
        x, w, dy = (rng.standard_normal(s) for s in (xs, ws, xs))
    else:
        x, w, dy = rng.integers(-15, 16, size=xs), _nonzero(rng, 7, ws), _nonzero(rng, 7, xs)
    x, w, dy = (a.astype(np.float32) for a in (x, w, dy))
    y = lookahead_forward(x, w, LCLAMP[family] if c.act else None).astype(np.float32)
    for a in (x, w, y, dy):
        a.setflags(write=False)
    return x, w, y, dy


def lookahead_want(c, family):
    x, w, y, dy = lookahead_make(c, family)
    g = gate(dy, y, LCLAMP[family] if c.act else None)
    return lookahead_backward(x, w, g), lookahead_backward(np.abs(x), np.abs(w), np.abs(g))


def lookahead_check(c, family, got, what):
    refs, scale = lookahead_want(c, family)
    for name, g, ref, s, n in zip(("dx", "dw"), got, refs, scale, (c.ctx, c.N * c.T)):
        assert g.shape == ref.shape and g.dtype == np.float32, (what, name, g.shape, ref.shape)
        if family == "dense":
            assert s.max() < CAP
            assert np.array_equal(g.astype(np.float64), ref), (what, name)
        else:
            err = np.abs(g.astype(np.float64) - ref)
            assert (err <= (n + 2) * U * s).all(), (what, name, float(err.max()))
