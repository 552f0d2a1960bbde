"""Cases, input families, an integer reference and a reads predicate for the convolution entry points of
include/ms_hotpath.h: ``ms_maskconv_forward`` (tap), ``ms_maskconv_cl_forward`` (cl), ``ms_maskconv_fwin_forward`` (fwin),
``ms_maskconv_fwin_planes_forward`` + ``ms_maskconv_cl_planes_forward`` (hand-over) and ``ms_maskconv1d_gemm_forward`` (gemm1d).
numpy only; imports nothing of the package.  tests/test_conv_exact_cpu.py proves what is promised here,
tests/test_conv_exact_gpu.py runs the cases through the C ABI (tests/conv_exact_run.py is the device runner).

The operation (include/ms_hotpath.h): y[n, co, fo, to] = b[co] + sum over (ci, kf, kt) of w[co, ci, kf, kt] .
xm[n, g Cin_g + ci, fo SF - pad_f + kf DF, to ST - pad_t + kt DT], where xm is x with frames t >= min(lens[n], Tin) and
everything outside [0, Fin) x [0, Tin) read as 0; pad_f / pad_t are the LEFT pads; the output is not masked again.

Input families.  A sum of integers whose absolute terms add up to less than 2^24 is exact in float32 in any order, and the
split kernels' operands (hi + lo planes in fp16 or bf16, the weights first scaled by the power of two ``weight_scale``)
carry the values below exactly, so the result is THE integer and is compared with ``array_equal``:

``dense``  x integers in [-15, 15], w integers in [-7, 7] \\ {0}, bias integers in [-1000, 1000]: every value fits ONE fp16
           or bf16 plane.
``xlo``    x odd integers in [2049, 4095] with random signs at a density chosen per case so that the cap holds, the other
           x integers in [-3, 3]; w in [-7, 7] \\ {0}.  Such an x needs its lo plane in fp16 (11 bits) and in bf16 (8 bits) and
           the lo is never 0; w_lo = 0, so the dropped lo.lo term is 0 and hi.hi + lo.hi + hi.lo is exact: a wrong or missing
           x lo plane is an integer error.  Not for the one-plane ``fp16`` mode.
``wlo``    the mirror image: every w an odd integer in [2049, 4095] with a random sign, x in [-7, 7] \\ {0} at a density
           chosen so that the cap holds (0 elsewhere): the packed weights' lo plane and their scale word.
``gauss``  N(0, 1) float32, for the exact-float32 tap kernel only: |y - ref| <= (terms + 2) 2^-24 (|x| . |w| + |b|) with
           terms = Cin_g KF KT2 (KT2 = KT rounded up to even: the kernel's products), one rounding per product and sum plus
           the bias (Higham, Accuracy and Stability, section 3.1).  Derived, not measured.

The cap of every exact case and family: |x| . |w| + |b| < 2^24, evaluated by ``reference`` itself on the absolute values."""
import functools
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
CAP = 2 ** 24
EXACT_FAMILIES = ("dense", "xlo", "wlo")
POISONS = (np.inf, np.nan)

Case = namedtuple("Case", "entry tag N Cin Fin Tin Cout Fout Tout KF KT SF ST DF DT pad_f pad_t groups lens bias act")


def cdiv(a, b):
    return -(-a // b)


def pad_same(length, k, stride, dilation):
    """(left pad, output size) of the SAME padding of model/cnn.py: ceil(length / stride) outputs, the smaller half left."""
    out = cdiv(length, stride)
    total = stride * out - 1 + dilation * (k - 1) + 1 - length
    return max(total, 0) // 2, out


def out_size(length, k, stride, dilation, pad_total=0):
    return (length + pad_total - dilation * (k - 1) - 1) // stride + 1


def ragged(N, Tin):
    """Full, then ever shorter: Tin, Tin - 3, about Tin / 2, ... (never below 1)."""
    return tuple(max(1, v) for v in ([Tin, Tin - 3, Tin // 2 + 1, Tin - 1, 2 * Tin // 3] * cdiv(N, 5))[:N])


def mk(entry, tag, N, Cin, Fin, Cout, KF, KT, Tout=None, Tin=None, SF=1, ST=1, DF=1, DT=1, same=True, groups=1,
       lens="ragged", bias=True, act=None):
    """A case with ``Tout`` output frames (or ``Tin`` input frames): SAME pads as the modules compute them, or none."""
    if Tin is None:
        Tin = (Tout - 1) * ST + 1 if same else (Tout - 1) * ST + DT * (KT - 1) + 1
    if same:
        pad_t, tout = pad_same(Tin, KT, ST, DT)
        pad_f, fout = pad_same(Fin, KF, SF, DF)
    else:
        pad_t, tout, pad_f, fout = 0, out_size(Tin, KT, ST, DT), 0, out_size(Fin, KF, SF, DF)
    assert tout >= 1 and fout >= 1 and (Tout is None or tout == Tout), (tag, tout, Tout)
    if isinstance(lens, str):
        lens = ragged(N, Tin)
    return Case(entry, tag, N, Cin, Fin, Tin, Cout, fout, tout, KF, KT, SF, ST, DF, DT, pad_f, pad_t, groups,
                None if lens is None else tuple(lens), bias, act)


def eff_lens(c):
    return [c.Tin if c.lens is None else min(int(v), c.Tin) for v in (c.lens or [0] * c.N)]


# ----------------------------------------------------------------------------- the reference
def reference(x, lens, w, b, stride, dilation, pads, groups, act, out):
    """float64 (exact on integers below 2^53) [N, Cout, Fout, Tout] from the index arithmetic above.  ``stride``,
    ``dilation``, ``pads`` are (feature, time); ``pads`` the LEFT pads; ``out`` = (Fout, Tout) as the C ABI takes them (what
    a window reads to the right of or below the input is 0)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    N, Cin, Fin, Tin = x.shape
    Cout, Cin_g, KF, KT = w.shape
    (SF, ST), (DF, DT), (PF, PT) = stride, dilation, pads
    Fout, Tout = out
    assert Cin == Cin_g * groups and Cout % groups == 0
    xm = x.copy()
    for n in range(N):
        ln = Tin if lens is None else min(int(lens[n]), Tin)
        xm[n, :, :, max(ln, 0):] = 0.0
    hf = (Fout - 1) * SF + (KF - 1) * DF + 1
    ht = (Tout - 1) * ST + (KT - 1) * DT + 1
    xp = np.zeros((N, Cin, max(hf, PF + Fin), max(ht, PT + Tin)))
    xp[:, :, PF:PF + Fin, PT:PT + Tin] = xm
    y = np.zeros((N, Cout, Fout, Tout))
    Cout_g = Cout // groups
    for g in range(groups):
        xg = xp[:, g * Cin_g:(g + 1) * Cin_g]
        wg = w[g * Cout_g:(g + 1) * Cout_g]
        for kf in range(KF):
            for kt in range(KT):
                xs = xg[:, :, kf * DF:kf * DF + (Fout - 1) * SF + 1:SF, kt * DT:kt * DT + (Tout - 1) * ST + 1:ST]
                y[:, g * Cout_g:(g + 1) * Cout_g] += np.tensordot(wg[:, :, kf, kt], xs, axes=([1], [1])).transpose(1, 0, 2, 3)
    if b is not None:
        y += np.asarray(b, dtype=np.float64)[None, :, None, None]
    return y if act is None else np.clip(y, act[0], act[1])


def case_reference(c, x, w, b, act="case"):
    return reference(x, c.lens, w, b if c.bias else None, (c.SF, c.ST), (c.DF, c.DT), (c.pad_f, c.pad_t), c.groups,
                     c.act if act == "case" else act, (c.Fout, c.Tout))


def abs_sum(c, x, w, b):
    """|x| . |w| + |b| by the reference's own arithmetic: the cap of the exact families, the scale of the gaussian bound."""
    return case_reference(c, np.abs(x), np.abs(w), None if b is None else np.abs(b), act=None)


def reads(c, n, ch, f, t):
    """Boolean [N, Cout, Fout, Tout]: the outputs whose receptive field contains input position (n, ch, f, t); empty for a
    masked frame."""
    m = np.zeros((c.N, c.Cout, c.Fout, c.Tout), dtype=bool)
    if not (0 <= t < eff_lens(c)[n] and 0 <= f < c.Fin):
        return m
    fos = [fo for fo in range(c.Fout) for kf in range(c.KF) if fo * c.SF - c.pad_f + kf * c.DF == f]
    tos = [to for to in range(c.Tout) for kt in range(c.KT) if to * c.ST - c.pad_t + kt * c.DT == t]
    g = ch // (c.Cin // c.groups)
    cg = c.Cout // c.groups
    if fos and tos:
        m[n, g * cg:(g + 1) * cg, np.array(sorted(set(fos)))[:, None], np.array(sorted(set(tos)))[None, :]] = True
    return m


def gauss_bound(c, x, w, b):
    kt2 = (c.KT + 1) // 2 * 2
    return ((c.Cin // c.groups) * c.KF * kt2 + 2) * U * abs_sum(c, x, w, b)


# ----------------------------------------------------------------------------- families
def weight_scale(w, half_planes=True):
    """csrc/api_common.cpp ``weight_scale_launch`` restated: 2^s with s = 12 - floor(log2 max |w|) for fp16 planes (the largest
    scaled weight lies in [2^12, 2^13)), 1 for bf16 planes."""
    m = float(np.max(np.abs(w)))
    if not half_planes or m == 0.0:
        return 1.0
    return 2.0 ** min(max(12 - int(np.floor(np.log2(m))), -100), 100)


def _signs(rng, shape):
    return rng.integers(0, 2, size=shape) * 2 - 1


def _nonzero(rng, lim, shape):
    return rng.integers(1, lim + 1, size=shape) * _signs(rng, shape)


def _big(rng, shape):
    return (2 * rng.integers(1024, 2048, size=shape) + 1) * _signs(rng, shape)          # odd, 2049 .. 4095


def _draw(c, family, density, seed):
    rng = np.random.default_rng([seed, EXACT_FAMILIES.index(family) if family in EXACT_FAMILIES else 9, c.N, c.Cin, c.Fin,
                                 c.Tin, c.Cout, c.KF, c.KT])
    xs, ws = (c.N, c.Cin, c.Fin, c.Tin), (c.Cout, c.Cin // c.groups, c.KF, c.KT)
    if family == "gauss":
        return (rng.standard_normal(xs).astype(np.float32), rng.standard_normal(ws).astype(np.float32),
                rng.standard_normal(c.Cout).astype(np.float32))
    b = rng.integers(-1000, 1001, size=c.Cout)
    if family == "dense":
        x, w = rng.integers(-15, 16, size=xs), _nonzero(rng, 7, ws)
    elif family == "xlo":
        x = np.where(rng.random(xs) < density, _big(rng, xs), rng.integers(-3, 4, size=xs))
        w = _nonzero(rng, 7, ws)
    elif family == "wlo":
        x = np.where(rng.random(xs) < density, _nonzero(rng, 7, xs), 0)
        w = _big(rng, ws)
    else:
        raise KeyError(family)
    return x.astype(np.float32), w.astype(np.float32), b.astype(np.float32)


def terms(c):
    return (c.Cin // c.groups) * c.KF * c.KT


def density(c, family):
    """Share of the 12-bit x (xlo) or of the nonzero x (wlo): the largest of 1, 1/2, 1/4, ... whose EXPECTED worst window stays
    under a third of the cap (the draw itself is then checked against the whole cap)."""
    per = {"xlo": 4095 * 7, "wlo": 7 * 4095}.get(family)
    if per is None:
        return 1.0
    d = 1.0
    while d * terms(c) * per > CAP / 3 and d > 1e-3:
        d /= 2
    return d


@functools.lru_cache(maxsize=None)
def make(c, family):
    """(x, w, b) float32 of a case; b is drawn also for a case that runs without a bias (it is then not passed)."""
    return _draw(c, family, density(c, family), 0)


@functools.lru_cache(maxsize=None)
def want(c, family):
    """The float64 reference of a case's draw, computed once; callers must not write to it."""
    x, w, b = make(c, family)
    y = case_reference(c, x, w, b)
    y.setflags(write=False)
    return y


def check(c, family, got, what):
    ref = want(c, family)
    assert got.shape == ref.shape and got.dtype == np.float32, (what, got.shape, ref.shape)
    if family == "gauss":
        x, w, b = make(c, family)
        a = (lambda v: v) if c.act is None else (lambda v: np.clip(v, c.act[0], c.act[1]))
        err = np.abs(a(got.astype(np.float64)) - ref)
        bound = gauss_bound(c, x, w, b if c.bias else None)
        bad = ~(err <= bound)
        assert not bad.any(), (what, "worst error / bound", float(np.nanmax(err / bound)), np.argwhere(bad)[:4].tolist())
    else:
        bad = ~(got.astype(np.float64) == ref)
        assert not bad.any(), (what, int(bad.sum()), "of", bad.size, "wrong; first at", np.argwhere(bad)[:4].tolist(),
                               got[bad][:4].tolist(), ref[bad][:4].tolist())


# ----------------------------------------------------------------------------- the case lists (one entry per edge)
def tap_cases():
    T = "tap"
    out = [
        # Cout_g x KT
        mk(T, "cout1_kt1", 2, 3, 5, 1, 3, 1, Tout=33),
        mk(T, "cout31_kt2", 2, 3, 5, 31, 3, 2, Tout=31),
        mk(T, "cout32_kt3", 2, 3, 5, 32, 3, 3, Tout=32),
        mk(T, "cout33_kt4", 2, 3, 5, 33, 3, 4, Tout=33, same=False),
        mk(T, "cout40_kt5", 2, 3, 5, 40, 3, 5, Tout=1, Tin=1),
        mk(T, "cout5_kt11", 3, 1, 9, 5, 5, 11, Tout=129, ST=2, SF=2),
        # Tout x ST x DT
        mk(T, "tout127_st1_dt2", 2, 2, 3, 5, 2, 3, Tout=127, DT=2),
        mk(T, "tout128_st3", 2, 2, 3, 5, 2, 5, Tout=128, ST=3),
        mk(T, "tout129_st2_dt2_nopad", 2, 2, 3, 5, 2, 11, Tout=129, ST=2, DT=2, same=False),
        # R = Cin_g KF
        mk(T, "r1", 2, 1, 4, 3, 1, 3, Tout=40),
        mk(T, "r15", 2, 5, 4, 3, 3, 3, Tout=40),
        mk(T, "r16", 2, 4, 6, 3, 4, 2, Tout=40),
        mk(T, "r17", 2, 17, 2, 3, 1, 3, Tout=40),
        mk(T, "r33", 2, 11, 4, 3, 3, 3, Tout=40),
        # SF, DF
        mk(T, "sf2_df3", 2, 2, 11, 4, 3, 3, Tout=20, SF=2, DF=3),
        mk(T, "sf3_df2", 2, 2, 11, 4, 3, 3, Tout=20, SF=3, DF=2),
        mk(T, "sf3_df2_nopad", 2, 2, 11, 4, 3, 3, Tout=20, SF=3, DF=2, same=False),
        # groups: two groups of 33 output channels (a 32-tile and a tail each), depthwise
        mk(T, "groups2", 2, 4, 3, 66, 2, 3, Tout=33, groups=2),
        mk(T, "depthwise_df2", 2, 3, 5, 6, 3, 5, Tout=130, groups=3, DF=2),
        # lens, bias, clamp
        mk(T, "lens_null", 2, 3, 4, 5, 3, 5, Tout=70, lens=None),
        mk(T, "lens_1_and_beyond", 3, 3, 4, 5, 3, 5, Tout=70, lens=(1, 99, 40)),
        mk(T, "bias_null", 2, 3, 4, 5, 3, 4, Tout=70, bias=False),
        mk(T, "clamp_cuts_some", 2, 3, 4, 5, 3, 3, Tout=70, act=(-50.0, 120.0)),
        mk(T, "conv1d_k11", 2, 33, 1, 40, 1, 11, Tout=129, ST=2),
    ]
    return out


def cl_cases():
    E = "cl"
    return [
        mk(E, "cin16_cout16_t47_kt1", 1, 16, 3, 16, 1, 1, Tout=47),
        mk(E, "cin32_cout32_t48_kt2", 2, 32, 4, 32, 3, 2, Tout=48, SF=2),
        mk(E, "cin48_cout33_t49_kt3", 2, 48, 5, 33, 3, 3, Tout=49, DF=2),
        mk(E, "cout40_t127_kt5_dt2", 2, 16, 8, 40, 5, 5, Tout=127, DT=2),
        mk(E, "cout64_t128_st2", 2, 16, 1, 64, 1, 3, Tout=128, ST=2),
        mk(E, "cout29_t129_kt11_st3", 2, 16, 3, 29, 3, 11, Tout=129, ST=3),
        mk(E, "fout2_sf2_df2_nopad", 2, 16, 7, 16, 3, 3, Tout=50, SF=2, DF=2, same=False),
        mk(E, "fout3", 2, 32, 3, 16, 5, 3, Tout=33),
        mk(E, "fout9_t48_kt11", 2, 16, 9, 33, 3, 11, Tout=48),
        mk(E, "n5_t47_st2_dt2", 5, 16, 2, 16, 1, 3, Tout=47, ST=2, DT=2),
        mk(E, "lens_null_bias_null", 2, 16, 3, 16, 3, 3, Tout=49, lens=None, bias=False),
        mk(E, "clamp", 2, 16, 3, 16, 3, 3, Tout=49, act=(0.0, 200.0), lens=(60, 1)),
        # the short kernel (Cin = 32, ST = DT = 1, Tout <= 16) and its neighbour on the 32-frame tile
        mk(E, "short_t1", 2, 32, 5, 16, 3, 3, Tout=1, Tin=1),
        mk(E, "short_t15_cout29", 5, 32, 9, 29, 5, 11, Tout=15, SF=2),
        mk(E, "short_t16_cout33_n70", 70, 32, 2, 33, 3, 5, Tout=16),
        mk(E, "short_t16_fout26", 1, 32, 26, 16, 3, 3, Tout=16),
        mk(E, "tile32_t17", 2, 32, 9, 29, 5, 11, Tout=17, SF=2),
        mk(E, "cin16_t16_not_short", 2, 16, 3, 16, 3, 3, Tout=16),
    ]


def fwin_cases():
    E = "fwin"
    return [
        mk(E, "kf15_sf2_t48", 2, 1, 20, 32, 15, 1, Tout=48, SF=2),
        mk(E, "kf16_sf4_t49", 2, 1, 33, 40, 16, 3, Tout=49, SF=4),
        mk(E, "kf17_sf2_t128_st2", 2, 1, 21, 32, 17, 3, Tout=128, SF=2, ST=2),
        mk(E, "kf41_sf2_t129_fin80", 2, 1, 80, 96, 41, 11, Tout=129, SF=2, ST=2),
        mk(E, "kf41_sf4_fin81_nopad", 2, 1, 81, 32, 41, 3, Tout=49, SF=4, same=False),
        mk(E, "ds2_fin81_tin301", 3, 1, 81, 32, 41, 11, Tin=301, SF=2, ST=2),
        mk(E, "lens_null_bias_null_clamp", 2, 1, 20, 32, 15, 3, Tout=50, SF=2, lens=None, bias=False, act=(0.0, 20.0)),
        mk(E, "kf41_t48_dt2", 1, 1, 80, 40, 41, 3, Tout=48, SF=2, DT=2),
    ]


def gemm1d_cases():
    E = "gemm1d"
    return [
        mk(E, "k31_t1_cout1", 2, 31, 1, 1, 1, 1, Tout=1, Tin=1),
        mk(E, "k32_t31_cout63", 2, 16, 1, 63, 1, 2, Tout=31, same=False),
        mk(E, "k33_t32_cout64_st2", 2, 11, 1, 64, 1, 3, Tout=32, ST=2),
        mk(E, "k55_t33_cout65_dt2", 3, 5, 1, 65, 1, 11, Tout=33, DT=2),
        mk(E, "k96_t33_st2_dt2_pad5", 2, 32, 1, 65, 1, 3, Tout=33, ST=2, DT=2)._replace(pad_t=5),
        mk(E, "k96_bias_null_clamp", 2, 8, 1, 33, 1, 12, Tout=40, bias=False, act=(-30.0, 500.0), lens=(1, 99)),
    ]


ENTRY_CASES = {"tap": tap_cases, "cl": cl_cases, "fwin": fwin_cases, "gemm1d": gemm1d_cases}


def cases(entry):
    return ENTRY_CASES[entry]()


def families(c, one_plane=False):
    """The exact families of a case; the one-plane fp16 mode has no lo plane to carry xlo / wlo."""
    return ("dense",) if one_plane else EXACT_FAMILIES


# hand-over pairs: (conv1 case [entry fwin], conv2 case [entry cl]); conv2's input is conv1's clamped output
def handover_pairs():
    c1 = mk("fwin", "ds2_conv1_80x130", 2, 1, 80, 32, 41, 11, Tin=130, SF=2, ST=2, act=(0.0, 20.0))
    c2 = mk("cl", "ds2_conv2", 2, 32, c1.Fout, 32, 21, 11, Tin=c1.Tout, SF=2, act=(0.0, 20.0), lens=pair_lens(c1))
    s1 = mk("fwin", "small_conv1", 2, 1, 24, 16, 9, 5, Tin=101, SF=2, ST=2, act=(0.0, 4095.0))
    s2 = mk("cl", "small_conv2", 2, 16, s1.Fout, 33, 3, 3, Tin=s1.Tout, act=None, lens=pair_lens(s1))
    assert terms(s2) <= 585
    return [(c1, c2), (s1, s2)]


def pair_lens(c1):
    """Lengths after conv1 (floor((len + pads - span) / stride) + 1 with the module's SAME pads), as the modules hand them on."""
    total = c1.ST * cdiv(c1.Tin, c1.ST) - 1 + c1.DT * (c1.KT - 1) + 1 - c1.Tin
    return tuple(max(1, (v + total - (c1.DT * (c1.KT - 1) + 1)) // c1.ST + 1) for v in eff_lens(c1))


PAIR_FAMILIES = ("dense", "xlo", "wlo")


@functools.lru_cache(maxsize=None)
def make_pair(c1, c2, family):
    """x, w1, b1 of ``family`` for conv1; conv2's weights are always the small nonzero integers of ``dense`` (its input,
    conv1's clamped output, is what it is), so that conv2's cap holds."""
    x, w1, b1 = make(c1, family)
    _, w2, b2 = make(c2, "dense")
    if family == "dense" and c1.act[1] > 2048:
        x = x * np.float32(16)      # (still one plane: 4 bits and a power of two) so that conv1's sums spread past 2048
    return x, w1, b1, w2, b2


@functools.lru_cache(maxsize=None)
def want_pair(c1, c2, family):
    x, w1, b1, w2, b2 = make_pair(c1, c2, family)
    y1 = case_reference(c1, x, w1, b1)
    y2 = case_reference(c2, y1, w2, b2)
    y1.setflags(write=False)
    y2.setflags(write=False)
    return y1, y2


# ----------------------------------------------------------------------------- isolation
def isolation_cases(entry):
    """Cases (no clamp, ``dense`` draw) whose windows have ghosts: an odd KT (the tap kernel pairs taps), KF below a multiple of
    16 (the feature-window kernels pad it), tile boundaries inside Tout, two utterances."""
    return {
        "tap": [mk("tap", "iso_kt11_st2", 2, 3, 6, 5, 3, 11, Tin=70, ST=2, lens=(70, 66)),
                mk("tap", "iso_kt3_dt2", 2, 17, 2, 33, 1, 3, Tin=140, DT=2, lens=(140, 131)),
                mk("tap", "iso_kt5_nopad", 2, 2, 4, 4, 2, 5, Tin=50, same=False, lens=(50, 45))],
        "cl": [mk("cl", "iso_cl_kt11", 2, 32, 5, 33, 3, 11, Tin=140, lens=(140, 131)),
               mk("cl", "iso_cl_short", 2, 32, 5, 16, 3, 5, Tin=16, lens=(16, 13)),
               mk("cl", "iso_cl_t40_st2", 2, 16, 4, 16, 3, 3, Tin=80, ST=2, lens=(80, 70))],
        "fwin": [mk("fwin", "iso_fwin_kf41", 2, 1, 80, 32, 41, 11, Tin=140, SF=2, ST=2, lens=(140, 131)),
                 mk("fwin", "iso_fwin_kf17_t40", 2, 1, 30, 32, 17, 3, Tin=40, SF=2, lens=(40, 33))],
        "gemm1d": [mk("gemm1d", "iso_gemm1d", 2, 5, 1, 33, 1, 11, Tin=70, ST=2, lens=(70, 66))],
    }[entry]


ISOLATION_CLAMP = (-50.0, 120.0)


def clamped_isolation_cases(entry):
    """The isolation cases with the clamp activation in the epilogue (same draw: ``make`` does not look at the activation).
    The dense outputs spread over thousands around a bias of up to 1000, so the clamp cuts most of them and not all
    (tests/test_conv_exact_cpu.py checks that)."""
    return [c._replace(tag=c.tag + "_clamp", act=ISOLATION_CLAMP) for c in isolation_cases(entry)]


def isolation_positions(c):
    """[(label, n, ch, f, t)]: single in-length input positions aimed at the ghosts of the kernels."""
    L = eff_lens(c)
    n1 = c.N - 1
    fm, cm = c.Fin // 2, (c.Cin - 1) // 2
    out = []
    # the frame one tap past the window of output frame `to` (the zero tap an odd KT is paired with)
    for to in (1, c.Tout // 2, 31, 32):
        t = to * c.ST - c.pad_t + c.KT * c.DT
        if 0 <= to < c.Tout and 0 <= t < L[n1]:
            out.append((f"one_tap_past_to{to}", n1, cm, fm, t))
    # feature rows just under a window: offsets KF .. 16 ceil(KF / 16) - 1 of the window of output row fo
    for fo in (0, 1, c.Fout // 2):
        for off in (c.KF, 16 * cdiv(c.KF, 16) - 1):
            f = fo * c.SF - c.pad_f + off * c.DF
            if 0 <= f < c.Fin and fo < c.Fout:
                out.append((f"row_under_window_fo{fo}_off{off}", n1, cm, f, L[n1] // 2))
    out.append(("last_real_frame", n1, cm, fm, L[n1] - 1))
    # the input frame that the last output frame of a 32- / 128-frame tile reads last
    for to in (31, 127):
        t = to * c.ST - c.pad_t + (c.KT - 1) * c.DT
        if to < c.Tout - 1 and 0 <= t < L[n1]:
            out.append((f"last_frame_of_tile_to{to}", n1, 0, 0, t))
    out.append(("last_channel_of_granule", n1, min(15, c.Cin - 1), fm, L[n1] // 3))
    out.append(("last_channel", n1, c.Cin - 1, c.Fin - 1, 0))
    out.append(("utterance0", 0, cm, fm, min(L[0] - 1, L[n1] // 2)))
    seen, uniq = set(), []
    for p in out:
        if p[1:] not in seen:
            seen.add(p[1:])
            uniq.append(p)
    return uniq


# ----------------------------------------------------------------------------- routes, restated from csrc/conv_cl.hip
def cl_tile(N, KG, Fout, Tout, KT, ST, DT, Cout):
    """``conv_cl_plan``: 4 = 32 frames x 8 rows per workgroup, 1 = 128 frames x 2 rows, 0 = neither fits 160 KiB of LDS."""
    if N * cdiv(Cout, 32) > 65535:
        return 0
    wbytes = 2 * ((KT + 1) // 2) * KG * 32 * 16
    for wf in (4 if Tout <= 48 else 1, 1):
        tt, rf = 128 // wf, 2 * wf
        pw = (tt - 1) * ST + (KT - 1) * DT + 1
        if 2 * rf * KG * pw * 16 + wbytes <= 160 * 1024 and cdiv(Fout, rf) <= 65535:
            return wf
    return 0


def cl_route(c):
    """'short', 'tile32', 'tile128' or None for a channels-last case (``conv_cl_short_plan`` restated for shapes whose staged
    rows fit LDS, which holds for every case here: at most 12 output rows per workgroup)."""
    wf = cl_tile(c.N, c.Cin // 8, c.Fout, c.Tout, c.KT, c.ST, c.DT, c.Cout)
    if wf == 0:
        return None
    if c.Cin == 32 and c.Tout <= 16 and c.ST == 1 and c.DT == 1 and c.KT <= 11:
        return "short"
    return "tile32" if wf == 4 else "tile128"


def fwin_kfp(KF):
    return cdiv(KF, 16) * 16


def fwin_route(c, variant=0):
    """'shared', 'tile32', 'tile128' or None for a feature-window case (``conv_fs_plan`` then ``conv_cl_plan``)."""
    KG = fwin_kfp(c.KF) // 8
    if variant == 0 and c.Tout > 48 and c.SF % 2 == 0:
        g = int(np.gcd(16, 2 * c.SF))
        cs = 16 // g
        rg = cs * c.SF // 8
        sg = 9 * rg + KG
        pw = 63 * c.ST + (c.KT - 1) * c.DT + 1
        lds = 2 * (sg * c.ST * cdiv(pw, c.ST) * 16 + 2 * KG * 32 * 16)
        if sg <= 16 and 2 * KG * 32 <= 512 and lds <= 160 * 1024:
            return "shared"
    wf = cl_tile(c.N, KG, c.Fout, c.Tout, c.KT, c.ST, c.DT, c.Cout)
    return {0: None, 4: "tile32", 1: "tile128"}[wf]


# ----------------------------------------------------------------------------- emulations (for the CPU test)
def round_fp16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float64)


def round_bf16(a):
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def split(a, rnd):
    """(hi, lo) of the kernels' plane split: hi = rn(a), lo = rn(a - hi)."""
    a = np.asarray(a, dtype=np.float64)
    hi = rnd(a)
    return hi, rnd(a - hi)
