"""Cases, input families and the float64 reference of the lookahead convolution (``ms_lookahead_forward`` /
``ms_lookahead_window_forward``).  Imports without a GPU; tests/test_lookahead_cpu.py proves the reference against the
definition (right-pad context - 1 frames, depthwise conv1d), tests/test_lookahead_gpu.py runs the cases through the C ABI.

    y[n, f, t] = sum_{k < ctx} w[f, k] x[n, f, t + k]   (x reads as zero for t + k >= T_in),   t < T_out

Two input families: ``exact`` (x integers in [-1023, 1023], w integers in [-7, 7]: at most 8100 . 1023 . 7 < 2^24 whatever
the order, compared with ``array_equal``) and ``gauss`` (N(0, 1); |y - ref| <= (ctx + 1) 2^-24 sum_k |w||x|, the bound of a
sum of ctx products rounded in any order, fused or not)."""
import numpy as np

U = 2.0 ** -24
FAMILIES = ("exact", "gauss")
ACTS = (None, (-0.2, 0.25))
LAYOUTS = ("nft", "ntf")


def _cycle(vals, i):
    return vals[i % len(vals)]


def tcontig_cases():
    """(N, F, T, ctx) for time-contiguous input: every T with every ctx; 256-frame blocks, so T = 257, 300, 513 need a halo
    across a block boundary (T = 300 with ctx = 80 reads 79 frames of the second block)."""
    out = []
    for T in (1, 255, 256, 257, 300, 513):
        for ctx in (1, 2, 17, 80):
            n, f = _cycle(((1, 1), (2, 3), (1, 3), (2, 1)), len(out) + len(out) // 4)
            out.append((n, f, T, ctx))
    return out


def fcontig_cases():
    """(N, F, T, ctx, wide) for feature-contiguous input [T, N, F]: every T with every ctx (16-tap chunks: ctx = 15, 16, 17,
    32, 33; 16- and 32-frame tiles: T = 16, 17, 32, 33), F cycling over one lane, the 256-lane block edge and a second block;
    ``wide``: x is the first F columns of a [T, N, 2 F] buffer, so its time stride is not N . F."""
    out = []
    for T in (1, 16, 17, 32, 33, 70):
        for ctx in (1, 15, 16, 17, 32, 33, 80):
            out.append((2, _cycle((1, 255, 256, 257, 300), len(out)), T, ctx, len(out) % 3 == 1))
    return out


def window_cases():
    """(T_in, T_out, ctx): T_out in {1, 16, 17, T_in}; T_in - T_out both below and above ctx - 1."""
    out = []
    for T_in, ctx in ((20, 17), (40, 17), (70, 33), (100, 80), (33, 1), (18, 2)):
        for T_out in (1, 16, 17, T_in):
            out.append((T_in, T_out, ctx))
    return out


ISOLATION_CTX = (3, 17, 32)


def make(family, N, F, T, ctx, seed=0):
    """(x [N, F, T], w [F, ctx]) float32; the gaussian weights are never zero (the isolation test needs that)."""
    rng = np.random.default_rng([FAMILIES.index(family), N, F, T, ctx, seed])
    if family == "exact":
        x = rng.integers(-1023, 1024, size=(N, F, T)).astype(np.float32)
        return x, rng.integers(-7, 8, size=(F, ctx)).astype(np.float32)
    x = rng.standard_normal((N, F, T)).astype(np.float32)
    w = rng.standard_normal((F, ctx)).astype(np.float32)
    return x, np.where(np.abs(w) < 0.05, np.float32(0.5), w).astype(np.float32)


def _taps(x, w, T_out):
    """sum_k w[f, k] x[n, f, t + k] in float64, for the given x and w (pass magnitudes for the bound's scale)."""
    N, F, T = x.shape
    ctx = w.shape[1]
    xp = np.zeros((N, F, T + ctx - 1), dtype=np.float64)
    xp[:, :, :T] = x
    y = np.zeros((N, F, T_out), dtype=np.float64)
    for k in range(ctx):
        y += w[None, :, k, None].astype(np.float64) * xp[:, :, k:k + T_out]
    return y


def clip(y, act):
    """The clamp as the C ABI receives it: its limits are float arguments, so -0.2 is float32's -0.2."""
    return y if act is None else np.clip(y, float(np.float32(act[0])), float(np.float32(act[1])))


def reference(x, w, T_out=None, act=None):
    """float64 [N, F, T_out]."""
    return clip(_taps(x, w, x.shape[2] if T_out is None else T_out), act)


def gauss_bound(x, w, T_out=None):
    return (w.shape[1] + 1) * U * _taps(np.abs(x), np.abs(w), x.shape[2] if T_out is None else T_out)


def check(family, got, x, w, T_out, act, what):
    """``got``: float32 [N, F, T_out]."""
    want = reference(x, w, T_out, act)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    if family == "exact":
        bad = ~(got.astype(np.float64) == want)
    else:
        err = np.abs(clip(got.astype(np.float64), act) - want)
        bad = ~(err <= gauss_bound(x, w, T_out))
    assert not bad.any(), (what, int(bad.sum()), "wrong; first at", np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(),
                           want[bad][:4].tolist())
