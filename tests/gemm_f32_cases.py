"""Cases, input families and float64 references for the exact-float32 GEMM (``ms_linear_forward`` /
``ms_linear_splitk_forward``): y[M, N] = act(x[M, K] . w[N, K]^T + bias[N]).  Imports without a GPU; tests/test_gemm_f32_cpu.py
proves what the families promise, tests/test_gemm_f32_gpu.py runs them through the C ABI.

Three input families.

``dense``   x integers in [-X, X], w integers in [-7, 7], bias integers in [-1000, 1000], X = 2047 for K <= 1024 (for the few
            longer K of the training and K-slice shapes X shrinks so that the cap below still holds).  sum_k |x||w| + |bias| <
            2^24, so every partial sum in every order of float32 accumulation -- K slices included -- is an integer below 2^24
            and therefore exact: the result is THE integer, compared with ``array_equal``.  A dropped, doubled or misrouted k,
            row or column is an integer error.
``onehot``  x[m, :] is zero except at k_m = (7 m + 3) mod K; that value and every w are odd integers in [2049, 2895] with
            random signs (12 significant bits; every product is below 2^23), bias integers in [-1000, 1000].
            y[m, n] = x[m, k_m] w[n, k_m] + bias[n] is exact in float32 for any K, compared with ``array_equal``.  A float32
            product is exact here; a hi + lo three-pass product (hi.hi + lo.hi + hi.lo, fp16 or bf16 halves) drops lo.lo, which
            is a nonzero integer for these values, so the family tells the two apart and visits k positions one at a time.
``gauss``   x, w, bias N(0, 1) float32.  |y - ref| <= (K + 9) 2^-24 (|x| . |w|^T + |bias|): the standard bound for a sum of
            K products and a bias with K + 1 IEEE roundings in any order (Higham, Accuracy and Stability, section 3.1), plus
            eight roundings for the additions of up to eight K slices.  Derived, not measured.  With a clamp both sides are
            clipped first (clipping never moves two numbers apart).
"""
import numpy as np

U = 2.0 ** -24                      # float32 unit roundoff
FAMILIES = ("dense", "onehot", "gauss")
ACTS = (None, (0.0, 20.0))
FEW_ROWS = 1                        # MS_LINEAR_FEW_ROWS

# ----------------------------------------------------------------------------- shapes
EDGE_M = (1, 31, 32, 33, 127, 128, 129, 257)
EDGE_N = (1, 31, 32, 33, 63, 64, 65, 129)
# the 32-wide K tile, one / two / three trips of the double buffer, K % 4 != 0
EDGE_K = (1, 2, 3, 4, 5, 31, 32, 33, 36, 64, 100, 127, 128, 129)
# the ones-row db product (M = 1, K = T.N) and a dW product, both with K % 4 != 0: the scalar-load path
TRAINING_SHAPES = ((1, 2001, 36), (64, 1999, 36))


def plain_shapes():
    """(M, K, N) for ms_linear_forward: 32 shapes in which every edge M meets four edge N, 28 in which every edge K occurs
    twice (with other M and N), and the two training shapes."""
    out = []
    for j in range(4):
        for i, m in enumerate(EDGE_M):
            out.append((m, EDGE_K[(5 * len(out)) % len(EDGE_K)], EDGE_N[(i + 2 * j + (j >> 1)) % 8]))
    for i, k in enumerate(EDGE_K):
        out.append((EDGE_M[(3 * i) % 8], k, EDGE_N[(3 * i + 1) % 8]))
        out.append((EDGE_M[(5 * i + 4) % 8], k, EDGE_N[(5 * i + 6) % 8]))
    seen, uniq = set(), []
    for s in out + list(TRAINING_SHAPES):
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


# N > 64 at N = 1000, K = 36: the tile configuration depends on the number of compute units
REGIME_N, REGIME_K = 1000, 36
REGIMES = ("128x32", "128x64", "128x128")


def cdiv(a, b):
    return -(-a // b)


def tile_regime(M, N, cus):
    """csrc/gemm.hip ``linear_launch`` restated: the tile configuration of ms_linear_forward."""
    if N <= 32:
        return "128x32"
    if N <= 64:
        return "128x64"
    wg128 = cdiv(M, 128) * cdiv(N, 128)
    if wg128 * 4 <= cus:
        return "128x32"
    if wg128 * 2 <= cus:
        return "128x64"
    return "128x128"


def regime_ms(cus):
    """Three ragged M that land in the three configurations at N = 1000 on a part with ``cus`` compute units: 100 rows, 37
    rows past the last row count of 128 x 32, 37 rows past the last of 128 x 64 (on 256 CUs: 100, 128.8 + 37, 128.16 + 37)."""
    cols = cdiv(REGIME_N, 128)
    return (100, 128 * (cus // (4 * cols)) + 37, 128 * (cus // (2 * cols)) + 37)


# split-K
SPLITK_M = (1, 127, 129, 300)
SPLITK_K = (512, 520, 641, 1000, 2560)
SPLITK_N = (1, 29, 64)
SPLITK_N_FEW_ROWS = (65, 200)
QUERY_K = (511, 512, 520, 641, 1000, 1024, 2560, 4100)
QUERY_N = (1, 29, 64, 65, 200, 4096, 4097)


def splitk_cases():
    """(K, N, flags): 15 with the plain flags, 10 with MS_LINEAR_FEW_ROWS; each runs at every M of SPLITK_M."""
    return [(k, n, 0) for k in SPLITK_K for n in SPLITK_N] + [(k, n, FEW_ROWS) for k in SPLITK_K for n in SPLITK_N_FEW_ROWS]


def splitk_slices(K, N, flags):
    """include/ms_hotpath.h restated: min(8, K / 128) slices when K >= 512 and (N <= 64, or MS_LINEAR_FEW_ROWS and N <= 4096)."""
    if K >= 512 and (N <= 64 or ((flags & FEW_ROWS) and N <= 4096)):
        return min(8, K // 128)
    return 0


def splitk_workspace_bytes(M, K, N, flags):
    return cdiv(splitk_slices(K, N, flags) * M * N * 4, 256) * 256


# ----------------------------------------------------------------------------- families
def dense_x_max(K):
    """2047 for K <= 1024; for a longer K the largest X with 7 K X + 1000 < 2^24."""
    return min(2047, (2 ** 24 - 1001) // (7 * K))


def _rng(family, M, K, N):
    return np.random.default_rng([FAMILIES.index(family), M, K, N])


def _signs(rng, shape):
    return rng.integers(0, 2, size=shape) * 2 - 1


def make(family, M, K, N):
    """(x [M, K], w [N, K], bias [N]) float32."""
    rng = _rng(family, M, K, N)
    if family == "dense":
        xm = dense_x_max(K)
        x = rng.integers(-xm, xm + 1, size=(M, K))
        w = rng.integers(-7, 8, size=(N, K))
    elif family == "onehot":
        x = np.zeros((M, K), dtype=np.int64)
        rows = np.arange(M)
        x[rows, onehot_k(M, K)] = (2 * rng.integers(1024, 1448, size=M) + 1) * _signs(rng, M)        # odd, 2049 .. 2895
        w = (2 * rng.integers(1024, 1448, size=(N, K)) + 1) * _signs(rng, (N, K))
    elif family == "gauss":
        return (rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32),
                rng.standard_normal(N).astype(np.float32))
    else:
        raise KeyError(family)
    b = rng.integers(-1000, 1001, size=N)
    return x.astype(np.float32), w.astype(np.float32), b.astype(np.float32)


def onehot_k(M, K):
    return (7 * np.arange(M) + 3) % K


def clip(y, act):
    return y if act is None else np.clip(y, act[0], act[1])


def reference(x, w, b, act=None):
    """float64 act(x . w^T + b); b may be None."""
    y = x.astype(np.float64) @ w.astype(np.float64).T
    if b is not None:
        y = y + b.astype(np.float64)
    return clip(y, act)


def abs_sum(x, w, b):
    """|x| . |w|^T + |b| in float64: the cap of the exact families, the scale of the gaussian bound."""
    s = np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T
    return s if b is None else s + np.abs(b).astype(np.float64)


def gauss_bound(x, w, b):
    return (x.shape[1] + 9) * U * abs_sum(x, w, b)


class Ref:
    """The float64 products of one draw, computed once and left unchanged: ``check`` serves every activation, the call
    without a bias, and calls on the leading ``M`` rows."""

    def __init__(self, family, x, w, b):
        self.family, self.K = family, x.shape[1]
        self.xw = reference(x, w, None)
        self.axw = abs_sum(x, w, None)
        self.b, self.ab = b.astype(np.float64), np.abs(b).astype(np.float64)

    def check(self, got, act, bias, what):
        """Assert a kernel result ``got`` (float32 [M, N], M leading rows of the draw) against the family's criterion."""
        M = got.shape[0]
        want = clip(self.xw[:M] + self.b if bias else self.xw[:M], act)
        assert got.shape == want.shape and got.dtype == np.float32, what
        if self.family == "gauss":
            err = np.abs(clip(got.astype(np.float64), act) - want)
            bound = (self.K + 9) * U * (self.axw[:M] + self.ab if bias else self.axw[:M])
            bad = ~(err <= bound)                    # (a NaN fails)
            assert not bad.any(), (what, "worst error / bound", float(np.nanmax(err / bound)), "at", np.argwhere(bad)[:4].tolist())
        else:
            bad = ~(got.astype(np.float64) == want)
            assert not bad.any(), (what, int(bad.sum()), "wrong; first at", np.argwhere(bad)[:4].tolist(),
                                   got[bad][:4].tolist(), want[bad][:4].tolist())


def check(family, got, x, w, b, act, what):
    """One-off form of ``Ref.check``; b None = the call without a bias."""
    Ref(family, x, w, np.zeros(w.shape[0], np.float32) if b is None else b).check(got, act, b is not None, what)


# ----------------------------------------------------------------------------- emulations (for the CPU test)
def round_fp16(a):
    return a.astype(np.float32).astype(np.float16).astype(np.float64)


def round_bf16(a):
    """float32 -> bfloat16, round to nearest even (finite values)."""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def three_pass(x, w, b, rnd):
    """A split-operand product: each operand hi + lo in the narrow format ``rnd``, hi.hi + lo.hi + hi.lo (lo.lo dropped),
    accumulated in float64 -- the arithmetic that must NOT pass for the exact-float32 kernel."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    xh, wh = rnd(x64), rnd(w64)
    xl, wl = rnd(x64 - xh), rnd(w64 - wh)
    return xh @ wh.T + xl @ wh.T + xh @ wl.T + b.astype(np.float64)


def chain_f32(x, w, b):
    """A sequential float32 chain, k ascending, product and sum rounded separately, then the bias."""
    acc = np.zeros((x.shape[0], w.shape[0]), dtype=np.float32)
    for k in range(x.shape[1]):
        acc = acc + x[:, k, None] * w[None, :, k]
    return acc + b[None, :]
