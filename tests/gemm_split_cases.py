"""Cases, operand families, the restated plane arithmetic and the restated launcher of the split-operand GEMM family
(csrc/gemm_split.hip behind ``ms_linear_split_forward`` / ``ms_linear_split_pack`` / ``ms_linear_split_forward_packed``):
y[M, N] = act(x[M, K] . w[N, K]^T + bias[N]) with every float32 operand split into narrow planes.  numpy only; imports
nothing from the package.  tests/test_gemm_split_cpu.py proves what this module promises, tests/gemm_split_run.py and
tests/test_gemm_split_gpu.py run it through the C ABI.  No tolerance appears anywhere: every expected value is exact.

The arithmetic, restated (csrc/common.h)
  mode      planes                      result
  f16x3     fp16 hi + lo (default)      sum_k (xh wh + xl wh + xh wl) + bias          (xl wl is absent)
  bf16x3    bf16 hi + lo                the same
  fp16      one fp16 plane              sum_k xh wh + bias
  hi = rn(x), lo = rn(x - hi) with the subtraction in float32 and rn = round to nearest even.  The fp16 formats clamp a
  finite value to +-65504 before EACH rounding ("operands are clamped to +-65504 before the split"), so 65504 + 32 and
  2 x 65504 still come out exact through the lo plane and anything beyond reads as 131008; the one-plane mode keeps 65504.
  Products and sums are float32.  The clamp activation applies after the sum.

Exactness.  A family is built per plane format so that, for every output element (m, n), every product lies on one
power-of-two grid g(m, n) and sum_k |term| + |bias| < 2^24 g(m, n).  Every partial sum of every summation order is then a
multiple of g below 2^24 g, i.e. a float32 number: the device result does not depend on the order, and the float64 BLAS
product of the planes (53 bits) is THE value.  ``exactness`` computes that ratio per output; the CPU test holds it below 2^24.

Families
  hi        x integers in [-127, 127], w in [-7, 7], bias in [-1000, 1000]: all lo planes are zero.
  lo        a + b 2^-s: a a non-zero integer with |a| <= A, b in {-1, 0, 1}, s = 9 (bf16: 8 significant bits) or 12 (fp16: 11),
            so b 2^-s is below half an ulp of a and the split is exactly (a, b 2^-s).  A = 3 where K allows it
            (K A^2 2^s + 8 2^s < 2^24), else 2 or 1; bias integers in [-8, 8].  Two thirds of the elements have b != 0.
  coded-w   x[m, :] is 1 at k_m = (37 m + 5) mod K and 0 elsewhere (37 is coprime to every K here: K consecutive rows visit
            every k; 32 consecutive rows every position of a K-block); w[n, k] = 1 + (k mod 64) + 64 (n mod R), R = 256
            (14 bits: exact in hi + lo of both formats) or 32 in the one-plane mode (<= 2048: exact in fp16).  y[m, n] names the
            single element that was read.  bias 0.
  coded-x   the mirror image: w[n, :] one-hot at k_n, x[m, k] the code of (m mod R, k mod 64).
  clamp     x in {-1, 0, 1}, w in {-1, 0, 1} with about 6 non-zeros per row, bias in [-1, 1], activation bounds (-2, 3):
            outputs are small integers that fall below, inside, above and exactly on both bounds.
  range     (fp16 formats) integers in [-3, 3] with single elements of x and of w at +-65504, 65504 + 32, 2 x 65504, 10^6
            and -3 10^5, and rows of x / w that are zero except for values 2^-10 + c 2^-24 whose lo part is fp16-subnormal.
            bias 0.  Needs 16 rows and 16 columns to keep the large and the tiny values in different rows.

The launcher (``gemm_bf16x3_launch_ld``), restated in ``route``: which kernel a call runs on, from the shape, the mode, the
``ms_gemm_set_variant`` value, the two per-call switches MS_GEMM_TILE64 / MS_GEMM_QUARTER_TILE and the CU count.  The case
list is sized for 256 CUs.  Every case runs under every configuration of ``CONFIGS``; the edges below are then counted per
kernel over everything that reaches it.  A kernel that only large outputs reach cannot see M = 1 (kernel4 would need N of four
million), so an edge is a property of the LAST tile: one row, tile - 1 rows, a full tile, and one row with a full tile before
it (tile + 1); the same for columns.
"""
import collections

import numpy as np

MODES = ("f16x3", "bf16x3", "fp16")
FAMILIES = ("hi", "lo", "coded-w", "coded-x", "clamp", "range")
CLAMP_ACT = (-2.0, 3.0)
F16_MAX = 65504.0
VARIANTS = (0, 2, 7, 8, 9, 10, 11)
# (variant, MS_GEMM_TILE64, MS_GEMM_QUARTER_TILE): None = unset
CONFIGS = tuple((v, None, None) for v in VARIANTS) + ((0, "0", None), (0, None, "0"))
CUS = 256
KBLOCKS = (1, 2, 3, 4, 5, 7, 8, 9)
TILES = {"tile64": (64, 64), "kernel": (256, 128), "kernel2": (256, 256), "kernel4": (256, 256), "kernel4h": (256, 128),
         "kernel4q": (128, 128), "kernel4n": (256, 128), "kernel4n<2>": (256, 128), "kernel4n<6>": (256, 128),
         "kernel4n<3,spaced>": (256, 128), "kernel4n<2,spaced>": (256, 128)}


def fmt_of(mode):
    return "bf16" if mode == "bf16x3" else "f16"


def two_planes(mode):
    return mode != "fp16"


# ----------------------------------------------------------------------------- plane arithmetic
def rn_f16(a):
    """float32 -> fp16 -> float32, round to nearest even."""
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def rn_bf16(a):
    """float32 -> bfloat16 -> float32, round to nearest even, in integer arithmetic on the bits (finite values)."""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def plane(a, fmt):
    """One plane of finite float32 values: the fp16 formats clamp to +-65504 first."""
    a = np.asarray(a, dtype=np.float32)
    assert np.isfinite(a).all()
    return rn_f16(np.clip(a, np.float32(-F16_MAX), np.float32(F16_MAX))) if fmt == "f16" else rn_bf16(a)


def split(a, fmt):
    """(hi, lo) float32: hi = rn(a), lo = rn(a - hi), the subtraction in float32."""
    a = np.asarray(a, dtype=np.float32)
    hi = plane(a, fmt)
    return hi, plane(a - hi, fmt)


def clip(y, act):
    return y if act is None else np.clip(y, act[0], act[1])


class Planes:
    """The planes of one (x, w) draw in one mode, float64, made once."""

    def __init__(self, x, w, mode):
        self.mode = mode
        f = fmt_of(mode)
        self.xh, self.xl = (p.astype(np.float64) for p in split(x, f))
        self.wh, self.wl = (p.astype(np.float64) for p in split(w, f))
        if not two_planes(mode):
            self.xl, self.wl = np.zeros_like(self.xl), np.zeros_like(self.wl)

    def product(self, lolo=False):
        """float64 xh wh^T + xl wh^T + xh wl^T (``lolo``: + xl wl^T, the term the kernels must NOT have)."""
        y = self.xh @ self.wh.T
        if self.xl.any():
            y = y + self.xl @ self.wh.T
        if self.wl.any():
            y = y + self.xh @ self.wl.T
        if lolo:
            y = y + self.xl @ self.wl.T
        return y


def expected(x, w, b, mode, act=None, planes=None):
    """float64 act(product + bias); b None = no bias."""
    y = (planes or Planes(x, w, mode)).product()
    if b is not None:
        y = y + b.astype(np.float64)
    return clip(y, act)


def grid(a):
    """Per row of a float64 matrix: the largest power of two that divides every element (inf for a row of zeros)."""
    m, e = np.frexp(a)
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    g = np.where(mi == 0, np.inf, np.ldexp(low, e - 53))
    return g.min(axis=1)


def exactness(p, b):
    """Per output: (sum_k |term| + |bias|) / g(m, n), g the common grid of the three products (and the bias must lie on it).
    Below 2^24 the float32 result is exact in any summation order."""
    gxh, gxl, gwh, gwl = grid(p.xh), grid(p.xl), grid(p.wh), grid(p.wl)
    g = np.minimum(np.minimum(np.outer(gxh, gwh), np.outer(gxl, gwh)), np.outer(gxh, gwl))
    total = np.abs(p.xh) @ np.abs(p.wh).T + np.abs(p.xl) @ np.abs(p.wh).T + np.abs(p.xh) @ np.abs(p.wl).T
    bb = np.zeros(p.wh.shape[0]) if b is None else np.abs(b.astype(np.float64))
    total = total + bb
    g = np.where(np.isinf(g), 1.0, g)                # an all-zero row or column: every term is 0
    assert np.all(np.floor(bb / g) == bb / g), "bias off the grid"
    return total / g


# ----------------------------------------------------------------------------- families
LO_SHIFT = {"bf16": 9, "f16": 12}


def lo_amax(K, fmt):
    s = LO_SHIFT[fmt]
    for a in (3, 2, 1):
        if (K * (a * a + 2 * a * 2.0 ** -s) + 8) * 2 ** s < 2 ** 24:
            return a
    raise ValueError(("K too long for the lo family", K, fmt))


def onehot_k(rows, K):
    return (37 * np.arange(rows) + 5) % K


def code_rows(mode):
    return 256 if two_planes(mode) else 32


def codes(rows, K, mode):
    return (1 + (np.arange(K)[None, :] % 64) + 64 * (np.arange(rows)[:, None] % code_rows(mode))).astype(np.float32)


def onehot(rows, K):
    a = np.zeros((rows, K), dtype=np.float32)
    a[np.arange(rows), onehot_k(rows, K)] = 1.0
    return a


RANGE_BIG = (65504.0, -65504.0, 65536.0, 131008.0, 1.0e6, -3.0e5)
RANGE_TINY = (1, -1, 3)              # c of 2^-10 + c 2^-24


def range_k(K):
    """k positions of the special values: x's in the first, an interior and the last granule; w's beside them."""
    return (1, K // 2 + 3, K - 2), (2, K // 2 + 5, K - 3)


def families(M, K, N, mode):
    out = list(FAMILIES[:5])
    if fmt_of(mode) == "f16" and M >= 16 and N >= 16:
        out.append("range")
    return tuple(out)


def act_of(fam):
    return CLAMP_ACT if fam == "clamp" else None


def make(fam, M, K, N, mode):
    """(x [M, K], w [N, K], bias [N]) float32."""
    rng = np.random.default_rng([FAMILIES.index(fam), M, K, N])
    fmt = fmt_of(mode)
    if fam == "hi":
        x, w, b = rng.integers(-127, 128, (M, K)), rng.integers(-7, 8, (N, K)), rng.integers(-1000, 1001, N)
    elif fam == "lo":
        a, s = lo_amax(K, fmt), LO_SHIFT[fmt]

        def draw(rows):
            mag = rng.integers(1, a + 1, (rows, K)) * (rng.integers(0, 2, (rows, K)) * 2 - 1)
            return mag + rng.integers(-1, 2, (rows, K)) * 2.0 ** -s
        x, w, b = draw(M), draw(N), rng.integers(-8, 9, N)
    elif fam == "coded-w":
        x, w, b = onehot(M, K), codes(N, K, mode), np.zeros(N)
    elif fam == "coded-x":
        x, w, b = codes(M, K, mode), onehot(N, K), np.zeros(N)
    elif fam == "clamp":
        x = rng.integers(-1, 2, (M, K))
        w = rng.integers(-1, 2, (N, K)) * (rng.random((N, K)) < min(1.0, 9.0 / K))
        b = rng.integers(-1, 2, N)
    elif fam == "range":
        assert fmt == "f16" and M >= 16 and N >= 16
        x, w, b = rng.integers(-3, 4, (M, K)).astype(np.float64), rng.integers(-3, 4, (N, K)).astype(np.float64), np.zeros(N)
        kx, kw = range_k(K)
        for a_, rows, ks in ((x, M, kx), (w, N, kw)):
            # big values: one per row, rows spread over the matrix (first, interior and last tile)
            for j, v in enumerate(RANGE_BIG):
                a_[range_row(rows, j), ks[j % 3]] = v
            # tiny rows: zero except three values with an fp16-subnormal lo part
            for j in range(2):
                r = range_row(rows, len(RANGE_BIG) + j)
                a_[r] = 0.0
                for k, c in zip(ks, RANGE_TINY):
                    a_[r, k] = (2.0 ** -10 + c * 2.0 ** -24) * (1 - 2 * j)
    else:
        raise KeyError(fam)
    return np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32), np.asarray(b, dtype=np.float32)


def range_row(rows, j):
    """Eight distinct rows: 0, 1, two in the middle, the last four."""
    return (0, rows - 1, rows // 2, 1, rows - 2, rows // 2 + 1, rows - 3, rows - 4)[j]


# ----------------------------------------------------------------------------- the launcher
def cdiv(a, b):
    return -(-a // b)


def route(M, K, N, prec, variant=0, tile64_env=None, quarter_env=None, num_cus=CUS):
    """``gemm_bf16x3_launch_ld`` restated for a dense whole-K call with the row count on the host (lda = ldw = K, no m_eff,
    the read-once tuning switches unset): the name of the kernel in ``TILES``."""
    assert prec in MODES and K % 32 == 0
    f16 = prec == "fp16"
    tiles256 = cdiv(M, 256) * cdiv(N, 256)
    tiles128 = cdiv(M, 256) * cdiv(N, 128)
    starved = tiles256 * 4 < num_cus * 3 and tiles128 > tiles256
    t64 = tile64_env != "0" and variant == 0 and cdiv(M, 64) * cdiv(N, 64) <= 2 * num_cus
    offsets32 = max(M * K, N * K) * 2 < 2 ** 31
    if t64 and tiles128 * 4 <= num_cus:
        return "tile64"
    if starved and M * N >= 1024 * 1024 and variant == 0 and offsets32:
        if quarter_env != "0" and tiles128 * 2 <= num_cus and cdiv(M, 128) > cdiv(M, 256):
            return "kernel4q"
        return "kernel4h"
    if f16 or (not starved and M * N >= 4 * 1024 * 1024):
        if variant != 2 and offsets32:
            if 7 <= variant <= 11:
                if prec == "bf16x3":
                    return {7: "kernel4n", 8: "kernel4n<2>", 9: "kernel4n<6>", 10: "kernel4n<3,spaced>", 11: "kernel4n<2,spaced>"}[variant]
                return "kernel4n"
            return "kernel4"
        return "kernel2"
    if t64:
        return "tile64"
    return "kernel"


def workspace_bytes(M, K, N):
    """include/ms_hotpath.h: the four planes, x's and w's each rounded up to 256 bytes."""
    if M <= 0 or K <= 0 or N <= 0:
        return 0
    return cdiv(M * K * 4, 256) * 256 + cdiv(N * K * 4, 256) * 256


def packed_bytes(K, N):
    return 0 if K <= 0 or N <= 0 else cdiv(N * K * 4, 256) * 256


def x_workspace_bytes(M, K):
    return cdiv(M * K * 4, 256) * 256


# ----------------------------------------------------------------------------- cases
Case = collections.namedtuple("Case", "group M K N")

# group -> the kernel its cases reach with nothing set, per mode, on 256 CUs
INTENDED = {"small": "tile64", "quarter": "kernel4q", "half": "kernel4h", "full": "kernel4"}
# K = 32 x (1, 2, 3, 4, 5, 7, 8, 9) and one long K in every group
SHAPES = {
    "small": ((1, 32, 1), (66, 32, 70), (63, 64, 65), (64, 96, 63), (65, 128, 64), (255, 160, 129), (256, 224, 127), (257, 256, 128),
              (130, 288, 132), (150, 2048, 140)),
    "quarter": ((129, 32, 8321), (255, 64, 8319), (256, 96, 8320), (257, 128, 4225), (383, 160, 4223), (384, 224, 4224),
                (300, 256, 4228), (130, 288, 8200), (300, 640, 4200)),
    "half": ((100, 32, 10500), (257, 64, 8321), (255, 96, 16511), (256, 128, 16512), (513, 160, 8447), (128, 224, 8193),
             (64, 256, 16388), (511, 288, 8320), (100, 640, 10500)),
    "full": ((3329, 32, 3329), (3583, 64, 3583), (3584, 96, 3584), (3330, 128, 3332), (3329, 160, 3584), (3400, 224, 3457),
             (3583, 256, 3330), (3584, 288, 3455), (3330, 640, 3330)),
}


def cases(group=None):
    return [Case(g, *s) for g in SHAPES if group in (None, g) for s in SHAPES[g]]


def tag(c):
    return f"{c.group}-{c.M}x{c.K}x{c.N}"


def routes(c, mode, num_cus=CUS):
    """{config: kernel} of one case in one mode."""
    return {cfg: route(c.M, c.K, c.N, mode, cfg[0], cfg[1], cfg[2], num_cus) for cfg in CONFIGS}


def reached(mode, num_cus=CUS):
    """{kernel: [(case, config)]} over the whole list in one mode."""
    out = collections.defaultdict(list)
    for c in cases():
        for cfg, k in routes(c, mode, num_cus).items():
            out[k].append((c, cfg))
    return out


def kernels_of(mode):
    """The kernel instantiations a mode has."""
    if mode == "bf16x3":
        return tuple(TILES)
    if mode == "f16x3":
        return ("tile64", "kernel", "kernel2", "kernel4", "kernel4h", "kernel4q", "kernel4n")
    return ("tile64", "kernel2", "kernel4", "kernel4h", "kernel4q", "kernel4n")      # one plane: never the 256 x 128 register kernel


def nonfinite_cases():
    """One small case per kernel for the non-finite contract: (case, config) with more than one tile and K-block where the
    kernel allows it at a small size."""
    return [(Case("small", 130, 96, 132), (0, None, None)),          # tile64
            (Case("small", 257, 96, 130), (0, "0", None)),           # kernel (one plane: kernel4)
            (Case("quarter", 300, 96, 4200), (0, None, None)),       # kernel4q
            (Case("half", 100, 96, 10500), (0, None, None)),         # kernel4h
            (Case("full", 3330, 96, 3330), (0, None, None)),         # kernel4
            (Case("full", 3330, 96, 3330), (2, None, None)),         # kernel2
            (Case("full", 3330, 96, 3330), (7, None, None)),         # kernel4n
            (Case("full", 3330, 96, 3330), (9, None, None))]         # kernel4n<6> with bf16 planes


def nonfinite_positions(rows, K):
    """(row, k) in the first, an interior and the last tile and K-block."""
    return ((0, 0), (rows // 2 + 1, K // 2 + 1), (rows - 1, K - 1))
