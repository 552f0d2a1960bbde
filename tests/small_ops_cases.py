"""Cases, inputs, float64 references and error bounds of the small operators that every model passes through:

    ms_clamp, ms_mask_time_, ms_nct_to_tnc                  (csrc/elementwise.hip)
    ms_log_softmax_axis, ms_log_softmax_axis_backward       (csrc/ctc.hip)
    ms_ctc_greedy_decode                                    (csrc/ctc.hip)
    ms_embedding_forward, ms_rnnt_joint_forward, ms_rnnt_topk   (csrc/rnnt.hip)

numpy only; imports nothing from the package.  tests/test_small_ops_cpu.py proves the references against torch and holds a
float32 restatement of each toleranced kernel inside its bound; tests/test_small_ops_gpu.py runs the cases through the C ABI.
Inputs come from a generator seeded with the case id.

Where an operator moves or selects values without arithmetic (clamp, mask, transpose, embedding, greedy decode, top-k) the
criterion is equality of bits.  The three toleranced operators have bounds derived from the arithmetic their kernels state.

The unit is one ulp of a float32 result, at most E = 2^-23 relative.  The HIP math documentation gives expf and logf a
maximum error of 1 ulp and tanhf of 2 ulp.  Every float32 addition, multiplication and fused multiply-add is charged 1 ulp as
well (faithful rounding; the hardware rounds correctly, to half of that): a bound that charges half ulps is ATTAINED by a
single rounding (the float32 restatement came to 0.97 of it on the two-entry axes), so it would not hold another association
of the same formula, and the rule here is that the restatement may use at most half of the bound.  G(k) = k E / (1 - k E)
bounds k stacked operations; a float32 sum of n terms in ANY order is off by at most G(n) of the sum of magnitudes (n - 1
additions and one spare, as the lookahead's ctx + 1).  Every bound is a first-order sum; the second-order terms it neglects
are below 2^-10 of it (every relative perturbation involved is below 2^-10), which the factor SECOND carries.

log-softmax over an axis of A entries (log_softmax_axis_kernel): m = max x (exact); e_a = expf(x_a - m): the difference's
rounding E |d_a| passes through exp as a relative error, expf adds E; S = sum e_a: G(A); so S is off by the relative
theta = G(A) + E sum_a e_a (|d_a| + 1) / S (+ A 2^-126 for terms flushed to zero).  logf(S (1 + theta)) = log S + theta, with
E |log S| of its own.  The tail, lz = logf(S) + m and y_a = x_a - lz, is a sum of the three terms x_a, -m, -log S; in
whichever association it is evaluated ((x_a - m) - log S is the same operation) it costs at most G(2) (|x_a| + |m| + |log S|):

    |y_a - ref| <= SECOND (theta + E |log S| + G(2) (|x_a| + |m| + |log S|))

its backward (log_softmax_axis_backward_kernel): s = sum_a g_a, off by G(A) sum |g_a| in any order; expf(y_j): E; the product
and the difference are two operations on the terms g_j and exp(y_j) s, fused or not, G(2) (|g_j| + exp(y_j) |s|):

    |gx_j - ref| <= SECOND (exp(y_j) (G(A) sum |g| + E |s|) + G(2) (|g_j| + exp(y_j) |s|))

the joint (rnnt_joint_kernel): z_k = tanhf(e_k + p_k): the sum's rounding E |e_k + p_k| passes through tanh with slope
1 - z_k^2, tanhf adds 2 E |z_k|: dz_k; logit_v = sum_k w_vk z_k + b_v over J products and a bias in the order of the lanes
and of the butterfly, fused or not: E_v = G(J + 2) (sum_k |w_vk| |z_k| + |b_v|) + sum_k |w_vk| dz_k; log-sum-exp moves by at
most max_v E_v when the logits move by E; the log-softmax over the V1 logits adds its own bound from above:

    |logp_v - ref| <= SECOND (E_v + max_v E_v + log-softmax bound at A = V1)

and, since log-sum-exp is 1-Lipschitz in the maximum norm, |logsumexp_v logp_v| <= max_v of that bound."""
import zlib

import numpy as np

E = 2.0 ** -23                                 # one ulp of a float32 result, relative
SECOND = 1.0 + 2.0 ** -10
ULP_EXP, ULP_LOG, ULP_TANH = 1, 1, 2          # maximum ulp errors of expf, logf, tanhf in the HIP math documentation


def G(k):
    return k * E / (1.0 - k * E)


def rng_of(case_id):
    return np.random.default_rng(zlib.crc32(str(case_id).encode()))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same_bits_or_both_nan(a, b):
    """Element mask: equal bits, or NaN on both sides (a NaN that went through a select keeps no promise about its payload)."""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


# ----------------------------------------------------------------------------- ms_clamp
CLAMP_N = (1, 255, 256, 257, 2048 * 256 + 3)          # the last: beyond the 2048-block cap, the grid-stride loop runs again
CLAMP_LIMITS = ((0.0, 20.0), (-0.2, 0.25), (0.0, float("inf")), (-1.0, 1.0))


def clamp_specials(lo, hi):
    f = np.float32
    lo, hi = f(lo), f(hi)
    inf = f(np.inf)
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, lo, hi, np.nextafter(lo, -inf), np.nextafter(lo, inf),
                     np.nextafter(hi, -inf), np.nextafter(hi, inf), 1e-45, -1e-45, 1e-39, -1e-39, 3e38, -3e38], dtype=np.float32)


def clamp_input(n, lo, hi):
    """float32 [n]: gaussians of scale 15 with the special values (+-0, +-Inf, NaN, lo, hi and their neighbours, denormals)
    at the front, at the 256-element block edge and at the very end, as far as they fit."""
    x = (rng_of(("clamp", n, lo, hi)).standard_normal(n) * 15).astype(np.float32)
    sp = clamp_specials(lo, hi)
    k = min(n, len(sp))
    x[:k] = sp[:k]
    x[n - k:] = sp[:k][::-1]
    if n > 256 + len(sp):
        x[256 - 8:256 - 8 + len(sp)] = sp
    return x


def clamp_ref(x, lo, hi):
    """np.clip on float32 with float32 limits: NaN stays NaN."""
    y = np.clip(x, np.float32(lo), np.float32(hi))
    assert y.dtype == np.float32
    return y


# ----------------------------------------------------------------------------- ms_mask_time_
MASK_INNER = (1, 63, 64, 65, 130)                      # 64-row groups: a short last group
MASK_T = (1, 255, 256, 257, 300)                       # the 256-thread stride


def mask_lens(T):
    return np.array([0, 1, T - 1, T, T + 5, -3], dtype=np.int32)


def mask_input(inner, T):
    """(x float32 [6, inner, T] with NaN and +-Inf in about one element of eight, lens int32 [6])."""
    r = rng_of(("mask", inner, T))
    x = r.standard_normal((6, inner, T)).astype(np.float32)
    kind = r.integers(0, 24, size=x.shape)
    x[kind == 0] = np.nan
    x[kind == 1] = np.inf
    x[kind == 2] = -np.inf
    return x, mask_lens(T)


def mask_ref(x, lens):
    """Negative lengths count as 0, lengths of T and more leave the utterance alone; the tail is +0.0."""
    y = x.copy()
    for n, ln in enumerate(lens):
        y[n, :, max(int(ln), 0):] = np.float32(0.0)
    return y


# ----------------------------------------------------------------------------- ms_nct_to_tnc
NCT_SIZES = (1, 31, 32, 33, 70)
NCT_N = (1, 3)


def nct_input(N, CF, T):
    """arange-coded: a wrong index is a wrong value (all below 2^24, exact in float32)."""
    assert N * CF * T < 2 ** 24
    return np.arange(N * CF * T, dtype=np.float32).reshape(N, CF, T)


def nct_ref(x):
    return np.ascontiguousarray(x.transpose(2, 0, 1))


# ----------------------------------------------------------------------------- ms_log_softmax_axis (+ backward)
LSM_SHAPES = ((1, 1, 1), (3, 29, 1), (2, 5, 7), (1, 64, 300), (5, 2, 257), (257, 3, 1))      # (outer, axis, inner)
LSM_SCALES = (1.0, 30.0)
LSM_VARIANTS = ("plain", "neg_inf_entries", "bad_columns")


def lsm_input(shape, scale, variant):
    """float32 [outer, axis, inner].  ``neg_inf_entries``: about one entry in five is -Inf, but never a whole column (for
    axis = 1 that leaves none).  ``bad_columns``: the first columns are one of all -Inf, one with a +Inf, one with a NaN (as
    many of the three as there are columns)."""
    outer, axis, inner = shape
    r = rng_of(("lsm", shape, scale, variant))
    x = (r.standard_normal(shape) * scale).astype(np.float32)
    if variant == "neg_inf_entries":
        hole = r.random(shape) < 0.2
        keep = r.integers(0, axis, size=(outer, inner))
        hole[np.arange(outer)[:, None], keep, np.arange(inner)[None, :]] = False
        x[hole] = -np.inf
    elif variant == "bad_columns":
        cols = [(o, i) for o in range(outer) for i in range(inner)][:3]
        for k, (o, i) in enumerate(cols):
            if k == 0:
                x[o, :, i] = -np.inf
            elif k == 1:
                x[o, axis // 2, i] = np.inf
            else:
                x[o, axis - 1, i] = np.nan
    return x


def lsm_ref(x):
    """float64 x - logsumexp over axis 1 with the maximum taken out.  A column of all -Inf, or with a +Inf, or with a NaN is
    NaN throughout (Inf - Inf), as torch.log_softmax gives; a -Inf entry of any other column is -Inf."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.max(x, axis=1, keepdims=True)
        d = x - m
        s = np.sum(np.exp(d), axis=1, keepdims=True)
        return x - (np.log(s) + m)


def lsm_bound(x):
    """The bound of the module docstring, [outer, axis, inner]; NaN or Inf where the reference is not finite."""
    x = np.asarray(x, dtype=np.float64)
    A = x.shape[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.max(x, axis=1, keepdims=True)
        d = x - m
        e = np.exp(d)
        S = np.sum(e, axis=1, keepdims=True)
        inner = np.where(e > 0, e * (np.abs(np.where(e > 0, d, 0.0)) + ULP_EXP), 0.0)
        theta = G(A) + E * np.sum(inner, axis=1, keepdims=True) / S + A * 2.0 ** -126
        return SECOND * (theta + ULP_LOG * E * np.abs(np.log(S)) + G(2) * (np.abs(x) + np.abs(m) + np.abs(np.log(S))))


def lsm_backward_input(shape, scale):
    """(y float32: the log-probabilities of the ``neg_inf_entries`` draw, so some are -Inf; g float32 gaussians)."""
    y = lsm_ref(lsm_input(shape, scale, "neg_inf_entries")).astype(np.float32)
    g = rng_of(("lsm_bwd", shape, scale)).standard_normal(shape).astype(np.float32)
    return y, g


def lsm_backward_ref(y, g):
    y, g = np.asarray(y, dtype=np.float64), np.asarray(g, dtype=np.float64)
    return g - np.exp(y) * np.sum(g, axis=1, keepdims=True)


def lsm_backward_bound(y, g):
    y, g = np.asarray(y, dtype=np.float64), np.asarray(g, dtype=np.float64)
    A = y.shape[1]
    s = np.sum(g, axis=1, keepdims=True)
    e = np.exp(y)
    return SECOND * (e * (G(A) * np.sum(np.abs(g), axis=1, keepdims=True) + ULP_EXP * E * np.abs(s))
                     + G(2) * (np.abs(g) + e * np.abs(s)))


def check_toleranced(got, ref, bound, what):
    """NaN where the reference is NaN, the same infinity where it is infinite, within the bound elsewhere.  Returns the
    largest error / bound over the finite part (0 if there is none)."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    got = np.asarray(got, dtype=np.float64)
    nan, inf = np.isnan(ref), np.isinf(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", np.argwhere(np.isnan(got) != nan)[:4].tolist())
    assert np.array_equal(got[inf], ref[inf]), (what, "infinite entries", got[inf][:4].tolist(), ref[inf][:4].tolist())
    fin = ~nan & ~inf
    if not fin.any():
        return 0.0
    err, b = np.abs(got[fin] - ref[fin]), bound[fin]
    bad = ~(err <= b)
    assert not bad.any(), (what, int(bad.sum()), "outside the bound; worst error / bound", float(np.max(err / b)),
                           got[fin][bad][:4].tolist(), ref[fin][bad][:4].tolist())
    return float(np.max(err / b))


# ----------------------------------------------------------------------------- ms_ctc_greedy_decode
GREEDY_V = (1, 2, 29, 64, 65, 130)                     # 64 | 65: the thread-per-frame kernel | the wave arg max
GREEDY_T = (1, 255, 256, 257, 513)
GREEDY_N = 4
GREEDY_PATHS = ("run_across_edges", "blank_on_edges", "all_blank", "no_blank_no_repeat", "ties_and_non_finite")
MARGIN = 16.0                                          # the chosen symbol's logit above a background clipped to [-4, 4]


def greedy_lens(T):
    return np.array([T, T // 2 + 1, 0, T + 5], dtype=np.int32)       # the last is clipped to T


def first_max(row):
    """The arg max the kernels define: a NaN counts as the maximum and the first NaN wins; otherwise the first maximum."""
    nan = np.isnan(row)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(row))


def _tie_row(r, V, t, n):
    """One frame of the ``ties_and_non_finite`` path: (row float32 [V], the symbol it must decode to)."""
    row = np.clip(r.standard_normal(V), -4, 4).astype(np.float32)
    kinds = ["two_max", "inf_then_nan", "two_nan", "all_neg_inf"] if V >= 2 else ["all_neg_inf", "one_nan"]
    if V == 130:
        kinds += ["max_64_apart", "max_across_64"]
    kind = kinds[(t + n) % len(kinds)]
    v = (7 * t + 3 * n) % max(V - 1, 1)
    if kind == "two_max":
        row[v] = row[v + 1] = MARGIN
        return row, v
    if kind == "max_64_apart":
        v %= 66
        row[v] = row[v + 64] = MARGIN
        return row, v
    if kind == "max_across_64":
        v %= 65
        row[v + 64] = row[v + 65] = MARGIN
        return row, v + 64
    if kind == "inf_then_nan":
        row[v], row[v + 1] = np.inf, np.nan
        return row, v + 1
    if kind == "two_nan":
        a, b = v, min(v + 1 + (t % 70), V - 1)
        row[a] = row[b] = np.nan
        return row, a
    if kind == "one_nan":
        row[0] = np.nan
        return row, 0
    row[:] = -np.inf
    return row, 0


def greedy_case(V, T, blank, path):
    """(x float32 [T, N, V], lens int32 [N], want: per utterance the list of decoded symbols), or None where the alphabet is
    too small for the path (``no_blank_no_repeat`` needs two symbols besides the blank).  The frame-wise path is chosen
    first and the logits built from it with a margin of 16 over a background in [-4, 4]; ``ties_and_non_finite`` builds
    frames whose arg max is decided by the tie and NaN rules."""
    assert blank in (0, V - 1) and path in GREEDY_PATHS
    symbols = [s for s in range(V) if s != blank]
    if path == "no_blank_no_repeat" and len(symbols) < 2:
        return None
    N = GREEDY_N
    r = rng_of(("greedy", V, T, blank, path))
    lens = greedy_lens(T)
    x = np.clip(r.standard_normal((T, N, V)), -4, 4).astype(np.float32)
    frames = np.zeros((T, N), dtype=np.int64)
    for n in range(N):
        a = symbols[(5 + 11 * n) % len(symbols)] if symbols else blank
        for t in range(T):
            if path == "run_across_edges":          # a run across 63 | 64 and one across 255 | 256, blanks between them
                s = a if (60 <= t < 68 or 250 <= t < 262 or t < 2) else blank
            elif path == "blank_on_edges":          # the same symbol on both sides of a blank at frame 64 and at 256
                s = blank if t in (64, 256) else a
            elif path == "all_blank":
                s = blank
            elif path == "no_blank_no_repeat":
                s = symbols[(t + 3 * n) % len(symbols)]
            else:
                x[t, n], s = _tie_row(r, V, t, n)
                frames[t, n] = s
                continue
            frames[t, n] = s
            x[t, n, s] += np.float32(MARGIN)
    for t in range(T):
        for n in range(N):
            assert first_max(x[t, n]) == frames[t, n], (V, T, blank, path, t, n)
    return x, lens, greedy_ref(x, lens, blank)


def greedy_ref(x, lens, blank):
    """Arg max per frame, repeats collapsed, blanks dropped; lengths clipped to [0, T]."""
    T, N, _ = x.shape
    out = []
    for n in range(N):
        ln = min(max(int(lens[n]), 0), T)
        prev, seq = -1, []
        for t in range(ln):
            s = first_max(x[t, n])
            if s != blank and s != prev:
                seq.append(s)
            prev = s
        out.append(seq)
    return out


# ----------------------------------------------------------------------------- ms_embedding_forward
EMB_D = (1, 127, 128, 129, 300)                        # 128 threads stride a row
EMB_V1 = (1, 5)


def embedding_input(D, V1):
    """(table float32 [V1, D] with a NaN, an Inf and a -0.0 in it, idx int32: 0, V1 - 1, the out-of-range -1 and V1 + 3,
    then in-range draws)."""
    r = rng_of(("emb", D, V1))
    table = r.standard_normal((V1, D)).astype(np.float32)
    flat = table.reshape(-1)
    for k, v in enumerate((np.nan, np.inf, -0.0)):
        flat[(k * 37) % flat.size] = v
    idx = np.concatenate([[0, V1 - 1, -1, V1 + 3], r.integers(0, V1, size=5)]).astype(np.int32)
    return table, idx


def embedding_ref(table, idx):
    """Out-of-range indices read the nearest row (the header's clamping rule)."""
    return table[np.clip(idx, 0, table.shape[0] - 1)]


# ----------------------------------------------------------------------------- ms_rnnt_joint_forward
JOINT_J = (1, 63, 64, 65, 256, 300)                    # 64 lanes stride J, 256 threads stride the tanh vector
JOINT_V1 = (1, 3, 4, 5, 29, 65, 130)                   # 4 waves stride V1, 64 lanes stride it in the log-softmax
JOINT_R = 7
JOINT_ENC_ROW = np.array([3, 0, 3, 1, 5, 0, 3], dtype=np.int32)     # repeated, out of order; rows 2 and 4 are never read
JOINT_ENC_ROWS = 6
JOINT_REFUSED = (16384, 1)                             # (J + V1) * 4 bytes > 64 KiB


def joint_input(J, V1):
    """(enc_p [6, J] whose unreferenced rows are NaN, enc_row, pred_p [7, J], w_out [V1, J], b_out [V1]) float32."""
    r = rng_of(("joint", J, V1))
    enc = r.standard_normal((JOINT_ENC_ROWS, J)).astype(np.float32)
    enc[[i for i in range(JOINT_ENC_ROWS) if i not in set(JOINT_ENC_ROW.tolist())]] = np.nan
    pred = r.standard_normal((JOINT_R, J)).astype(np.float32)
    w = (r.standard_normal((V1, J)) * (2.0 / np.sqrt(J))).astype(np.float32)
    b = r.standard_normal(V1).astype(np.float32)
    return enc, JOINT_ENC_ROW.copy(), pred, w, b


def _joint_parts(enc, enc_row, pred, w, b):
    f = np.float64
    s = enc.astype(f)[enc_row] + pred.astype(f)
    z = np.tanh(s)
    bb = np.zeros(w.shape[0]) if b is None else b.astype(f)
    return s, z, z @ w.astype(f).T + bb, bb


def joint_ref(enc, enc_row, pred, w, b):
    """float64 [R, V1]: log_softmax(w . tanh(enc[enc_row] + pred) + b); b may be None."""
    logits = _joint_parts(enc, enc_row, pred, w, b)[2]
    return lsm_ref(logits[:, :, None])[:, :, 0]


def joint_bound(enc, enc_row, pred, w, b):
    s, z, logits, bb = _joint_parts(enc, enc_row, pred, w, b)
    J = w.shape[1]
    aw = np.abs(w.astype(np.float64))
    dz = E * np.abs(s) * (1.0 - z * z) + ULP_TANH * E * np.abs(z)
    el = G(J + 2) * (np.abs(z) @ aw.T + np.abs(bb)) + dz @ aw.T                 # E_v of the module docstring
    return SECOND * (el + np.max(el, axis=1, keepdims=True)) + lsm_bound(logits[:, :, None])[:, :, 0]


def logsumexp_rows(a):
    a = np.asarray(a, dtype=np.float64)
    m = np.max(a, axis=1, keepdims=True)
    return (np.log(np.sum(np.exp(a - m), axis=1, keepdims=True)) + m)[:, 0]


# ----------------------------------------------------------------------------- ms_rnnt_topk
TOPK_C = (1, 3, 255, 256, 257, 1000)
TOPK_B = 3


def topk_ks(C):
    return sorted({1, 5, C, C + 2})


def topk_input(C):
    """float32 [3, C] from the integers -2 .. 2, so ties are everywhere.  Row 1: about a third of the entries are -Inf.
    Row 2: about one entry in six is NaN, one in six -Inf."""
    r = rng_of(("topk", C))
    x = r.integers(-2, 3, size=(TOPK_B, C)).astype(np.float32)
    x[1, r.random(C) < 0.34] = -np.inf
    kind = r.integers(0, 6, size=C)
    x[2, kind == 0] = np.nan
    x[2, kind == 1] = -np.inf
    return x


def topk_ref(x, k):
    """(idx int32 [B, k], val float32 [B, k]): the entries above -Inf in descending order, among equals the lowest index first;
    a NaN is never selected (no comparison with it holds), nor is a -Inf; the places left over hold (-1, -Inf)."""
    B, C = x.shape
    idx = np.full((B, k), -1, dtype=np.int32)
    val = np.full((B, k), -np.inf, dtype=np.float32)
    for b in range(B):
        cand = [c for c in range(C) if x[b, c] > -np.inf]            # False for NaN and for -Inf
        cand.sort(key=lambda c: (-float(x[b, c]), c))
        for j, c in enumerate(cand[:k]):
            idx[b, j], val[b, j] = c, x[b, c]
    return idx, val
