"""numpy restatement of the transducer-loss specification (the comment on ``ms_rnnt_loss_forward`` in include/ms_hotpath.h),
with plain loops (TEST INFRASTRUCTURE ONLY).  OWN specification: the reference snapshot has no transducer.

``rnnt_loss(logits, in_lens, targets, tgt_lens, blank, grad_nll=None, dtype=np.float64)`` returns ``Result(nll, grad, Z,
alpha, beta, exists)``; ``dtype`` is the arithmetic (float64: the yardstick; float32: what the specification's own number
format gives).  ``brute_force_ll`` enumerates every alignment.  ``gpu_cases()`` builds the inputs the GPU tests run, so that
the CPU tests can hold the float32 restatement to the same bounds.
"""
import itertools
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "nll grad Z alpha beta exists")


def lens_ok(Tn, Un, T, U1):
    return 1 <= Tn <= T and 0 <= Un <= U1 - 1


def labels_ok(y, V1, blank):
    return all(0 <= int(v) < V1 and int(v) != blank for v in y)


def logsumexp_row(row, dtype):
    """Z of one row, max-subtracted; NaN when it is not finite (a NaN or +inf logit, a row of -inf only)."""
    row = row.astype(dtype)
    with np.errstate(all="ignore"):
        m = np.max(row)
        if not np.isfinite(m):
            return dtype(np.nan)
        z = m + np.log(np.sum(np.exp(row - m), dtype=dtype))
    return dtype(z) if np.isfinite(z) else dtype(np.nan)


class _Sums:
    """The running sums of the recursion as (h, l) pairs.  ``compensated`` (the float32 arithmetic of the device): h + l carries
    the sum to about twice the format's precision (Knuth's two-sum), so that a step's rounding is that of the TERMS added, not
    2^-24 of a running sum that reaches several hundred off the likely alignments; the lattice stores h + l rounded once.
    Otherwise l stays 0 and every operation is the plain one of ``dtype`` (the float64 yardstick)."""

    def __init__(self, dt, compensated):
        self.dt, self.compensated = dt, compensated
        self.none = (dt(-np.inf), dt(0))

    def add(self, p, b):
        """p + b for a pair p and a plain value b."""
        dt = self.dt
        s = dt(p[0] + b)
        if not self.compensated or not np.isfinite(s):
            return (s, dt(0))
        bb = dt(s - p[0])
        e = dt(dt(dt(p[0] - dt(s - bb)) + dt(b - bb)) + p[1])
        h = dt(s + e)
        return (h, dt(e - dt(h - s)))

    def logaddexp(self, p, q):
        if min(p[0], q[0]) == self.none[0]:
            return q if p[0] == self.none[0] else p
        dt = self.dt
        hi, lo = (p, q) if p[0] >= q[0] else (q, p)
        d = dt(dt(lo[0] - hi[0]) + dt(lo[1] - hi[1]))
        return self.add(hi, dt(np.log1p(np.exp(d))))

    def value(self, p):
        return self.dt(p[0] + p[1])


def rnnt_loss(logits, in_lens, targets, tgt_lens, blank, grad_nll=None, dtype=np.float64, compensated=None):
    """``compensated`` (default: for float32 only) -- see ``_Sums``; ``rnnt_loss(..., dtype=np.float32, compensated=False)`` is
    the specification in plain float32."""
    logits = np.asarray(logits)
    S = _Sums(np.dtype(dtype).type, np.dtype(dtype) == np.float32 if compensated is None else bool(compensated))
    N, T, U1, V1 = logits.shape
    dt = np.dtype(dtype).type
    ninf = dt(-np.inf)
    grad_nll = np.ones(N, dtype=dtype) if grad_nll is None else np.asarray(grad_nll, dtype=dtype)
    nll = np.zeros(N, dtype=dtype)
    grad = np.zeros((N, T, U1, V1), dtype=dtype)
    Z = np.zeros((N, T, U1), dtype=dtype)
    alpha = np.zeros((N, T, U1), dtype=dtype)
    beta = np.zeros((N, T, U1), dtype=dtype)
    exists = np.zeros((N, T, U1), dtype=bool)
    for n in range(N):
        Tn, Un = int(in_lens[n]), int(tgt_lens[n])
        if not lens_ok(Tn, Un, T, U1):
            nll[n] = np.inf
            continue
        y = [int(targets[n][u]) for u in range(Un)]
        if not labels_ok(y, V1, blank):
            nll[n] = np.inf
            continue
        exists[n, :Tn, :Un + 1] = True
        x = logits[n].astype(dtype)
        with np.errstate(all="ignore"):
            for t in range(Tn):
                for u in range(Un + 1):
                    Z[n, t, u] = logsumexp_row(x[t, u], dt)
            if not np.isfinite(Z[n, :Tn, :Un + 1]).all():
                nll[n] = np.nan
                grad[n, :Tn, :Un + 1, :] = np.nan
                alpha[n, :Tn, :Un + 1] = np.nan
                beta[n, :Tn, :Un + 1] = np.nan
                continue
            b = np.full((Tn, Un + 1), ninf, dtype=dtype)
            e = np.full((Tn, Un + 1), ninf, dtype=dtype)
            for t in range(Tn):
                for u in range(Un + 1):
                    b[t, u] = x[t, u, blank] - Z[n, t, u]
                    if u < Un:
                        e[t, u] = x[t, u, y[u]] - Z[n, t, u]
            a = np.full((Tn, Un + 1), ninf, dtype=dtype)
            run = {}                                           # (t, u) -> the running pair behind a[t, u]
            for t in range(Tn):
                for u in range(Un + 1):
                    if t == 0 and u == 0:
                        run[0, 0] = (dt(0), dt(0))
                    else:
                        top = S.add(run[t - 1, u], b[t - 1, u]) if t > 0 else S.none
                        left = S.add(run[t, u - 1], e[t, u - 1]) if u > 0 else S.none
                        run[t, u] = S.logaddexp(top, left)
                    a[t, u] = S.value(run[t, u])
            ll = S.value(S.add(run[Tn - 1, Un], b[Tn - 1, Un]))
            bt = np.full((Tn, Un + 1), ninf, dtype=dtype)
            run = {}
            for t in range(Tn - 1, -1, -1):
                for u in range(Un, -1, -1):
                    if t == Tn - 1 and u == Un:
                        run[t, u] = (b[t, u], dt(0))
                    else:
                        down = S.add(run[t + 1, u], b[t, u]) if t + 1 < Tn else S.none
                        right = S.add(run[t, u + 1], e[t, u]) if u < Un else S.none
                        run[t, u] = S.logaddexp(down, right)
                    bt[t, u] = S.value(run[t, u])
            alpha[n, :Tn, :Un + 1] = a
            beta[n, :Tn, :Un + 1] = bt
            nll[n] = -ll
            if ll == ninf:
                continue                      # impossible transcript: nll = +inf, zero gradient
            for t in range(Tn):
                for u in range(Un + 1):
                    lp = x[t, u] - Z[n, t, u]
                    g = np.exp(lp + a[t, u] + bt[t, u] - ll)
                    if t + 1 < Tn:
                        g[blank] -= np.exp(a[t, u] + b[t, u] + bt[t + 1, u] - ll)
                    elif u == Un:
                        g[blank] -= np.exp(a[t, u] + b[t, u] - ll)
                    if u < Un:
                        g[y[u]] -= np.exp(a[t, u] + e[t, u] + bt[t, u + 1] - ll)
                    grad[n, t, u] = grad_nll[n] * g
    return Result(nll, grad, Z, alpha, beta, exists)


def brute_force_ll(logits_n, Tn, y, blank):
    """log of the sum over ALL alignments of one utterance, float64: an alignment is an order of T_n - 1 blanks and U_n labels
    followed by the final blank out of (T_n - 1, U_n)."""
    x = np.asarray(logits_n, dtype=np.float64)
    Un = len(y)
    lp = x - np.log(np.sum(np.exp(x - x.max(-1, keepdims=True)), -1, keepdims=True)) - x.max(-1, keepdims=True)
    terms = []
    for label_moves in itertools.combinations(range(Tn - 1 + Un), Un):
        t = u = 0
        s = 0.0
        for k in range(Tn - 1 + Un):
            if k in label_moves:
                s += lp[t, u, y[u]]
                u += 1
            else:
                s += lp[t, u, blank]
                t += 1
        assert (t, u) == (Tn - 1, Un)
        terms.append(s + lp[t, u, blank])
    return float(np.logaddexp.reduce(terms))


def bound(Tn, Un, nll_n):
    """B_n = 8 (T_n + U_n) 2^-24 max(1, |nll_n|): the depth of the recursion times one rounding of the running sum, a factor 8 for
    the hardware exp / log forms (the argument of tests/test_ctc_align_gpu.py)."""
    return 8.0 * (Tn + Un) * 2.0 ** -24 * max(1.0, abs(float(nll_n)))


def worst_ratios(got_nll, got_alpha, got_beta, got_grad, ref, in_lens, tgt_lens, grad_nll=None):
    """Per utterance with a finite reference nll: the worst |got - ref| over its bound (B_n for nll, alpha, beta on existing
    cells; 4 B_n |grad_nll[n]| for the gradient).  Entries given as None are skipped."""
    worst = {"nll": 0.0, "alpha": 0.0, "beta": 0.0, "grad": 0.0}
    N = len(ref.nll)
    for n in range(N):
        if not np.isfinite(ref.nll[n]):
            continue
        Tn, Un = int(in_lens[n]), int(tgt_lens[n])
        B = bound(Tn, Un, ref.nll[n])
        ex = ref.exists[n]

        def lattice_err(got, want):
            g, w = np.asarray(got[n], dtype=np.float64)[ex], want[n][ex].astype(np.float64)
            same_inf = np.isinf(w) & (g == w)
            with np.errstate(invalid="ignore"):
                d = np.where(same_inf, 0.0, np.abs(g - w))
            return float(np.max(np.where(np.isnan(d), np.inf, d)))

        worst["nll"] = max(worst["nll"], abs(float(got_nll[n]) - float(ref.nll[n])) / B)
        if got_alpha is not None:
            worst["alpha"] = max(worst["alpha"], lattice_err(got_alpha, ref.alpha) / B)
        if got_beta is not None:
            worst["beta"] = max(worst["beta"], lattice_err(got_beta, ref.beta) / B)
        if got_grad is not None:
            gn = 1.0 if grad_nll is None else abs(float(grad_nll[n]))
            d = np.abs(np.asarray(got_grad[n], dtype=np.float64) - ref.grad[n].astype(np.float64))
            d = float(np.max(np.where(np.isnan(d), np.inf, d)))
            worst["grad"] = max(worst["grad"], d / (4 * B * gn) if gn > 0 else (0.0 if d == 0 else np.inf))
    return worst


def random_targets(rng, N, U_max, V1, blank):
    labels = np.array([v for v in range(V1) if v != blank])
    return labels[rng.integers(0, len(labels), size=(N, U_max))].astype(np.int32)


def pad_targets(y, tgt_lens, pad):
    y = np.array(y, dtype=np.int32, copy=True)
    for n, un in enumerate(tgt_lens):
        y[n, un:] = pad
    return y


def monotone_alignment_cells(rng, T, U):
    """Cells (t, u) of one alignment from (0, 0) to (T - 1, U), and the move out of each (True: a label)."""
    moves = np.array([True] * U + [False] * (T - 1))
    rng.shuffle(moves)
    t = u = 0
    cells = []
    for mv in moves:
        cells.append((t, u, bool(mv)))
        if mv:
            u += 1
        else:
            t += 1
    cells.append((t, u, False))
    return cells


def gpu_cases():
    """name -> dict(logits, in_lens, targets, tgt_lens, blank): the inputs of tests/test_rnnt_loss_gpu.py's cases (a) .. (g).
    logits are 3 randn unless said, blank = last symbol, the target padding holds the blank."""
    cases = {}

    def make(name, seed, N, T, U_max, V1, in_lens, tgt_lens, scale=3.0):
        rng = np.random.default_rng(seed)
        blank = V1 - 1
        x = (rng.standard_normal((N, T, U_max + 1, V1)) * scale).astype(np.float32)
        y = random_targets(rng, N, U_max, V1, blank)
        y = pad_targets(y, tgt_lens, blank)
        cases[name] = dict(logits=x, in_lens=np.array(in_lens, dtype=np.int32), targets=y,
                           tgt_lens=np.array(tgt_lens, dtype=np.int32), blank=blank)
        return rng, cases[name]

    make("a_ragged", 1, 4, 7, 4, 5, [7, 5, 1, 3], [4, 0, 3, 2])
    make("b_cross_wave", 2, 2, 40, 69, 29, [40, 33], [69, 12])
    make("c_several_waves", 3, 1, 20, 300, 29, [20], [300])
    make("d_edge_u1_1024", 4, 1, 3, 1023, 4, [3], [1023])
    make("e_long_odd_row", 5, 2, 6, 5, 1031, [6, 6], [5, 5])
    rng, f = make("f_peaked", 6, 2, 64, 20, 29, [64, 64], [20, 20], scale=2.0)
    for n in range(2):                                   # + 10 on the cells of one monotone alignment
        for t, u, is_label in monotone_alignment_cells(rng, int(f["in_lens"][n]), int(f["tgt_lens"][n])):
            f["logits"][n, t, u, f["targets"][n, u] if is_label else f["blank"]] += 10.0
    rng, g = make("g_inf_column", 7, 2, 9, 6, 7, [9, 6], [6, 4])
    g["targets"][g["targets"] == 2] = 3                  # symbol 2 is off every target ...
    g["logits"][..., 2] = -np.inf                        # ... and impossible everywhere
    return cases
