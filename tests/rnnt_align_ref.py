"""numpy restatement of the transducer forced-alignment specification (the comment on ``ms_rnnt_align`` in
include/ms_hotpath.h), with plain loops (TEST INFRASTRUCTURE ONLY).  OWN specification: the reference snapshot has no
transducer.

``rnnt_align(x, in_lens, targets, tgt_lens, blank, log_probs, dtype)`` takes the dense ``[N, T, U1, V1]`` tensor and returns
``Result(score, token_frame, token_logp, frame_u, frame_logp)`` with the shapes and fills of the device's outputs.  With
``dtype=np.float32`` and ``log_probs=True`` it is the specification bit for bit (every addition rounded once, nothing else
computed); ``dtype=np.float64`` is the yardstick for the modes whose b / e carry an error (logits in, the fused entry).
``align_planes`` is the recursion on one utterance's b / e tables, ``path_score`` the in-order sum of a GIVEN path under given
tables, ``brute_force`` the maximum of that sum over every monotone path.
"""
import itertools
from collections import namedtuple

import numpy as np

import rnnt_loss_ref as R

Result = namedtuple("Result", "score token_frame token_logp frame_u frame_logp")


def cell_tables(x_n, Tn, y, blank, log_probs, dtype):
    """b [T_n, U_n + 1], e [T_n, U_n] of one utterance from its dense rows x_n [T, U1, V1]; (None, None) when a cell poisons
    the utterance (a NaN or +inf b / e, a non-finite normaliser).  The normaliser is ``rnnt_loss_ref.logsumexp_row``'s
    formula, over all cells at once."""
    Un = len(y)
    x = np.asarray(x_n)[:Tn, :Un + 1].astype(dtype)
    xb = x[:, :, blank]
    xe = np.take_along_axis(x[:, :Un], np.asarray(y, dtype=np.int64).reshape(1, Un, 1), axis=2)[:, :, 0] if Un else x[:, :0, 0]
    with np.errstate(all="ignore"):
        if log_probs:
            b, e = xb.copy(), xe.copy()
        else:
            m = np.max(x, axis=-1)
            if not np.isfinite(m).all():
                return None, None
            z = (m + np.log(np.sum(np.exp(x - m[..., None]), axis=-1, dtype=dtype))).astype(dtype)
            if not np.isfinite(z).all():
                return None, None
            b, e = (xb - z).astype(dtype), (xe - z[:, :Un]).astype(dtype)
    for tab in (b, e):
        if np.isnan(tab).any() or (tab == np.inf).any():
            return None, None
    return b, e


def align_planes(b, e, dtype=np.float32):
    """The recursion and the back-trace on b [T_n, U_n + 1], e [T_n, U_n] (poison-free).  Returns (score, token_frame [U_n],
    frame_u [T_n]); the two lists are None when score is -inf.  The cells of an anti-diagonal do not depend on each other:
    they are formed together, every addition rounded once in ``dtype``."""
    dt = np.dtype(dtype).type
    Tn, U1n = b.shape
    Un = U1n - 1
    b, e = b.astype(dtype), e.astype(dtype)
    d = np.full((Tn, Un + 1), -np.inf, dtype=dtype)
    k = np.zeros((Tn, Un + 1), dtype=np.int8)
    d[0, 0] = 0
    with np.errstate(all="ignore"):
        for diag in range(1, Tn + Un):
            u = np.arange(max(0, diag - Tn + 1), min(Un, diag) + 1)
            t = diag - u
            has_top, has_left = t > 0, u > 0
            top = np.where(has_top, d[np.maximum(t - 1, 0), u] + b[np.maximum(t - 1, 0), u], dt(-np.inf)).astype(dtype)
            ul = np.maximum(u - 1, 0)
            left = (d[t, ul] + (e[t, np.minimum(ul, max(Un - 1, 0))] if Un else dt(-np.inf))).astype(dtype)
            take_left = has_left & (~has_top | (left > top))         # a tie takes the blank predecessor
            d[t, u] = np.where(take_left, left, top)
            k[t, u] = take_left
        score = dt(d[Tn - 1, Un] + b[Tn - 1, Un])
    if score == -np.inf:
        return score, None, None
    token_frame, frame_u = [-1] * Un, [-1] * Tn
    t, u = Tn - 1, Un
    frame_u[t] = u
    while (t, u) != (0, 0):
        if k[t, u]:
            u -= 1
            token_frame[u] = t
        else:
            t -= 1
            frame_u[t] = u
    return score, token_frame, frame_u


def path_terms(b, e, token_frame, frame_u):
    """The log-probabilities of a path in path order: per frame its emitted labels in order of u, then its blank."""
    terms, u = [], 0
    for t in range(len(frame_u)):
        while u < frame_u[t]:
            assert token_frame[u] == t
            terms.append(e[t, u])
            u += 1
        terms.append(b[t, frame_u[t]])
    return terms


def ordered_sum(terms, dtype=np.float32):
    dt = np.dtype(dtype).type
    s = dt(0)
    with np.errstate(all="ignore"):
        for v in terms:
            s = dt(s + dt(v))
    return s


def path_score(b, e, token_frame, frame_u, dtype=np.float32):
    """The in-order sum, starting from 0, of a given path under given tables."""
    return ordered_sum(path_terms(b, e, token_frame, frame_u), dtype)


def brute_force(b, e, dtype=np.float32):
    """(best in-order sum, the paths that reach it as (token_frame, frame_u)) over ALL monotone paths."""
    Tn, Un = b.shape[0], b.shape[1] - 1
    best, arg = None, []
    for label_moves in itertools.combinations(range(Tn - 1 + Un), Un):
        t = u = 0
        token_frame, frame_u = [-1] * Un, [-1] * Tn
        for i in range(Tn - 1 + Un):
            if i in label_moves:
                token_frame[u] = t
                u += 1
            else:
                frame_u[t] = u
                t += 1
        frame_u[t] = u
        s = path_score(b, e, token_frame, frame_u, dtype)
        if best is None or s > best:
            best, arg = s, [(token_frame, frame_u)]
        elif s == best:
            arg.append((token_frame, frame_u))
    return best, arg


def rnnt_align(x, in_lens, targets, tgt_lens, blank, log_probs=True, dtype=np.float32, tables=None):
    """The five outputs for a dense x [N, T, U1, V1], in ``dtype`` arithmetic, with the fills of the specification.  ``tables``
    (a list) collects every utterance's (b, e), or None where it has no cells or a poisoned one."""
    x = np.asarray(x)
    N, T, U1, V1 = x.shape
    score = np.zeros(N, dtype=dtype)
    token_frame = np.full((N, U1 - 1), -1, dtype=np.int32)
    token_logp = np.zeros((N, U1 - 1), dtype=dtype)
    frame_u = np.full((N, T), -1, dtype=np.int32)
    frame_logp = np.zeros((N, T), dtype=dtype)

    def no_path(n, sc, Tc, Uc):
        score[n] = sc
        token_logp[n, :Uc] = sc
        frame_logp[n, :Tc] = sc

    for n in range(N):
        Tn, Un = int(in_lens[n]), int(tgt_lens[n])
        Tc, Uc = min(max(Tn, 0), T), min(max(Un, 0), U1 - 1)
        if tables is not None:
            tables.append(None)
        if not R.lens_ok(Tn, Un, T, U1):
            no_path(n, -np.inf, Tc, Uc)
            continue
        y = [int(targets[n][u]) for u in range(Un)]
        if not R.labels_ok(y, V1, blank):
            no_path(n, -np.inf, Tc, Uc)
            continue
        b, e = cell_tables(x[n], Tn, y, blank, log_probs, dtype)
        if tables is not None and b is not None:
            tables[-1] = (b, e)
        if b is None:
            no_path(n, np.nan, Tn, Un)
            continue
        sc, tf, fu = align_planes(b, e, dtype)
        if tf is None:
            no_path(n, sc, Tn, Un)
            continue
        score[n] = sc
        token_frame[n, :Un] = tf
        token_logp[n, :Un] = [e[tf[u], u] for u in range(Un)]
        frame_u[n, :Tn] = fu
        frame_logp[n, :Tn] = [b[t, fu[t]] for t in range(Tn)]
    return Result(score, token_frame, token_logp, frame_u, frame_logp)


def check_consistent(res, in_lens, tgt_lens):
    """The properties every mode's outputs have, bit-exact: the score is the float32 in-order sum of the returned
    log-probabilities; token_frame is non-decreasing and < T_n; frame_u is non-decreasing and ends at U_n; the counts implied by
    token_frame agree with frame_u; the rows that do not exist hold -1 / 0."""
    N, T = res.frame_u.shape
    for n in range(N):
        Tn, Un = int(in_lens[n]), int(tgt_lens[n])
        sc = res.score[n]
        Tc, Uc = min(max(Tn, 0), T), min(max(Un, 0), res.token_frame.shape[1])
        assert (res.token_frame[n, Uc:] == -1).all() and (res.frame_u[n, Tc:] == -1).all()
        assert (res.token_logp[n, Uc:] == 0).all() and (res.frame_logp[n, Tc:] == 0).all()
        if not np.isfinite(sc):
            assert np.isnan(sc) or sc == -np.inf, (n, sc)
            assert (res.token_frame[n] == -1).all() and (res.frame_u[n] == -1).all()
            for lp in (res.token_logp[n, :Uc], res.frame_logp[n, :Tc]):
                assert np.isnan(lp).all() if np.isnan(sc) else (lp == -np.inf).all()
            continue
        tf, fu = res.token_frame[n, :Un], res.frame_u[n, :Tn]
        assert (np.diff(tf) >= 0).all() and (tf >= 0).all() and (tf < Tn).all(), (n, tf)
        assert (np.diff(fu) >= 0).all() and (fu >= 0).all() and fu[-1] == Un, (n, fu)
        for t in range(Tn):
            assert int((tf <= t).sum()) == int(fu[t]), (n, t)
        terms, u = [], 0
        for t in range(Tn):
            while u < fu[t]:
                terms.append(res.token_logp[n, u])
                u += 1
            terms.append(res.frame_logp[n, t])
        total = ordered_sum(terms, np.float32)
        assert np.float32(sc).tobytes() == np.float32(total).tobytes(), (n, sc, total)


def grid_table(rng, N, T, U1, V1, p_inf=0.01):
    """Log-probabilities on a grid of 1/8 (ties abound), a sprinkle of -inf."""
    x = -(rng.integers(0, 64, size=(N, T, U1, V1)) / 8.0).astype(np.float32)
    if p_inf:
        x[rng.random(x.shape) < p_inf] = -np.inf
    return x


def continuous_table(rng, N, T, U1, V1, p_inf=0.01):
    x = -np.abs(rng.standard_normal((N, T, U1, V1)) * 3).astype(np.float32)
    if p_inf:
        x[rng.random(x.shape) < p_inf] = -np.inf
    return x


def ragged_lengths(rng, N, T, U1):
    """Lengths inside the batch: utterance 0 full, the others ragged, with U_n = 0 and T_n = 1 among them when N allows."""
    in_lens = [T] + [int(rng.integers(1, T + 1)) for _ in range(N - 1)]
    tgt_lens = [U1 - 1] + [int(rng.integers(0, U1)) for _ in range(N - 1)]
    if N >= 2:
        tgt_lens[1] = 0
    if N >= 3:
        in_lens[2] = 1
    return np.array(in_lens, dtype=np.int32), np.array(tgt_lens, dtype=np.int32)
