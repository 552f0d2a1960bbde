"""numpy restatement of the CTC forced-alignment specification (the comment on ``ms_ctc_align`` in include/ms_hotpath.h).

A test helper, not product code: nothing under ``myrtlespeech_amd/`` imports it.  The float type is a parameter: float32
restates what the kernel computes (one rounding per addition, strict comparisons), float64 is the yardstick for the logits
mode, whose log-softmax the device rounds differently from numpy.
"""
import numpy as np


def extended(target, blank):
    """e_s, s = 0 .. 2L: blank for even s, y_{(s-1)/2} for odd s."""
    ext = np.full(2 * len(target) + 1, blank, dtype=np.int64)
    ext[1::2] = np.asarray(target, dtype=np.int64)
    return ext


def log_softmax(x, dtype):
    x = np.asarray(x, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.max(x, axis=-1, keepdims=True)
        lz = np.log(np.sum(np.exp(x - m), axis=-1, keepdims=True, dtype=dtype)) + m
    return x - lz, lz[..., 0]


class Result:
    """score; states [T_n] (None: no path); start / end / logp per token (-1 / -1 / -inf or NaN without a path)."""

    def __init__(self, score, states, start, end, logp):
        self.score, self.states, self.start, self.end, self.logp = score, states, start, end, logp


def align(x, target, blank, log_probs=True, dtype=np.float32):
    """One utterance: x [T_n, V] (only the existing rows), target a list of labels."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, dtype=dtype)
    Tn, L = x.shape[0], len(target)
    ext = extended(target, blank)
    S = 2 * L + 1
    ninf = dt(-np.inf)

    def no_path(score):
        return Result(score, None, np.full(L, -1), np.full(L, -1), np.full(L, score, dtype=dtype))

    if log_probs:
        lp = x
        poisoned = bool(np.isnan(x).any() or (x == np.inf).any())
    else:
        lp, lz = log_softmax(x, dtype)
        poisoned = bool((~np.isfinite(lz)).any())
    if poisoned:
        return no_path(dt(np.nan))
    if Tn == 0:
        return Result(dt(0), np.zeros(0, dtype=np.int64), np.zeros(0, int), np.zeros(0, int), np.zeros(0, dtype)) if L == 0 \
            else no_path(ninf)
    d = np.full(S, ninf, dtype=dtype)
    d[0] = lp[0, ext[0]]
    if S > 1:
        d[1] = lp[0, ext[1]]
    back = np.zeros((Tn, S), dtype=np.int8)
    # the skip into state s is allowed where s >= 2, e_s != blank and e_s != e_{s-2}
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    with np.errstate(invalid="ignore"):
        for t in range(1, Tn):      # every state of a frame at once; per state exactly the specification's three steps
            best, k = d.copy(), np.zeros(S, dtype=np.int8)
            a1 = np.concatenate([[ninf], d[:-1]]).astype(dtype)
            take = a1 > best                                  # (state 0 sees -inf: never strictly greater)
            best[take], k[take] = a1[take], 1
            a2 = np.concatenate([[ninf, ninf], d[:-2]]).astype(dtype)[:S]
            take = skip & (a2 > best)
            best[take], k[take] = a2[take], 2
            d = (best + lp[t, ext]).astype(dtype)
            back[t] = k
    fs = S - 1
    if S >= 2 and d[S - 2] > d[S - 1]:
        fs = S - 2
    score = d[fs]
    if score == ninf:
        return no_path(ninf)
    states = np.zeros(Tn, dtype=np.int64)
    s = fs
    for t in range(Tn - 1, 0, -1):
        states[t] = s
        s -= int(back[t, s])
    states[0] = s
    start, end, logp = spans(states, lp, ext, dtype)
    return Result(score, states, start, end, logp)


def spans(states, lp, ext, dtype=np.float32):
    """token i = the frames whose state is 2i+1: first frame, one past the last, the sum of lp[t, y_i] in ascending t."""
    dt = np.dtype(dtype).type
    L = (len(ext) - 1) // 2
    start, end, logp = np.full(L, -1), np.full(L, -1), np.zeros(L, dtype=dtype)
    for i in range(L):
        frames = np.nonzero(np.asarray(states) == 2 * i + 1)[0]
        start[i], end[i] = frames[0], frames[-1] + 1
        acc = dt(lp[frames[0], ext[2 * i + 1]])
        for t in frames[1:]:
            acc = dt(acc + lp[t, ext[2 * i + 1]])
        logp[i] = acc
    return start, end, logp


def rescore(states, lp64, ext):
    """float64 score of a given state path under log-probabilities lp64 [T_n, V]."""
    return float(sum(np.float64(lp64[t, ext[s]]) for t, s in enumerate(states)))


def collapse(states, ext, blank):
    """The labels a state path spells: repeats of a state merged, blanks dropped."""
    out, prev = [], -1
    for s in states:
        if s != prev and ext[s] != blank:
            out.append(int(ext[s]))
        prev = s
    return out


def is_valid_path(states, ext, blank):
    """Starts in state 0 or 1, ends in S-1 or S-2, steps by 0, 1 or an allowed 2."""
    S = len(ext)
    states = [int(s) for s in states]
    if not states or states[0] not in (0, 1) or states[-1] not in (S - 1, S - 2) or min(states) < 0 or max(states) >= S:
        return False
    for a, b in zip(states[:-1], states[1:]):
        step = b - a
        if step not in (0, 1, 2):
            return False
        if step == 2 and (ext[b] == blank or ext[b] == ext[b - 2]):
            return False
    return True


def all_paths(Tn, ext, blank):
    """Every valid state path of Tn frames (brute force; tiny shapes only)."""
    S = len(ext)
    if Tn == 0:
        return
    stack = [[s] for s in (0, 1) if s < S]
    while stack:
        p = stack.pop()
        if len(p) == Tn:
            if p[-1] in (S - 1, S - 2):
                yield p
            continue
        s = p[-1]
        for step in (0, 1, 2):
            b = s + step
            if b >= S or (step == 2 and (ext[b] == blank or ext[b] == ext[b - 2])):
                continue
            stack.append(p + [b])
