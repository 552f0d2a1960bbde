"""Cases, input families, the float64 reference and the ONE derived tolerance of the CTC loss (``ms_ctc_loss_forward`` /
``ms_ctc_loss_backward``, csrc/ctc.hip).  numpy and Python integers only: nothing of the package is imported.
tests/test_ctc_loss_cpu.py proves this file (reference against exact integer path counts and against torch's float64 CPU
loss, a float32 restatement of the kernel's recursion inside half of the bound, every case on its intended side of its gate);
tests/test_ctc_loss_gpu.py runs the cases through the C ABI.

Reference.  ``reference`` is the alpha-beta recursion in float64, vectorised over the 2L + 1 states with time as the only
Python loop.  It takes logits or (``log_probs_in``, MS_CTC_LOG_PROBS_IN) log-probabilities, -inf entries, in_lens of 0, empty
targets and zero_infinity, and returns nll, the gradient of sum_n grad_nll[n] nll[n] and the per-utterance figures the bound
needs.  With log-probabilities given the gradient is what torch.nn.CTCLoss's backward returns, exp(lp) - posterior (the
header, ms_ctc_loss_backward).  An utterance with a frame (t < in_lens) whose log-softmax normaliser is not finite, or with
a NaN log-probability, is *poisoned*: nll NaN, NaN in every gradient element of its existing frames, zeros behind them,
whatever zero_infinity says.  An impossible target has nll = +inf; with zero_infinity nll = 0 and an all-zero gradient;
without it the gradient of +inf is not defined and ``grad_defined[n]`` is False (the tests then only require the rows to
be written and the padding rows to be zero).

Input families.
  count  every frame's logits are one constant c_t: lp = -ln V everywhere, so nll = T_n ln V - ln(#alignments) and
         grad[t, k] = 1/V - (#alignments through symbol k at t) / (#alignments), both from Python-integer path counts
         (``count_exact``).  T_n = L + repeats has exactly one alignment, one frame fewer has none.
  path   logits 0 except +24 on the symbol of a prescribed alignment.  ``early`` / ``late`` / ``spread`` are valid (loss ~ 0;
         a kernel that drops one transition of it is off by ~24 per frame); ``trap_repeat`` (a repeated label emitted with no
         blank between) and ``trap_skip`` (one label stepped over) are INVALID: the reference gives a loss of order 24, a
         kernel that allows the forbidden move gives ~0.
  gauss  3 N(0, 1).
Frames at or past in_lens hold gaussian garbage in every family.

The tolerance (log2 units per frame, times ln 2 . T_n):

    bound_nll(n) = ln 2 . T_n . (6 . 2^-24 . A_n  +  2^-19  +  z_n)

  6 . 2^-24 . A_n   alpha_wave_body's ``nw[j] = (__builtin_amdgcn_logf(e) + m) + lp``: two float32 additions per frame and state at
                    the magnitude of alpha, half an ulp each = 2 . 2^-24 . |alpha| log2 units, with a margin of 3.  A_n is the
                    largest |alpha| / ln 2 over the *occupied* cells (posterior >= 2^-24): an error in a cell below that
                    reaches the loss scaled by its posterior.  The LDS-row kernels do the same two additions in natural
                    logarithms (``lse3(...) + (row[lab] - lz)``): the same relative figure.  The last line of either kernel
                    (log of the last two states, times ln 2) is one more step of the same kind.
  2^-19             ``exp2f(a0 - m) + exp2f(a1 - m) + exp2f(a2 - m)`` and ``logf(e)``: three v_exp_f32 and one v_log_f32 at 1 ulp
                    (the ISA documentation; the comment at csrc/rnn.hip:301) plus the two additions of a sum in [1, 3] come to
                    2^-19.7.  lse3 of the LDS-row kernels wraps the same instructions in one multiplication each
                    (__expf / __logf): arguments that matter are above -17, so that adds < 2 . 2^-24, inside the margin.
  z_n               phase 1, one frame's log2-domain log-probability ``(r[v] - lz) * LOG2E`` with
                    ``lz = logf(sum_v expf(r[v] - m)) + m``.  With w_v = exp(r_v - m), W = sum w and u = 2^-24, in natural units:
                      expf at <= 2 ulp, exact at the maximum (expf(0) = 1):      4 u . sum_{w_v != 1} w_v / W
                      the V - 1 additions, each off by at most min(half an ulp of its result, its smaller operand):
                          serial (``sum += expf(...)``: alpha_wave_normalise, ctc_alpha_kernel, ctc_grad_kernel):
                                                                                sum_v min(u W, w_v) / W
                          tree (ctc_normalise_wide_frame: <= ceil(V / 64) serial terms per lane, six shuffle steps):
                                                                                depth . min(u W, W - 1) / W
                      logf at <= 2 ulp of its result:                            2 u |ln W|
                      ``+ m``: the result is no farther from the exact sum than m itself, which is a float32:
                                                                                min(u |lz|, ln W)
                    z_n = log2(e) . (the largest frame's total)  +  3 u . P_n, the last term for the subtraction, the
                    multiplication and the rounded constant LOG2E at the magnitude P_n = the largest |lp| / ln 2 an occupied
                    cell reads.  With log-probabilities given only that last term remains.
                    ``z_serial`` and ``z_tree`` are both returned; a test takes the one of the route it runs (``z_of``).

    |g - g64| <= |grad_nll[n]| . (3 . bound_nll(n) + 2^-18)      per gradient element

  (the posterior is exp2 of alpha + beta - ll2 - lp2, three quantities each within bound_nll, so its relative error is within
  3 bound_nll; 2^-18 covers the two v_exp_f32, the v_log_f32 and the bucket sum of ctc_grad_rows_kernel on values <= 1.)

Every toleranced case has bound_nll <= 1e-2 (asserted by ``bounds`` for each case a test tolerances; the one exception is
named there): gauss and count fit up to T = 64 at V <= 29; larger lattices use ``path``, where A_n and z_n are ~0 and the
bound is ~7e-4 at T = 530 and 9.0e-3 at T = 6 827.  No tolerance comes from a run of the kernel."""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

U = 2.0 ** -24
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
BOUND_CAP = 1e-2
PATH_LOGIT = 24.0
FAMILIES = ("count", "path", "gauss")
VALID_VARIANTS = ("early", "late", "spread")

# ---- the dispatch gates of csrc/ctc.hip, restated ---------------------------------------------------------------------------
LDS_BYTES = 160 * 1024              # ms_ctc_loss_forward: ``alpha_wave_lds(T) <= 160 * 1024``, ``lds <= 160 * 1024``
PIPELINE_S_MAX = 1024               # ``S_max <= 1024`` in wave_ok (forward) and in the backward's condition
GRAD_ROWS_LDS_BYTES = 64 * 1024     # ms_ctc_loss_backward: ``rows_lds <= 64 * 1024``
GRAD_LDS_MAX = 160 * 1024 - 256     # ms_ctc_loss_backward: GRAD_LDS_MAX (ctc_grad_kernel also has a static word)
STATUS_BYTES = 256                  # CTC_STATUS_BYTES
WIDE_V = 64                         # ``V > 64``: ctc_normalise_wide_frame, the per-state copy of the rows
MS_OK, MS_ERR_INVALID, MS_ERR_WORKSPACE = 0, 1, 3
LOG_PROBS_IN = 2                    # MS_CTC_LOG_PROBS_IN


def mailbox_bytes(T):
    """alpha_wave_lds(T)."""
    return (6 * T + 4) * 4


def states_per_lane(S_max):
    """K of ctc_alpha_wave_kernel<K, D> (``S_max <= 256`` / ``<= 512`` / else)."""
    return 1 if S_max <= 256 else 2 if S_max <= 512 else 4


def forward_route(T, V, S_max, wave=True):
    """"pipeline" or "lds_row" (ctc_alpha_kernel): ``wave_ok`` of ms_ctc_loss_forward; ``wave`` False = MS_CTC_WAVE=0."""
    ok = wave and S_max <= PIPELINE_S_MAX and mailbox_bytes(T) <= LDS_BYTES and T * V * 4 < 2 ** 31
    return "pipeline" if ok else "lds_row"


def backward_route(T, V, S_max, wave=True):
    """"pipeline" (two recursions + ctc_grad_rows_kernel) or "lds_row" (ctc_grad_kernel): the condition in ms_ctc_loss_backward."""
    ok = (wave and S_max <= PIPELINE_S_MAX and mailbox_bytes(T) <= LDS_BYTES and (5 * S_max + V + 1) * 4 <= GRAD_ROWS_LDS_BYTES
          and T * max(V, S_max) * 4 < 2 ** 31)
    return "pipeline" if ok else "lds_row"


def forward_refuses(S_max):
    """``MS_REQUIRE(lds <= 160 * 1024)`` with lds = 3 S_max floats (checked before the route is chosen)."""
    return 3 * S_max * 4 > LDS_BYTES


def backward_refuses(T, V, S_max, wave=True):
    """``MS_REQUIRE(lds <= GRAD_LDS_MAX)`` with lds = 4 S_max floats, off the pipeline only."""
    return backward_route(T, V, S_max, wave) == "lds_row" and 4 * S_max * 4 > GRAD_LDS_MAX


def z_of(route, V):
    """Which normaliser order a route sums in: the key of ``reference``'s result."""
    return "z_tree" if route == "pipeline" and V > WIDE_V else "z_serial"


# the first target lengths the entry points refuse (S_max = 2 L + 1)
FIRST_REFUSED_FORWARD_L = 6827      # 3 . 13 655 . 4 = 163 860 > 163 840; L = 6 826: 163 836
FIRST_REFUSED_BACKWARD_L = 5112     # 4 . 10 225 . 4 = 163 600 > 163 584; L = 5 111: 163 568
LAST_MAILBOX_T = 6826               # (6 . 6 826 + 4) . 4 = 163 840 = every byte; 6 827: 163 864


# ---- the reference -------------------------------------------------------------------------------------------------------------
def ext_labels(target, blank):
    e = np.full(2 * len(target) + 1, blank, dtype=np.int64)
    e[1::2] = target
    return e


def _lse3(a, b, c):
    m = np.maximum(np.maximum(a, b), c)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(m == -np.inf, -np.inf, ms + np.log(np.exp(a - ms) + np.exp(b - ms) + np.exp(c - ms)))


def _recursion(lpe, skip):
    """alpha [Tn, S] for the per-state log-probabilities lpe [Tn, S]; skip[s]: the move s - 2 -> s is allowed."""
    Tn, S = lpe.shape
    al = np.full((Tn, S), -np.inf)
    al[0, :2] = lpe[0, :2]
    ninf1, ninf2 = np.full(1, -np.inf), np.full(2, -np.inf)
    for t in range(1, Tn):
        a = al[t - 1]
        a1 = np.concatenate((ninf1, a[:-1]))
        a2 = np.where(skip, np.concatenate((ninf2, a[:-2])), -np.inf) if S > 1 else ninf1
        al[t] = _lse3(a, a1, a2) + lpe[t]
    return al


def _normaliser_terms(xs):
    """(lz [Tn], z_serial, z_tree) in natural units per frame (the module docstring), for logits xs [Tn, V] float64."""
    V = xs.shape[1]
    m = xs.max(axis=1)
    w = np.exp(xs - m[:, None])
    W = w.sum(axis=1)
    lnW = np.log(W)
    lz = m + lnW
    e_exp = 4 * U * np.where(w != 1.0, w, 0.0).sum(axis=1) / W
    add_serial = np.minimum(U * W[:, None], w).sum(axis=1) / W
    depth = min(V - 1, -(-V // 64) + 6)
    add_tree = depth * np.minimum(U * W, W - 1.0) / W
    rest = 2 * U * np.abs(lnW) + np.minimum(U * np.abs(lz), lnW)
    return lz, float((e_exp + add_serial + rest).max()), float((e_exp + add_tree + rest).max())


def reference(x, in_lens, targets, blank, zero_infinity=False, log_probs_in=False, grad_nll=None):
    """x [T, N, V] float32; targets: a list of N label lists.  Returns a dict: nll [N] (before any zero_infinity
    replacement: ``nll_out`` has it applied), grad [T, N, V], A, P, z_serial, z_tree, poisoned, infeasible, grad_defined [N]."""
    T, N, V = x.shape
    go = np.ones(N) if grad_nll is None else np.asarray(grad_nll, dtype=np.float64)
    out = dict(nll=np.zeros(N), grad=np.zeros((T, N, V)), A=np.zeros(N), P=np.zeros(N), z_serial=np.zeros(N), z_tree=np.zeros(N),
               poisoned=np.zeros(N, bool), infeasible=np.zeros(N, bool), grad_defined=np.ones(N, bool), Tn=np.zeros(N, int))
    for n in range(N):
        Tn = int(min(max(in_lens[n], 0), T))
        out["Tn"][n] = Tn
        tgt = np.asarray(targets[n], dtype=np.int64)
        L = len(tgt)
        if Tn == 0:
            out["nll"][n] = 0.0 if L == 0 else np.inf
            out["infeasible"][n] = L != 0
            continue
        xs = x[:Tn, n, :].astype(np.float64)
        zs = zt = 0.0
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if log_probs_in:
                bad = bool(np.isnan(xs).any())
                lp = xs
            else:
                lz, zs, zt = _normaliser_terms(xs)
                bad = not bool(np.isfinite(lz).all())
                lp = xs - lz[:, None]
        if bad:
            out["poisoned"][n] = True
            out["nll"][n] = np.nan
            out["grad"][:Tn, n, :] = np.nan
            continue
        ext = ext_labels(tgt, blank)
        S = len(ext)
        skip = np.zeros(S, bool)
        skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
        lpe = lp[:, ext]
        al = _recursion(lpe, skip)
        # beta: the same recursion on the time- and state-reversed utterance (the move s -> s + 2 is allowed when ext[s + 2]
        # is a label other than ext[s])
        skip_r = np.zeros(S, bool)
        skip_r[2:] = skip[::-1][:-2]
        be = _recursion(lpe[::-1, ::-1], skip_r)[::-1, ::-1]
        ll = float(_lse3(al[-1, S - 1], al[-1, S - 2] if S > 1 else -np.inf, -np.inf))
        if ll == -np.inf:
            out["nll"][n] = np.inf
            out["infeasible"][n] = True
            if not zero_infinity:
                out["grad_defined"][n] = False
                out["grad"][:Tn, n, :] = np.nan
            continue
        out["nll"][n] = -ll
        with np.errstate(invalid="ignore"):
            g = np.where(np.isfinite(lpe), al + be - lpe - ll, -np.inf)      # log posterior of (t, s)
        occ = np.exp(g)
        post = np.zeros((Tn, V))
        for s in range(S):
            post[:, ext[s]] += occ[:, s]
        out["grad"][:Tn, n, :] = (np.exp(lp) - post) * go[n]
        cells = occ >= U
        out["A"][n] = float(np.abs(al[cells]).max()) / LN2
        out["P"][n] = float(np.abs(lpe[cells]).max()) / LN2
        out["z_serial"][n] = LOG2E * zs + 3 * U * out["P"][n]
        out["z_tree"][n] = LOG2E * zt + 3 * U * out["P"][n]
    nll_out = out["nll"].copy()
    if zero_infinity:
        nll_out[np.isinf(nll_out)] = 0.0
    out["nll_out"] = nll_out
    return out


def bound_nll(ref, zkey):
    """[N] the loss bound of the module docstring; ``zkey`` from ``z_of``."""
    return LN2 * ref["Tn"] * (6 * U * ref["A"] + 2.0 ** -19 + ref[zkey])


def bound_grad(ref, zkey, grad_nll=None):
    """[N] the per-element gradient bound."""
    go = np.ones(len(ref["nll"])) if grad_nll is None else np.abs(np.asarray(grad_nll, dtype=np.float64))
    return go * (3 * bound_nll(ref, zkey) + 2.0 ** -18)


# ---- exact integer path counts (the ``count`` family) ----------------------------------------------------------------------
def count_paths(Tn, target, blank):
    """(A, B, total): A[t][s] alignments of frames 0..t that end in state s, B[t][s] alignments of frames t..Tn-1 that start
    in state s, as Python integers; total = #alignments of the whole utterance."""
    ext = [int(v) for v in ext_labels(target, blank)]
    S = len(ext)
    skip = [s >= 2 and ext[s] != blank and ext[s] != ext[s - 2] for s in range(S)]
    A = [[0] * S for _ in range(Tn)]
    B = [[0] * S for _ in range(Tn)]
    if Tn == 0:
        return A, B, (1 if S == 1 else 0)
    A[0][0] = 1
    if S > 1:
        A[0][1] = 1
    for t in range(1, Tn):
        p, q = A[t - 1], A[t]
        for s in range(S):
            q[s] = p[s] + (p[s - 1] if s >= 1 else 0) + (p[s - 2] if skip[s] else 0)
    B[Tn - 1][S - 1] = 1
    if S > 1:
        B[Tn - 1][S - 2] = 1
    for t in range(Tn - 2, -1, -1):
        p, q = B[t + 1], B[t]
        for s in range(S):
            q[s] = p[s] + (p[s + 1] if s + 1 < S else 0) + (p[s + 2] if s + 2 < S and skip[s + 2] else 0)
    return A, B, A[Tn - 1][S - 1] + (A[Tn - 1][S - 2] if S > 1 else 0)


def count_exact(Tn, target, blank, V):
    """(nll, grad [Tn, V]) of frame-constant logits from the integer counts, as exact rationals rounded once to float64."""
    A, B, total = count_paths(Tn, target, blank)
    if total == 0:
        return math.inf, None
    nll = Tn * math.log(V) - math.log(total)
    ext = [int(v) for v in ext_labels(target, blank)]
    grad = np.zeros((Tn, V))
    for t in range(Tn):
        through = {}
        for s, k in enumerate(ext):
            through[k] = through.get(k, 0) + A[t][s] * B[t][s]
        for k in range(V):
            grad[t, k] = float(Fraction(1, V) - Fraction(through.get(k, 0), total))
    return nll, grad


# ---- alignments of the ``path`` family -------------------------------------------------------------------------------------
def min_frames(target):
    """L + repeats: the fewest frames that can emit ``target``."""
    return len(target) + sum(1 for a, b in zip(target[:-1], target[1:]) if a == b)


def collapse(symbols, blank):
    """What a frame-wise symbol sequence reads as: merge repeats, drop blanks."""
    out, prev = [], None
    for s in symbols:
        if s != prev and s != blank:
            out.append(int(s))
        prev = s
    return out


def alignment(variant, Tn, target, blank):
    """The Tn symbols of the prescribed alignment (an utterance too short for its target gets a truncated one: its loss is
    +inf whatever the logits).  Trap variants fall back to ``spread`` where the target offers no place for the trap."""
    target = [int(v) for v in target]
    core = []                                   # the shortest valid emission: a blank only between equal neighbours
    for i, k in enumerate(target):
        if i and target[i - 1] == k:
            core.append(blank)
        core.append(k)
    if Tn <= 0:
        return []
    if not core:
        return [blank] * Tn
    spare = Tn - len(core)
    if spare < 0:
        return core[:Tn]
    if variant == "early":
        return [blank] * spare + core
    if variant == "late":
        return core + [blank] * spare
    if variant == "trap_repeat":                # the blank between two equal labels becomes that label
        core = [core[i - 1] if k == blank else k for i, k in enumerate(core)]
    elif variant == "trap_skip":                # the middle label becomes a blank
        pos = [i for i, k in enumerate(core) if k != blank][len(target) // 2]
        core = core[:pos] + [blank] + core[pos + 1:]
    elif variant != "spread":
        raise ValueError(variant)
    reps = [Tn // len(core) + (1 if i < Tn % len(core) else 0) for i in range(len(core))]
    return [k for k, r in zip(core, reps) for _ in range(r)]


# ---- batches ---------------------------------------------------------------------------------------------------------------
def labels(L, V, blank, repeats=3, seed=0):
    """L labels cycling through the non-blank symbols from a seeded start, lowest and highest among them, with equal
    neighbours at the first, a middle and the last pair (at most ``repeats`` of them; V = 2 has one symbol: all repeats)."""
    sym = [k for k in range(V) if k != blank]
    if L == 0 or not sym:
        return []
    order = [sym[0], sym[-1]] + sym[1:-1] if len(sym) > 2 else sym
    out = [order[(seed + i) % len(order)] for i in range(L)]
    if len(sym) > 1 and L >= 2:
        for p in sorted({L - 1, L // 2, 1})[-repeats:] if repeats else ():
            out[p] = out[p - 1]
    return out


class Batch:
    """One call's inputs: x [T, N, V] float32 (``logits()``), in_lens, targets (a list of label lists), blank."""

    def __init__(self, name, T, V, blank, in_lens, targets, family, variant=None, gate=None, log_probs_in=False, seed=0):
        self.name, self.T, self.V, self.blank = name, T, V, blank
        self.in_lens, self.targets = [int(v) for v in in_lens], [list(map(int, t)) for t in targets]
        self.family, self.variant, self.gate, self.log_probs_in, self.seed = family, variant, gate, log_probs_in, seed
        self.N = len(self.in_lens)
        assert len(self.targets) == self.N and family in FAMILIES and 0 <= blank < V
        assert all(0 <= k < V and k != blank for t in self.targets for k in t), name
        self.S_max = 2 * max(len(t) for t in self.targets) + 1
        self.id = f"{name}-{family}" + (f"-{variant}" if variant else "")
        self._x = self._ref = None

    def logits(self):
        if self._x is None:
            rng = np.random.default_rng([FAMILIES.index(self.family), self.T, self.N, self.V, self.blank, self.seed])
            x = (3.0 * rng.standard_normal((self.T, self.N, self.V))).astype(np.float32)
            for n in range(self.N):
                Tn = min(max(self.in_lens[n], 0), self.T)
                if self.family == "count":
                    x[:Tn, n, :] = x[:Tn, n, :1]
                elif self.family == "path":
                    x[:Tn, n, :] = 0.0
                    sym = alignment(self.variant, Tn, self.targets[n], self.blank)
                    x[np.arange(Tn), n, sym] = PATH_LOGIT
            if self.log_probs_in:               # log-probabilities: normalised here, in float64, rounded once
                x64 = x.astype(np.float64)
                m = x64.max(axis=2, keepdims=True)
                x = (x64 - m - np.log(np.exp(x64 - m).sum(axis=2, keepdims=True))).astype(np.float32)
            x.setflags(write=False)
            self._x = x
        return self._x

    def reference(self, zero_infinity=False):
        """Computed once, shared and read-only; the zero_infinity form differs only at impossible targets."""
        if self._ref is None:
            base = reference(self.logits(), self.in_lens, self.targets, self.blank, False, self.log_probs_in)
            zi = {k: v.copy() for k, v in base.items()}
            zi["nll_out"][base["infeasible"]] = 0.0
            zi["grad"][:, base["infeasible"], :] = 0.0
            zi["grad_defined"][:] = True
            for r in (base, zi):
                for v in r.values():
                    v.setflags(write=False)
            self._ref = {False: base, True: zi}
        return self._ref[bool(zero_infinity)]

    def replaced(self, x, name):
        """The same call with other logits (a float32 array of the same shape; kept as it is)."""
        b = Batch(name, self.T, self.V, self.blank, self.in_lens, self.targets, self.family, self.variant, self.gate, self.log_probs_in)
        assert x.shape == (self.T, self.N, self.V) and x.dtype == np.float32
        b._x = x.copy()
        b._x.setflags(write=False)
        return b

    def routes(self, wave=True):
        return forward_route(self.T, self.V, self.S_max, wave), backward_route(self.T, self.V, self.S_max, wave)


# the one toleranced batch whose BACKWARD bound exceeds BOUND_CAP: at V = 16 000 behind the 64 KiB gate the gradient comes from
# ctc_grad_kernel, whose normaliser is one thread's serial sum of 16 000 terms -- the a-priori bound of that sum alone is
# ~0.8 V 2^-24 per frame on gaussian logits.  Its forward bound (the tree sum of the pipeline) is inside the cap.
SERIAL_WIDE_BACKWARD = "gate_V16000_L38-gauss"
SERIAL_WIDE_BACKWARD_CAP = 5e-2


def bounds(batch, ref, fwd_route, bwd_route):
    """(bound_nll [N], bound_grad [N]) of a toleranced batch on the given routes; asserts the <= 1e-2 condition."""
    bn = bound_nll(ref, z_of(fwd_route, batch.V))
    bb = bound_nll(ref, z_of(bwd_route, batch.V))
    ok = ~(ref["poisoned"] | ref["infeasible"])
    assert np.all(bn[ok] <= BOUND_CAP), (batch.id, fwd_route, bn)
    cap = SERIAL_WIDE_BACKWARD_CAP if (batch.id == SERIAL_WIDE_BACKWARD and bwd_route == "lds_row") else BOUND_CAP
    assert np.all(bb[ok] <= cap), (batch.id, bwd_route, bb)
    return bn, 3 * bb + 2.0 ** -18


WITHOUT_WAVE = ("lane", "ring", "alphabet", "feasibility", "small", "trap")     # gates whose batches run again under MS_CTC_WAVE=0


def _blanks(V):
    return sorted({0, V // 2, V - 1})


def _families(name, T, V, blank, in_lens, targets, fams, gate=None, variants=VALID_VARIANTS):
    out = []
    for fam in fams:
        for var in (variants if fam == "path" else (None,)):
            out.append(Batch(name, T, V, blank, in_lens, targets, fam, var, gate))
    return out


LANE_FORMS = (
    ("lane_K1", (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 127), 140, (125, 126, 140, 139, 138, 137, 136, 135, 134, 133, 132)),
    ("lane_K2", (63, 64, 65, 128, 191, 192, 255), 270, tuple(270 - 2 * n for n in range(7))),
    ("lane_K4", (127, 128, 129, 256, 383, 384, 511, 127, 128), 530, (530, 529, 528, 527, 526, 525, 524, 523, 522)),
    ("lane_lds_row", (512, 2, 129), 530, (530, 523, 522)),
)


@lru_cache(maxsize=None)
def lane_batches():
    """One batch per states-per-lane form (S_max selects the form for the whole batch) and one past S_max = 1 024, ``path``
    only: the lattices are past the T at which gauss and count stay inside the cap.  K = 1 has the last two states in different
    waves at S = 65, 129, 193 (L = 32, 64, 96) and, with the ring batch, in_lens on every residue of its 16-deep ring; K = 4's in_lens 522 .. 530 cover
    every residue of its 8-deep ring."""
    out = []
    for k, (name, Ls, T, lens) in enumerate(LANE_FORMS):
        blank = _blanks(5)[k % 3]
        tg = [labels(L, 5, blank, seed=i) for i, L in enumerate(Ls)]
        out += _families(name, T, 5, blank, lens, tg, ("path",), "lane")
    return tuple(out)


@lru_cache(maxsize=None)
def ring_batches():
    """in_lens on every residue that matters of the 16-deep register ring, in a T = 40 buffer (rows lie past every length); up
    to 3 labels; utterance 3 (3 frames for a, a, b) is impossible, utterance 0 has no frame and no label."""
    lens = [0, 1, 2, 3, 15, 16, 17, 18, 31, 32, 33, 34]
    out = []
    for blank in _blanks(5):
        a, b, c = [k for k in range(5) if k != blank][:3]
        tg = [[], [a], [b], [a, a, b], [a, b, c], [c, c, c], [b, a], [], [c, b, a], [a], [b, b], [a, c, c]]
        out += _families(f"ring_b{blank}", 40, 5, blank, lens, tg, FAMILIES, "ring")
    return tuple(out)


@lru_cache(maxsize=None)
def feasibility_batches():
    """T_n = L + repeats (exactly one alignment) and one frame fewer (none), with and without repeats."""
    out = []
    for blank in (0, 4):
        a, b = [k for k in range(5) if k != blank][:2]
        tg = [[a, b, a], [a, b, a], [a, a, b, b], [a, a, b, b], [a], [a], [], []]
        lens = [3, 2, 6, 5, 1, 0, 1, 0]
        out += _families(f"feasible_b{blank}", 8, 5, blank, lens, tg, FAMILIES, "feasibility")
    return tuple(out)


@lru_cache(maxsize=None)
def small_lattice_batches():
    """The largest lattice at which gauss and count are toleranced (T = 64, V = 29, 31 labels: S = 63, 64 is one wave)."""
    out = []
    for blank in _blanks(29):
        tg = [labels(L, 29, blank, seed=L) for L in (31, 30, 12, 0)]
        out += _families(f"small_b{blank}", 64, 29, blank, [64, 63, 49, 17], tg, ("count", "gauss"), "small")
    return tuple(out)


ALPHABETS = (1, 2, 32, 33, 64, 65, 128, 1024, 1025, 2049)


@lru_cache(maxsize=None)
def alphabet_batches():
    """T = 6, N = 3, L <= 3, the lowest and the highest non-blank symbol among the labels; every blank of {0, middle, V - 1}.
    V = 1 has only the blank: empty targets.  32 / 33 and 64 / 65: alpha_wave_normalise<32> / <64> / the wide frame; 1 024 /
    1 025: the 64 x 16 slab edge of ctc_normalise_wide_frame; 2 049: a third slab of one symbol."""
    out = []
    for V in ALPHABETS:
        for blank in _blanks(V):
            sym = [k for k in range(V) if k != blank]
            if not sym:
                tg = [[], [], []]
            else:
                lo, hi, mid = sym[0], sym[-1], sym[len(sym) // 2]
                tg = [[lo, hi, lo], [hi, hi], [mid]]
            out += _families(f"alphabet_V{V}_b{blank}", 6, V, blank, [6, 5, 4], tg, FAMILIES, "alphabet", ("spread",))
    return tuple(out)


@lru_cache(maxsize=None)
def gate_batches():
    """Either side of the mailbox gate (T = 6 826 uses every byte of the 160 KiB, 6 827 runs the LDS-row kernels) and of the
    gradient-row gate ((5 S_max + V + 1) 4 <= 64 KiB: at V = 16 000 between 37 and 38 labels; past it the forward still runs the
    pipeline and the backward ctc_grad_kernel)."""
    out = []
    for T in (LAST_MAILBOX_T, LAST_MAILBOX_T + 1):
        out += _families(f"gate_T{T}", T, 3, 1, [T, T - 9], [[0, 2], [2, 2]], ("path",), "mailbox")
    for L in (37, 38):
        blank = 8000
        tg = [labels(L, 16000, blank, repeats=2, seed=1), labels(5, 16000, blank, seed=2)]   # 38 + 2 repeats = T
        out += _families(f"gate_V16000_L{L}", 40, 16000, blank, [40, 33], tg, ("path", "gauss"), "grad_rows", ("spread", "late"))
    return tuple(out)


# which side of which gate a batch is meant to reach: (forward route, backward route, states per lane or None)
INTENDED = {
    "lane_K1": ("pipeline", "pipeline", 1), "lane_K2": ("pipeline", "pipeline", 2), "lane_K4": ("pipeline", "pipeline", 4),
    "lane_lds_row": ("lds_row", "lds_row", None),
    f"gate_T{LAST_MAILBOX_T}": ("pipeline", "pipeline", 1), f"gate_T{LAST_MAILBOX_T + 1}": ("lds_row", "lds_row", None),
    "gate_V16000_L37": ("pipeline", "pipeline", 1), "gate_V16000_L38": ("pipeline", "lds_row", 1),
}


@lru_cache(maxsize=None)
def trap_batches():
    """Invalid alignments: every target has an equal pair (trap_repeat) and a middle label that differs from its neighbours'
    merge (trap_skip)."""
    out = []
    for blank in _blanks(5):
        a, b, c = [k for k in range(5) if k != blank][:3]
        tg = [[a, a, b], [a, b, b, c], [c, a, a], [b, b]]
        tg_skip = [[a, b, c], [a, b, c, a], [c, a, b], [b, c, a, c, b]]
        out.append(Batch(f"trap_b{blank}", 20, 5, blank, [20, 17, 12, 9], tg, "path", "trap_repeat", "trap"))
        out.append(Batch(f"trap_b{blank}", 20, 5, blank, [20, 17, 12, 9], tg_skip, "path", "trap_skip", "trap"))
    return tuple(out)


def toleranced_batches():
    """Every batch whose values a test compares within the bound."""
    return (lane_batches() + ring_batches() + feasibility_batches() + small_lattice_batches() + alphabet_batches()
            + gate_batches() + trap_batches())


# ---- non-finite input ------------------------------------------------------------------------------------------------------
def nonfinite_batch(V, S_long=0, log_probs_in=False):
    """N = 5, T = 40: utterance 0 clean; 1 a NaN at frame 3 in a symbol its target does not use; 2 a +inf logit; 3 a row of
    -inf; 4 a NaN only in a padding frame.  With log-probabilities given, utterances 1 to 3 all get a NaN (+inf and a row of
    -inf are legal log-probabilities of their own kind).  ``S_long`` > 0 gives utterance 0 that many labels (S_max > 1 024
    reaches the LDS-row kernels naturally; T grows to fit)."""
    blank = V // 2
    sym = [k for k in range(V) if k != blank]
    tg = [labels(S_long or 4, V, blank, seed=0), [sym[0], sym[1]], [sym[1], sym[1], sym[0]], [sym[0]], [sym[1], sym[0]]]
    T = 40 if not S_long else min_frames(tg[0]) + 6
    lens = [T, 33, 40, 25, 30]
    # (a long utterance 0 is far past the T at which gaussian logits stay inside the cap: ``path`` there)
    b = Batch(f"nonfinite_V{V}_S{S_long}", T, V, blank, lens, tg, "path" if S_long else "gauss", "spread" if S_long else None,
              log_probs_in=log_probs_in, seed=7)
    x = b.logits().copy()
    unused = [k for k in range(V) if k != blank and k not in tg[1]][-1]
    x[3, 1, unused] = np.nan
    if log_probs_in:
        x[20, 2, sym[0]] = np.nan
        x[11, 3, blank] = np.nan
    else:
        x[20, 2, sym[0]] = np.inf
        x[11, 3, :] = -np.inf
    x[35, 4, blank] = np.nan                    # in_lens[4] = 30
    return b.replaced(x, b.name)


# ---- the float32 restatement of the pipeline's recursion (CPU only: proves the bound has room) -----------------------------
CTC_NEG = np.float32(-1.0e30)


def restate_f32(x, in_lens, targets, blank, log_probs_in=False):
    """nll [N] float32 the way ctc_alpha_wave_kernel computes it: phase 1 in float32 with a serial normaliser sum, clamped
    log2-domain log-probabilities, the max3 / exp2 / log2 recursion on finite numbers (numpy's exp2 / log2 stand in for
    v_exp_f32 / v_log_f32).  Finite inputs only."""
    f = np.float32
    T, N = x.shape[:2]
    nll = np.zeros(N, dtype=f)
    for n in range(N):
        Tn = int(min(max(in_lens[n], 0), T))
        ext = ext_labels(targets[n], blank)
        S = len(ext)
        if Tn == 0:
            nll[n] = f(0.0) if S == 1 else f(np.inf)
            continue
        r = x[:Tn, n, :].astype(f)
        if log_probs_in:
            lz = np.zeros(Tn, dtype=f)
        else:
            m = r.max(axis=1)
            with np.errstate(under="ignore"):
                lz = np.log(np.cumsum(np.exp(r - m[:, None]), axis=1, dtype=f)[:, -1]).astype(f) + m
        lp2 = np.clip((r - lz[:, None]) * f(1.4426950408889634), CTC_NEG, -CTC_NEG).astype(f)[:, ext]
        skip = np.zeros(S, bool)
        skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
        a = np.full(S, CTC_NEG, dtype=f)
        a[:2] = lp2[0, :2]
        neg1, neg2 = np.full(1, CTC_NEG, dtype=f), np.full(2, CTC_NEG, dtype=f)
        with np.errstate(under="ignore", over="ignore"):
            for t in range(1, Tn):
                a1 = np.concatenate((neg1, a[:-1]))
                a2 = np.where(skip, np.concatenate((neg2, a[:-2])), CTC_NEG) if S > 1 else neg1
                m = np.maximum(np.maximum(a, a1), a2)
                e = (np.exp2(a - m) + np.exp2(a1 - m)) + np.exp2(a2 - m)
                a = ((np.log2(e) + m) + lp2[t]).astype(f)
            l1, l2 = a[S - 1], (a[S - 2] if S > 1 else CTC_NEG)
            m = max(l1, l2)
            ll2 = np.log2(np.exp2(l1 - m) + np.exp2(l2 - m)) + m
        nll[n] = f(np.inf) if m < f(0.5) * CTC_NEG else -(f(ll2) * f(0.6931471805599453))
    return nll


# ---- the check the GPU tests share ------------------------------------------------------------------------------------------
RATIOS = {}                                     # family -> [largest loss error / bound, largest gradient error / bound]


def check(batch, got_nll, got_grad, zero_infinity, fwd_route, bwd_route, what, grad_nll=None):
    """got_nll [N] float32, got_grad [T, N, V] float32 (or None: forward only) against the reference of ``batch``: the
    finiteness pattern, +inf (0 and a zero gradient under zero_infinity) for impossible targets, exact zeros on padding
    frames, values inside the bound.  Records error / bound per family in RATIOS."""
    ref = batch.reference(zero_infinity)
    bn, bg = bounds(batch, ref, fwd_route, bwd_route)
    go = np.ones(batch.N) if grad_nll is None else np.asarray(grad_nll, dtype=np.float64)
    want = ref["nll_out"]
    fin = np.isfinite(want)
    assert got_nll.dtype == np.float32 and got_nll.shape == want.shape, what
    assert np.array_equal(np.isnan(got_nll), np.isnan(want)), (what, "NaN pattern", got_nll.tolist(), want.tolist())
    assert np.array_equal(np.isposinf(got_nll), np.isposinf(want)), (what, "+inf pattern", got_nll.tolist(), want.tolist())
    err = np.abs(got_nll[fin].astype(np.float64) - want[fin])
    zi_zero = ref["infeasible"][fin] & bool(zero_infinity)
    assert np.all(err[zi_zero] == 0.0), (what, "zero_infinity must give exactly 0")
    rat = RATIOS.setdefault(batch.family, [0.0, 0.0])
    pos = bn[fin] > 0                           # (an utterance without frames has a bound of 0: its loss is exact)
    if pos.any():
        rat[0] = max(rat[0], float((err[pos] / bn[fin][pos]).max()))
    assert np.all(err <= bn[fin]), (what, "nll", got_nll.tolist(), want.tolist(), bn.tolist())
    if got_grad is None:
        return
    assert got_grad.dtype == np.float32 and got_grad.shape == ref["grad"].shape, what
    for n in range(batch.N):
        Tn = int(ref["Tn"][n])
        g = got_grad[:, n, :]
        assert np.all(g[Tn:] == 0.0), (what, n, "padding frames must be exact zeros")
        if not ref["grad_defined"][n]:
            continue
        w = ref["grad"][:Tn, n, :] * go[n]
        assert np.array_equal(np.isnan(g[:Tn]), np.isnan(w)), (what, n, "gradient NaN pattern")
        if ref["poisoned"][n]:
            continue
        if ref["infeasible"][n]:
            assert np.all(g[:Tn] == 0.0), (what, n, "zero_infinity: the gradient of an impossible target is exactly 0")
            continue
        e = np.abs(g[:Tn].astype(np.float64) - w)
        b = bg[n] * abs(go[n])
        if e.size:
            rat[1] = max(rat[1], float(e.max() / b))
        assert np.all(e <= b), (what, n, "gradient", float(e.max()), float(b), np.argwhere(e > b)[:4].tolist())
