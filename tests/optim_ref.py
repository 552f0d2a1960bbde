"""The numpy float32 restatement of csrc/optim.hip and myrtlespeech_amd/optim.py (TEST INFRASTRUCTURE ONLY), and the tensor
lists the GPU tests run on.

One function per entry point.  Every operator below is one rounded float32 operation on float32 arrays (numpy rounds each
ufunc on its own, ``np.sqrt`` and ``/`` are correctly rounded), which is what the device does with ``-ffp-contract=off``.  Where a
clip coefficient is needed the functions take the DEVICE's own ``norm_out`` as an input, so the update's bits do not depend on
the order in which the norm was summed; the norm itself is checked against float64 within ``norm_rel_bound``.

tests/test_optim_cpu.py holds these functions to ``torch.optim`` in float64.
"""
import math

import numpy as np

F = np.float32
U = 2.0 ** -24            # unit roundoff of float32
CHUNK = 4096              # csrc/optim.hip: elements per (tensor, chunk) pair
THREADS = 256
PAGE = 48                 # tensors per launch
SENTINEL = 12345.0


def clip_coef(norm, max_norm):
    """``q = max_norm / (norm[0] + 1e-6)``; ``q`` where it is below 1 or NaN, else 1 (float32)."""
    with np.errstate(all="ignore"):
        q = F(max_norm) / (F(norm[0]) + F(1e-6))
    return q if (q < 1 or np.isnan(q)) else F(1.0)


def grad_norm64(grads):
    """``[norm, flag]`` in float64 from float32 gradients: the yardstick of the device's order of additions."""
    s = sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads)
    r = math.sqrt(s) if s == s else float("nan")
    return r, 0.0 if math.isfinite(r) else 1.0


def grad_clip(g, norm, max_norm):
    with np.errstate(all="ignore"):
        return g * clip_coef(norm, max_norm)


def _skipped(norm, skip_nonfinite):
    return bool(skip_nonfinite) and norm is not None and norm[1] != 0


def sgd_step(p, g, b, lr, momentum=0.0, weight_decay=0.0, nesterov=False, norm=None, max_norm=0.0, skip_nonfinite=False):
    """``(p, b)`` after one step; ``b`` is None without momentum.  Inputs are not written."""
    if _skipped(norm, skip_nonfinite):
        return p.copy(), (None if b is None else b.copy())
    lr, momentum, weight_decay = F(lr), F(momentum), F(weight_decay)
    with np.errstate(all="ignore"):
        d = g * clip_coef(norm, max_norm) if norm is not None else g
        if weight_decay != 0:
            d = d + weight_decay * p
        u = d
        if momentum != 0:
            b = momentum * b + d
            u = d + momentum * b if nesterov else b
        return p - lr * u, b


def adam_scalars(lr, beta1, beta2, t):
    """``(step_size, rsqrt_bc2)`` as myrtlespeech_amd/optim.py forms them: in float64, rounded once, from the FLOAT32 values of
    the betas -- the ones the kernel multiplies by.  (With the float64 betas in the corrections and their float32 roundings in
    the moments, the first steps' ``m / (1 - beta1^t)`` is off by the betas' rounding error over ``1 - beta1``: three times
    torch's float32 error on tests/test_optim_cpu.py's cases.)"""
    b1, b2 = float(F(beta1)), float(F(beta2))
    return F(float(lr) / (1.0 - b1 ** t)), F(math.sqrt(1.0 - b2 ** t))


def adam_step(p, g, m, v, vmax, lr, t, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, norm=None, max_norm=0.0,
              skip_nonfinite=False):
    """``(p, m, v, vmax)`` after step number ``t`` (1 for the first); ``vmax`` None: no amsgrad."""
    if _skipped(norm, skip_nonfinite):
        return p.copy(), m.copy(), v.copy(), (None if vmax is None else vmax.copy())
    step_size, rsqrt_bc2 = adam_scalars(lr, beta1, beta2, t)
    beta1, beta2, eps, weight_decay = F(beta1), F(beta2), F(eps), F(weight_decay)
    omb1, omb2 = F(1.0 - float(beta1)), F(1.0 - float(beta2))
    with np.errstate(all="ignore"):
        d = g * clip_coef(norm, max_norm) if norm is not None else g
        if weight_decay != 0:
            d = d + weight_decay * p
        m = beta1 * m + omb1 * d
        v = beta2 * v + (omb2 * d) * d
        w = v
        if vmax is not None:
            vmax = np.where((v > vmax) | np.isnan(v), v, vmax)
            w = vmax
        den = np.sqrt(w) / rsqrt_bc2 + eps
        return p - step_size * (m / den), m, v, vmax


# ---- the order of the norm's additions, as far as a bound needs it --------------------------------------------------------
def norm_rel_bound(numels):
    """Relative bound of the device's ``norm_out[0]`` against float64 for the list ``numels`` (csrc/optim.hip's order).

    An element's square (one rounding) passes through at most: 3 additions inside its quad (or the 2 of a 1..3 element rest
    and the one that adds the rest), ``CHUNK / 4 / THREADS`` = 4 additions onto its thread's running sum, 6 of the wave's
    butterfly, 3 across the four waves; then, among the partials, ``ceil(P / THREADS)`` on a thread of the second launch, 6 and
    3 again.  Every term is non-negative, so the sum's relative error is at most ``(1 + u)^(depth + 1) - 1`` (Higham, 4.4:
    each addition scales what it adds by ``1 + delta``, ``|delta| <= u``); the root halves a relative error and rounds once.
    """
    partials = sum(-(-n // CHUNK) for n in numels)
    depth = 3 + CHUNK // 4 // THREADS + 1 + 6 + 3 + -(-max(partials, 1) // THREADS) + 6 + 3
    return 0.5 * ((1.0 + U) ** (depth + 1) - 1.0) * (1.0 + 1e-6) + U


# ---- tensor lists ----------------------------------------------------------------------------------------------------------
def case_numels():
    """Element counts of the GPU tests' list: empty, below / at / above a quad, a chunk and its neighbours, the view whose
    parameter starts one element past a 16-byte boundary (index ``ODD_VIEW``), 300 one-element tensors (seven pages), and one
    parameter that gets no gradient (index ``NO_GRAD``)."""
    return [0, 1, 3, 4, 5, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 1001] + [1] * 300 + [7]


ODD_VIEW = 8
NO_GRAD = 9 + 300


def layout(numels, role):
    """``(starts, total)``: where tensor ``i`` of a role (0 parameter, 1 gradient, 2.. state) starts in that role's flat
    buffer.  Tensors are separated by at least 4 sentinel elements; the start's offset from a 16-byte boundary is
    ``(i * (role + 1)) % 4`` elements, so the roles of one tensor are aligned differently from each other, except that the
    parameter of ``ODD_VIEW`` is pinned one element past a boundary and its gradient on one."""
    starts, pos = [], 4
    for i, n in enumerate(numels):
        mis = (i * (role + 1)) % 4
        if i == ODD_VIEW:
            mis = 1 if role == 0 else 0
        pos = (pos + 3) // 4 * 4 + mis
        starts.append(pos)
        pos += n + 4
    return starts, pos + 4
