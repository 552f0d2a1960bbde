"""numpy side of the fused transducer loss with gradient (``ms_rnnt_joint_loss_forward`` / ``_backward``; TEST INFRASTRUCTURE
ONLY).  OWN specification: the comment on ``ms_rnnt_joint_loss_forward`` in include/ms_hotpath.h.  Built on
tests/rnnt_loss_ref.py (the recursion and the logits' gradient) and tests/rnnt_score_ref.py (the dense logits, the device's
product arithmetic, the forward's bounds, the cases); neither is restated.

``gradients(c, grad_nll)``       float64: d_enc_p, d_pred_p, d_w_out, d_b_out chained from ``R.rnnt_loss(...).grad`` on
                                 ``S.joint_logits``, with everything the bounds need.
``weighted_nll(...)``            float64 ``sum_n grad_nll[n] nll[n]``: what the finite differences differentiate.
``emulate(c, grad_nll, planes)`` the device's arithmetic in float32: the forward's emulated logits reused, g split as 2^12 g
                                 into fp16 hi + lo planes, three products per matrix product, float32 sums.  ``planes=1``
                                 keeps the hi planes only, in all three products: what a plain fp16 MFMA would give.
``bounds(ref)``                  the error bounds, per element of each gradient.

The bounds, derived (not fitted); all absolute, all proportional to |grad_nll|.  With bound_n = B_n + (T_n + U_n) delta_n the
scorer's bound on nll, alpha and beta (tests/test_rnnt_score_gpu.py), a cell's exponent alpha + beta - ll is off by at most
3 bound_n and x - Z by delta_n, so each of the (at most three) exponential terms of g_c[v] is off by the factor

  E_n = expm1(3 bound_n + delta_n) + 8 * 2^-24          (8: the hardware exp, the product with grad_nll, the hi + lo split)

of itself.  The terms' magnitudes add up to mass_c[v] = 2 exp(x - Z + alpha + beta - ll) - g_c[v] / grad_nll[n], hence

  dg_c[v] = |grad_nll[n]| mass_c[v] E_n + 2^-36         (2^-36: the subnormal step of the fp16 planes of 2^12 g)

The products add, in units of 2^-24 of the sum of the magnitudes of their terms, their K extent (one float32 rounding per
term in whatever order, zero rows add nothing) + 32 (the dropped lo.lo term and the roundings of the lo planes, 16 as for
the logits; the factor 1 - h^2 with h recomputed, 8; spare 8):

  d_b_out[v]     sum_c dg_c[v] + 2^-24 C sum_c |g_c[v]|                          C = the number of existing cells
  da_c[j]        sum_v dg_c[v] |w[v, j]| + 2^-24 (V1 + 32) sum_v |g_c[v]| |w[v, j]|
  d_enc_p[t, n]  sum_u (da's bound) + 2^-24 U1 sum_u |da|;    d_pred_p[u, n]: the same over t, with T
  d_w_out[v, j]  sum_c dg_c[v] |h_c[j]| + 2^-24 (C + 32) sum_c |g_c[v]| |h_c[j]|

stated for |w_out| within [2^-10, 2^10] (the scorer's range) and |grad_nll| within [2^-10, 8]: 2^12 g stays inside fp16,
and the 2^-36 step is below 2^-26 |grad_nll|.
"""
from collections import namedtuple

import numpy as np

import rnnt_loss_ref as R
import rnnt_score_ref as S

U24 = 2.0 ** -24
G_SCALE = 4096.0
GN_MIN, GN_MAX = 2.0 ** -10, 8.0             # the |grad_nll| the bounds are stated for
CASE_NAMES = ("a_ragged", "b_tiles", "c_columns_blank150", "d_peaked", "e_vocabulary")
TENSORS = ("d_enc_p", "d_pred_p", "d_w_out", "d_b_out")

Grads = namedtuple("Grads", "d_enc_p d_pred_p d_w_out d_b_out")
Ref = namedtuple("Ref", "grads loss g h da w grad_nll score_bounds eps exists")


def draw_grad_nll(name, N):
    """Random signs, magnitudes log-uniform over the stated range (the first one at its upper end)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    mag = np.exp(rng.uniform(np.log(GN_MIN), np.log(GN_MAX), size=N))
    mag[0] = GN_MAX
    return (np.where(rng.random(N) < 0.5, -1.0, 1.0) * mag).astype(np.float32)


def _hidden(enc_p, pred_p, dtype):
    e = np.asarray(enc_p).astype(dtype).transpose(1, 0, 2)
    p = np.asarray(pred_p).astype(dtype).transpose(1, 0, 2)
    with np.errstate(all="ignore"):
        return np.tanh((e[:, :, None, :] + p[:, None, :, :]).astype(dtype).astype(np.float64)).astype(dtype)   # [N, T, U1, J]


def _chain(g, h, w, exists, dtype, sum_dtype):
    """(d_enc_p [T, N, J], d_pred_p [U1, N, J], d_w_out, d_b_out, da) from g [N, T, U1, V1] (0 outside the existing cells)."""
    h = np.where(exists[..., None], h, 0).astype(dtype)
    da = ((g @ w) * (1 - h * h)).astype(dtype)
    d_enc = da.sum(2, dtype=sum_dtype).transpose(1, 0, 2)
    d_pred = da.sum(1, dtype=sum_dtype).transpose(1, 0, 2)
    d_w = np.einsum("ntuv,ntuj->vj", g, h).astype(sum_dtype)
    d_b = g.sum((0, 1, 2), dtype=sum_dtype)
    return Grads(d_enc, d_pred, d_w, d_b), da


def weighted_nll(enc_p, pred_p, w_out, b_out, c, grad_nll):
    x = S.joint_logits(enc_p, pred_p, w_out, b_out)
    nll = R.rnnt_loss(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"]).nll
    return float(np.dot(np.asarray(grad_nll, dtype=np.float64), nll))


def gradients(c, grad_nll):
    """The float64 yardstick (``Ref``) of a case under ``grad_nll``."""
    grad_nll = np.asarray(grad_nll, dtype=np.float64)
    x = S.joint_logits(c["enc_p"], c["pred_p"], c["w_out"], c["b_out"])
    loss = R.rnnt_loss(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"], grad_nll=grad_nll)
    h = _hidden(c["enc_p"], c["pred_p"], np.float64)
    w = np.asarray(c["w_out"], dtype=np.float64)
    g = np.where(loss.exists[..., None], loss.grad, 0.0)
    grads, da = _chain(g, h, w, loss.exists, np.float64, np.float64)
    eps = S.eps_v(c["w_out"], c["b_out"], c["enc_p"].shape[2])
    sb = S.utterance_bounds(loss, c["in_lens"], c["tgt_lens"], eps)
    # (mass needs the logits once more; kept out of the tuple: bounds() recomputes it)
    return Ref(grads, loss, g, np.where(loss.exists[..., None], h, 0.0), da, w, grad_nll, sb, eps, loss.exists), x


def gradients_given_lattice(c, grad_nll, lattice):
    """The float64 gradients that follow from a GIVEN forward result ``lattice`` (a ``rnnt_loss_ref.Result`` whose nll, Z, alpha
    and beta are taken as they are, e.g. the float32 emulation's): the formula of the header on the float64 logits.  Against
    it a backward shows its OWN error -- ``bounds(..., lattice_share=False)`` -- without the forward's allowance."""
    grad_nll = np.asarray(grad_nll, dtype=np.float64)
    x = S.joint_logits(c["enc_p"], c["pred_p"], c["w_out"], c["b_out"])
    N, T, U1, V1 = x.shape
    ex = lattice.exists
    Z, al, be = (np.asarray(a, dtype=np.float64) for a in (lattice.Z, lattice.alpha, lattice.beta))
    g = np.zeros_like(x)
    with np.errstate(all="ignore"):
        for n in range(N):
            Tn, Un, nl = int(c["in_lens"][n]), int(c["tgt_lens"][n]), float(lattice.nll[n])
            if not ex[n].any() or not np.isfinite(nl):
                continue
            lp = x[n, :Tn, :Un + 1] - Z[n, :Tn, :Un + 1, None]
            a, b = al[n, :Tn, :Un + 1], be[n, :Tn, :Un + 1]
            gg = np.exp(lp + (a + b + nl)[..., None])
            tb = np.full((Tn, Un + 1), -np.inf)
            tb[:-1] = b[1:]
            tb[Tn - 1, Un] = 0.0
            gg[..., c["blank"]] -= np.exp(lp[..., c["blank"]] + a + tb + nl)
            for u in range(Un):
                y = int(c["targets"][n, u])
                gg[:, u, y] -= np.exp(lp[:, u, y] + a[:, u] + b[:, u + 1] + nl)
            g[n, :Tn, :Un + 1] = grad_nll[n] * gg
    h = _hidden(c["enc_p"], c["pred_p"], np.float64)
    w = np.asarray(c["w_out"], dtype=np.float64)
    grads, da = _chain(g, h, w, ex, np.float64, np.float64)
    eps = S.eps_v(c["w_out"], c["b_out"], c["enc_p"].shape[2])
    loss = R.Result(np.asarray(lattice.nll, dtype=np.float64), g, Z, al, be, ex)
    return Ref(grads, loss, g, np.where(ex[..., None], h, 0.0), da, w, grad_nll, np.zeros(N), eps, ex), x


def bounds(ref, x, lattice_share=True):
    """``Grads`` of per-element bounds (module docstring) from the float64 yardstick ``ref`` and its logits ``x``.
    ``lattice_share=False``: the backward's own share, for a yardstick that takes the forward's lattice as given
    (``gradients_given_lattice``) -- the exponent is then off by the logit's eps_v alone: E_n = expm1(max_v eps_v) + 8 * 2^-24."""
    loss, g, h, w = ref.loss, ref.g, ref.h, ref.w
    N, T, U1, V1 = g.shape
    J = h.shape[-1]
    gn = np.abs(ref.grad_nll)
    eps_max = float(np.max(ref.eps))
    dg = np.zeros_like(g)
    for n in range(N):
        if not np.isfinite(loss.nll[n]) or gn[n] == 0:
            continue
        ex = loss.exists[n]
        zmax = float(np.max(np.abs(loss.Z[n][ex])))
        E = np.expm1(3.0 * ref.score_bounds[n] + S.delta(eps_max, zmax) if lattice_share else eps_max) + 8 * U24
        with np.errstate(all="ignore"):
            occ = np.where(ex, loss.alpha[n] + loss.beta[n] + loss.nll[n], -np.inf)
            t1 = np.exp(x[n] - loss.Z[n][..., None] + occ[..., None])
        t1 = np.where(ex[..., None], t1, 0.0)
        mass = 2.0 * t1 - g[n] / ref.grad_nll[n]
        dg[n] = np.where(ex[..., None], gn[n] * mass * E + 2.0 ** -36, 0.0)
    C = int(loss.exists.sum())
    ag, aw, ah = np.abs(g), np.abs(w), np.abs(h)
    b_db = dg.sum((0, 1, 2)) + U24 * C * ag.sum((0, 1, 2))
    b_da = dg @ aw + U24 * (V1 + 32) * (ag @ aw)
    ada = np.abs(ref.da)
    b_enc = (b_da.sum(2) + U24 * U1 * ada.sum(2)).transpose(1, 0, 2)
    b_pred = (b_da.sum(1) + U24 * T * ada.sum(1)).transpose(1, 0, 2)
    b_dw = np.einsum("ntuv,ntuj->vj", dg, ah) + U24 * (C + 32) * np.einsum("ntuv,ntuj->vj", ag, ah)
    return Grads(b_enc, b_pred, b_dw, b_db)


def _emulate_logits_one_plane(c):
    e = np.asarray(c["enc_p"], dtype=np.float32).transpose(1, 0, 2)
    p = np.asarray(c["pred_p"], dtype=np.float32).transpose(1, 0, 2)
    z = np.tanh((e[:, :, None, :] + p[:, None, :, :]).astype(np.float32).astype(np.float64)).astype(np.float32)
    x = (S.split16(z)[0] @ S.split16(c["w_out"])[0].T).astype(np.float32)
    if c["b_out"] is not None:
        x = x + np.asarray(c["b_out"], dtype=np.float32)
    return x.astype(np.float32)


def emulate(c, grad_nll, planes=2):
    """``Grads`` in the device's float32 arithmetic (module docstring); ``planes=1``: hi planes only."""
    assert planes in (1, 2)
    x32 = S.emulate_logits(c["enc_p"], c["pred_p"], c["w_out"], c["b_out"]) if planes == 2 else _emulate_logits_one_plane(c)
    r32 = R.rnnt_loss(x32, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"], grad_nll=np.asarray(grad_nll, dtype=np.float32),
                      dtype=np.float32)
    ex = r32.exists
    g = np.where(ex[..., None], r32.grad, 0).astype(np.float32)
    gh, gl = S.split16(g * np.float32(G_SCALE))
    wh, wl = S.split16(c["w_out"])
    h = np.where(ex[..., None], _hidden(c["enc_p"], c["pred_p"], np.float32), 0).astype(np.float32)
    hh, hl = S.split16(h)
    inv = np.float32(1.0 / G_SCALE)
    f32 = np.float32

    def three(a_hi, a_lo, b_hi, b_lo, prod):
        out = prod(a_hi, b_hi).astype(f32)
        if planes == 2:
            out = (out + prod(a_hi, b_lo).astype(f32)).astype(f32) + prod(a_lo, b_hi).astype(f32)
        return out.astype(f32)

    dh = three(gh, gl, wh, wl, lambda a, b: a @ b)
    da = (dh * inv * (f32(1) - h * h)).astype(f32)
    d_enc = da.sum(2, dtype=f32).transpose(1, 0, 2)
    d_pred = da.sum(1, dtype=f32).transpose(1, 0, 2)
    d_w = (three(gh, gl, hh, hl, lambda a, b: np.einsum("ntuv,ntuj->vj", a, b)) * inv).astype(f32)
    d_b = ((gh + gl).sum((0, 1, 2), dtype=f32) * inv).astype(f32)
    return Grads(d_enc, d_pred, d_w, d_b), r32


def worst_ratios(got, ref, bnd):
    """name -> the worst |got - ref| / bound over the elements of each gradient (``got`` entries may be None: skipped)."""
    out = {}
    for name in TENSORS:
        a = getattr(got, name)
        if a is None:
            continue
        d = np.abs(np.asarray(a, dtype=np.float64) - getattr(ref.grads, name))
        d = np.where(np.isnan(d), np.inf, d)
        b = getattr(bnd, name)
        with np.errstate(all="ignore"):
            ratio = np.where(d == 0, 0.0, d / b)
        out[name] = float(np.max(ratio))
    return out


_refs = {}


def reference(name):
    """(grad_nll, Ref, bounds) of a case: computed once, never edited."""
    if name not in _refs:
        c = S.cases()[name]
        gn = draw_grad_nll(name, len(c["in_lens"]))
        ref, x = gradients(c, gn)
        _refs[name] = (gn, ref, bounds(ref, x))
    return _refs[name]
