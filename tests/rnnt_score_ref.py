"""numpy side of the fused transducer scorer (``ms_rnnt_score``; TEST INFRASTRUCTURE ONLY).  OWN specification: the comment on
``ms_rnnt_score`` in include/ms_hotpath.h.

``joint_logits(enc_p, pred_p, w_out, b_out, dtype)`` builds the dense ``[N, T, U1, V1]`` array the device never stores; it is
handed to ``rnnt_loss_ref.rnnt_loss`` for nll, alpha and beta -- the recursion is not restated here.  ``emulate_logits`` is
the device's product arithmetic in float32 (tanh rounded to float32, both operands split into fp16 hi + lo, hi.hi + hi.lo +
lo.hi summed in float32), ``online_logsumexp`` its log-sum-exp over column tiles of a given width.  ``eps_v`` / ``delta`` /
``utterance_bounds`` are the error bounds derived in tests/test_rnnt_score_gpu.py; ``cases()`` builds the inputs both test
files run.
"""
import numpy as np

import rnnt_loss_ref as R

U24 = 2.0 ** -24
W_MIN, W_MAX = 2.0 ** -10, 2.0 ** 10          # the weight magnitudes the bound is stated for


def joint_logits(enc_p, pred_p, w_out, b_out, dtype=np.float64):
    """enc_p [T, N, J], pred_p [U1, N, J], w_out [V1, J], b_out [V1] or None -> x [N, T, U1, V1] in ``dtype``."""
    e = np.asarray(enc_p).astype(dtype).transpose(1, 0, 2)          # [N, T, J]
    p = np.asarray(pred_p).astype(dtype).transpose(1, 0, 2)         # [N, U1, J]
    with np.errstate(all="ignore"):
        z = np.tanh(e[:, :, None, :] + p[:, None, :, :])
        x = z @ np.asarray(w_out).astype(dtype).T
        if b_out is not None:
            x = x + np.asarray(b_out).astype(dtype)
    return x.astype(dtype)


def split16(a):
    """float32 -> (hi, lo) float32 arrays holding fp16 values: hi = fp16(a), lo = fp16(a - hi)."""
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(all="ignore"):
        hi = a.astype(np.float16).astype(np.float32)
        lo = (a - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def emulate_logits(enc_p, pred_p, w_out, b_out):
    """The device's arithmetic in float32: [N, T, U1, V1] float32."""
    e = np.asarray(enc_p, dtype=np.float32).transpose(1, 0, 2)
    p = np.asarray(pred_p, dtype=np.float32).transpose(1, 0, 2)
    with np.errstate(all="ignore"):
        arg = (e[:, :, None, :] + p[:, None, :, :]).astype(np.float32)
        z = np.tanh(arg.astype(np.float64)).astype(np.float32)
        zh, zl = split16(z)
        wh, wl = split16(w_out)
        x = ((zh @ wh.T).astype(np.float32) + (zh @ wl.T).astype(np.float32)).astype(np.float32) + (zl @ wh.T).astype(np.float32)
        if b_out is not None:
            x = x + np.asarray(b_out, dtype=np.float32)
    return x.astype(np.float32)


def online_logsumexp(x, width):
    """Z over the last axis of float32 ``x`` the way the kernel forms it: column tiles of ``width``, a running maximum and a
    running sum per row; the sum stays 0 while every column so far is -inf; NaN where Z is not finite."""
    x = np.asarray(x, dtype=np.float32)
    m = np.full(x.shape[:-1], -np.inf, dtype=np.float32)
    s = np.zeros(x.shape[:-1], dtype=np.float32)
    with np.errstate(all="ignore"):
        for c0 in range(0, x.shape[-1], width):
            tile = x[..., c0:c0 + width]
            mn = np.maximum(m, np.fmax.reduce(tile, axis=-1))
            ms = np.where(mn == -np.inf, np.float32(0), mn).astype(np.float32)
            s = (s * np.exp(m - ms) + np.sum(np.exp(tile - ms[..., None]), axis=-1, dtype=np.float32)).astype(np.float32)
            m = mn.astype(np.float32)
        z = (m + np.log(s)).astype(np.float32)
    return np.where(np.isfinite(z), z, np.float32(np.nan)).astype(np.float32)


def eps_v(w_out, b_out, J):
    """Per symbol: 2^-24 ((J + 16) sum_j |w_out[v, j]| + |b_out[v]|); a symbol whose bias is -inf is exactly -inf: 0."""
    w = np.abs(np.asarray(w_out, dtype=np.float64)).sum(-1)
    e = (J + 16) * w
    if b_out is not None:
        b = np.asarray(b_out, dtype=np.float64)
        e = np.where(np.isfinite(b), e + np.abs(np.where(np.isfinite(b), b, 0.0)), 0.0)
    return U24 * e


def delta(eps_max, z_abs_max):
    """A cell's b / e: 2 max_v eps_v (the picked logit and Z move by at most eps each) + 16 * 2^-24 max(1, |Z|)."""
    return 2.0 * eps_max + 16.0 * U24 * max(1.0, float(z_abs_max))


def utterance_bounds(ref, in_lens, tgt_lens, eps):
    """B_n + (T_n + U_n) delta_n per utterance (NaN where the reference nll is not finite); ``ref`` is the float64
    ``rnnt_loss_ref.Result`` on ``joint_logits``."""
    out = np.full(len(ref.nll), np.nan)
    eps_max = float(np.max(eps))
    for n in range(len(ref.nll)):
        if not np.isfinite(ref.nll[n]):
            continue
        Tn, Un = int(in_lens[n]), int(tgt_lens[n])
        zmax = float(np.max(np.abs(ref.Z[n][ref.exists[n]])))
        out[n] = R.bound(Tn, Un, ref.nll[n]) + (Tn + Un) * delta(eps_max, zmax)
    return out


def worst_ratios(nll, alpha, beta, ref, bounds):
    """Worst |got - ref| / bound over the utterances with a finite reference nll: nll, and alpha / beta on existing cells."""
    worst = {"nll": 0.0, "alpha": 0.0, "beta": 0.0}
    for n in range(len(ref.nll)):
        if not np.isfinite(ref.nll[n]):
            continue
        ex = ref.exists[n]

        def lattice_err(got, want):
            g, w = np.asarray(got[n], dtype=np.float64)[ex], want[n][ex].astype(np.float64)
            with np.errstate(invalid="ignore"):
                d = np.where(np.isinf(w) & (g == w), 0.0, np.abs(g - w))
            return float(np.max(np.where(np.isnan(d), np.inf, d)))

        d = abs(float(nll[n]) - float(ref.nll[n]))
        worst["nll"] = max(worst["nll"], (np.inf if np.isnan(d) else d) / bounds[n])
        if alpha is not None:
            worst["alpha"] = max(worst["alpha"], lattice_err(alpha, ref.alpha) / bounds[n])
        if beta is not None:
            worst["beta"] = max(worst["beta"], lattice_err(beta, ref.beta) / bounds[n])
    return worst


def draw_weights(rng, V1, J, scale):
    """w_out with magnitudes inside [2^-10, 2^10]."""
    w = rng.standard_normal((V1, J)) * scale
    w = np.where(w < 0, -1.0, 1.0) * np.clip(np.abs(w), W_MIN, W_MAX)
    return w.astype(np.float32)


def make_case(seed, N, T, U1, J, V1, in_lens, tgt_lens, blank, w_scale=None, labels=None):
    """enc_p, pred_p standard normal; w_out of a spread that gives logits of a few units; targets random over ``labels``
    (default: every symbol but the blank), the padding holds the blank."""
    rng = np.random.default_rng(seed)
    enc_p = rng.standard_normal((T, N, J)).astype(np.float32)
    pred_p = rng.standard_normal((U1, N, J)).astype(np.float32)
    w_out = draw_weights(rng, V1, J, (4.0 / np.sqrt(J)) if w_scale is None else w_scale)
    b_out = rng.standard_normal(V1).astype(np.float32)
    if labels is None:
        labels = [v for v in range(V1) if v != blank]
    labels = np.array([v for v in labels if v != blank])
    y = labels[rng.integers(0, len(labels), size=(N, U1 - 1))].astype(np.int32)
    y = R.pad_targets(y, tgt_lens, blank)
    return dict(enc_p=enc_p, pred_p=pred_p, w_out=w_out, b_out=b_out, in_lens=np.array(in_lens, dtype=np.int32), targets=y,
                tgt_lens=np.array(tgt_lens, dtype=np.int32), blank=blank)


def peaked_case():
    """Case d: the shape of case b with a model that KNOWS the transcript: symbol v has a random +-1 code c_v over the J
    features, pred_p[u] carries 2 c of the symbol due after y[:u] (the blank after the last label) on top of small noise,
    and w_out[v] = (16 / J) c_v on top of small weights: the right symbol leads by ~12 in every cell of the path that emits
    all labels in frame 0."""
    c = make_case(24, 2, 19, 70, 64, 29, [19, 14], [69, 33], 28, w_scale=0.02)
    rng = np.random.default_rng(25)
    J, V1 = 64, 29
    codes = np.where(rng.standard_normal((V1, J)) < 0, -1.0, 1.0).astype(np.float32)
    c["enc_p"] *= 0.1
    c["pred_p"] *= 0.1
    for n in range(2):
        Un = int(c["tgt_lens"][n])
        for u in range(70):
            due = int(c["targets"][n, u]) if u < Un else c["blank"]
            c["pred_p"][u, n] += 2.0 * codes[due]
    c["w_out"] = (c["w_out"] + (16.0 / J) * codes).astype(np.float32)
    return c


_cases = None


def cases():
    """name -> inputs of the cases (a) .. (e) of the issue (c in three variants: blank first, in the middle, last)."""
    global _cases
    if _cases is None:
        _cases = {
            "a_ragged": make_case(21, 3, 5, 4, 24, 7, [5, 1, 3], [3, 2, 0], 6),
            "b_tiles": make_case(22, 2, 19, 70, 64, 29, [19, 14], [69, 33], 28),
            "c_columns_blank0": make_case(23, 2, 9, 6, 96, 300, [9, 6], [5, 3], 0),
            "c_columns_blank150": make_case(23, 2, 9, 6, 96, 300, [9, 6], [5, 3], 150),
            "c_columns_blank299": make_case(23, 2, 9, 6, 96, 300, [9, 6], [5, 3], 299),
            "d_peaked": peaked_case(),
            "e_vocabulary": make_case(26, 2, 40, 12, 128, 4096, [40, 31], [11, 7], 4095),
        }
    return _cases


_refs = {}


def reference(name):
    """(float64 Result on the dense logits, eps_v, per-utterance bounds) of a case: computed once, never edited."""
    if name not in _refs:
        c = cases()[name]
        x = joint_logits(c["enc_p"], c["pred_p"], c["w_out"], c["b_out"])
        ref = R.rnnt_loss(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"])
        eps = eps_v(c["w_out"], c["b_out"], c["enc_p"].shape[2])
        _refs[name] = (ref._replace(grad=None), eps, utterance_bounds(ref, c["in_lens"], c["tgt_lens"], eps))
    return _refs[name]


def column_tile_width(V1):
    """The width of the kernel's column tiles: 32, 64 or 128 symbols by V1."""
    return 32 if V1 <= 32 else 64 if V1 <= 64 else 128
