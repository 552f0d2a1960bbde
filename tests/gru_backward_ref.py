"""numpy side of the GRU backward (``ms_gru_recompute`` / ``ms_gru_backward_steps``; TEST INFRASTRUCTURE ONLY).  OWN
specification: the comment on ``ms_gru_recompute`` in include/ms_hotpath.h.  One layer of ``torch.nn.GRU``: gate order r, z, n,
  r = sig(x w_ir^T + b_ir + h_prev w_hr^T + b_hr),  z alike,  q = h_prev w_hn^T + b_hn,  n = tanh(x w_in^T + b_in + r q),
  h_t = (1 - z) n + z h_prev;
``lens`` sorted descending or None; rows ``t >= lens[n]`` of the output are 0 and carry no gradient, ``h_n`` is the state at
``lens[n] - 1``.  The reverse direction of sequence n is the same cell walked from ``lens[n] - 1`` down to 0 from ``h0[1][n]``,
which is the forward cell on the sequence flipped within its own length (``flip_time``): direction 1 of everything below is the
direction-0 function on ``dir_view(k, 1)``, its per-step results flipped back (``back``).

``forward(p, x, h0, lens)``                            float64 layer forward: out [T,N,H], h_n.
``recompute(p, x, h, h0, lens)``                       float64 gates [T,N,3H] (activated), q [T,N,H] from a GIVEN output h.
``backward_steps(p, gates, q, h, h0, d_out, d_hn, lens)``   float64 dGi, dGh, d_h0, d_b_ih, d_b_hh.
``batch_products(p, dGi, dGh, x, h, h0, lens)``        float64 dx, d_w_ih, d_w_hh.
``emulate(name, d)``                                   the two device calls in float32, in the device's order of operations.
``recompute_bounds`` / ``backward_steps(..., e_gates, e_q)``   error bounds for the device, derived below.
``cases()``                                            the bidirectional layer cases; ``stack_case()`` a two-layer bidirectional stack.

The bounds, derived (not fitted), in tests/lstm_backward_ref.py's form.  u = 2^-24.  Everything is first-order forward-error
propagation evaluated on the float64 values, each tensor's bound feeding the next one, the sum scaled by 1 + 2^-10 for the
second-order terms.  A float32 sum of K terms in ANY order is off by at most K u times the sum of the terms' magnitudes; a
product of m factors by the factors' own errors times the other factors, plus m u of the product; expf 1 ulp, tanhf 2 ulp.

Recompute.  The inputs are the device's own float32 values, so they carry no error.
  p1 = x w_i^T + b_i:   e_p1 = (In + 2) u (|x| |w_i|^T + |b_i|) = (In + 2) u m1;   p2 = h_prev w_h^T + b_h:   e_p2 = (H + 2) u m2
  a_r = p1_r + p2_r:    e_a = e_p1 + e_p2 + u (m1 + m2)  (a_z alike);   q = p2_n:   e_q = e_p2
  s = 1 / (1 + expf(-a)):   e_s = s (1 - s) e_a + 6 u s
  a_n = p1_n + r q (fused or not):   e_an = e_p1 + |q| e_r + r e_q + 2 u (m1 + |r q|)
  n = tanhf(a_n):       e_n = (1 - n^2) e_an + 4 u |n|
Nothing is carried from step to step: every h_prev is an input.

Backward steps, from gates and q that are off by e_gates and e_q (h, h0, d_out, d_hn are inputs).  With the coefficients
  k_n = (1 - z)(1 - n^2),   k_z = (h_prev - n) z (1 - z),   k_r = k_n q r (1 - r),   k_nr = k_n r
the step is dGi = [k_r, k_z, k_n] dh, dGh = [k_r, k_z, k_nr] dh, and the carried state is dh ALONE, H numbers per sequence:
  dh_t = d_out[t] + z_{t+1} dh_{t+1} + dGh_{t+1} w_hh
so to first order  e_dh_t = M_t e_dh_{t+1} + r_t,   M_t = diag(z) + W_r^T diag(k_r) + W_z^T diag(k_z) + W_n^T diag(k_nr)  (all at
t + 1; W_g the [H, H] blocks of w_hh), with r_t the FRESH roundings, bounded per element:
  the coefficients' own errors at t + 1 (the product rule on their factors; 1 - z carries e_z + u, 1 - n^2 carries 2 |n| e_n + 2 u,
  h_prev - n carries e_n + u |h_prev - n|) times |dh_{t+1}|, through |w_hh| for the three dGh blocks and directly for z dh;
  the product's rounding (3H + 4) u |dGh_{t+1}| |w_hh|;   the three-term sum 2 u (|d_out| + |rec| + |z dh|).
As in the LSTM file the carried part is propagated with the recurrence's OWN Jacobian, not element by element with |w_hh|:
  |e_dh_t|_2 <= sum_{t' >= t} |M_t M_{t+1} .. M_{t'-1}|_2 |r_t'|_2   (2-norms, the products formed explicitly), nothing being
carried into a sequence's last step (there r = 2 u (|d_out| + |d_hn|)), and
  E_dGi(t, n) = max_j sqrt(k_r^2 + k_z^2 + k_n^2) |e_dh_t|_2 + |fresh error of dGi_t|_2      (E_dGh with k_nr for k_n)
  d_h0 = z_0 dh_0 + dGh_0 w_hh is one more step of the same recurrence with d_out = 0:  E_h0(n) = that step's |e_dh|_2
  d_b_ih = sum over the existing rows of dGi:  |e|_2 <= sum E_dGi + |(rows + 8) u sum |dGi||_2      (d_b_hh alike)
So gates and q are held per element, dGi and dGh per (t, n) row, d_h0 per n, d_b_ih and d_b_hh as wholes, all in the 2-norm.
"""
import numpy as np

U24 = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -10


def _sig(a):
    return 1.0 / (1.0 + np.exp(-a))


def _lens(lens, T, N):
    return np.full(N, T, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _bias(p, H):
    b_ih = np.zeros(3 * H) if p.get("b_ih") is None else _f64(p["b_ih"])
    b_hh = np.zeros(3 * H) if p.get("b_hh") is None else _f64(p["b_hh"])
    return b_ih, b_hh


def flip_time(a, lens):
    """a [T, N, ...]: every sequence reversed within its own length; rows past a length stay where they are."""
    if a is None:
        return None
    a = np.asarray(a)
    T, N = a.shape[:2]
    Ln = _lens(lens, T, N)
    t = np.arange(T)[:, None]
    src = np.where(t < Ln[None, :], Ln[None, :] - 1 - t, t)          # [T, N]
    return a[src, np.arange(N)[None, :]]


def back(a, d, lens):
    """A per-step tensor of direction d's unidirectional run, in the layer's own time order."""
    return flip_time(a, lens) if d == 1 else a


def forward(p, x, h0, lens):
    x = _f64(x)
    T, N, _ = x.shape
    w_ih, w_hh = _f64(p["w_ih"]), _f64(p["w_hh"])
    H = w_hh.shape[1]
    b_ih, b_hh = _bias(p, H)
    L = _lens(lens, T, N)
    h = np.zeros((N, H)) if h0 is None else _f64(h0).copy()
    out = np.zeros((T, N, H))
    for t in range(T):
        gi, gh = x[t] @ w_ih.T + b_ih, h @ w_hh.T + b_hh
        r, z = _sig(gi[:, :H] + gh[:, :H]), _sig(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        hn = (1 - z) * n + z * h
        live = (t < L)[:, None]
        h = np.where(live, hn, h)
        out[t] = np.where(live, hn, 0.0)
    return out, h


def h_prev_of(h, h0, lens):
    """h shifted one step: h0 in row 0, zero past the length."""
    h = _f64(h)
    T, N, H = h.shape
    L = _lens(lens, T, N)
    hp = np.zeros_like(h)
    hp[0] = 0.0 if h0 is None else _f64(h0)
    hp[1:] = h[:-1]
    return np.where((np.arange(T)[:, None] < L[None, :])[..., None], hp, 0.0)


def recompute(p, x, h, h0, lens, dtype=np.float64):
    """gates [T,N,3H], q [T,N,H] (rows past a length: 0 here, unspecified on the device), and the magnitude sums (m1, m2) the
    bounds need.  ``dtype=np.float32``: every operation rounded to float32 (the emulation)."""
    f = dtype
    x = np.asarray(x, dtype=f)
    T, N, In = x.shape
    w_ih, w_hh = np.asarray(p["w_ih"], dtype=f), np.asarray(p["w_hh"], dtype=f)
    H = w_hh.shape[1]
    b_ih, b_hh = (b.astype(f) for b in _bias(p, H))
    L = _lens(lens, T, N)
    hp = h_prev_of(h, h0, lens).astype(f)
    p1 = ((x.reshape(T * N, In) @ w_ih.T).astype(f) + b_ih).astype(f).reshape(T, N, 3 * H)
    p2 = ((hp.reshape(T * N, H) @ w_hh.T).astype(f) + b_hh).astype(f).reshape(T, N, 3 * H)
    a64 = lambda a: np.abs(a.astype(np.float64))      # noqa: E731
    m1 = (a64(x).reshape(T * N, In) @ a64(w_ih).T + np.abs(b_ih)).reshape(T, N, 3 * H)
    m2 = (a64(hp).reshape(T * N, H) @ a64(w_hh).T + np.abs(b_hh)).reshape(T, N, 3 * H)
    one = f(1)
    sig = lambda a: (one / (one + np.exp(-a).astype(f))).astype(f)      # noqa: E731
    r = sig((p1[..., :H] + p2[..., :H]).astype(f))
    z = sig((p1[..., H:2 * H] + p2[..., H:2 * H]).astype(f))
    q = p2[..., 2 * H:]
    n = np.tanh((p1[..., 2 * H:] + (r * q).astype(f)).astype(f)).astype(f)
    live = (np.arange(T)[:, None] < L[None, :])[..., None]
    gates = np.where(live, np.concatenate([r, z, n], 2), 0).astype(f)
    return gates, np.where(live, q, 0).astype(f), (m1, m2)


def recompute_bounds(p, gates, q, mag):
    """(e_gates [T,N,3H], e_q [T,N,H]) from the float64 ``recompute`` (module docstring)."""
    H = q.shape[2]
    In = np.asarray(p["w_ih"]).shape[1]
    m1, m2 = mag
    e_p1, e_p2 = (In + 2) * U24 * m1, (H + 2) * U24 * m2
    e_a = e_p1 + e_p2 + U24 * (m1 + m2)
    r, z, n = gates[..., :H], gates[..., H:2 * H], gates[..., 2 * H:]
    e_r = r * (1 - r) * e_a[..., :H] + 6 * U24 * r
    e_z = z * (1 - z) * e_a[..., H:2 * H] + 6 * U24 * z
    e_q = e_p2[..., 2 * H:]
    e_an = e_p1[..., 2 * H:] + np.abs(q) * e_r + r * e_q + 2 * U24 * (m1[..., 2 * H:] + np.abs(r * q))
    e_n = (1 - n * n) * e_an + 4 * U24 * np.abs(n)
    return np.concatenate([e_r, e_z, e_n], 2) * SECOND_ORDER, e_q * SECOND_ORDER


def _prod_err(vals, errs):
    """First-order error of a float32 product of factors ``vals`` that are off by ``errs``."""
    av = [np.abs(v) for v in vals]
    total = len(vals) * U24 * np.prod(av, axis=0)
    for k, e in enumerate(errs):
        others = np.prod([av[j] for j in range(len(vals)) if j != k], axis=0) if len(vals) > 1 else 1.0
        total = total + e * others
    return total


def _norm(e):
    return np.sqrt((np.asarray(e, dtype=np.float64) ** 2).sum(-1))


def backward_steps(p, gates, q, h, h0, d_out, d_hn, lens, dtype=np.float64, e_gates=None, e_q=None):
    """(dGi, dGh, d_h0, d_b_ih, d_b_hh) in ``dtype``; with ``e_gates`` / ``e_q`` (float64 run only) also the five bounds, on the
    2-norms of the rows: dGi and dGh [T, N], d_h0 [N], d_b_ih and d_b_hh (one number each)."""
    f = dtype
    gates, q, d_out = np.asarray(gates, dtype=f), np.asarray(q, dtype=f), np.asarray(d_out, dtype=f)
    T, N, H = q.shape
    w_hh = np.asarray(p["w_hh"], dtype=f)
    L = _lens(lens, T, N)
    hp_all = h_prev_of(h, h0, lens).astype(f)
    want_b = e_gates is not None
    aw = np.abs(w_hh.astype(np.float64))
    dGi, dGh = np.zeros((T, N, 3 * H), dtype=f), np.zeros((T, N, 3 * H), dtype=f)
    d_bi, d_bh = np.zeros(3 * H, dtype=f), np.zeros(3 * H, dtype=f)
    carry = np.zeros((N, H), dtype=f)
    # fresh errors (given an exact dh) and the factors the carried error goes through
    fr = dict(dh=np.zeros((T, N, H)), Gi=np.zeros((T, N, 3 * H)), Gh=np.zeros((T, N, 3 * H)), cin=np.zeros((T, N, H)))
    co = dict(k=np.zeros((T, 4, N, H)), z=np.zeros((T, N, H)))
    zero = np.zeros((N, H), dtype=f)
    dhn = zero if d_hn is None else np.asarray(d_hn, dtype=f)
    one = f(1)
    max_len = int(L.max())
    for t in range(max_len - 1, -1, -1):
        live = (t < L)[:, None]
        last = (t == L - 1)[:, None]
        if t + 1 < max_len:
            rec = (dGh[t + 1] @ w_hh).astype(f)
            e_rec = (3 * H + 4) * U24 * (np.abs(dGh[t + 1].astype(np.float64)) @ aw) if want_b else 0.0
        else:
            rec, e_rec = zero, 0.0
        inj = np.where(last, dhn, carry).astype(f)
        dh = ((rec + d_out[t]).astype(f) + inj).astype(f)
        r, z, n = gates[t, :, :H], gates[t, :, H:2 * H], gates[t, :, 2 * H:]
        qv, hp = q[t], hp_all[t]
        omz, omr = (one - z).astype(f), (one - r).astype(f)
        omn = (one - (n * n).astype(f)).astype(f)
        hmn = (hp - n).astype(f)
        da_n = ((dh * omz).astype(f) * omn).astype(f)
        da_z = (((dh * hmn).astype(f) * z).astype(f) * omz).astype(f)
        da_r = (((da_n * qv).astype(f) * r).astype(f) * omr).astype(f)
        da_nr = (da_n * r).astype(f)
        dGi[t] = np.where(live, np.concatenate([da_r, da_z, da_n], 1), 0).astype(f)
        dGh[t] = np.where(live, np.concatenate([da_r, da_z, da_nr], 1), 0).astype(f)
        d_bi = (d_bi + dGi[t].sum(0, dtype=f)).astype(f)
        d_bh = (d_bh + dGh[t].sum(0, dtype=f)).astype(f)
        new_carry = (dh * z).astype(f)
        if want_b:
            er, ez, en = (e_gates[t, :, k * H:(k + 1) * H] for k in range(3))
            zero_e = np.zeros((N, H))
            e_omz, e_omr = ez + U24, er + U24
            e_omn = 2 * np.abs(n) * en + 2 * U24
            e_hmn = en + U24 * np.abs(hmn)
            f_n = _prod_err([dh, omz, omn], [zero_e, e_omz, e_omn])
            f_z = _prod_err([dh, hmn, z, omz], [zero_e, e_hmn, ez, e_omz])
            f_r = _prod_err([da_n, qv, r, omr], [f_n, e_q[t], er, e_omr])
            f_nr = _prod_err([da_n, r], [f_n, er])
            fr["dh"][t] = e_rec + 2 * U24 * (np.abs(d_out[t]) + np.abs(rec) + np.abs(inj))
            fr["Gi"][t] = np.concatenate([f_r, f_z, f_n], 1)
            fr["Gh"][t] = np.concatenate([f_r, f_z, f_nr], 1)
            fr["cin"][t] = _prod_err([dh, z], [zero_e, ez])
            k_n = omz * omn
            co["k"][t] = np.stack([k_n * qv * r * omr, hmn * z * omz, k_n, k_n * r])      # k_r, k_z, k_n, k_nr
            co["z"][t] = z
        carry = np.where(live, new_carry, carry).astype(f)
    rec0 = (dGh[0] @ w_hh).astype(f)
    d_h0 = (carry + rec0).astype(f)
    out = (dGi, dGh, d_h0, d_bi, d_bh)
    if not want_b:
        return out
    w64 = w_hh.astype(np.float64)
    wt = [w64[k * H:(k + 1) * H].T for k in range(3)]          # the three [H, H] blocks, transposed: they act on columns
    E_Gi, E_Gh, E_h0 = np.zeros((T, N)), np.zeros((T, N)), np.zeros(N)
    eye = np.eye(H)
    e_rec0 = (3 * H + 4) * U24 * (np.abs(dGh[0]) @ aw)
    for n_ in range(N):
        phis, rn = [], []
        for t in range(int(L[n_]) - 1, -2, -1):            # t = -1: the d_h0 step
            if t == L[n_] - 1:                             # nothing is carried into a sequence's last step
                r_dh = fr["dh"][t, n_]
            else:
                kr, kz, _, knr = co["k"][t + 1][:, n_]
                m = np.diag(co["z"][t + 1][n_]) + wt[0] * kr[None, :] + wt[1] * kz[None, :] + wt[2] * knr[None, :]
                phis = [m @ ph for ph in phis]
                fresh_sum = fr["dh"][t, n_] if t >= 0 else e_rec0[n_] + 2 * U24 * (np.abs(rec0[n_]) + np.abs(carry[n_]))
                r_dh = fr["Gh"][t + 1, n_] @ aw + fr["cin"][t + 1, n_] + fresh_sum
            phis.append(eye)
            rn.append(float(np.sqrt((r_dh ** 2).sum())))
            s_norm = sum(float(np.linalg.norm(ph, 2)) * r_ for ph, r_ in zip(phis, rn))
            if t < 0:
                E_h0[n_] = s_norm
                continue
            kr, kz, kn, knr = co["k"][t][:, n_]
            E_Gi[t, n_] = float(np.max(np.sqrt(kr * kr + kz * kz + kn * kn))) * s_norm + _norm(fr["Gi"][t, n_])
            E_Gh[t, n_] = float(np.max(np.sqrt(kr * kr + kz * kz + knr * knr))) * s_norm + _norm(fr["Gh"][t, n_])
    rows = int(L.sum())
    E_bi = E_Gi.sum() + float(np.linalg.norm((rows + 8) * U24 * np.abs(dGi).sum((0, 1))))
    E_bh = E_Gh.sum() + float(np.linalg.norm((rows + 8) * U24 * np.abs(dGh).sum((0, 1))))
    return out, tuple(b * SECOND_ORDER for b in (E_Gi, E_Gh, E_h0, E_bi, E_bh))


def batch_products(p, dGi, dGh, x, h, h0, lens):
    """(dx, d_w_ih, d_w_hh) in float64: the three GEMMs over T N rows that finish the layer."""
    dGi, dGh, x = _f64(dGi), _f64(dGh), _f64(x)
    T, N, In = x.shape
    H = dGi.shape[2] // 3
    gi2, gh2 = dGi.reshape(T * N, 3 * H), dGh.reshape(T * N, 3 * H)
    dx = (gi2 @ _f64(p["w_ih"])).reshape(T, N, In)
    return dx, gi2.T @ x.reshape(T * N, In), gh2.T @ h_prev_of(h, h0, lens).reshape(T * N, H)


def dir_layer_backward(p, x, h0, lens, d_out, d_hn):
    """One direction-0 layer in float64: outputs and every gradient."""
    out, hn = forward(p, x, h0, lens)
    gates, q, _ = recompute(p, x, out, h0, lens)
    dGi, dGh, d_h0, d_bi, d_bh = backward_steps(p, gates, q, out, h0, d_out, d_hn, lens)
    dx, d_w_ih, d_w_hh = batch_products(p, dGi, dGh, x, out, h0, lens)
    return dict(out=out, h_n=hn, dx=dx, d_w_ih=d_w_ih, d_w_hh=d_w_hh, d_b_ih=d_bi, d_b_hh=d_bh, d_h0=d_h0)


def dir_view(k, d):
    """Direction d of a layer case as a direction-0 case (d = 1: x and d_out flipped within the lengths)."""
    H = k["H"]
    pick = lambda a: None if a is None else a[d]      # noqa: E731
    x = k["x"]
    d_out = None if k.get("d_out") is None else np.ascontiguousarray(k["d_out"][..., d * H:(d + 1) * H])
    if d == 1:
        x, d_out = flip_time(x, k["lens"]), flip_time(d_out, k["lens"])
    return dict(p=k["p"][d], T=k["T"], N=k["N"], H=H, In=k["In"], lens=k["lens"], x=x, h0=pick(k["h0"]), d_out=d_out,
                d_hn=pick(k.get("d_hn")))


def layer_backward(k, ndir=2):
    """The whole layer (``ndir`` directions of case k) in float64: out [T, N, ndir H], h_n [ndir, N, H] and every gradient (dx
    summed over the directions, the others stacked per direction)."""
    parts = []
    for d in range(ndir):
        u = dir_view(k, d)
        r = dir_layer_backward(u["p"], u["x"], u["h0"], u["lens"], u["d_out"], u["d_hn"])
        r["out"], r["dx"] = back(r["out"], d, k["lens"]), back(r["dx"], d, k["lens"])
        parts.append(r)
    res = dict(out=np.concatenate([r["out"] for r in parts], 2), dx=sum(r["dx"] for r in parts))
    for key in ("h_n", "d_h0", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh"):
        res[key] = np.stack([r[key] for r in parts])
    return res


def stack_backward(layers, x, h0, lens, d_out, d_hn):
    """A bidirectional stack in float64.  ``layers``: per layer the pair of parameter dicts; h0 / d_hn [2 L, N, H] or None.
    Returns out, h_n, dx, d_h0 and per layer the stacked weight gradients."""
    H = layers[0][0]["w_hh"].shape[1]
    T, N, _ = x.shape
    sl = lambda a, i: None if a is None else a[2 * i:2 * i + 2]      # noqa: E731
    mk = lambda i, xin, dtop: dict(p=layers[i], T=T, N=N, H=H, In=xin.shape[2], lens=lens, x=xin, h0=sl(h0, i), d_out=dtop,      # noqa: E731
                                   d_hn=sl(d_hn, i))
    ins = [_f64(x)]
    for i in range(len(layers)):
        ins.append(layer_backward(mk(i, ins[-1], np.zeros((T, N, 2 * H))))["out"])
    res, top = [None] * len(layers), _f64(d_out)
    for i in range(len(layers) - 1, -1, -1):
        res[i] = layer_backward(mk(i, ins[i], top))
        top = res[i]["dx"]
    return dict(out=ins[-1], h_n=np.concatenate([r["h_n"] for r in res]), dx=top, d_h0=np.concatenate([r["d_h0"] for r in res]),
                layers=res)


# name: T, N, H, In, bias, state (h0 given), d_hn, lens kind.  The step kernel's tiles are 32 hidden units x 32 batch rows and
# its K = 3H runs in quads: H in {7, 40, 74} puts 3H at 21 / 120 / 222 -- below a tile with an odd K tail and unaligned rows;
# one tile plus a tail with 16-byte rows; two tiles plus a tail with rows only 8-byte aligned.  N in {1, 3, 33} lies on both
# sides of a pass, every option appears in both settings.
_CASES = (
    ("t1_n1_h7", 1, 1, 7, 5, True, False, False, None),
    ("t2_n3_h40_equal", 2, 3, 40, 5, False, True, True, "equal"),
    ("t9_n33_h74_ragged", 9, 33, 74, 33, True, True, True, "ragged"),
    ("t9_n3_h7_ragged", 9, 3, 7, 5, True, False, True, "ragged"),
    ("t9_n33_h7", 9, 33, 7, 5, False, True, False, None),
    ("t2_n33_h74_ragged", 2, 33, 74, 33, True, False, False, "ragged"),
    ("t1_n3_h74_equal", 1, 3, 74, 5, True, True, True, "equal"),
    ("t9_n1_h74_short", 9, 1, 74, 33, True, True, True, "short"),
    ("t9_n33_h40_ragged", 9, 33, 40, 33, True, False, True, "ragged"),
)
CASE_NAMES = tuple(c[0] for c in _CASES)
LARGEST_RAGGED = "t9_n33_h74_ragged"


def _params(rng, In, H, bias):
    f32 = lambda a: a.astype(np.float32)       # noqa: E731
    return dict(w_ih=f32(rng.standard_normal((3 * H, In)) * 2 / np.sqrt(In)), w_hh=f32(rng.standard_normal((3 * H, H)) * 2 / np.sqrt(H)),
                b_ih=f32(rng.standard_normal(3 * H) * 0.5) if bias else None,
                b_hh=f32(rng.standard_normal(3 * H) * 0.5) if bias else None)


def _make_lens(rng, kind, T, N):
    if kind is None:
        return None
    if kind == "equal":
        return np.full(N, T, dtype=np.int32)
    if kind == "short":                        # all equal and below T: steps the backward never runs
        return np.full(N, max(1, T - 3), dtype=np.int32)
    lens = np.sort(np.concatenate([[T, 1], rng.integers(1, T + 1, size=N)])[:N].astype(np.int32))[::-1].copy()
    if N >= 2:                                 # ragged down to 1 (rows past a length hold values that must be ignored)
        lens[0], lens[-1] = T, 1
    return lens


def _make(name, T, N, H, In, bias, state, dhn, kind):
    rng = np.random.default_rng(sum(map(ord, name)) + 4)
    f32 = lambda a: a.astype(np.float32)       # noqa: E731
    p = (_params(rng, In, H, bias), _params(rng, In, H, bias))
    return dict(name=name, p=p, T=T, N=N, H=H, In=In, lens=_make_lens(rng, kind, T, N),
                x=f32(rng.standard_normal((T, N, In))),
                h0=f32(rng.standard_normal((2, N, H)) * 0.5) if state else None,
                d_out=f32(rng.standard_normal((T, N, 2 * H))),
                d_hn=f32(rng.standard_normal((2, N, H))) if dhn else None)


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = {c[0]: _make(*c) for c in _CASES}
    return _cases


def dir_case(name, d):
    return dir_view(cases()[name], d)


def stack_case():
    """Two bidirectional layers, 5 -> 2 x 7 -> 2 x 7, [T, N] = [6, 3] ragged, with hx and d_hn: what the node test runs."""
    rng = np.random.default_rng(2560)
    f32 = lambda a: a.astype(np.float32)       # noqa: E731
    T, N, H, In = 6, 3, 7, 5
    layers = [(_params(rng, In, H, True), _params(rng, In, H, True)), (_params(rng, 2 * H, H, True), _params(rng, 2 * H, H, True))]
    return dict(layers=layers, T=T, N=N, H=H, In=In, lens=np.array([6, 4, 1], dtype=np.int32), x=f32(rng.standard_normal((T, N, In))),
                h0=f32(rng.standard_normal((4, N, H)) * 0.5), d_out=f32(rng.standard_normal((T, N, 2 * H))),
                d_hn=f32(rng.standard_normal((4, N, H))))


def torch_stack(layers, x, h0, lens, d_out, d_hn, bidirectional=True, dtype=np.float64, tanh=False):
    """``torch.nn.GRU`` (``tanh``: ``torch.nn.RNN``) on the CPU with autograd (``pack_padded_sequence`` under lengths):
    out, h_n, dx, d_h0 and per layer and direction the weight gradients as ``stack_backward`` lays them out.  ``layers``: per
    layer a tuple of ``ndir`` parameter dicts."""
    import torch
    ndir = 2 if bidirectional else 1
    H, In = layers[0][0]["w_hh"].shape[1], layers[0][0]["w_ih"].shape[1]
    T, N, _ = x.shape
    bias = layers[0][0]["b_ih"] is not None
    td = torch.float64 if dtype == np.float64 else torch.float32
    cls = torch.nn.RNN if tanh else torch.nn.GRU
    m = cls(In, H, num_layers=len(layers), bias=bias, bidirectional=bidirectional).to(td)
    names = (("w_ih", "weight_ih"), ("w_hh", "weight_hh")) + ((("b_ih", "bias_ih"), ("b_hh", "bias_hh")) if bias else ())
    with torch.no_grad():
        for i, lp in enumerate(layers):
            for d, sfx in enumerate(("", "_reverse")[:ndir]):
                for key, tname in names:
                    getattr(m, f"{tname}_l{i}{sfx}").copy_(torch.from_numpy(np.asarray(lp[d][key]).astype(dtype)))
    t = lambda a: torch.from_numpy(np.asarray(a).astype(dtype))      # noqa: E731
    xt = t(x).requires_grad_(True)
    h0t = t(np.zeros((ndir * len(layers), N, H)) if h0 is None else h0).clone().requires_grad_(True)
    if lens is None:
        out, hn = m(xt, h0t)
    else:
        packed = torch.nn.utils.rnn.pack_padded_sequence(xt, torch.from_numpy(np.asarray(lens).astype(np.int64)), enforce_sorted=True)
        out, hn = m(packed, h0t)
        out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
    total = (out * t(d_out)).sum()
    if d_hn is not None:
        total = total + (hn * t(d_hn)).sum()
    total.backward()
    res = []
    for i in range(len(layers)):
        g = lambda n_: np.stack([getattr(m, f"{n_}_l{i}{sfx}").grad.numpy() for sfx in ("", "_reverse")[:ndir]])      # noqa: E731
        r = dict(d_w_ih=g("weight_ih"), d_w_hh=g("weight_hh"))
        if bias:
            r.update(d_b_ih=g("bias_ih"), d_b_hh=g("bias_hh"))
        res.append(r)
    return dict(out=out.detach().numpy(), h_n=hn.detach().numpy(), dx=xt.grad.numpy(), d_h0=h0t.grad.numpy(), layers=res)


def torch_layer(k, dtype=np.float64):
    """``torch.nn.GRU(bidirectional=True)`` on a layer case, with ``layer_backward``'s keys."""
    r = torch_stack([k["p"]], k["x"], k["h0"], k["lens"], k["d_out"], k["d_hn"], dtype=dtype)
    return dict(out=r["out"], h_n=r["h_n"], dx=r["dx"], d_h0=r["d_h0"], **r["layers"][0])


_refs = {}


def reference(name):
    """Per direction, computed once and never edited, in the LAYER's time order: h32 (the float32 output the device is given),
    the float64 gates, q, dGi, dGh, d_h0, d_b_ih, d_b_hh on it and their bounds.  dict of 2-lists."""
    if name not in _refs:
        k = cases()[name]
        out = {}
        for d in (0, 1):
            u = dir_case(name, d)
            o, _ = forward(u["p"], u["x"], u["h0"], u["lens"])
            h32 = o.astype(np.float32)
            gates, q, mag = recompute(u["p"], u["x"], h32, u["h0"], u["lens"])
            e_gates, e_q = recompute_bounds(u["p"], gates, q, mag)
            (dGi, dGh, d_h0, d_bi, d_bh), (e_Gi, e_Gh, e_h0, e_bi, e_bh) = backward_steps(
                u["p"], gates, q, h32, u["h0"], u["d_out"], u["d_hn"], u["lens"], e_gates=e_gates, e_q=e_q)
            r = dict(h32=h32, gates=gates, q=q, e_gates=e_gates, e_q=e_q, dGi=dGi, dGh=dGh, e_dGi=e_Gi[..., None], e_dGh=e_Gh[..., None])
            r = {key: back(v, d, k["lens"]) for key, v in r.items()}
            r["e_dGi"], r["e_dGh"] = r["e_dGi"][..., 0], r["e_dGh"][..., 0]
            r.update(d_h0=d_h0, d_b_ih=d_bi, d_b_hh=d_bh, e_h0=e_h0, e_b_ih=e_bi, e_b_hh=e_bh)
            for key, v in r.items():
                out.setdefault(key, []).append(v)
        _refs[name] = out
    return _refs[name]


def live_mask(name):
    k = cases()[name]
    return (np.arange(k["T"])[:, None] < _lens(k["lens"], k["T"], k["N"])[None, :])[..., None]


def worst_ratio(got, ref, bnd, mask=None):
    """The worst |got - ref| / bound over the elements (``mask``: the elements that are specified)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    d = np.where(np.isnan(d), np.inf, d)
    with np.errstate(all="ignore"):
        r = np.where(d == 0, 0.0, d / bnd)
    if mask is not None:
        r = np.where(np.broadcast_to(mask, r.shape), r, 0.0)
    return float(np.max(r))


def norm_ratio(got, ref, bnd):
    """The worst |got - ref|_2 / bound over the rows (last axis); a scalar ``bnd`` takes the whole tensor as one row."""
    d = np.asarray(got, dtype=np.float64) - ref
    d = np.where(np.isnan(d), np.inf, d)
    nrm = np.sqrt((d.reshape(-1) ** 2).sum()) if np.ndim(bnd) == 0 else _norm(d)
    with np.errstate(all="ignore"):
        return float(np.max(np.where(nrm == 0, 0.0, nrm / bnd)))


def recompute_ratios(name, d, gates, q):
    r = reference(name)
    live = live_mask(name)
    return dict(gates=worst_ratio(gates, r["gates"][d], r["e_gates"][d], live), q=worst_ratio(q, r["q"][d], r["e_q"][d], live))


def backward_ratios(name, d, dGi, dGh, d_h0, d_b_ih, d_b_hh):
    r = reference(name)
    return dict(dGi=norm_ratio(dGi, r["dGi"][d], r["e_dGi"][d]), dGh=norm_ratio(dGh, r["dGh"][d], r["e_dGh"][d]),
                d_h0=norm_ratio(d_h0, r["d_h0"][d], r["e_h0"][d]), d_b_ih=norm_ratio(d_b_ih, r["d_b_ih"][d], r["e_b_ih"][d]),
                d_b_hh=norm_ratio(d_b_hh, r["d_b_hh"][d], r["e_b_hh"][d]))


def emulate(name, d):
    """Direction d in float32 in the device's order of operations, in the layer's time order: gates, q, dGi, dGh, d_h0,
    d_b_ih, d_b_hh."""
    k, u = cases()[name], dir_case(name, d)
    h32 = back(reference(name)["h32"][d], d, k["lens"])          # (flip is its own inverse: the run's own order)
    g32, q32, _ = recompute(u["p"], u["x"], h32, u["h0"], u["lens"], dtype=np.float32)
    dGi, dGh, d_h0, d_bi, d_bh = backward_steps(u["p"], g32, q32, h32, u["h0"], u["d_out"], u["d_hn"], u["lens"], dtype=np.float32)
    return tuple(back(a, d, k["lens"]) for a in (g32, q32, dGi, dGh)) + (d_h0, d_bi, d_bh)


def regime_shares(name, d):
    """Shares of the live elements of direction d with r < 0.1, r > 0.9, z < 0.1, z > 0.9, |n| > 0.9, |n| < 0.5, and their count."""
    k, r = cases()[name], reference(name)
    H = k["H"]
    live = np.broadcast_to(live_mask(name), (k["T"], k["N"], H))
    g = r["gates"][d]
    rr, z, n = g[..., :H][live], g[..., H:2 * H][live], np.abs(g[..., 2 * H:][live])
    return dict(r_lo=np.mean(rr < 0.1), r_hi=np.mean(rr > 0.9), z_lo=np.mean(z < 0.1), z_hi=np.mean(z > 0.9), n_hi=np.mean(n > 0.9),
                n_lo=np.mean(n < 0.5)), int(live.sum())


def rel_err(got, ref):
    """max |got - ref| relative to the tensor's largest magnitude."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)) / max(float(np.max(np.abs(ref))), 1e-300))
