"""numpy side of the HardLSTM backward (``ms_hard_lstm_recompute`` / ``ms_hard_lstm_backward_steps``; TEST INFRASTRUCTURE
ONLY).  OWN specification: the comment on ``ms_hard_lstm_recompute`` in include/ms_hotpath.h.  One direction of one
``HardLSTM`` layer: gate order i, f, g, o, no lengths (every sequence has T steps),

  a = x w_ih^T + b_ih + h_prev w_hh^T + b_hh;   z_k = 0.2 a_k + 0.5 (k in i, f, o);   i, f, o = clip(z_k, 0, 1);   g = clip(a_g, -1, 1)
  c_t = f c_prev + i g;   h_t = o clip(c_t, -1, 1)

with the derivative of the reference's ops under torch autograd: ``P(z) = [0 <= z <= 1]`` (``torch.clamp``, closed) for i, f, o
and ``Q(v) = [-1 < v < 1]`` (``torch.nn.Hardtanh``, open) for g and c.  tests/test_hard_lstm_backward_cpu.py pins both
conventions, and this restatement, to torch.  The reverse direction is the same cell on the case flipped in time
(``dir_view``), its per-step results flipped back (``back``).

``forward(p, x, h0, c0)``                       float64 layer forward: out [T,N,H], h_n, c_n.
``recompute(p, x, h, h0, c0)``                  float64 PRE-CLAMP plane [T,N,4H] = (z_i, z_f, a_g, z_o) and c [T,N,H] from a GIVEN
                                                output h (on the GPU: the device's own), and the magnitude sums the bounds need.
``backward_steps(p, pre, c, c0, d_out, d_hn, d_cn)``   float64 dA, d_h0, d_c0, d_b (+ the bounds with ``e_pre`` / ``e_c``).
``layer_backward(k)``                           the whole layer, both directions, in float64 (what the CPU test pins to torch).
``margin(pre, c)``                              the kink margin: the least of |z_k|, |z_k - 1|, |a_g +- 1|, |c +- 1|.
``cases()``                                     the shapes, seeds and weight scales the tests run.

The bounds, derived (not fitted), in the manner of tests/lstm_backward_ref.py (``L``): u = 2^-24, first-order forward-error
propagation on the float64 values, scaled by 1 + 2^-10 for the second-order terms.  They hold for a device that decides every
gate as the float64 run does, which is what the margin conditions of the tests secure: a clamp is then the identity (error
passed on unchanged) or a constant (error 0) on both sides, and P, Q are the same 0 / 1.

Recompute (the inputs are the device's own float32 values and carry no error):
  a:    e_a = (In + H + 4) u (|x| |w_ih|^T + |b_ih| + |h_prev| |w_hh|^T + |b_hh|)                         (as in ``L``)
  z:    fl(fl(0.2f a) + 0.5f), the hard cell's single roundings:  e_z = 0.2 e_a + |0.2f - 0.2| |a| + u |0.2 a| + u |z|
  a_g:  e_a itself
  gate values: e_i = P(z_i) e_z (f, o alike), e_g = Q(a_g) e_a
  c_t = f c_prev + i g:   e_c = f e_c(t-1) + |c_prev| e_f + i e_g + |g| e_i + 2 u (|f c_prev| + |i g|)

Backward steps.  The carried error goes through the recurrence's own Jacobian exactly as in ``L`` (2-norms per sequence, the
products of the step matrices formed explicitly), with the hard cell's coefficients
  k_i = 0.2 g P(z_i),  k_f = 0.2 c_prev P(z_f),  k_g = i Q(a_g),  k_o = 0.2 clip(c) P(z_o);   dc <- dh: o Q(c);   dc <- dc: f
and the fresh roundings of a step, per element:
  rec = dA_next w_hh:      (4H + 4) u |dA_next| |w_hh| + (the fresh error of dA_next) |w_hh|
  dh  = d_out + rec + d_hn:   2 u (|d_out| + |rec| + |d_hn|)
  dc  = dc_in + Q(c) (dh o):  the product rule on o + u of the term, + 2 u (|dc_in| + |term|)
  dc_in = f dc:               the product rule on f + 2 u of it
  dA:  (dc g) 0.2, (dc c_prev) 0.2, dc i, (dh clip(c)) 0.2, each under its select: the product rule on the factors that carry an
       error (0.2f carries |0.2f - 0.2|) + one u per multiply
dA is held per (t, n) row, d_h0 and d_c0 per n, d_b as a whole, all in the 2-norm; the plane and c per element.
"""
import numpy as np

import lstm_backward_ref as L

U24 = L.U24
SECOND_ORDER = L.SECOND_ORDER
C02_ERR = abs(float(np.float32(0.2)) - 0.2)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def clip01(v):
    return np.minimum(np.maximum(v, 0.0), 1.0)


def clip11(v):
    return np.minimum(np.maximum(v, -1.0), 1.0)


def P(z):
    """torch.clamp(., 0, 1): the gradient passes on the CLOSED interval."""
    return ((z >= 0.0) & (z <= 1.0)).astype(np.float64)


def Q(v):
    """torch.nn.Hardtanh: the gradient passes on the OPEN interval."""
    return ((v > -1.0) & (v < 1.0)).astype(np.float64)


def _pre(a, H):
    """a [.., 4H] -> the pre-clamp plane (z_i, z_f, a_g, z_o)."""
    out = 0.2 * a + 0.5
    out[..., 2 * H:3 * H] = a[..., 2 * H:3 * H]
    return out


def forward(p, x, h0, c0):
    x = _f64(x)
    T, N, _ = x.shape
    w_ih, w_hh = _f64(p["w_ih"]), _f64(p["w_hh"])
    H = w_hh.shape[1]
    b_ih, b_hh = L._bias(p, H)
    h = np.zeros((N, H)) if h0 is None else _f64(h0).copy()
    c = np.zeros((N, H)) if c0 is None else _f64(c0).copy()
    out = np.zeros((T, N, H))
    for t in range(T):
        z = _pre(x[t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh, H)
        i, f, g, o = clip01(z[:, :H]), clip01(z[:, H:2 * H]), clip11(z[:, 2 * H:3 * H]), clip01(z[:, 3 * H:])
        c = f * c + i * g
        h = o * clip11(c)
        out[t] = h
    return out, h, c


def recompute(p, x, h, h0, c0):
    """(pre [T,N,4H], c [T,N,H], mag [T,N,4H]) in float64 from a GIVEN output h."""
    x = _f64(x)
    T, N, In = x.shape
    w_ih, w_hh = _f64(p["w_ih"]), _f64(p["w_hh"])
    H = w_hh.shape[1]
    b_ih, b_hh = L._bias(p, H)
    hp = L.h_prev_of(h, h0, None)
    a = (x.reshape(T * N, In) @ w_ih.T + b_ih + hp.reshape(T * N, H) @ w_hh.T + b_hh).reshape(T, N, 4 * H)
    mag = (np.abs(x).reshape(T * N, In) @ np.abs(w_ih).T + np.abs(b_ih) + np.abs(hp).reshape(T * N, H) @ np.abs(w_hh).T
           + np.abs(b_hh)).reshape(T, N, 4 * H)
    pre = _pre(a, H)
    c = np.zeros((T, N, H))
    cprev = np.zeros((N, H)) if c0 is None else _f64(c0)
    for t in range(T):
        cprev = clip01(pre[t, :, H:2 * H]) * cprev + clip01(pre[t, :, :H]) * clip11(pre[t, :, 2 * H:3 * H])
        c[t] = cprev
    return pre, c, mag


def recompute_bounds(p, pre, c, c0, mag):
    """(e_pre [T,N,4H], e_c [T,N,H]) from the float64 ``recompute`` (module docstring)."""
    T, N, H4 = pre.shape
    H = H4 // 4
    In = np.asarray(p["w_ih"]).shape[1]
    e_a = (In + H + 4) * U24 * mag
    a = (pre - 0.5) / 0.2
    e_pre = 0.2 * e_a + C02_ERR * np.abs(a) + U24 * np.abs(0.2 * a) + U24 * np.abs(pre)
    e_pre[..., 2 * H:3 * H] = e_a[..., 2 * H:3 * H]
    e_c = np.zeros((T, N, H))
    e_prev = np.zeros((N, H))
    cprev = np.zeros((N, H)) if c0 is None else _f64(c0)
    for t in range(T):
        zi, zf, ag = pre[t, :, :H], pre[t, :, H:2 * H], pre[t, :, 2 * H:3 * H]
        i, f, g = clip01(zi), clip01(zf), clip11(ag)
        ei, ef, eg = P(zi) * e_pre[t, :, :H], P(zf) * e_pre[t, :, H:2 * H], Q(ag) * e_pre[t, :, 2 * H:3 * H]
        e_prev = f * e_prev + np.abs(cprev) * ef + i * eg + np.abs(g) * ei + 2 * U24 * (np.abs(f * cprev) + np.abs(i * g))
        e_c[t] = e_prev
        cprev = c[t]
    return e_pre * SECOND_ORDER, e_c * SECOND_ORDER


def margin(pre, c):
    """The least distance of any pre-clamp value or cell state from a kink of its clamp."""
    H = c.shape[-1]
    z = np.concatenate([pre[..., :2 * H], pre[..., 3 * H:]], -1)
    ag = pre[..., 2 * H:3 * H]
    return float(min(np.min(np.abs(z)), np.min(np.abs(z - 1.0)), np.min(np.abs(ag - 1.0)), np.min(np.abs(ag + 1.0)),
                     np.min(np.abs(c - 1.0)), np.min(np.abs(c + 1.0))))


def regions(pre, c):
    """name -> fraction of the elements in it: the saturated regions and the interiors of every clamp."""
    H = c.shape[-1]
    out = {}
    for name, v in (("i", pre[..., :H]), ("f", pre[..., H:2 * H]), ("o", pre[..., 3 * H:])):
        out[name + "_low"], out[name + "_high"], out[name + "_in"] = np.mean(v < 0), np.mean(v > 1), np.mean((v >= 0) & (v <= 1))
    for name, v in (("g", pre[..., 2 * H:3 * H]), ("c", c)):
        out[name + "_out"], out[name + "_in"] = np.mean(np.abs(v) >= 1), np.mean(np.abs(v) < 1)
    return {k: float(v) for k, v in out.items()}


def backward_steps(p, pre, c, c0, d_out, d_hn, d_cn, e_pre=None, e_c=None):
    """(dA, d_h0, d_c0, d_b) in float64 for direction 0's order of time; with ``e_pre`` / ``e_c`` also the four bounds, on the
    2-norms of the rows: dA [T, N], d_h0 [N], d_c0 [N], d_b (one number)."""
    pre, c, d_out = _f64(pre), _f64(c), _f64(d_out)
    T, N, H = c.shape
    w_hh = _f64(p["w_hh"])
    aw = np.abs(w_hh)
    want_b = e_pre is not None
    dA = np.zeros((T, N, 4 * H))
    d_b = np.zeros(4 * H)
    dc_in = np.zeros((N, H))
    fr = dict(dh=np.zeros((T, N, H)), dc=np.zeros((T, N, H)), G=np.zeros((T, N, 4 * H)), cin=np.zeros((T, N, H)))   # fresh errors
    co = dict(k=np.zeros((T, 4, N, H)), f=np.zeros((T, N, H)), os=np.zeros((T, N, H)))      # the factors errors are carried through
    c0v = np.zeros((N, H)) if c0 is None else _f64(c0)
    zero = np.zeros((N, H))
    dhn = zero if d_hn is None else _f64(d_hn)
    dcn = zero if d_cn is None else _f64(d_cn)
    for t in range(T - 1, -1, -1):
        last = t == T - 1
        rec = zero if last else dA[t + 1] @ w_hh
        e_rec = 0.0 if (last or not want_b) else (4 * H + 4) * U24 * (np.abs(dA[t + 1]) @ aw)
        inj = dhn if last else zero
        dh = rec + d_out[t] + inj
        zi, zf, ag, zo = pre[t, :, :H], pre[t, :, H:2 * H], pre[t, :, 2 * H:3 * H], pre[t, :, 3 * H:]
        i, f, g, o, tc = clip01(zi), clip01(zf), clip11(ag), clip01(zo), clip11(c[t])
        pi, pf, po, qg, qc = P(zi), P(zf), P(zo), Q(ag), Q(c[t])
        cprev = c[t - 1] if t > 0 else c0v
        term = dh * o * qc
        dcs = dcn if last else dc_in
        dc = dcs + term
        row = np.concatenate([0.2 * dc * g * pi, 0.2 * dc * cprev * pf, dc * i * qg, 0.2 * dh * tc * po], 1)
        dA[t] = row
        d_b = d_b + row.sum(0)
        if want_b:
            ei, ef, eo = pi * e_pre[t, :, :H], pf * e_pre[t, :, H:2 * H], po * e_pre[t, :, 3 * H:]
            eg = qg * e_pre[t, :, 2 * H:3 * H]
            e_tc = qc * e_c[t]
            e_cprev = e_c[t - 1] if t > 0 else zero
            fifth, e5 = np.full((N, H), 0.2), np.full((N, H), C02_ERR)
            fr["dh"][t] = e_rec + 2 * U24 * (np.abs(d_out[t]) + np.abs(rec) + np.abs(inj))
            fr["dc"][t] = qc * L._prod_err([dh, o], [zero, eo]) + 2 * U24 * (np.abs(dcs) + np.abs(term))
            fr["G"][t] = np.concatenate([pi * L._prod_err([dc, g, fifth], [zero, eg, e5]),
                                         pf * L._prod_err([dc, cprev, fifth], [zero, e_cprev, e5]),
                                         qg * L._prod_err([dc, i], [zero, ei]),
                                         po * L._prod_err([dh, tc, fifth], [zero, e_tc, e5])], 1)
            fr["cin"][t] = L._prod_err([dc, f], [zero, ef])
            co["k"][t] = np.stack([0.2 * g * pi, 0.2 * cprev * pf, i * qg, 0.2 * tc * po])
            co["f"][t], co["os"][t] = f, o * qc
        dc_in = dc * f
    d_h0 = dA[0] @ w_hh
    out = (dA, d_h0, dc_in, d_b)
    if not want_b:
        return out
    sigma = float(np.linalg.norm(w_hh, 2))
    wt = [w_hh[k * H:(k + 1) * H].T for k in range(4)]          # the four [H, H] blocks, transposed: they act on columns
    E_dA, E_c0 = np.zeros((T, N)), np.zeros(N)
    eye = np.eye(2 * H)
    for n in range(N):
        phis, rn = [], []
        for t in range(T - 1, -1, -1):
            if t == T - 1:                                     # nothing is carried into the last step
                r_dh, r_dc = fr["dh"][t, n], fr["dc"][t, n]
            else:
                ki, kf, kg, ko = co["k"][t + 1][:, n]
                os_t, f_next = co["os"][t][n], co["f"][t + 1][n]
                p_hh = wt[3] * ko[None, :]
                p_hc = wt[0] * ki[None, :] + wt[1] * kf[None, :] + wt[2] * kg[None, :]
                m = np.block([[p_hh, p_hc], [os_t[:, None] * p_hh, np.diag(f_next) + os_t[:, None] * p_hc]])
                phis = [m @ ph for ph in phis]
                r_dh = fr["G"][t + 1, n] @ aw + fr["dh"][t, n]
                r_dc = fr["cin"][t + 1, n] + np.abs(os_t) * r_dh + fr["dc"][t, n]
            phis.append(eye)
            rn.append(float(np.sqrt((r_dh ** 2).sum() + (r_dc ** 2).sum())))
            s_norm = sum(float(np.linalg.norm(ph, 2)) * r for ph, r in zip(phis, rn))
            ki, kf, kg, ko = co["k"][t][:, n]
            d_max = float(max(np.max(np.sqrt(ki * ki + kf * kf + kg * kg)), np.max(np.abs(ko))))
            E_dA[t, n] = d_max * s_norm + L._norm(fr["G"][t, n])
            if t == 0:
                E_c0[n] = float(np.max(np.abs(co["f"][0][n]))) * s_norm + L._norm(fr["cin"][0, n])
    E_h0 = sigma * E_dA[0] + L._norm((4 * H + 4) * U24 * (np.abs(dA[0]) @ aw))
    E_b = E_dA.sum() + float(np.linalg.norm((T * N + 8) * U24 * np.abs(dA).sum((0, 1))))
    return out, tuple(b * SECOND_ORDER for b in (E_dA, E_h0, E_c0, E_b))


def batch_products(p, dA, x, h, h0):
    """(dx, d_w_ih, d_w_hh) in float64 of one direction in its own order of time."""
    return L.batch_products(p, dA, x, h, h0, None)


# ---- directions ---------------------------------------------------------------------------------------------------------------

def back(a, d):
    """A per-step tensor of direction d's own run, in the layer's order of time (the flip is its own inverse)."""
    return a if (a is None or d == 0) else np.ascontiguousarray(a[::-1])


def dir_view(k, d):
    """Direction d of a case as a forward-in-time case: d = 1 has x and d_out flipped in time."""
    H = k["H"]
    pick = lambda a: None if a is None else a[d]      # noqa: E731
    d_out = None if k.get("d_out") is None else np.ascontiguousarray(k["d_out"][..., d * H:(d + 1) * H])
    return dict(p=k["p"][d], T=k["T"], N=k["N"], H=H, In=k["In"], x=back(k["x"], d), h0=pick(k["h0"]), c0=pick(k["c0"]),
                d_out=back(d_out, d), d_hn=pick(k.get("d_hn")), d_cn=pick(k.get("d_cn")))


def layer_forward(k):
    """out [T, N, ndir H], h_n, c_n [ndir, N, H] in float64."""
    outs, hns, cns = [], [], []
    for d in range(k["ndir"]):
        u = dir_view(k, d)
        o, hn, cn = forward(u["p"], u["x"], u["h0"], u["c0"])
        outs.append(back(o, d))
        hns.append(hn)
        cns.append(cn)
    return np.concatenate(outs, 2), np.stack(hns), np.stack(cns)


def layer_backward(k):
    """The whole layer in float64: out [T, N, ndir H], h_n / c_n [ndir, N, H] and every gradient (dx summed over the directions,
    the others direction major)."""
    parts = []
    for d in range(k["ndir"]):
        u = dir_view(k, d)
        out, hn, cn = forward(u["p"], u["x"], u["h0"], u["c0"])
        pre, c, _ = recompute(u["p"], u["x"], out, u["h0"], u["c0"])
        dA, d_h0, d_c0, d_b = backward_steps(u["p"], pre, c, u["c0"], u["d_out"], u["d_hn"], u["d_cn"])
        dx, d_w_ih, d_w_hh = batch_products(u["p"], dA, u["x"], out, u["h0"])
        parts.append(dict(out=back(out, d), h_n=hn, c_n=cn, dx=back(dx, d), d_w_ih=d_w_ih, d_w_hh=d_w_hh, d_b=d_b, d_h0=d_h0,
                          d_c0=d_c0))
    res = dict(out=np.concatenate([q["out"] for q in parts], 2), dx=sum(q["dx"] for q in parts))
    for key in ("h_n", "c_n", "d_h0", "d_c0", "d_w_ih", "d_w_hh", "d_b"):
        res[key] = np.stack([q[key] for q in parts])
    return res


def reference(k, h=None):
    """Per direction, in the LAYER's order of time, from the outputs ``h`` [T, N, ndir H] (None: the float64 forward rounded to
    float32; on the GPU the device's own): h32, the float64 pre, c, dA, d_h0, d_c0, d_b on it, their bounds, the kink margin
    and the largest bound on a recomputed value a kink is tested on (``e_kink``).  dict of ndir-lists."""
    H = k["H"]
    if h is None:
        h = layer_forward(k)[0].astype(np.float32)
    out = {}
    for d in range(k["ndir"]):
        u = dir_view(k, d)
        h32 = back(np.ascontiguousarray(np.asarray(h)[..., d * H:(d + 1) * H]), d)
        pre, c, mag = recompute(u["p"], u["x"], h32, u["h0"], u["c0"])
        e_pre, e_c = recompute_bounds(u["p"], pre, c, u["c0"], mag)
        (dA, d_h0, d_c0, d_b), (e_dA, e_h0, e_c0, e_b) = backward_steps(u["p"], pre, c, u["c0"], u["d_out"], u["d_hn"], u["d_cn"],
                                                                         e_pre=e_pre, e_c=e_c)
        r = dict(h32=back(h32, d), pre=back(pre, d), c=back(c, d), e_pre=back(e_pre, d), e_c=back(e_c, d), dA=back(dA, d),
                 e_dA=back(e_dA, d), d_h0=d_h0, d_c0=d_c0, d_b=d_b, e_h0=e_h0, e_c0=e_c0, e_b=e_b, margin=margin(pre, c),
                 e_kink=float(max(e_pre.max(), e_c.max())), regions=regions(pre, c))
        for key, v in r.items():
            out.setdefault(key, []).append(v)
    return out


def ratios(r, d, pre, c, dA, d_h0, d_c0, d_b):
    """name -> the worst ratio to the bound of a device's outputs for direction d of ``reference``'s ``r``."""
    return dict(gates=L.worst_ratio(pre, r["pre"][d], r["e_pre"][d]), c=L.worst_ratio(c, r["c"][d], r["e_c"][d]),
                dA=L.norm_ratio(dA, r["dA"][d], r["e_dA"][d]), d_h0=L.norm_ratio(d_h0, r["d_h0"][d], r["e_h0"][d]),
                d_c0=L.norm_ratio(d_c0, r["d_c0"][d], r["e_c0"][d]), d_b=L.norm_ratio(d_b, r["d_b"][d], r["e_b"][d]))


# ---- cases --------------------------------------------------------------------------------------------------------------------

# name: (T, N, In, H, ndir), bias, state (h0 / c0 given), d_hn, d_cn, weight scale (None: ``_profiled``), seed.  Each shape is the smallest that crosses
# one edge of the kernels (32 batch rows per pass, 32 hidden units per workgroup).  Default init (+-1/sqrt(H)) never leaves the
# clamps' interiors, so the weights are drawn from +-scale/sqrt(H): every saturated region then holds >= 5 % of its elements and
# every interior >= 20 % (cases with T >= 3).  The seeds were chosen on the CPU, by tests/test_hard_lstm_backward_cpu.py's
# conditions alone: the float64 kink margin is >= 16 x the case's largest derived bound on a recomputed value.
_CASES = (
    ("smallest", (1, 1, 1, 1, 1), True, False, False, False, 5.0, 1),
    ("t3_n2_h8_states", (3, 2, 5, 8, 1), True, True, True, True, 5.0, 0),
    ("t3_n2_h8_plain", (3, 2, 5, 8, 1), False, False, False, False, 5.0, 4),
    ("t3_n2_h8_bidir", (3, 2, 5, 8, 2), True, True, True, True, 5.0, 7),
    ("t4_n33_h40_bidir", (4, 33, 7, 40, 2), True, True, True, True, None, 0),
    ("t2_n65_h32", (2, 65, 3, 32, 1), True, True, True, True, 4.5, 12941),
    ("t6_n3_h33_bidir", (6, 3, 4, 33, 2), True, True, True, False, 5.0, 4715),
)
CASE_NAMES = tuple(c[0] for c in _CASES)
# The g block's rows are drawn at a third of the scale: hard tanh saturates at |a| = 1 where the hard sigmoid does at |a| = 2.5,
# and a cell with f = 0, i = 1 and |g| = 1 all saturated has c = +-1 EXACTLY -- margin 0 -- so the three regions are kept near the
# 5 % the conditions ask for, and the seeds are those at which no element does that.
G_ROWS = 1.0 / 3.0


def _profiled(rng, T, N, In, H, ndir):
    """The parameters and states of a case too large for a seed to keep its distance from every kink (4 x 33 x 160 x 2
    pre-activations within reach of 2 kinks each: over 120 000 seeds of the scaled draw, none came near 16 bounds).  The biases
    carry a PROFILE per unit and the weights are small (|w_ih x| <= 0.35, |w_hh h| <= 0.8, typically 0.05), so a unit stays in
    the regime its bias puts it in:
      one unit in ten   i, f high, g = +1, c0 in [0.2, 0.8]:     c climbs by 1 a step, beyond +1 and never near it
      one in ten        the same with g = -1, c0 in [-0.8, -0.2]
      one in ten        i, f low:                                   c = 0
      the rest          i, f, g inside (c stays inside), and of these one in ten has o low and one in ten o high.
    Everything else -- x, the weights, the biases inside a regime, h0, c0 inside its range, the gradients -- is drawn."""
    f32 = lambda a: a.astype(np.float32)       # noqa: E731
    kind = np.arange(H) % 10                    # 0: climbs, 1: falls, 2: closed, 3: o low, 4: o high, others: inside
    ps, c0s = [], []
    for _ in range(ndir):
        kind = rng.permutation(kind)
        b = np.zeros((4, H))
        sat = rng.uniform(4.0, 5.0, (4, H))
        b[0] = np.where(kind <= 1, sat[0], np.where(kind == 2, -sat[0], rng.uniform(-1, 1, H)))
        b[1] = np.where(kind <= 1, sat[1], np.where(kind == 2, -sat[1], rng.uniform(-1, 1, H)))
        b[2] = np.where(kind == 0, 2.2, np.where(kind == 1, -2.2, rng.uniform(-0.3, 0.3, H)))
        b[3] = np.where(kind == 3, -sat[3], np.where(kind == 4, sat[3], rng.uniform(-1, 1, H)))
        split = rng.uniform(0.2, 0.8, 4 * H)       # the bias, dealt to b_ih and b_hh
        ps.append(dict(w_ih=f32(rng.uniform(-0.05, 0.05, (4 * H, In))), w_hh=f32(rng.uniform(-0.02, 0.02, (4 * H, H))),
                       b_ih=f32(b.reshape(-1) * split), b_hh=f32(b.reshape(-1) * (1 - split))))
        c0 = rng.uniform(-0.3, 0.3, (N, H))
        c0 = np.where(kind == 0, rng.uniform(0.2, 0.8, (N, H)), np.where(kind == 1, rng.uniform(-0.8, -0.2, (N, H)), c0))
        c0s.append(c0)
    return tuple(ps), f32(rng.uniform(-1, 1, (T, N, In))), f32(np.stack(c0s))


def make_case(name, shape, bias, state, dhn, dcn, scale, seed):
    T, N, In, H, ndir = shape
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)       # noqa: E731
    if scale is None:
        assert bias and state
        p, x, c0 = _profiled(rng, T, N, In, H, ndir)
    else:
        s = scale / np.sqrt(H)
        rows = np.repeat([s, s, s * G_ROWS, s], H)      # per row of the 4H: the g block's own scale
        p = tuple(dict(w_ih=f32(rng.uniform(-1, 1, (4 * H, In)) * rows[:, None]), w_hh=f32(rng.uniform(-1, 1, (4 * H, H)) * rows[:, None]),
                       b_ih=f32(rng.uniform(-1, 1, 4 * H) * rows) if bias else None,
                       b_hh=f32(rng.uniform(-1, 1, 4 * H) * rows) if bias else None)
                  for _ in range(ndir))
        x = f32(rng.standard_normal((T, N, In)))
    h0 = f32(rng.uniform(-1, 1, (ndir, N, H))) if state else None
    if scale is not None:
        c0 = f32(rng.uniform(-2, 2, (ndir, N, H))) if state else None
    return dict(name=name, p=p, T=T, N=N, In=In, H=H, ndir=ndir, x=x, h0=h0, c0=c0,
                d_out=f32(rng.standard_normal((T, N, ndir * H))),
                d_hn=f32(rng.standard_normal((ndir, N, H))) if dhn else None,
                d_cn=f32(rng.standard_normal((ndir, N, H))) if dcn else None)


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = {c[0]: make_case(*c) for c in _CASES}
    return _cases


_refs = {}


def case_reference(name):
    """``reference`` of a case on its float64 forward, computed once and never edited."""
    if name not in _refs:
        _refs[name] = reference(cases()[name])
    return _refs[name]


# ---- torch ---------------------------------------------------------------------------------------------------------------------

def torch_cell_stack(layers, x, h0, c0, dtype):
    """The hard stack under torch autograd, in ``dtype``: tests/rnn_ref64.py's hard cell (0.2 a + 0.5 as a multiply and an add)
    with ``torch.clamp`` for the hard sigmoid and ``torch.nn.Hardtanh`` for the hard tanh, as the reference model has them.
    layers: per layer a list over the directions of (w_ih, w_hh, b_ih | None, b_hh | None) tensors; x [T, N, In]; h0 / c0
    [num_layers * ndir, N, H] tensors or None -> (out, h_n, c_n)."""
    import torch
    hardtanh = torch.nn.Hardtanh()
    T, N = x.shape[0], x.shape[1]
    hns, cns = [], []
    cur = x
    for li, dirs in enumerate(layers):
        outs = []
        for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(dirs):
            H = w_hh.shape[1]
            s = li * len(dirs) + d
            h = torch.zeros((N, H), dtype=dtype) if h0 is None else h0[s]
            c = torch.zeros((N, H), dtype=dtype) if c0 is None else c0[s]
            steps = [None] * T
            for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
                a = cur[t] @ w_ih.t() + h @ w_hh.t()
                if b_ih is not None:
                    a = a + b_ih
                if b_hh is not None:
                    a = a + b_hh
                ai, af, ag, ao = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
                i, f, o = (torch.clamp(0.2 * v + 0.5, 0.0, 1.0) for v in (ai, af, ao))
                c = f * c + i * hardtanh(ag)
                h = o * hardtanh(c)
                steps[t] = h
            outs.append(torch.stack(steps))
            hns.append(h)
            cns.append(c)
        cur = torch.cat(outs, 2)
    return cur, torch.stack(hns), torch.stack(cns)


def torch_layer(k, dtype=np.float64):
    """One layer of case ``k`` under torch autograd on the CPU, with ``layer_backward``'s keys."""
    import torch
    td = torch.float64 if dtype == np.float64 else torch.float32
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a).astype(dtype))      # noqa: E731
    params = [[None if k["p"][d][key] is None else t(k["p"][d][key]).requires_grad_(True) for key in ("w_ih", "w_hh", "b_ih", "b_hh")]
              for d in range(k["ndir"])]
    x = t(k["x"]).requires_grad_(True)
    zeros = np.zeros((k["ndir"], k["N"], k["H"]), dtype=dtype)
    h0 = t(zeros if k["h0"] is None else k["h0"]).clone().requires_grad_(True)
    c0 = t(zeros if k["c0"] is None else k["c0"]).clone().requires_grad_(True)
    out, hn, cn = torch_cell_stack([params], x, h0, c0, td)
    total = (out * t(k["d_out"])).sum()
    if k["d_hn"] is not None:
        total = total + (hn * t(k["d_hn"])).sum()
    if k["d_cn"] is not None:
        total = total + (cn * t(k["d_cn"])).sum()
    total.backward()
    got = dict(out=out, h_n=hn, c_n=cn, dx=x.grad, d_h0=h0.grad, d_c0=c0.grad,
               d_w_ih=torch.stack([q[0].grad for q in params]), d_w_hh=torch.stack([q[1].grad for q in params]))
    if params[0][2] is not None:
        got["d_b"] = torch.stack([q[2].grad for q in params])
    return {name: v.detach().numpy() for name, v in got.items()}


# ---- the kink table -----------------------------------------------------------------------------------------------------------

def _nbrs(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def kink_table():
    """One T = 1, N = 1 step whose H units are the rows of the table: (a_i, a_f, a_g, a_o, c0) float32, each row putting ONE
    quantity on a kink or a float32 neighbour of it and keeping every product of the forward exact (a factor that is 0, 0.5 or
    1), so that float32 torch and the device see the same c.  Rows:
      a_i in {-2.5, 2.5} and neighbours   (c0 = 0, g = 0.5: c = 0.5 i)
      a_f alike                            (c0 = 0.5, g = 0: c = 0.5 f)
      a_o alike                            (c0 = 0, i = 1, g = 0.5: c = 0.5)
      a_g in {-1, 1} and neighbours        (c0 = 0, z_i = 0.5: c = 0.5 g)
      c   in {-1, 1} and neighbours        (f = 1, i = 0: c = c0)
    -> dict(a [4H] in gate-major order, c0 [H], names)."""
    rows, names = [], []
    for v0 in (-2.5, 2.5):
        for v in _nbrs(v0):
            rows.append((v, 0.0, 0.5, 1.25, 0.0))
            names.append(f"a_i={v!r}")
            rows.append((1.25, v, 0.0, 1.25, 0.5))
            names.append(f"a_f={v!r}")
            rows.append((5.0, 0.0, 0.5, v, 0.0))
            names.append(f"a_o={v!r}")
    for v0 in (-1.0, 1.0):
        for v in _nbrs(v0):
            rows.append((0.0, 0.0, v, 1.25, 0.0))
            names.append(f"a_g={v!r}")
            rows.append((-5.0, 5.0, 0.5, 1.25, v))
            names.append(f"c={v!r}")
    t = np.asarray(rows, dtype=np.float32)
    return dict(a=np.ascontiguousarray(t[:, :4].T).reshape(-1), c0=np.ascontiguousarray(t[:, 4]), names=names, H=len(rows))


def kink_expected(dtype=np.float32):
    """torch autograd (CPU, ``dtype``) on the kink table under d_out = 1 + j / 64, d_cn = 0.75: dict(dA [4H], d_c0 [H], c [H])."""
    import torch
    kt = kink_table()
    H = kt["H"]
    td = torch.float32 if dtype == np.float32 else torch.float64
    a = torch.from_numpy(kt["a"].astype(dtype)).requires_grad_(True)
    c0 = torch.from_numpy(kt["c0"].astype(dtype)).requires_grad_(True)
    hardtanh = torch.nn.Hardtanh()
    i, f, o = (torch.clamp(0.2 * a[s * H:(s + 1) * H] + 0.5, 0.0, 1.0) for s in (0, 1, 3))
    c = f * c0 + i * hardtanh(a[2 * H:3 * H])
    h = o * hardtanh(c)
    d_out, d_cn = kink_d_out(H).astype(dtype), np.full(H, 0.75, dtype=dtype)
    ((h * torch.from_numpy(d_out)).sum() + (c * torch.from_numpy(d_cn)).sum()).backward()
    assert a.dtype == td
    return dict(dA=a.grad.numpy(), d_c0=c0.grad.numpy(), c=c.detach().numpy())


def kink_d_out(H):
    return (1.0 + np.arange(H) / 64.0).astype(np.float32)


def kink_emulate(fused=False):
    """The specification on the kink table in float32 numpy, every operation rounded on its own in the device's order:
    dict(dA [4H], d_c0 [H], c [H]).  ``fused``: z formed as ONE rounding of 0.2f a + 0.5f (a fused multiply-add) -- what the
    specification forbids; it puts a = -2.5 outside the clamp."""
    f = np.float32
    kt = kink_table()
    H = kt["H"]
    a, c0 = kt["a"].reshape(4, H), kt["c0"]

    def z_of(v):
        if fused:
            return (np.float64(f(0.2)) * v.astype(np.float64) + 0.5).astype(f)
        m = f(0.2) * v
        return m + f(0.5)
    zi, zf, ag, zo = z_of(a[0]), z_of(a[1]), a[2], z_of(a[3])
    i, fg, g, o = clip01(zi).astype(f), clip01(zf).astype(f), clip11(ag).astype(f), clip01(zo).astype(f)
    c = fg * c0 + i * g                  # (every product is exact by construction, so the order of roundings is immaterial)
    tc = clip11(c).astype(f)
    dh, zero = kink_d_out(H), f(0)
    dc = f(0.75) + np.where(Q(c) > 0, dh * o, zero)
    dA = np.concatenate([np.where(P(zi) > 0, (dc * g) * f(0.2), zero), np.where(P(zf) > 0, (dc * c0) * f(0.2), zero),
                         np.where(Q(ag) > 0, dc * i, zero), np.where(P(zo) > 0, (dh * tc) * f(0.2), zero)])
    assert dA.dtype == f and c.dtype == f
    return dict(dA=dA, d_c0=dc * fg, c=c)


# ---- stacks (tests/test_hard_lstm_train_gpu.py) -------------------------------------------------------------------------------

def scaled_stack(In, H, num_layers, bidirectional, scale, seed):
    """Weights of a ``HardLSTM`` stack under its state_dict keys (``layers.{k}[.fwd|.bwd].cell.*``), drawn as the cases' are: the
    rows at +-scale / sqrt(H), the g block at ``G_ROWS`` of that."""
    rng = np.random.default_rng(seed)
    s = scale / np.sqrt(H)
    rows = np.repeat([s, s, s * G_ROWS, s], H)
    ndir = 2 if bidirectional else 1
    w = {}
    for layer in range(num_layers):
        fin = In if layer == 0 else ndir * H
        for sub in (("fwd.", "bwd.") if bidirectional else ("",)):
            pre = f"layers.{layer}.{sub}cell."
            w[pre + "weight_ih"] = (rng.uniform(-1, 1, (4 * H, fin)) * rows[:, None]).astype(np.float32)
            w[pre + "weight_hh"] = (rng.uniform(-1, 1, (4 * H, H)) * rows[:, None]).astype(np.float32)
            w[pre + "bias_ih"] = (rng.uniform(-1, 1, 4 * H) * rows).astype(np.float32)
            w[pre + "bias_hh"] = (rng.uniform(-1, 1, 4 * H) * rows).astype(np.float32)
    return w


def stack_layers(w, num_layers, bidirectional, conv=lambda a: a):
    """``scaled_stack``'s dict -> per layer a list over the directions of (w_ih, w_hh, b_ih, b_hh), each through ``conv``."""
    out = []
    for layer in range(num_layers):
        out.append([tuple(conv(w[f"layers.{layer}.{sub}cell.{n}"]) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                    for sub in (("fwd.", "bwd.") if bidirectional else ("",))])
    return out


def stack_margin_ratio(layers, x, h0=None, c0=None):
    """The least, over the layers and directions of a stack in float64, of (kink margin) / (largest derived bound on a recomputed
    value): the condition of ``test_case_conditions`` per layer.  layers as ``stack_layers`` gives them (numpy); x [T, N, In];
    h0 / c0 [num_layers * ndir, N, H] or None."""
    cur, worst = _f64(x), np.inf
    for li, dirs in enumerate(layers):
        ndir = len(dirs)
        k = dict(T=cur.shape[0], N=cur.shape[1], In=cur.shape[2], H=dirs[0][1].shape[1], ndir=ndir, x=cur,
                 p=tuple(dict(w_ih=q[0], w_hh=q[1], b_ih=q[2], b_hh=q[3]) for q in dirs),
                 h0=None if h0 is None else _f64(h0)[li * ndir:(li + 1) * ndir],
                 c0=None if c0 is None else _f64(c0)[li * ndir:(li + 1) * ndir])
        out = layer_forward(k)[0]
        for d in range(ndir):
            u = dir_view(k, d)
            pre, c, mag = recompute(u["p"], u["x"], back(np.ascontiguousarray(out[..., d * k["H"]:(d + 1) * k["H"]]), d), u["h0"], u["c0"])
            e_pre, e_c = recompute_bounds(u["p"], pre, c, u["c0"], mag)
            worst = min(worst, margin(pre, c) / max(e_pre.max(), e_c.max()))
        cur = out
    return float(worst)
