"""numpy side of the LSTM backward (``ms_lstm_recompute`` / ``ms_lstm_backward_steps``; TEST INFRASTRUCTURE ONLY).  OWN
specification: the comment on ``ms_lstm_recompute`` in include/ms_hotpath.h.  One layer of a unidirectional
``torch.nn.LSTM``: gate order i, f, g, o, ``c_t = f c_{t-1} + i g``, ``h_t = o tanh(c_t)``; ``lens`` sorted descending or
None; rows ``t >= lens[n]`` of the output are 0 and carry no gradient, ``h_n`` / ``c_n`` is the state at ``lens[n] - 1``.

``forward(p, x, h0, c0, lens)``               float64 layer forward: out [T,N,H], h_n, c_n.
``recompute(p, x, h, h0, c0, lens)``          float64 gates [T,N,4H] (activated) and c [T,N,H] from a GIVEN output h.
``backward_steps(p, gates, c, c0, d_out, d_hn, d_cn, lens)``   float64 dG, d_h0, d_c0, d_b.
``batch_products(p, dG, x, h, h0, lens)``     float64 dx, d_w_ih, d_w_hh.
``emulate_*``                                 the same two device calls in float32, in the device's order of operations.
``recompute_bounds`` / ``backward_bounds``    per-element absolute error bounds for the device, derived below.
``cases()``                                   the shapes and options the tests run.

The bounds, derived (not fitted).  u = 2^-24.  Everything is first-order forward-error propagation, evaluated on the
float64 values, each tensor's bound feeding the next one; the sum is scaled by 1 + 2^-10 for the second-order terms (every
relative error below is under 2^-12 at these sizes).  A float32 sum of K terms in ANY order (the MFMA's chain, the waves'
partial tiles) is off by at most K u times the sum of the terms' magnitudes; a product of m factors by the factors' own
errors times the other factors, plus m u of the product.

Recompute.  The inputs are the device's own float32 values, so they carry no error.
  a     = x w_ih^T + b_ih + h_prev w_hh^T + b_hh:   e_a = (In + H + 4) u (|x| |w_ih|^T + |b_ih| + |h_prev| |w_hh|^T + |b_hh|)
  s     = 1 / (1 + expf(-a))  (expf 1 ulp, the sum, the division; the error of the exponential weighs e / (1 + e) < 1):
          e_s = s (1 - s) e_a + 6 u s
  g     = tanhf(a) (2 ulp):   e_g = (1 - g^2) e_a + 4 u |g|
  c_t   = f c_{t-1} + i g:    e_c = |f| e_c(t-1) + |c_{t-1}| e_f + |i| e_g + |g| e_i + 2 u (|f c_{t-1}| + |i g|)
The last line is the recurrence: T steps of it, the forget gate damping what it carries.

Backward steps, from gates and c that are off by e_gate and e_c (the bounds above when the device's recompute feeds it).
An error carried from step t + 1 to step t goes through the product with w_hh.  Element by element with |w_hh| it would
grow by sum_k |w_hh[k, j]| ~ 0.5 sqrt(H) x 4 per step, and in a norm by w_hh's largest singular value per step: neither is a
statement about a recurrence that is stable.  The carried part is therefore propagated with the recurrence's OWN Jacobian.
Per sequence n the carried error is s_t = (e_dh_t, e_dc_t), 2H numbers, and to first order
  s_t = M_t s_{t+1} + r_t
  e_dh_t = w_hh^T [k_i e_dc, k_f e_dc, k_g e_dc, k_o e_dh]_{t+1} + ...        k_i = g i (1 - i), k_f = c_{t-1} f (1 - f),
  e_dc_t = f_{t+1} e_dc_{t+1} + o_t (1 - tc_t^2) e_dh_t + ...                 k_g = i (1 - g^2), k_o = tc o (1 - o)
with M_t built from the float64 gates and r_t the FRESH roundings of the step, bounded per element:
  rec   = dG_{t+1} w_hh:      (4H + 4) u |dG_{t+1}| |w_hh| + (the fresh error of dG_{t+1}) |w_hh|
  dh    = d_out + rec + d_hn: + 2 u (|d_out| + |rec| + |d_hn|)
  tc    = tanhf(c):           e_tc = (1 - tc^2) e_c + 4 u |tc|;      1 - v^2 (v = tc or g): 2 |v| e_v + 2 u
  dc    = dc_in + dh o (1 - tc^2):   the product rule on o and 1 - tc^2 + 3 u of the term + 2 u (|dc_in| + |term|)
  dc_in = f dc for step t - 1:       the product rule on f + 2 u of it
  dG    : four blocks, each dc (or dh) times gate factors (1 - s carries e_s + u): the product rule on the gate factors + 4 u
so that  |s_t|_2 <= sum_{t' >= t} |M_t M_{t+1} .. M_{t'-1}|_2 |r_t'|_2  (2-norms, the products formed explicitly: T steps of the
recurrence without compounding a per-step worst case), nothing being carried into a sequence's last step, and
  E_dG(t, n) = max_j max(sqrt(k_i^2 + k_f^2 + k_g^2), |k_o|) |s_t|_2 + |fresh error of dG_t|_2
  d_h0  = rec at t = -1: sigma E_dG(0) + fresh, sigma = w_hh's largest singular value;   d_c0: max |f_0| |s_0|_2 + fresh
  d_b   = sum over the existing rows of dG:  |e|_2 <= sum E_dG + |(rows + 8) u sum |dG||_2
So dG is held per (t, n) row, d_h0 and d_c0 per n, d_b as a whole, all in the 2-norm.
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
    b_ih = np.zeros(4 * H) if p.get("b_ih") is None else _f64(p["b_ih"])
    b_hh = np.zeros(4 * H) if p.get("b_hh") is None else _f64(p["b_hh"])
    return b_ih, b_hh


def forward(p, x, h0, c0, lens):
    x = _f64(x)
    T, N, _ = x.shape
    w_ih, w_hh = _f64(p["w_ih"]), _f64(p["w_hh"])
    H = w_hh.shape[1]
    b_ih, b_hh = _bias(p, H)
    L = _lens(lens, T, N)
    h = np.zeros((N, H)) if h0 is None else _f64(h0).copy()
    c = np.zeros((N, H)) if c0 is None else _f64(c0).copy()
    out = np.zeros((T, N, H))
    for t in range(T):
        a = x[t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh
        i, f, g, o = _sig(a[:, :H]), _sig(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), _sig(a[:, 3 * H:])
        cn = f * c + i * g
        hn = o * np.tanh(cn)
        live = (t < L)[:, None]
        c = np.where(live, cn, c)
        h = np.where(live, hn, h)
        out[t] = np.where(live, hn, 0.0)
    return out, h, c


def h_prev_of(h, h0, lens):
    """h shifted one step: h0 in row 0, zero past the length."""
    h = _f64(h)
    T, N, H = h.shape
    L = _lens(lens, T, N)
    hp = np.zeros_like(h)
    hp[0] = 0.0 if h0 is None else _f64(h0)
    hp[1:] = h[:-1]
    return np.where((np.arange(T)[:, None] < L[None, :])[..., None], hp, 0.0)


def recompute(p, x, h, h0, c0, lens, dtype=np.float64):
    """gates [T,N,4H], c [T,N,H] (rows past a length: 0 here, unspecified on the device), and the magnitude sums the bounds
    need.  ``dtype=np.float32``: every operation rounded to float32 (the emulation)."""
    f = dtype
    x = np.asarray(x, dtype=f)
    T, N, In = x.shape
    w_ih, w_hh = np.asarray(p["w_ih"], dtype=f), np.asarray(p["w_hh"], dtype=f)
    H = w_hh.shape[1]
    b_ih, b_hh = (b.astype(f) for b in _bias(p, H))
    L = _lens(lens, T, N)
    hp = h_prev_of(h, h0, lens).astype(f)
    p1 = ((x.reshape(T * N, In) @ w_ih.T).astype(f) + b_ih).astype(f)
    p2 = ((hp.reshape(T * N, H) @ w_hh.T).astype(f) + b_hh).astype(f)
    a = (p1 + p2).astype(f).reshape(T, N, 4 * H)
    mag = (np.abs(x.astype(np.float64)).reshape(T * N, In) @ np.abs(w_ih.astype(np.float64)).T + np.abs(b_ih)
           + np.abs(hp.astype(np.float64)).reshape(T * N, H) @ np.abs(w_hh.astype(np.float64)).T + np.abs(b_hh)).reshape(T, N, 4 * H)
    gates = np.zeros((T, N, 4 * H), dtype=f)
    c = np.zeros((T, N, H), dtype=f)
    cprev = np.zeros((N, H), dtype=f) if c0 is None else np.asarray(c0, dtype=f)
    one = f(1)
    for t in range(T):
        at = a[t]
        gi = (one / (one + np.exp(-at[:, :H]).astype(f))).astype(f)
        gf = (one / (one + np.exp(-at[:, H:2 * H]).astype(f))).astype(f)
        gg = np.tanh(at[:, 2 * H:3 * H]).astype(f)
        go = (one / (one + np.exp(-at[:, 3 * H:]).astype(f))).astype(f)
        cc = ((gf * cprev).astype(f) + (gi * gg).astype(f)).astype(f)
        live = (t < L)[:, None]
        gates[t] = np.where(live, np.concatenate([gi, gf, gg, go], 1), 0)
        c[t] = np.where(live, cc, 0)
        cprev = np.where(live, cc, cprev)
    return gates, c, mag


def recompute_bounds(p, gates, c, c0, mag, lens):
    """(e_gates [T,N,4H], e_c [T,N,H]) from the float64 ``recompute`` (module docstring)."""
    T, N, H4 = gates.shape
    H = H4 // 4
    In = np.asarray(p["w_ih"]).shape[1]
    L = _lens(lens, T, N)
    e_a = (In + H + 4) * U24 * mag
    e_g = np.empty_like(gates)
    for k in (0, 1, 3):
        s = gates[..., k * H:(k + 1) * H]
        e_g[..., k * H:(k + 1) * H] = s * (1 - s) * e_a[..., k * H:(k + 1) * H] + 6 * U24 * s
    g = gates[..., 2 * H:3 * H]
    e_g[..., 2 * H:3 * H] = (1 - g * g) * e_a[..., 2 * H:3 * H] + 4 * U24 * np.abs(g)
    e_c = np.zeros((T, N, H))
    e_prev = np.zeros((N, H))
    cprev = np.zeros((N, H)) if c0 is None else _f64(c0)
    for t in range(T):
        i, f, gg = gates[t, :, :H], gates[t, :, H:2 * H], gates[t, :, 2 * H:3 * H]
        ei, ef, eg = e_g[t, :, :H], e_g[t, :, H:2 * H], e_g[t, :, 2 * H:3 * H]
        e = (f * e_prev + np.abs(cprev) * ef + i * eg + np.abs(gg) * ei + 2 * U24 * (np.abs(f * cprev) + np.abs(i * gg)))
        live = (t < L)[:, None]
        e_c[t] = np.where(live, e, 0.0)
        e_prev = np.where(live, e, e_prev)
        cprev = np.where(live, c[t], cprev)
    return e_g * SECOND_ORDER, e_c * SECOND_ORDER


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


def _cmax(coef):
    return np.max(np.abs(coef), axis=-1)


def backward_steps(p, gates, c, c0, d_out, d_hn, d_cn, lens, dtype=np.float64, e_gates=None, e_c=None):
    """(dG, d_h0, d_c0, d_b) in ``dtype``; with ``e_gates`` / ``e_c`` (float64 run only) also the four bounds, on the
    2-norms of the rows: dG [T, N], d_h0 [N], d_c0 [N], d_b (one number)."""
    f = dtype
    gates, c, d_out = np.asarray(gates, dtype=f), np.asarray(c, dtype=f), np.asarray(d_out, dtype=f)
    T, N, H = c.shape
    w_hh = np.asarray(p["w_hh"], dtype=f)
    L = _lens(lens, T, N)
    want_b = e_gates is not None
    aw = np.abs(w_hh.astype(np.float64))
    dG = np.zeros((T, N, 4 * H), dtype=f)
    d_b = np.zeros(4 * H, dtype=f)
    dc_in = np.zeros((N, H), dtype=f)
    fr = dict(dh=np.zeros((T, N, H)), dc=np.zeros((T, N, H)), G=np.zeros((T, N, 4 * H)), cin=np.zeros((T, N, H)))   # fresh errors
    co = dict(k=np.zeros((T, 4, N, H)), f=np.zeros((T, N, H)), os=np.zeros((T, N, H)))      # the factors errors are carried through
    c0v = np.zeros((N, H), dtype=f) if c0 is None else np.asarray(c0, dtype=f)
    zero = np.zeros((N, H), dtype=f)
    dhn = zero if d_hn is None else np.asarray(d_hn, dtype=f)
    dcn = zero if d_cn is None else np.asarray(d_cn, dtype=f)
    one = f(1)
    max_len = int(L.max())
    for t in range(max_len - 1, -1, -1):
        live = (t < L)[:, None]
        last = (t == L - 1)[:, None]
        if t + 1 < max_len:
            rec = (dG[t + 1] @ w_hh).astype(f)
            e_rec = (4 * H + 4) * U24 * (np.abs(dG[t + 1].astype(np.float64)) @ aw) if want_b else 0.0
        else:
            rec, e_rec = zero, 0.0
        inj = np.where(last, dhn, 0).astype(f)
        dh = ((rec + d_out[t]).astype(f) + inj).astype(f)
        i, fg, g, o = gates[t, :, :H], gates[t, :, H:2 * H], gates[t, :, 2 * H:3 * H], gates[t, :, 3 * H:]
        cprev = c[t - 1] if t > 0 else c0v
        tc = np.tanh(c[t]).astype(f)
        s = (one - (tc * tc).astype(f)).astype(f)
        term = ((dh * o).astype(f) * s).astype(f)
        dcs = np.where(last, dcn, dc_in).astype(f)
        dc = (dcs + term).astype(f)
        omi, omf, omo = (one - i).astype(f), (one - fg).astype(f), (one - o).astype(f)
        omg = (one - (g * g).astype(f)).astype(f)
        dgi = (((dc * g).astype(f) * i).astype(f) * omi).astype(f)
        dgf = (((dc * cprev).astype(f) * fg).astype(f) * omf).astype(f)
        dgg = ((dc * i).astype(f) * omg).astype(f)
        dgo = (((dh * tc).astype(f) * o).astype(f) * omo).astype(f)
        row = np.where(live, np.concatenate([dgi, dgf, dgg, dgo], 1), 0).astype(f)
        dG[t] = row
        d_b = (d_b + row.sum(0, dtype=f)).astype(f)
        new_in = (dc * fg).astype(f)
        if want_b:
            ei, ef, eg, eo = (e_gates[t, :, k * H:(k + 1) * H] for k in range(4))
            e_cprev = e_c[t - 1] if t > 0 else 0.0
            zero_e = np.zeros((N, H))
            # the fresh errors of this step, per element (the carried ones follow below, once every step's factors exist)
            e_tc = (1 - tc * tc) * e_c[t] + 4 * U24 * np.abs(tc)
            e_s = 2 * np.abs(tc) * e_tc + 2 * U24
            e_omg = 2 * np.abs(g) * eg + 2 * U24
            fr["dh"][t] = e_rec + 2 * U24 * (np.abs(d_out[t]) + np.abs(rec) + np.abs(inj))
            fr["dc"][t] = _prod_err([dh, o, s], [zero_e, eo, e_s]) + 2 * U24 * (np.abs(dcs) + np.abs(term))
            fr["G"][t] = np.concatenate([_prod_err([dc, g, i, omi], [zero_e, eg, ei, ei + U24]),
                                         _prod_err([dc, cprev, fg, omf], [zero_e, e_cprev, ef, ef + U24]),
                                         _prod_err([dc, i, omg], [zero_e, ei, e_omg]),
                                         _prod_err([dh, tc, o, omo], [zero_e, e_tc, eo, eo + U24])], 1)
            fr["cin"][t] = _prod_err([dc, fg], [zero_e, ef])
            co["k"][t] = np.stack([g * i * omi, cprev * fg * omf, i * omg, tc * o * omo])
            co["f"][t], co["os"][t] = fg, o * s
        dc_in = np.where(live, new_in, dc_in).astype(f)
    d_h0 = (dG[0] @ w_hh).astype(f)
    out = (dG, d_h0, dc_in, d_b)
    if not want_b:
        return out
    w64 = w_hh.astype(np.float64)
    sigma = float(np.linalg.norm(w64, 2))
    wt = [w64[k * H:(k + 1) * H].T for k in range(4)]          # the four [H, H] blocks, transposed: they act on columns
    E_dG, E_c0 = np.zeros((T, N)), np.zeros(N)
    eye = np.eye(2 * H)
    for n in range(N):
        phis, rn = [], []
        for t in range(int(L[n]) - 1, -1, -1):
            if t == L[n] - 1:                                  # nothing is carried into a sequence's last step
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
            E_dG[t, n] = d_max * s_norm + _norm(fr["G"][t, n])
            if t == 0:
                E_c0[n] = float(np.max(np.abs(co["f"][0][n]))) * s_norm + _norm(fr["cin"][0, n])
    E_h0 = sigma * E_dG[0] + _norm((4 * H + 4) * U24 * (np.abs(dG[0]) @ aw))
    rows = int(L.sum())
    E_b = E_dG.sum() + float(np.linalg.norm((rows + 8) * U24 * np.abs(dG).sum((0, 1))))
    return out, tuple(b * SECOND_ORDER for b in (E_dG, E_h0, E_c0, E_b))


def batch_products(p, dG, x, h, h0, lens):
    """(dx, d_w_ih, d_w_hh) in float64: the three GEMMs over T N rows that finish the layer."""
    dG, x = _f64(dG), _f64(x)
    T, N, In = x.shape
    H = dG.shape[2] // 4
    g2 = dG.reshape(T * N, 4 * H)
    dx = (g2 @ _f64(p["w_ih"])).reshape(T, N, In)
    return dx, g2.T @ x.reshape(T * N, In), g2.T @ h_prev_of(h, h0, lens).reshape(T * N, H)


def layer_backward(p, x, h0, c0, lens, d_out, d_hn, d_cn):
    """The whole layer in float64: outputs and every gradient (what tests/test_lstm_backward_cpu.py pins to torch)."""
    out, hn, cn = forward(p, x, h0, c0, lens)
    gates, c, _ = recompute(p, x, out, h0, c0, lens)
    dG, d_h0, d_c0, d_b = backward_steps(p, gates, c, c0, d_out, d_hn, d_cn, lens)
    dx, d_w_ih, d_w_hh = batch_products(p, dG, x, out, h0, lens)
    return dict(out=out, h_n=hn, c_n=cn, dx=dx, d_w_ih=d_w_ih, d_w_hh=d_w_hh, d_b=d_b, d_h0=d_h0, d_c0=d_c0)


# name: T, N, H, In, bias, state (h0 / c0 given), d_hn, d_cn, lens kind.  The step kernel's tiles are 32 hidden units x 32
# batch rows; H in {7, 8, 40, 72} and N in {1, 3, 33} lie on both sides of each, every option appears in both settings.
_CASES = (
    ("t1_n1_h8", 1, 1, 8, 5, True, False, False, False, None),
    ("t2_n3_h40_equal", 2, 3, 40, 33, False, True, True, True, "equal"),
    ("t9_n33_h72_ragged", 9, 33, 72, 5, True, True, True, True, "ragged"),
    ("t9_n3_h40_ragged", 9, 3, 40, 33, True, False, True, False, "ragged"),
    ("t9_n33_h8", 9, 33, 8, 5, False, True, False, True, None),
    ("t2_n33_h72_ragged", 2, 33, 72, 33, True, False, False, False, "ragged"),
    ("t1_n3_h72_equal", 1, 3, 72, 5, True, True, True, True, "equal"),
    ("t9_n1_h40_short", 9, 1, 40, 5, True, True, True, True, "short"),
    ("t9_n33_h40_ragged", 9, 33, 40, 33, True, False, True, True, "ragged"),
    # odd H: the product's last k-octet is half empty (4H / 8 = 3.5), over two passes of batch rows
    ("t9_n33_h7_ragged", 9, 33, 7, 5, True, True, True, True, "ragged"),
)
CASE_NAMES = tuple(c[0] for c in _CASES)


def _make(name, T, N, H, In, bias, state, dhn, dcn, kind):
    rng = np.random.default_rng(sum(map(ord, name)))
    k = 2.0 / np.sqrt(H)
    f32 = lambda a: a.astype(np.float32)       # noqa: E731
    p = dict(w_ih=f32(rng.uniform(-k, k, (4 * H, In))), w_hh=f32(rng.uniform(-k, k, (4 * H, H))),
             b_ih=f32(rng.uniform(-k, k, 4 * H)) if bias else None, b_hh=f32(rng.uniform(-k, k, 4 * H)) if bias else None)
    if kind is None:
        lens = None
    elif kind == "equal":
        lens = np.full(N, T, dtype=np.int32)
    elif kind == "short":                      # all equal and below T: steps the backward never runs
        lens = np.full(N, max(1, T - 3), dtype=np.int32)
    else:                                      # ragged down to 1 (rows past a length hold values that must be ignored)
        lens = np.sort(np.concatenate([[T, 1], rng.integers(1, T + 1, size=N)])[:N].astype(np.int32))[::-1].copy()
        if N >= 2:
            lens[0], lens[-1] = T, 1
    return dict(name=name, p=p, T=T, N=N, H=H, In=In, lens=lens,
                x=f32(rng.standard_normal((T, N, In))),
                h0=f32(rng.uniform(-1, 1, (N, H))) if state else None,
                c0=f32(rng.uniform(-2, 2, (N, H))) if state else None,
                d_out=f32(rng.standard_normal((T, N, H))),
                d_hn=f32(rng.standard_normal((N, H))) if dhn else None,
                d_cn=f32(rng.standard_normal((N, H))) if dcn else None)


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = {c[0]: _make(*c) for c in _CASES}
    return _cases


def torch_layer(k, dtype=np.float64):
    """torch.nn.LSTM on the CPU with autograd on the case, in ``dtype``: outputs and gradients under the case's d_out, d_hn,
    d_cn (``pack_padded_sequence`` for ragged lengths).  float64: what the restatement is pinned to; float32: the error a
    float32 backward is expected to make, which the device's error is printed as a multiple of."""
    import torch
    p, T, N, H, In = k["p"], k["T"], k["N"], k["H"], k["In"]
    bias = p["b_ih"] is not None
    m = torch.nn.LSTM(In, H, num_layers=1, bias=bias).to(torch.float64 if dtype == np.float64 else torch.float32)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.from_numpy(p["w_ih"].astype(dtype)))
        m.weight_hh_l0.copy_(torch.from_numpy(p["w_hh"].astype(dtype)))
        if bias:
            m.bias_ih_l0.copy_(torch.from_numpy(p["b_ih"].astype(dtype)))
            m.bias_hh_l0.copy_(torch.from_numpy(p["b_hh"].astype(dtype)))
    x = torch.from_numpy(k["x"].astype(dtype)).requires_grad_(True)
    zeros = np.zeros((N, H), dtype=dtype)
    h0 = torch.from_numpy((zeros if k["h0"] is None else k["h0"]).astype(dtype))[None].clone().requires_grad_(True)
    c0 = torch.from_numpy((zeros if k["c0"] is None else k["c0"]).astype(dtype))[None].clone().requires_grad_(True)
    if k["lens"] is None:
        out, (hn, cn) = m(x, (h0, c0))
    else:
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.from_numpy(k["lens"].astype(np.int64)), enforce_sorted=True)
        out, (hn, cn) = m(packed, (h0, c0))
        out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
    total = (out * torch.from_numpy(k["d_out"].astype(dtype))).sum()
    if k["d_hn"] is not None:
        total = total + (hn[0] * torch.from_numpy(k["d_hn"].astype(dtype))).sum()
    if k["d_cn"] is not None:
        total = total + (cn[0] * torch.from_numpy(k["d_cn"].astype(dtype))).sum()
    total.backward()
    got = dict(out=out, h_n=hn[0], c_n=cn[0], dx=x.grad, d_w_ih=m.weight_ih_l0.grad, d_w_hh=m.weight_hh_l0.grad, d_h0=h0.grad[0],
               d_c0=c0.grad[0])
    if bias:
        got["d_b"] = m.bias_ih_l0.grad
        # (one gradient for both biases; torch's two differ in summation order only)
        tol = 1e-12 if dtype == np.float64 else 1e-4
        assert torch.allclose(m.bias_ih_l0.grad, m.bias_hh_l0.grad, rtol=tol, atol=tol)
    return {name: v.detach().numpy() for name, v in got.items()}


_refs = {}


def reference(name):
    """Computed once per case, never edited: the float32 output the device is given (h), the float64 recompute and backward
    on it, and the bounds.  dict: h32, gates, c, e_gates, e_c, dG, d_h0, d_c0, d_b, e_dG, e_h0, e_c0, e_b."""
    if name not in _refs:
        k = cases()[name]
        out, _, _ = forward(k["p"], k["x"], k["h0"], k["c0"], k["lens"])
        h32 = out.astype(np.float32)
        gates, c, mag = recompute(k["p"], k["x"], h32, k["h0"], k["c0"], k["lens"])
        e_gates, e_c = recompute_bounds(k["p"], gates, c, k["c0"], mag, k["lens"])
        (dG, d_h0, d_c0, d_b), (e_dG, e_h0, e_c0, e_b) = backward_steps(k["p"], gates, c, k["c0"], k["d_out"], k["d_hn"], k["d_cn"],
                                                                         k["lens"], e_gates=e_gates, e_c=e_c)
        _refs[name] = dict(h32=h32, gates=gates, c=c, e_gates=e_gates, e_c=e_c, dG=dG, d_h0=d_h0, d_c0=d_c0, d_b=d_b, e_dG=e_dG,
                           e_h0=e_h0, e_c0=e_c0, e_b=e_b)
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


def backward_ratios(name, dG, d_h0, d_c0, d_b):
    """name -> worst ratio to the bound, of a device's (or the emulation's) backward outputs on case ``name``."""
    r = reference(name)
    return dict(dG=norm_ratio(dG, r["dG"], r["e_dG"]), d_h0=norm_ratio(d_h0, r["d_h0"], r["e_h0"]),
                d_c0=norm_ratio(d_c0, r["d_c0"], r["e_c0"]), d_b=norm_ratio(d_b, r["d_b"], r["e_b"]))


def recompute_ratios(name, gates, c):
    r = reference(name)
    live = live_mask(name)
    return dict(gates=worst_ratio(gates, r["gates"], r["e_gates"], live), c=worst_ratio(c, r["c"], r["e_c"], live))


def rel_err(got, ref):
    """max |got - ref| relative to the tensor's largest magnitude."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)) / max(float(np.max(np.abs(ref))), 1e-300))
