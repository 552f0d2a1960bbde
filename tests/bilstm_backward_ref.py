"""numpy side of the bidirectional LSTM backward (``ms_lstm_recompute_dir`` / ``ms_lstm_backward_steps_bidir``; TEST
INFRASTRUCTURE ONLY).  OWN specification: the comment on ``ms_lstm_recompute`` in include/ms_hotpath.h.  Built on
tests/lstm_backward_ref.py (``L``) without editing it:

  direction 0 is ``L``'s restatement on the case as it stands;
  direction 1 is the SAME restatement on the case with every sequence flipped within its own length (``flip_time``: row t of
  sequence n goes to row lens[n] - 1 - t, rows past a length stay), its per-step results flipped back.  The reverse cell of
  sequence n walks t = lens[n] - 1 .. 0 from h0[1][n], which is the forward cell on the flipped sequence from the same state;
  h_n / c_n is then the flipped run's last state, d_hn / d_cn enter at the flipped run's last step (t = 0) and d_h0 / d_c0
  leave at its first (t = lens[n] - 1).  The dx of the two directions add.

``tests/test_bilstm_backward_cpu.py`` pins this composition to ``torch.nn.LSTM(bidirectional=True)`` in float64 with
``pack_padded_sequence`` to 1e-10 on every output and gradient, the ``_reverse`` weights included.

Cases: the nine geometries of ``L.cases()`` (H in {8, 40, 72}, N in {1, 3, 33}, T in {1, 2, 9}: lengths ragged down to 1, the
"short" case with max_len < T, lens = None, states and state gradients present and absent; at length 1 the reverse
direction's first and last step coincide), each with a second parameter set for the reverse direction, d_out [T, N, 2H] and
states / state gradients [2, N, H].  ``dir_case(name, d)`` is direction d's unidirectional view of a case (d = 1: flipped).

Bounds: ``L.recompute_bounds`` / ``L.backward_steps(..., e_gates, e_c)`` evaluated on ``dir_case(name, d)``.  The reverse
direction's arithmetic IS the forward arithmetic on the flipped rows (the same products of the same lengths, the same cell, the
same carried recurrence), so the derivation in ``L``'s docstring carries over unchanged; d_b sums the same rows in another
order, which its bound (any order) already allows.
"""
import numpy as np

import lstm_backward_ref as L

CASE_NAMES = L.CASE_NAMES


def flip_time(a, lens):
    """a [T, N, ...]: every sequence reversed within its own length; rows past a length stay where they are."""
    if a is None:
        return None
    a = np.asarray(a)
    T, N = a.shape[:2]
    Ln = L._lens(lens, T, N)
    t = np.arange(T)[:, None]
    src = np.where(t < Ln[None, :], Ln[None, :] - 1 - t, t)          # [T, N]
    return a[src, np.arange(N)[None, :]]


def _make(name):
    """The unidirectional case ``name`` widened: its parameters and tensors serve direction 0 unchanged."""
    k = L.cases()[name]
    T, N, H, In = k["T"], k["N"], k["H"], k["In"]
    rng = np.random.default_rng(sum(map(ord, name)) + 977)
    s = 2.0 / np.sqrt(H)
    f32 = lambda a: a.astype(np.float32)       # noqa: E731
    bias = k["p"]["b_ih"] is not None
    p_rev = dict(w_ih=f32(rng.uniform(-s, s, (4 * H, In))), w_hh=f32(rng.uniform(-s, s, (4 * H, H))),
                 b_ih=f32(rng.uniform(-s, s, 4 * H)) if bias else None, b_hh=f32(rng.uniform(-s, s, 4 * H)) if bias else None)

    def two(a, make):
        return None if a is None else np.stack([a, f32(make())])

    return dict(name=name, p=(k["p"], p_rev), T=T, N=N, H=H, In=In, lens=k["lens"], x=k["x"],
                h0=two(k["h0"], lambda: rng.uniform(-1, 1, (N, H))), c0=two(k["c0"], lambda: rng.uniform(-2, 2, (N, H))),
                d_out=np.ascontiguousarray(np.concatenate([k["d_out"], f32(rng.standard_normal((T, N, H)))], 2)),
                d_hn=two(k["d_hn"], lambda: rng.standard_normal((N, H))), d_cn=two(k["d_cn"], lambda: rng.standard_normal((N, H))))


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = {name: _make(name) for name in CASE_NAMES}
    return _cases


def dir_view(k, d):
    """Direction d of a bidirectional case dict as a unidirectional case of ``L`` (d = 1: x and d_out flipped within the
    lengths)."""
    H = k["H"]
    pick = lambda a: None if a is None else a[d]      # noqa: E731
    x = k["x"]
    d_out = None if k.get("d_out") is None else np.ascontiguousarray(k["d_out"][..., d * H:(d + 1) * H])
    if d == 1:
        x, d_out = flip_time(x, k["lens"]), flip_time(d_out, k["lens"])
    return dict(p=k["p"][d], T=k["T"], N=k["N"], H=H, In=k["In"], lens=k["lens"], x=x, h0=pick(k["h0"]), c0=pick(k["c0"]),
                d_out=d_out, d_hn=pick(k.get("d_hn")), d_cn=pick(k.get("d_cn")))


def dir_case(name, d):
    return dir_view(cases()[name], d)


def back(a, d, lens):
    """A per-step tensor of direction d's unidirectional run, in the layer's own time order."""
    return flip_time(a, lens) if d == 1 else a


def layer_backward(k):
    """The whole bidirectional layer in float64: out [T, N, 2H], h_n / c_n [2, N, H] and every gradient (dx summed over the
    directions, the weight gradients as pairs)."""
    parts = []
    for d in (0, 1):
        u = dir_view(k, d)
        r = L.layer_backward(u["p"], u["x"], u["h0"], u["c0"], u["lens"], u["d_out"], u["d_hn"], u["d_cn"])
        r["out"], r["dx"] = back(r["out"], d, k["lens"]), back(r["dx"], d, k["lens"])
        parts.append(r)
    res = dict(out=np.concatenate([parts[0]["out"], parts[1]["out"]], 2), dx=parts[0]["dx"] + parts[1]["dx"])
    for key in ("h_n", "c_n", "d_h0", "d_c0", "d_w_ih", "d_w_hh", "d_b"):
        res[key] = np.stack([parts[0][key], parts[1][key]])
    return res


def layer_forward(k):
    """out [T, N, 2H], h_n, c_n [2, N, H] in float64."""
    outs, hns, cns = [], [], []
    for d in (0, 1):
        u = dir_view(k, d)
        o, hn, cn = L.forward(u["p"], u["x"], u["h0"], u["c0"], u["lens"])
        outs.append(back(o, d, k["lens"]))
        hns.append(hn)
        cns.append(cn)
    return np.concatenate(outs, 2), np.stack(hns), np.stack(cns)


def torch_layer(k, dtype=np.float64):
    """``torch.nn.LSTM(bidirectional=True)`` on the CPU with autograd on the case (``pack_padded_sequence`` under lengths), with
    ``layer_backward``'s keys."""
    import torch
    T, N, H, In = k["T"], k["N"], k["H"], k["In"]
    bias = k["p"][0]["b_ih"] is not None
    td = torch.float64 if dtype == np.float64 else torch.float32
    m = torch.nn.LSTM(In, H, num_layers=1, bias=bias, bidirectional=True).to(td)
    names = (("w_ih", "weight_ih"), ("w_hh", "weight_hh")) + ((("b_ih", "bias_ih"), ("b_hh", "bias_hh")) if bias else ())
    with torch.no_grad():
        for d, sfx in enumerate(("", "_reverse")):
            for key, tname in names:
                getattr(m, f"{tname}_l0{sfx}").copy_(torch.from_numpy(k["p"][d][key].astype(dtype)))
    t = lambda a: torch.from_numpy(np.asarray(a).astype(dtype))      # noqa: E731
    x = t(k["x"]).requires_grad_(True)
    zeros = np.zeros((2, N, H), dtype=dtype)
    h0 = t(zeros if k["h0"] is None else k["h0"]).clone().requires_grad_(True)
    c0 = t(zeros if k["c0"] is None else k["c0"]).clone().requires_grad_(True)
    if k["lens"] is None:
        out, (hn, cn) = m(x, (h0, c0))
    else:
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.from_numpy(k["lens"].astype(np.int64)), enforce_sorted=True)
        out, (hn, cn) = m(packed, (h0, c0))
        out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
    total = (out * t(k["d_out"])).sum()
    if k["d_hn"] is not None:
        total = total + (hn * t(k["d_hn"])).sum()
    if k["d_cn"] is not None:
        total = total + (cn * t(k["d_cn"])).sum()
    total.backward()
    g = lambda n_: torch.stack([getattr(m, f"{n_}_l0").grad, getattr(m, f"{n_}_l0_reverse").grad])      # noqa: E731
    got = dict(out=out, h_n=hn, c_n=cn, dx=x.grad, d_h0=h0.grad, d_c0=c0.grad, d_w_ih=g("weight_ih"), d_w_hh=g("weight_hh"))
    if bias:
        got["d_b"] = g("bias_ih")
    return {name: v.detach().numpy() for name, v in got.items()}


_refs = {}


def reference(name):
    """Per direction, computed once and never edited, in the LAYER's time order: h32 (the float32 output the device is given),
    the float64 gates, c, dG, d_h0, d_c0, d_b on it and their bounds.  dict of 2-lists keyed like ``L.reference``."""
    if name not in _refs:
        k = cases()[name]
        out = {}
        for d in (0, 1):
            u = dir_case(name, d)
            o, _, _ = L.forward(u["p"], u["x"], u["h0"], u["c0"], u["lens"])
            h32 = o.astype(np.float32)
            gates, c, mag = L.recompute(u["p"], u["x"], h32, u["h0"], u["c0"], u["lens"])
            e_gates, e_c = L.recompute_bounds(u["p"], gates, c, u["c0"], mag, u["lens"])
            (dG, d_h0, d_c0, d_b), (e_dG, e_h0, e_c0, e_b) = L.backward_steps(u["p"], gates, c, u["c0"], u["d_out"], u["d_hn"], u["d_cn"],
                                                                             u["lens"], e_gates=e_gates, e_c=e_c)
            r = dict(h32=h32, gates=gates, c=c, e_gates=e_gates, e_c=e_c, dG=dG, e_dG=e_dG[..., None])
            r = {key: back(v, d, k["lens"]) for key, v in r.items()}
            r["e_dG"] = r["e_dG"][..., 0]
            r.update(d_h0=d_h0, d_c0=d_c0, d_b=d_b, e_h0=e_h0, e_c0=e_c0, e_b=e_b)
            for key, v in r.items():
                out.setdefault(key, []).append(v)
        _refs[name] = out
    return _refs[name]


def live_mask(name):
    k = cases()[name]
    return (np.arange(k["T"])[:, None] < L._lens(k["lens"], k["T"], k["N"])[None, :])[..., None]


def recompute_ratios(name, d, gates, c):
    r = reference(name)
    live = live_mask(name)
    return dict(gates=L.worst_ratio(gates, r["gates"][d], r["e_gates"][d], live), c=L.worst_ratio(c, r["c"][d], r["e_c"][d], live))


def backward_ratios(name, d, dG, d_h0, d_c0, d_b):
    r = reference(name)
    return dict(dG=L.norm_ratio(dG, r["dG"][d], r["e_dG"][d]), d_h0=L.norm_ratio(d_h0, r["d_h0"][d], r["e_h0"][d]),
                d_c0=L.norm_ratio(d_c0, r["d_c0"][d], r["e_c0"][d]), d_b=L.norm_ratio(d_b, r["d_b"][d], r["e_b"][d]))


def emulate(name, d):
    """Direction d in float32 in the device's order of operations (``L``'s emulation on ``dir_case``), in the layer's time
    order: gates, c, dG, d_h0, d_c0, d_b."""
    k, u = cases()[name], dir_case(name, d)
    h32 = back(reference(name)["h32"][d], d, k["lens"])          # (flip is its own inverse: the run's own order)
    g32, c32, _ = L.recompute(u["p"], u["x"], h32, u["h0"], u["c0"], u["lens"], dtype=np.float32)
    dG, d_h0, d_c0, d_b = L.backward_steps(u["p"], g32, c32, u["c0"], u["d_out"], u["d_hn"], u["d_cn"], u["lens"], dtype=np.float32)
    return back(g32, d, k["lens"]), back(c32, d, k["lens"]), back(dG, d, k["lens"]), d_h0, d_c0, d_b
