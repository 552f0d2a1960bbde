"""A float64 witness for the recurrent layers (test-only; imports nothing from the package under test nor from the oracle).

Written from the cell equations of torch.nn.LSTM / GRU / RNN(tanh) and of the hard-activation LSTM, with the semantics of
``pack_padded_sequence -> RNN -> pad_packed_sequence(total_length)`` stated the way a packed sequence works: lengths are
sorted in decreasing order, so the sequences alive at time ``t`` are the first ``count(lens > t)`` rows, and a step updates
that prefix only.  A row that is not alive is never read -- neither its input frame nor its state -- so the amount and the
content of the padding cannot reach a result.  Consequences, none of them coded as a special case:

* ``out[t, n]`` stays exactly 0 for ``t >= lens[n]``;
* the reverse direction walks ``t`` downwards, a row joins the prefix at ``t = lens[n] - 1`` with its initial state;
* ``h_n / c_n`` hold each row's state after its own last step;
* state order ``[l0_fwd, l0_bwd, l1_fwd, ...]``.

Inputs and parameters are float32 (as the modules hold them); they are widened once and everything stays float64.
"""
import numpy as np

LSTM, GRU, RNN_TANH, HARD_LSTM = 0, 1, 2, 3
_GATES = {LSTM: 4, GRU: 3, RNN_TANH: 1, HARD_LSTM: 4}


def _f64(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float64)


def _logistic(v):
    # 1 / (1 + e^-v) without overflow for large |v|
    e = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _hard_logistic(v):
    return np.minimum(np.maximum(0.2 * v + 0.5, 0.0), 1.0)


def _hard_tanh(v):
    return np.minimum(np.maximum(v, -1.0), 1.0)


def _step(cell, H, a_x, h, c, w_hh_t, b_hh):
    """One step for the rows alive: a_x = W_ih x_t + b_ih [k, G*H], h / c [k, H] -> (h', c')."""
    a_h = h @ w_hh_t + b_hh
    if cell in (LSTM, HARD_LSTM):
        sig, tnh = (_logistic, np.tanh) if cell == LSTM else (_hard_logistic, _hard_tanh)
        a = a_x + a_h
        i, f, g, o = sig(a[:, :H]), sig(a[:, H:2 * H]), tnh(a[:, 2 * H:3 * H]), sig(a[:, 3 * H:])
        c2 = f * c + i * g
        return o * tnh(c2), c2
    if cell == GRU:
        r = _logistic(a_x[:, :H] + a_h[:, :H])
        z = _logistic(a_x[:, H:2 * H] + a_h[:, H:2 * H])
        n = np.tanh(a_x[:, 2 * H:] + r * a_h[:, 2 * H:])
        return (1.0 - z) * n + z * h, None
    return np.tanh(a_x + a_h), None


def stack_forward(cell, x, lens, layers, hidden_size, h0=None, c0=None):
    """x [T, N, In] time-major; lens [N] sorted in decreasing order, each in [1, T]; layers: per layer a list over directions
    of (w_ih, w_hh, b_ih | None, b_hh | None).  -> (out [T, N, D * H], h_n [L * D, N, H], c_n | None), float64."""
    x = _f64(x)
    T, N, _ = x.shape
    lens = np.asarray(lens).astype(np.int64).reshape(-1)
    if lens.shape[0] != N or lens.min() < 1 or lens.max() > T:
        raise ValueError("lengths must be N values in [1, T]")
    if np.any(np.diff(lens) > 0):
        raise ValueError("lengths must be sorted in decreasing order")
    H, L, D, G = hidden_size, len(layers), len(layers[0]), _GATES[cell]
    steps = int(lens[0])
    alive = [int(np.count_nonzero(lens > t)) for t in range(steps)]      # the packed sequence's batch sizes
    has_c = cell in (LSTM, HARD_LSTM)
    h_n = np.zeros((L * D, N, H)) if h0 is None else _f64(h0).copy()
    c_n = (np.zeros((L * D, N, H)) if c0 is None else _f64(c0).copy()) if has_c else None
    if h_n.shape != (L * D, N, H) or (has_c and c_n.shape != h_n.shape):
        raise ValueError("initial state must be [layers * directions, N, H]")
    inp = x
    for l, dirs in enumerate(layers):
        out = np.zeros((T, N, D * H))
        for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(dirs):
            w_ih, w_hh_t = _f64(w_ih), _f64(w_hh).T.copy()
            if w_ih.shape != (G * H, inp.shape[2]) or w_hh_t.shape != (H, G * H):
                raise ValueError("weight shapes do not match the cell")
            b_ih = np.zeros(G * H) if b_ih is None else _f64(b_ih)
            b_hh = np.zeros(G * H) if b_hh is None else _f64(b_hh)
            h = h_n[l * D + d]                       # updated in place, prefix by prefix: a row's last write is its last step
            c = c_n[l * D + d] if has_c else None
            for t in (range(steps) if d == 0 else range(steps - 1, -1, -1)):
                k = alive[t]
                a_x = inp[t, :k] @ w_ih.T + b_ih
                h2, c2 = _step(cell, H, a_x, h[:k], c[:k] if has_c else None, w_hh_t, b_hh)
                h[:k] = h2
                if has_c:
                    c[:k] = c2
                out[t, :k, d * H:(d + 1) * H] = h2
        inp = out
    return inp, h_n, c_n


def torch_layers(params, num_layers, bidirectional, bias=True):
    """torch.nn.LSTM / GRU / RNN parameter names (``weight_ih_l{k}[_reverse]`` ...) -> ``layers`` of ``stack_forward``."""
    out = []
    for l in range(num_layers):
        dirs = []
        for sfx in ["", "_reverse"][:2 if bidirectional else 1]:
            tag = f"_l{l}{sfx}"
            dirs.append((params["weight_ih" + tag], params["weight_hh" + tag],
                         params["bias_ih" + tag] if bias else None, params["bias_hh" + tag] if bias else None))
        out.append(dirs)
    return out


def hard_layers(params, num_layers, bidirectional):
    """The hard LSTM's parameter names (``layers.{k}[.fwd|.bwd].cell.*``) -> ``layers`` of ``stack_forward``."""
    out = []
    for l in range(num_layers):
        dirs = []
        for sub in (["fwd.", "bwd."] if bidirectional else [""]):
            pre = f"layers.{l}.{sub}cell."
            dirs.append(tuple(params[pre + n] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
        out.append(dirs)
    return out


def rnn_forward(kind, x, lens, params, hidden_size, num_layers=1, bidirectional=False, hx=None, batch_first=False,
                bias=True):
    """``RNN.forward`` for kind LSTM / GRU / RNN_TANH: -> (out, (h_n, c_n)) for the LSTM, (out, h_n) otherwise."""
    x = np.asarray(x)
    if batch_first:
        x = x.transpose(1, 0, 2)
    h0, c0 = (None, None) if hx is None else (hx if kind == LSTM else (hx, None))
    out, h_n, c_n = stack_forward(kind, x, lens, torch_layers(params, num_layers, bidirectional, bias), hidden_size, h0, c0)
    if batch_first:
        out = out.transpose(1, 0, 2)
    return (out, (h_n, c_n)) if kind == LSTM else (out, h_n)


def hard_lstm_forward(x, params, hidden_size, num_layers=1, bidirectional=False, hx=None, batch_first=False):
    """``HardLSTM.forward``: no lengths, every sequence fills the buffer.  -> (out, (h_n, c_n))."""
    x = np.asarray(x)
    if batch_first:
        x = x.transpose(1, 0, 2)
    T, N, _ = x.shape
    h0, c0 = (None, None) if hx is None else hx
    out, h_n, c_n = stack_forward(HARD_LSTM, x, np.full(N, T), hard_layers(params, num_layers, bidirectional), hidden_size,
                                  h0, c0)
    if batch_first:
        out = out.transpose(1, 0, 2)
    return out, (h_n, c_n)
