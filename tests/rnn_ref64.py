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

``operands=`` (default None: everything above, untouched) turns the witness into an emulation of what the recurrent kernels do
to their OPERANDS under MS_PRECISION=bf16x3 ("bf16x3") or MS_PRECISION=fp16 ("fp16"): every sum, every bias and every
activation stays float64, only the factors of the two matrix products of a layer are rounded the way csrc/rnn.hip rounds
them.  Restated from the code (plane arithmetic: csrc/common.h, restated once in tests/gemm_split_cases.py and used from there):

  weights      ``pack_rows_split_kernel<P>`` (W_ih), ``pack_whh_split_kernel<P>`` / ``pack_whh_gru_kernel`` (W_hh), and
               ``split_planes_launch`` for the W_ih of a layer without a persistent LSTM kernel: bf16 pairs hi = rn(w),
               lo = rn(w - hi); the one-plane form keeps rn_fp16(w) alone.  No per-tensor scale: the power-of-two scale word
               restated in tests/conv_exact_cases.py (``weight_scale``) goes with fp16 weight planes packed through
               ``weight_scale_launch``; it is 1 for bf16 planes, and these pack kernels take none in any format.
  layer input  ``split_planes_kernel`` / ``split_planes_packed_kernel`` / ``to_f16_plane_kernel`` for x, and the same
               arithmetic where a chained layer writes the next layer's planes itself (``p.out_hi``): untagged hi, lo of the
               float32 value (fp16: one plane).  A first layer whose input width is no multiple of 32 and whose hidden
               width is not padded keeps the float32 GEMM: no rounding at all (LSTM-64 fed 24 features).
  h            ``publish_split<P>`` / ``publish_elem``: the 16-bit word of rn(h) with its lowest bit REPLACED by the epoch
               tag, lo = the word of rn(h - tagged hi) with its lowest bit replaced likewise; fp16: the tagged word of
               rn_fp16(h) alone.  The tag of the h that the step at sequence time t consumes is (t >> 1) & 1
               (``epoch_clock`` with the default two exchange slots), in both directions and for the initial state.
  products     hi hi + lo hi + hi lo (lo lo is absent); one product in the one-plane form.  Here a (wh + wl) + al wh: wh + wl
               is exact in float64, so the three terms are the same numbers.
  own state    c, the h of z * h in the GRU, the outputs and h_n / c_n are the float32 state of the owning thread: not rounded.

Which form a layer takes (``_layer_plan``) restates ``ms_rnn_padded_hidden``, ``use_f16`` and ``use_split_gemm`` for a
device whose CUs hold every persistent kernel (an MI355X: 256): under "fp16" only an LSTM / hard LSTM that runs at 256, 512,
768 or 1 024 units (padded widths count) is one fp16 plane, every other layer is bf16 pairs; a layer with no persistent kernel
(a tanh-RNN or GRU wider than 2 560, an LSTM wider than 2 048 -- under "fp16" wider than 1 024) multiplies h and W_hh in exact
float32 a step at a time and rounds only its projection.  Zero-padded units are exact zeros and are not modelled.
"""
import numpy as np

import gemm_split_cases as GS

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


# ---- operand rounding (``operands=``)
_PAIR = ("bf16", 2)        # bf16 hi + lo: every layer of "bf16x3", and the layers "fp16" has no one-plane kernel for
_ONE = ("f16", 1)          # one fp16 plane
_TWO_STREAM = (256, 512, 768, 1024)
_WIDE_LSTM = (1280, 1536, 2048)
_GRU_WIDTHS = (512, 768, 1024, 1280, 1536, 2048, 2560)


def _next_width(H, widths):
    return next((w for w in widths if w >= H), None)


def _layer_plan(cell, H, in_size, first, operands):
    """-> (projection format | None, recurrence format | None): a format is (plane type, number of planes), None = float32
    operands, no rounding."""
    if operands not in ("bf16x3", "fp16"):
        raise ValueError("operands must be None, 'bf16x3' or 'fp16'")
    if cell in (LSTM, HARD_LSTM):
        if H <= 128:
            hp = -(-H // 64) * 64                       # the one-stream kernel: any multiple of 64
        elif H <= 1024:
            hp = _next_width(H, _TWO_STREAM)
        else:
            hp = _next_width(H, _WIDE_LSTM) if operands == "bf16x3" else None
        rec = None if hp is None else (_ONE if operands == "fp16" and hp in _TWO_STREAM else _PAIR)
    else:                                               # GRU, and the tanh-RNN written as one
        hp = _next_width(H, _GRU_WIDTHS)
        rec = None if hp is None else _PAIR
    if hp is None:
        hp = -(-H // 64) * 64                           # a launch per step at the next multiple of 64
    split_gemm = (not first) or hp != H or in_size % 32 == 0
    return ((rec or _PAIR) if split_gemm else None), rec


def _planes(a, fmt):
    """float32 values (weights, a layer's input: ``split_planes_kernel``) -> (hi, lo | None) float64 in the plane format ``fmt``:
    hi = rn(a), lo = rn(a - hi), no tag."""
    kind, planes = fmt
    a = np.asarray(a, dtype=np.float32)
    hi = GS.plane(a, kind)
    return hi.astype(np.float64), (GS.plane(a - hi, kind).astype(np.float64) if planes == 2 else None)


def _w_planes(w, fmt):
    """A float32 weight matrix [rows, K] -> (wh + wl, wh) as [K, rows] views, float64 (wl = 0 in a one-plane format)."""
    hi, lo = _planes(w, fmt)
    return (hi if lo is None else hi + lo).T, hi.T


def _tagged(v, kind, tag):
    """float32 -> the value of the 16-bit word of rn(v) with its lowest bit replaced by ``tag``."""
    if kind == "f16":
        bits = (v.astype(np.float16).view(np.uint16) & np.uint16(0xFFFE)) | np.uint16(tag)
        return bits.view(np.float16).astype(np.float32)
    bits = (GS.rn_bf16(v).view(np.uint32) & np.uint32(0xFFFE0000)) | np.uint32(tag << 16)
    return bits.view(np.float32)


def _h_planes(h, fmt, tag):
    """``publish_split``: the state as the other workgroups read it -> (hi, lo | None) float64."""
    kind, planes = fmt
    h32 = np.ascontiguousarray(h, dtype=np.float32)
    hi = _tagged(h32, kind, tag)
    lo = _tagged(h32 - hi, kind, tag) if planes == 2 else None
    return hi.astype(np.float64), (None if lo is None else lo.astype(np.float64))


def _product(a, w):
    """(hi, lo | None) x (wh + wl, wh): hi (wh + wl) + lo wh."""
    y = a[0] @ w[0]
    return y if a[1] is None else y + a[1] @ w[1]


def _step(cell, H, a_x, h, c, w_hh_t, b_hh, a_h=None):
    """One step for the rows alive: a_x = W_ih x_t + b_ih [k, G*H], h / c [k, H] -> (h', c')."""
    if a_h is None:
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


def stack_forward(cell, x, lens, layers, hidden_size, h0=None, c0=None, operands=None):
    """x [T, N, In] time-major; lens [N] sorted in decreasing order, each in [1, T]; layers: per layer a list over directions
    of (w_ih, w_hh, b_ih | None, b_hh | None).  -> (out [T, N, D * H], h_n [L * D, N, H], c_n | None), float64.
    ``operands``: None, "bf16x3" or "fp16" (module docstring)."""
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
        proj, rec = (None, None) if operands is None else _layer_plan(cell, H, inp.shape[2], l == 0, operands)
        if proj is not None:      # (a padded frame is never read: it enters the planes as 0 and its projection is not looked at)
            live = np.arange(steps)[:, None] < lens[None, :]
            inp_planes = _planes(np.where(live[:, :, None], inp[:steps], 0.0).reshape(steps * N, -1), proj)
        for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(dirs):
            w_ih, w_hh_t = _f64(w_ih), _f64(w_hh).T.copy()
            if w_ih.shape != (G * H, inp.shape[2]) or w_hh_t.shape != (H, G * H):
                raise ValueError("weight shapes do not match the cell")
            b_ih = np.zeros(G * H) if b_ih is None else _f64(b_ih)
            b_hh = np.zeros(G * H) if b_hh is None else _f64(b_hh)
            h = h_n[l * D + d]                       # updated in place, prefix by prefix: a row's last write is its last step
            c = c_n[l * D + d] if has_c else None
            # the projection of every frame at once, as the device runs it (float64 sums: the order does not matter here)
            a_x_all = None if proj is None else (_product(inp_planes, _w_planes(w_ih, proj)) + b_ih).reshape(steps, N, G * H)
            w_hh_planes = None if rec is None else _w_planes(w_hh_t.T, rec)
            for t in (range(steps) if d == 0 else range(steps - 1, -1, -1)):
                k = alive[t]
                a_x = inp[t, :k] @ w_ih.T + b_ih if proj is None else a_x_all[t, :k]
                a_h = None if rec is None else _product(_h_planes(h[:k], rec, (t >> 1) & 1), w_hh_planes) + b_hh
                h2, c2 = _step(cell, H, a_x, h[:k], c[:k] if has_c else None, w_hh_t, b_hh, a_h)
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
                bias=True, operands=None):
    """``RNN.forward`` for kind LSTM / GRU / RNN_TANH: -> (out, (h_n, c_n)) for the LSTM, (out, h_n) otherwise."""
    x = np.asarray(x)
    if batch_first:
        x = x.transpose(1, 0, 2)
    h0, c0 = (None, None) if hx is None else (hx if kind == LSTM else (hx, None))
    out, h_n, c_n = stack_forward(kind, x, lens, torch_layers(params, num_layers, bidirectional, bias), hidden_size, h0, c0,
                                  operands)
    if batch_first:
        out = out.transpose(1, 0, 2)
    return (out, (h_n, c_n)) if kind == LSTM else (out, h_n)


def hard_lstm_forward(x, params, hidden_size, num_layers=1, bidirectional=False, hx=None, batch_first=False, operands=None):
    """``HardLSTM.forward``: no lengths, every sequence fills the buffer.  -> (out, (h_n, c_n))."""
    x = np.asarray(x)
    if batch_first:
        x = x.transpose(1, 0, 2)
    T, N, _ = x.shape
    h0, c0 = (None, None) if hx is None else hx
    out, h_n, c_n = stack_forward(HARD_LSTM, x, np.full(N, T), hard_layers(params, num_layers, bidirectional), hidden_size,
                                  h0, c0, operands)
    if batch_first:
        out = out.transpose(1, 0, 2)
    return out, (h_n, c_n)
