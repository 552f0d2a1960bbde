"""Training pieces for the transducer's prediction network and for DeepSpeech1 -- this repository's OWN specification (the comment on
``ms_lstm_recompute`` in include/ms_hotpath.h; tests/lstm_backward_ref.py restates it in numpy).

``lstm_train(rnn, x, lens, hx)`` is ``RNN.forward`` on a unidirectional LSTM stack as an autograd node.  The forward is the
existing ``run_layers`` called one layer at a time with the stack's own ``PackedLayer`` objects, so every layer's output
exists as a tensor (a padded width is sliced by ``run_layers`` as always).  The forward kernels save no gates: the backward
rebuilds them per layer, top down (``ms_lstm_recompute``: two batch GEMMs and a scan), runs the recurrence backwards
(``ms_lstm_backward_steps``: one launch per step, float32 MFMA) and finishes with three batch GEMMs through
``ms_linear_forward`` -- dx = dG w_ih, d_w_ih = dG^T x, d_w_hh = dG^T h_prev.  Gradients reach x, every
``weight_ih_l*`` / ``weight_hh_l*`` / ``bias_*_l*`` and hx.

``linear_train`` and ``embedding_train`` are the two small nodes around it: a linear layer whose forward and backward
products all run through ``ms_linear_forward`` (db is a ones-row product), and the embedding look-up whose backward is
``ms_embedding_backward``.

``rnn_train(rnn, x, lens, hx)`` is the same for LSTM stacks of either kind.  A bidirectional stack's backward runs, per layer,
two ``ms_lstm_recompute_dir`` calls (the reverse direction's gates from ``h[t + 1]``), ONE ``ms_lstm_backward_steps_bidir``
(both recurrences in the same launches, the layer's ``[T, N, 2H]`` output gradient read in place) and the batch products per
direction; tests/bilstm_backward_ref.py restates it.  ``RNN.forward(..., differentiable=True)`` and
``DeepSpeech1.forward(..., differentiable=True)`` are built on it, the latter with ``linear_clamp_train``: a linear layer with
its ``Hardtanh`` fused, whose backward passes dy where the saved OUTPUT is strictly inside the clamp.

``linear_stack_train`` runs a whole Linear / activation chain (``linear_stack_plan``'s list) through those two nodes.  The masked
convolutions and the lookahead have their nodes in ``model/conv_autograd.py`` (``maskconv_train``, ``lookahead_train``), and
``DeepSpeech2.forward(..., differentiable=True)`` strings all of them together.

``gru_train(rnn, x, lens, hx)`` is the same for GRU and tanh stacks of either kind (``_GRUStackFunction``: per layer
``ms_gru_recompute`` per direction, ONE ``ms_gru_backward_steps`` and the batch products; OWN specification: the comment on
``ms_gru_recompute`` in the header, restated by tests/gru_backward_ref.py).  It is opt-in: ``rnn_train`` and ``lstm_train``
keep refusing those cells because earlier tests pin the refusals, and ``RNN.forward(differentiable=True)`` /
``DeepSpeech2.forward(differentiable=True)`` reach it only with ``rnn.gru_backward = True``.

Out of scope, and refused with ValueError before a device is needed: ``HardLSTM``, inter-layer dropout in training mode
(``lstm_train`` also refuses ``bidirectional=True``: ``rnn_train`` serves it; both refuse GRU and tanh cells: ``gru_train``
serves them), convolutions with ``groups > 1``.  There is no dropout mask, no single-launch (persistent) backward recurrence
and no mixed-precision gradient.
"""
from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from myrtlespeech_amd import _lib
from myrtlespeech_amd.model.rnn import RNN, RNNType, run_layers


def gemm_nt(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a [M, K] . b [N, K]^T (+ bias [N]) -> [M, N] through ``ms_linear_forward`` (exact float32 MFMA, one k-ordered chain)."""
    a, b = a.contiguous(), b.contiguous()
    m, k = a.shape
    n = b.shape[0]
    y = torch.empty((m, n), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().ms_linear_forward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(bias), _lib.ptr(y), m, k, n, _lib.ACT_NONE, 0.0,
                                             0.0, _lib.stream_ptr()), "ms_linear_forward")
    return y


def _like(g: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    return g.to(device=ref.device, dtype=ref.dtype).reshape(ref.shape)


class _LinearFunction(torch.autograd.Function):
    """y = x w^T + b; backward: dx = dy w, dw = dy^T x, db = 1^T dy, each a product of ``ms_linear_forward``."""

    @staticmethod
    def forward(ctx, x2d, weight, bias):
        x = _lib.f32c(x2d.detach())
        w = _lib.f32c(weight.detach())
        b = None if bias is None else _lib.f32c(bias.detach())
        ctx.save_for_backward(x, w)
        ctx.like = (x2d, weight, bias)
        return gemm_nt(x, w, b)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        x_like, w_like, b_like = ctx.like
        dy = _lib.f32c(dy)
        need = ctx.needs_input_grad
        dx = _like(gemm_nt(dy, w.t()), x_like) if need[0] else None
        dy_t = dy.t().contiguous() if (need[1] or (b_like is not None and need[2])) else None
        dw = _like(gemm_nt(dy_t, x.t()), w_like) if need[1] else None
        db = None
        if b_like is not None and need[2]:
            ones = torch.ones((1, dy.shape[0]), dtype=torch.float32, device="cuda")
            db = _like(gemm_nt(ones, dy_t), b_like)
        return dx, dw, db


def linear_train(x2d: torch.Tensor, lin: torch.nn.Linear) -> torch.Tensor:
    """``lin(x2d)`` for x2d [M, K] as an autograd node on the device."""
    return _LinearFunction.apply(x2d, lin.weight, lin.bias)


class _EmbeddingFunction(torch.autograd.Function):
    """out[r] = table[clamp(idx[r])] (``ms_embedding_forward``); backward ``ms_embedding_backward``."""

    @staticmethod
    def forward(ctx, table, idx):
        w = _lib.f32c(table.detach())
        rows = idx.numel()
        out = torch.empty(tuple(idx.shape) + (w.shape[1],), dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().ms_embedding_forward(_lib.ptr(w), _lib.ptr(idx), _lib.ptr(out), rows, w.shape[1], w.shape[0],
                                                    _lib.stream_ptr()), "ms_embedding_forward")
        ctx.save_for_backward(idx)
        ctx.like = table
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        (idx,) = ctx.saved_tensors
        table = ctx.like
        v1, d = table.shape
        d_out = _lib.f32c(d_out)
        d_table = torch.empty((v1, d), dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().ms_embedding_backward(_lib.ptr(d_out), _lib.ptr(idx), _lib.ptr(d_table), idx.numel(), d, v1,
                                                     _lib.stream_ptr()), "ms_embedding_backward")
        return _like(d_table, table), None


class _LinearClampFunction(torch.autograd.Function):
    """y = clamp(x w^T + b, lo, hi) with the clamp fused into the product (``ACT_CLAMP``); backward: dy passes where
    lo < y < hi strictly -- ``Hardtanh``'s rule, and y sits strictly inside exactly where the pre-activation does, so the
    saved OUTPUT decides and no pre-activation is kept -- then ``_LinearFunction``'s three products."""

    @staticmethod
    def forward(ctx, x2d, weight, bias, lo, hi):
        x = _lib.f32c(x2d.detach())
        w = _lib.f32c(weight.detach())
        b = None if bias is None else _lib.f32c(bias.detach())
        m, k = x.shape
        n = w.shape[0]
        y = torch.empty((m, n), dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().ms_linear_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), m, k, n, _lib.ACT_CLAMP,
                                                 float(lo), float(hi), _lib.stream_ptr()), "ms_linear_forward")
        ctx.save_for_backward(x, w, y)
        ctx.like = (x2d, weight, bias)
        ctx.clamp = (float(lo), float(hi))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        x_like, w_like, b_like = ctx.like
        lo, hi = ctx.clamp
        dy = torch.where((y > lo) & (y < hi), _lib.f32c(dy), torch.zeros((), dtype=torch.float32, device="cuda"))
        need = ctx.needs_input_grad
        dx = _like(gemm_nt(dy, w.t()), x_like) if need[0] else None
        dy_t = dy.t().contiguous() if (need[1] or (b_like is not None and need[2])) else None
        dw = _like(gemm_nt(dy_t, x.t()), w_like) if need[1] else None
        db = None
        if b_like is not None and need[2]:
            ones = torch.ones((1, dy.shape[0]), dtype=torch.float32, device="cuda")
            db = _like(gemm_nt(ones, dy_t), b_like)
        return dx, dw, db, None, None


def linear_clamp_train(x2d: torch.Tensor, lin: torch.nn.Linear, lo: float, hi: float) -> torch.Tensor:
    """``Hardtanh(lo, hi)(lin(x2d))`` for x2d [M, K] as one autograd node on the device."""
    if not lo < hi:
        raise ValueError(f"linear_clamp_train needs lo < hi, got [{lo}, {hi}]")
    return _LinearClampFunction.apply(x2d, lin.weight, lin.bias, lo, hi)


def linear_stack_train(x2d: torch.Tensor, stack, training: bool = False) -> torch.Tensor:
    """``run_linear_stack`` as a chain of autograd nodes: ``stack`` is ``linear_stack_plan``'s list, or the Linear / activation /
    Dropout chain itself (then ``training`` is the owning module's mode).  A layer with a clamp is ``linear_clamp_train``
    (``ReLU`` is the clamp (0, +inf)), one without ``linear_train``.  ValueError, before a device is needed, for
    ``Dropout(p > 0)`` in training mode: there is no dropout mask in this project (DeepSpeech1's rule)."""
    if isinstance(stack, torch.nn.Module):
        from myrtlespeech_amd.model.fully_connected import linear_stack_plan
        mods = [stack] if isinstance(stack, torch.nn.Linear) else list(stack)
        if training and any(isinstance(m, torch.nn.Dropout) and m.p > 0 for m in mods):
            raise ValueError("linear_stack_train does not serve dropout masks: train in .eval() or with dropout = 0")
        stack = linear_stack_plan(stack, training)
    h = x2d
    for lin, clamp in stack:
        h = linear_train(h, lin) if clamp is None else linear_clamp_train(h, lin, clamp[0], clamp[1])
    return h


def embedding_train(table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """idx [...] int32 on the device -> [..., D], differentiable in ``table``."""
    return _EmbeddingFunction.apply(table, idx)


def _stack_forward(ctx, ndir, rnn, lens_dev, max_len, ragged, has_hx, x, h0, c0, flat, cell=_lib.CELL_LSTM):
    """The forward of every stack node: ``run_layers`` one layer at a time, every layer's output kept for the backward.
    ``cell`` is the stack's own (``CELL_GRU`` / ``CELL_RNN_TANH``: there is no ``c``, ``c0`` is None and ``(out, h_n)`` comes
    back), so the values are the default path's."""
    lstm = cell == _lib.CELL_LSTM
    nl = rnn.rnn.num_layers
    hidden = rnn.rnn.hidden_size
    params = rnn._layer_params()
    xin = _lib.f32c(x.detach())
    h0d = _lib.f32c(h0.detach()) if has_hx else None
    c0d = _lib.f32c(c0.detach()) if (has_hx and lstm) else None
    layer_in, hns, cns = [xin], [], []
    for layer in range(nl):
        sl = slice(ndir * layer, ndir * (layer + 1))
        out, hn, cn = run_layers(cell, layer_in[-1], lens_dev, max_len, [params[layer]], [rnn._packed[layer]], hidden,
                                 None if h0d is None else h0d[sl], None if c0d is None else c0d[sl],
                                 rnn._workspace, rnn.check_status, ragged=ragged)
        layer_in.append(out.contiguous())
        hns.append(hn)
        cns.append(cn)
    weights = [None if p is None else _lib.f32c(p.detach()) for p in flat]
    ctx.save_for_backward(*layer_in, *(([h0d, c0d] if lstm else [h0d]) if has_hx else []), *[w for w in weights if w is not None])
    ctx.meta = dict(nl=nl, hidden=hidden, lens_dev=lens_dev, max_len=max_len, has_hx=has_hx, lstm=lstm,
                    has_w=[w is not None for w in weights], like=(x, h0, c0) + tuple(flat))
    if not lstm:
        return layer_in[-1], torch.cat(hns, 0)
    return layer_in[-1], torch.cat(hns, 0), torch.cat(cns, 0)


def _stack_saved(ctx):
    """(layer_in, h0, c0, weights) as ``_stack_forward`` saved them (absent biases back as None)."""
    m = ctx.meta
    saved = list(ctx.saved_tensors)
    layer_in = saved[:m["nl"] + 1]
    pos = m["nl"] + 1
    h0 = c0 = None
    if m["has_hx"]:
        h0, c0 = saved[pos], (saved[pos + 1] if m["lstm"] else None)
        pos += 2 if m["lstm"] else 1
    weights = []
    for has in m["has_w"]:
        weights.append(saved[pos] if has else None)
        pos += has
    return layer_in, h0, c0, weights


def _stack_grads(ctx, d_top, d_h0, d_c0, w_grads):
    """The backward's return value: gradients shaped and typed like the inputs they belong to, None where none is wanted."""
    m = ctx.meta
    x_like, h_like, c_like = m["like"][:3]
    dx = _like(d_top, x_like) if ctx.needs_input_grad[5] else None
    dh0 = _like(d_h0, h_like) if (m["has_hx"] and ctx.needs_input_grad[6]) else None
    dc0 = _like(d_c0, c_like) if (m["has_hx"] and ctx.needs_input_grad[7]) else None
    flat = []
    for k, (g, like) in enumerate(zip(w_grads, m["like"][3:])):
        flat.append(None if (g is None or like is None or not ctx.needs_input_grad[8 + k]) else _like(g, like))
    return (None, None, None, None, None, dx, dh0, dc0, *flat)


class _LSTMStackFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rnn, lens_dev, max_len, ragged, has_hx, x, h0, c0, *flat):
        return _stack_forward(ctx, 1, rnn, lens_dev, max_len, ragged, has_hx, x, h0, c0, flat)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out, d_hn, d_cn):
        m = ctx.meta
        nl, hidden, lens_dev, max_len = m["nl"], m["hidden"], m["lens_dev"], m["max_len"]
        layer_in, h0, c0, weights = _stack_saved(ctx)
        lib = _lib.load()
        t, n, _ = layer_in[0].shape
        rows = t * n
        nbytes = lib.ms_lstm_recompute_workspace_bytes(t, n, hidden)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")                      # transient
        gates = torch.empty((t, n, 4 * hidden), dtype=torch.float32, device="cuda")
        cells = torch.empty((t, n, hidden), dtype=torch.float32, device="cuda")
        live = (torch.arange(t, device="cuda")[:, None] < lens_dev[None, :]).unsqueeze(-1)     # [T, N, 1]: the rows that exist
        d_top = _lib.f32c(d_out)
        d_hn = None if d_hn is None else _lib.f32c(d_hn)
        d_cn = None if d_cn is None else _lib.f32c(d_cn)
        d_h0s, d_c0s = [None] * nl, [None] * nl
        w_grads = [None] * (4 * nl)
        for layer in range(nl - 1, -1, -1):
            w_ih, w_hh, b_ih, b_hh = weights[4 * layer:4 * layer + 4]
            xl, hl = layer_in[layer], layer_in[layer + 1]
            in_size = xl.shape[2]
            h0l = None if h0 is None else h0[layer].contiguous()
            c0l = None if c0 is None else c0[layer].contiguous()
            _lib.check(lib.ms_lstm_recompute(_lib.ptr(xl), _lib.ptr(hl), _lib.ptr(h0l), _lib.ptr(c0l), _lib.ptr(lens_dev),
                                             _lib.ptr(w_ih), _lib.ptr(w_hh), _lib.ptr(b_ih), _lib.ptr(b_hh), _lib.ptr(gates),
                                             _lib.ptr(cells), t, n, in_size, hidden, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "ms_lstm_recompute")
            d_g = torch.empty((t, n, 4 * hidden), dtype=torch.float32, device="cuda")
            d_h0 = torch.empty((n, hidden), dtype=torch.float32, device="cuda")
            d_c0 = torch.empty((n, hidden), dtype=torch.float32, device="cuda")
            d_b = torch.empty(4 * hidden, dtype=torch.float32, device="cuda")
            _lib.check(lib.ms_lstm_backward_steps(_lib.ptr(gates), _lib.ptr(cells), _lib.ptr(c0l), _lib.ptr(w_hh), _lib.ptr(d_top),
                                                  _lib.ptr(None if d_hn is None else d_hn[layer].contiguous()),
                                                  _lib.ptr(None if d_cn is None else d_cn[layer].contiguous()),
                                                  _lib.ptr(lens_dev), max_len, _lib.ptr(d_g), _lib.ptr(d_h0), _lib.ptr(d_c0),
                                                  _lib.ptr(d_b), t, n, hidden, _lib.stream_ptr()), "ms_lstm_backward_steps")
            g2 = d_g.reshape(rows, 4 * hidden)
            g2_t = g2.t().contiguous()
            h_prev = torch.cat([(torch.zeros((1, n, hidden), dtype=torch.float32, device="cuda") if h0l is None else h0l[None]),
                                hl[:-1]], 0)
            # (dG is exactly 0 in the rows past a length and the layers' outputs are 0 there; what the CALLER left in those
            # rows of x may be anything, a NaN included, and must not reach the sum)
            x_rows = torch.where(live, xl, torch.zeros((), dtype=torch.float32, device="cuda")) if layer == 0 else xl
            w_grads[4 * layer] = gemm_nt(g2_t, x_rows.reshape(rows, in_size).t())
            w_grads[4 * layer + 1] = gemm_nt(g2_t, h_prev.reshape(rows, hidden).t())
            w_grads[4 * layer + 2] = d_b if b_ih is not None else None
            w_grads[4 * layer + 3] = d_b if b_hh is not None else None
            d_h0s[layer], d_c0s[layer] = d_h0, d_c0
            if layer > 0 or ctx.needs_input_grad[5]:
                d_top = gemm_nt(g2, w_ih.t()).reshape(t, n, in_size)
        return _stack_grads(ctx, d_top, torch.stack(d_h0s, 0), torch.stack(d_c0s, 0), w_grads)


class _BiLSTMStackFunction(torch.autograd.Function):
    """``_LSTMStackFunction`` for bidirectional stacks: per layer two ``ms_lstm_recompute_dir`` calls into the halves of
    gates / c, ONE ``ms_lstm_backward_steps_bidir`` (both recurrences in the same launches) and the batch products per
    direction.  ``flat`` holds eight tensors per layer: direction 0's (w_ih, w_hh, b_ih, b_hh), then the ``_reverse`` ones."""

    @staticmethod
    def forward(ctx, rnn, lens_dev, max_len, ragged, has_hx, x, h0, c0, *flat):
        return _stack_forward(ctx, 2, rnn, lens_dev, max_len, ragged, has_hx, x, h0, c0, flat)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out, d_hn, d_cn):
        m = ctx.meta
        nl, hidden, lens_dev, max_len = m["nl"], m["hidden"], m["lens_dev"], m["max_len"]
        layer_in, h0, c0, weights = _stack_saved(ctx)
        lib = _lib.load()
        t, n, _ = layer_in[0].shape
        rows = t * n
        nbytes = lib.ms_lstm_recompute_workspace_bytes(t, n, hidden)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")                      # transient
        gates = torch.empty((2, t, n, 4 * hidden), dtype=torch.float32, device="cuda")
        cells = torch.empty((2, t, n, hidden), dtype=torch.float32, device="cuda")
        steps = torch.arange(t, device="cuda")[:, None]
        live = (steps < lens_dev[None, :]).unsqueeze(-1)            # [T, N, 1]: the rows that exist
        final = (steps == lens_dev[None, :] - 1).unsqueeze(-1)      # ... and each sequence's last one
        zero = torch.zeros((), dtype=torch.float32, device="cuda")
        d_top = _lib.f32c(d_out)
        d_hn = None if d_hn is None else _lib.f32c(d_hn)
        d_cn = None if d_cn is None else _lib.f32c(d_cn)
        d_h0s, d_c0s = [None] * nl, [None] * nl
        w_grads = [None] * (8 * nl)
        for layer in range(nl - 1, -1, -1):
            lw = weights[8 * layer:8 * layer + 8]
            xl, out = layer_in[layer], layer_in[layer + 1]
            in_size = xl.shape[2]
            sl = slice(2 * layer, 2 * layer + 2)
            h0l = None if h0 is None else h0[sl].contiguous()
            c0l = None if c0 is None else c0[sl].contiguous()
            hs = [out[..., :hidden].contiguous(), out[..., hidden:].contiguous()]      # each direction's [T, N, H] output
            for d in (0, 1):
                w_ih, w_hh, b_ih, b_hh = lw[4 * d:4 * d + 4]
                _lib.check(lib.ms_lstm_recompute_dir(_lib.ptr(xl), _lib.ptr(hs[d]), _lib.ptr(None if h0l is None else h0l[d]),
                                                     _lib.ptr(None if c0l is None else c0l[d]), _lib.ptr(lens_dev), _lib.ptr(w_ih),
                                                     _lib.ptr(w_hh), _lib.ptr(b_ih), _lib.ptr(b_hh), _lib.ptr(gates[d]),
                                                     _lib.ptr(cells[d]), t, n, in_size, hidden, d, _lib.ptr(ws), ws.numel(),
                                                     _lib.stream_ptr()), "ms_lstm_recompute_dir")
            d_g = torch.empty((2, t, n, 4 * hidden), dtype=torch.float32, device="cuda")
            d_h0 = torch.empty((2, n, hidden), dtype=torch.float32, device="cuda")
            d_c0 = torch.empty((2, n, hidden), dtype=torch.float32, device="cuda")
            d_b = torch.empty((2, 4 * hidden), dtype=torch.float32, device="cuda")
            _lib.check(lib.ms_lstm_backward_steps_bidir(_lib.ptr(gates), _lib.ptr(cells), _lib.ptr(c0l), _lib.ptr(lw[1]), _lib.ptr(lw[5]),
                                                        _lib.ptr(d_top), _lib.ptr(None if d_hn is None else d_hn[sl].contiguous()),
                                                        _lib.ptr(None if d_cn is None else d_cn[sl].contiguous()),
                                                        _lib.ptr(lens_dev), max_len, _lib.ptr(d_g), _lib.ptr(d_h0), _lib.ptr(d_c0),
                                                        _lib.ptr(d_b), t, n, hidden, _lib.stream_ptr()),
                       "ms_lstm_backward_steps_bidir")
            # (dG is exactly 0 in the rows past a length and the layers' outputs are 0 there; what the CALLER left in those
            # rows of x may be anything, a NaN included, and must not reach the sum)
            x_rows = (torch.where(live, xl, zero) if layer == 0 else xl).reshape(rows, in_size).t()
            pad = torch.zeros((1, n, hidden), dtype=torch.float32, device="cuda")
            # h_prev: direction 0 is h shifted down with h0[0] in row 0; the reverse direction is h shifted UP, and its
            # initial state sits at each sequence's last live row
            h_prev = [torch.cat([pad if h0l is None else h0l[0][None], hs[0][:-1]], 0),
                      torch.where(final, zero if h0l is None else h0l[1][None], torch.cat([hs[1][1:], pad], 0))]
            need_dx = layer > 0 or ctx.needs_input_grad[5]
            dx = None
            for d in (0, 1):
                g2 = d_g[d].reshape(rows, 4 * hidden)
                g2_t = g2.t().contiguous()
                base = 8 * layer + 4 * d
                w_grads[base] = gemm_nt(g2_t, x_rows)
                w_grads[base + 1] = gemm_nt(g2_t, h_prev[d].reshape(rows, hidden).t())
                w_grads[base + 2] = d_b[d] if lw[4 * d + 2] is not None else None
                w_grads[base + 3] = d_b[d] if lw[4 * d + 3] is not None else None
                if need_dx:
                    part = gemm_nt(g2, lw[4 * d].t())
                    dx = part if dx is None else dx + part
            d_h0s[layer], d_c0s[layer] = d_h0, d_c0
            if need_dx:
                d_top = dx.reshape(t, n, in_size)
        return _stack_grads(ctx, d_top, torch.cat(d_h0s, 0), torch.cat(d_c0s, 0), w_grads)


class _GRUStackFunction(torch.autograd.Function):
    """GRU and tanh stacks of either kind.  Per layer, top down: ``ms_gru_recompute`` per direction (gates and q from the
    layer's own output), ONE ``ms_gru_backward_steps`` (both recurrences in the same launches, the ``[T, N, ndir H]`` output
    gradient read in place) and the batch products per direction through ``gemm_nt``.  ``flat`` holds four tensors per layer
    and direction: (w_ih, w_hh, b_ih, b_hh), direction 0 first.  A tanh layer runs on ``tanh_rnn_as_gru``'s parameters: with
    exact ``expf`` its r is exactly 1 and its z exactly 0, so da_r, da_z and the carried z dh are exact zeros, the layer's
    gradients are the n-block rows ``[2H:3H]`` of the GRU's, and dx / d_h0 are used as they are."""

    @staticmethod
    def forward(ctx, rnn, lens_dev, max_len, ragged, has_hx, x, h0, *flat):
        ctx.tanh = rnn.rnn_type == RNNType.BASIC_RNN
        ctx.ndir = 2 if rnn.bidirectional else 1
        # (the GRU form of a tanh layer is the cached one the forward itself runs on where that width has a persistent kernel)
        ctx.as_gru = [pk.tanh_as_gru(lp) for pk, lp in zip(rnn._packed, rnn._layer_params())] if ctx.tanh else None
        return _stack_forward(ctx, ctx.ndir, rnn, lens_dev, max_len, ragged, has_hx, x, h0, None, flat,
                              cell=_lib.CELL_RNN_TANH if ctx.tanh else _lib.CELL_GRU)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out, d_hn):
        m = ctx.meta
        nl, hidden, lens_dev, max_len, ndir = m["nl"], m["hidden"], m["lens_dev"], m["max_len"], ctx.ndir
        layer_in, h0, _, weights = _stack_saved(ctx)
        lib = _lib.load()
        t, n, _ = layer_in[0].shape
        rows, h3 = t * n, 3 * hidden
        ws = torch.empty(lib.ms_gru_recompute_workspace_bytes(t, n, hidden), dtype=torch.uint8, device="cuda")      # transient
        gates = torch.empty((ndir, t, n, h3), dtype=torch.float32, device="cuda")
        q = torch.empty((ndir, t, n, hidden), dtype=torch.float32, device="cuda")
        steps = torch.arange(t, device="cuda")[:, None]
        live = (steps < lens_dev[None, :]).unsqueeze(-1)            # [T, N, 1]: the rows that exist
        final = (steps == lens_dev[None, :] - 1).unsqueeze(-1)      # ... and each sequence's last one
        zero = torch.zeros((), dtype=torch.float32, device="cuda")
        pad = torch.zeros((1, n, hidden), dtype=torch.float32, device="cuda")
        d_top = _lib.f32c(d_out)
        d_hn = None if d_hn is None else _lib.f32c(d_hn)
        d_h0s = [None] * nl
        w_grads = [None] * (4 * ndir * nl)
        for layer in range(nl - 1, -1, -1):
            own = [tuple(weights[4 * (ndir * layer + d):4 * (ndir * layer + d) + 4]) for d in range(ndir)]
            lw = ctx.as_gru[layer] if ctx.tanh else own      # per direction (w_ih, w_hh, b_ih, b_hh) of the GRU
            xl, out = layer_in[layer], layer_in[layer + 1]
            in_size = xl.shape[2]
            sl = slice(ndir * layer, ndir * (layer + 1))
            h0l = None if h0 is None else h0[sl].contiguous()
            # each direction's [T, N, H] output, direction major (a unidirectional layer's is the output itself)
            hs = out[None] if ndir == 1 else torch.stack([out[..., :hidden], out[..., hidden:]], 0)
            for d in range(ndir):
                w_ih, w_hh, b_ih, b_hh = lw[d]
                _lib.check(lib.ms_gru_recompute(_lib.ptr(xl), _lib.ptr(hs[d]), _lib.ptr(None if h0l is None else h0l[d]),
                                                _lib.ptr(lens_dev), _lib.ptr(w_ih), _lib.ptr(w_hh), _lib.ptr(b_ih), _lib.ptr(b_hh),
                                                _lib.ptr(gates[d]), _lib.ptr(q[d]), t, n, in_size, hidden, d, _lib.ptr(ws),
                                                ws.numel(), _lib.stream_ptr()), "ms_gru_recompute")
            d_gi = torch.empty((ndir, t, n, h3), dtype=torch.float32, device="cuda")
            d_gh = torch.empty((ndir, t, n, h3), dtype=torch.float32, device="cuda")
            d_h0 = torch.empty((ndir, n, hidden), dtype=torch.float32, device="cuda")
            d_bi = torch.empty((ndir, h3), dtype=torch.float32, device="cuda")
            d_bh = torch.empty((ndir, h3), dtype=torch.float32, device="cuda")
            _lib.check(lib.ms_gru_backward_steps(_lib.ptr(gates), _lib.ptr(q), _lib.ptr(hs), _lib.ptr(h0l), _lib.ptr(lw[0][1]),
                                                 _lib.ptr(lw[1][1] if ndir == 2 else None), _lib.ptr(d_top),
                                                 _lib.ptr(None if d_hn is None else d_hn[sl].contiguous()), _lib.ptr(lens_dev),
                                                 max_len, _lib.ptr(d_gi), _lib.ptr(d_gh), _lib.ptr(d_h0), _lib.ptr(d_bi),
                                                 _lib.ptr(d_bh), t, n, hidden, ndir, _lib.stream_ptr()), "ms_gru_backward_steps")
            # (dGi is exactly 0 in the rows past a length and the layers' outputs are 0 there; what the CALLER left in those
            # rows of x may be anything, a NaN included, and must not reach the sum)
            x_rows = (torch.where(live, xl, zero) if layer == 0 else xl).reshape(rows, in_size).t()
            # h_prev: direction 0 is h shifted down with h0[0] in row 0; the reverse direction is h shifted UP, and its
            # initial state sits at each sequence's last live row
            h_prev = [torch.cat([pad if h0l is None else h0l[0][None], hs[0][:-1]], 0)]
            if ndir == 2:
                h_prev.append(torch.where(final, zero if h0l is None else h0l[1][None], torch.cat([hs[1][1:], pad], 0)))
            need_dx = layer > 0 or ctx.needs_input_grad[5]
            own_rows = slice(2 * hidden, h3) if ctx.tanh else slice(None)
            dx = None
            for d in range(ndir):
                gi2 = d_gi[d].reshape(rows, h3)
                base = 4 * (ndir * layer + d)
                w_grads[base] = gemm_nt(gi2.t().contiguous(), x_rows)[own_rows]
                w_grads[base + 1] = gemm_nt(d_gh[d].reshape(rows, h3).t().contiguous(), h_prev[d].reshape(rows, hidden).t())[own_rows]
                w_grads[base + 2] = d_bi[d][own_rows] if own[d][2] is not None else None
                w_grads[base + 3] = d_bh[d][own_rows] if own[d][3] is not None else None
                if need_dx:
                    part = gemm_nt(gi2, lw[d][0].t())
                    dx = part if dx is None else dx + part
            d_h0s[layer] = d_h0
            if need_dx:
                d_top = dx.reshape(t, n, in_size)
        x_like, h_like = m["like"][:2]
        grads = [None if (g is None or like is None or not ctx.needs_input_grad[7 + k]) else _like(g, like)
                 for k, (g, like) in enumerate(zip(w_grads, m["like"][3:]))]
        return (None, None, None, None, None, _like(d_top, x_like) if ctx.needs_input_grad[5] else None,
                _like(torch.cat(d_h0s, 0), h_like) if (m["has_hx"] and ctx.needs_input_grad[6]) else None, *grads)


def _checked_lens(rnn: RNN, x: torch.Tensor, lens: torch.Tensor, hx, single_state: bool = False) -> torch.Tensor:
    """The host lengths of a time-major batch for ``rnn``, after every shape check that needs no device (``single_state``: the
    cell has no ``c``, so ``hx`` is ONE tensor)."""
    if x.dim() != 3 or x.shape[2] != rnn.rnn.input_size or min(x.shape) <= 0:
        raise ValueError(f"x must be [T, N, In] with In = {rnn.rnn.input_size}, got {tuple(x.shape)}")
    t, n, _ = x.shape
    if not isinstance(lens, torch.Tensor) or lens.is_floating_point():
        raise ValueError("lens must be an integer tensor")
    lens_cpu = _lib.host_lens(lens).reshape(-1)
    if lens_cpu.numel() != n:
        raise ValueError(f"expected {n} lengths, got {lens_cpu.numel()}")
    if bool((lens_cpu[:-1] < lens_cpu[1:]).any()):
        raise ValueError("lens must be sorted in decreasing order")
    if int(lens_cpu.min()) < 1 or int(lens_cpu.max()) > t:
        raise ValueError(f"lengths must be in [1, {t}]")
    states, hidden = rnn.rnn.num_layers * (2 if rnn.bidirectional else 1), rnn.rnn.hidden_size
    if hx is not None and single_state:
        if not isinstance(hx, torch.Tensor) or tuple(hx.shape) != (states, n, hidden):
            raise ValueError(f"hx must be ONE tensor [{states}, {n}, {hidden}] (a GRU or tanh stack has no cell state)")
    elif hx is not None:
        if len(hx) != 2 or any(tuple(s.shape) != (states, n, hidden) for s in hx):
            raise ValueError(f"hx must be (h0, c0), each [{states}, {n}, {hidden}]")
    return lens_cpu


def _stack_train(rnn: RNN, x: torch.Tensor, lens: torch.Tensor, hx):
    """The autograd node of an LSTM stack the caller has vetted: ``_LSTMStackFunction`` or ``_BiLSTMStackFunction``."""
    lens_cpu = _checked_lens(rnn, x, lens, hx)
    _lib.require_gpu()
    max_len = int(lens_cpu[0])
    if rnn.bidirectional:
        node, flat = _BiLSTMStackFunction, [p for layer in rnn._layer_params() for d in layer for p in d]
    else:
        node, flat = _LSTMStackFunction, [p for layer in rnn._layer_params() for p in layer[0]]
    h0, c0 = hx if hx is not None else (None, None)
    out, hn, cn = node.apply(rnn, _lib.lens_i32(lens_cpu), max_len, bool(int(lens_cpu[-1]) < max_len), hx is not None, x, h0, c0,
                             *flat)
    return out, (hn, cn)


def rnn_train(rnn: RNN, x: torch.Tensor, lens: torch.Tensor, hx: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
              ) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """``lstm_train`` for LSTM stacks of either kind: x [T, N, In] TIME-MAJOR (whatever ``rnn.batch_first`` says:
    ``RNN.forward(differentiable=True)`` does the transposes), lens [N] sorted descending, hx = (h0, c0)
    [num_layers * ndir, N, H] or None (zeros) -> ``(out [T, N, ndir H], (h_n, c_n))`` with ``RNN.forward``'s values,
    differentiable in x, hx and every parameter, the ``_reverse`` ones included.  A unidirectional stack is ``lstm_train``'s
    node; a bidirectional one runs both directions' backward recurrences in the same launches."""
    if not isinstance(rnn, RNN):
        raise ValueError(f"rnn_train serves RNN modules, not {type(rnn).__name__} (HardLSTM has no backward in this project)")
    if rnn.rnn_type != RNNType.LSTM:
        raise ValueError("rnn_train serves LSTM stacks only (GRU and tanh cells have no backward in this project)")
    if rnn.training and rnn.rnn.dropout > 0 and rnn.rnn.num_layers > 1:
        raise ValueError("rnn_train does not serve inter-layer dropout in training mode")
    return _stack_train(rnn, x, lens, hx)


def lstm_train(rnn: RNN, x: torch.Tensor, lens: torch.Tensor, hx: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
               ) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """x [T, N, In] time-major, lens [N] sorted descending, hx = (h0, c0) [num_layers, N, H] or None (zeros) ->
    ``(out [T, N, H], (h_n, c_n))`` with ``RNN.forward``'s values (rows past a length are 0, the states are those at
    ``lens[n] - 1``), differentiable in x, hx and every parameter of the stack.  ``RNN.forward`` itself is untouched."""
    if not isinstance(rnn, RNN) or rnn.rnn_type != RNNType.LSTM:
        raise ValueError("lstm_train serves LSTM stacks only (GRU and tanh cells have no backward in this project)")
    if rnn.bidirectional:
        raise ValueError("lstm_train does not serve bidirectional=True (rnn_train does)")
    if rnn.training and rnn.rnn.dropout > 0 and rnn.rnn.num_layers > 1:
        raise ValueError("lstm_train does not serve inter-layer dropout in training mode")
    if rnn.batch_first:
        raise ValueError("lstm_train takes time-major input (batch_first=False)")
    return _stack_train(rnn, x, lens, hx)


def gru_train(rnn: RNN, x: torch.Tensor, lens: torch.Tensor, hx: Optional[torch.Tensor] = None
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``rnn_train`` for GRU and tanh (``RNNType.BASIC_RNN``) stacks of either kind: x [T, N, In] TIME-MAJOR (whatever
    ``rnn.batch_first`` says), lens [N] sorted descending, hx ONE tensor [num_layers * ndir, N, H] or None (zeros) ->
    ``(out [T, N, ndir H], h_n)`` with ``RNN.forward``'s values, differentiable in x, hx and every parameter, the ``_reverse``
    ones included (``_GRUStackFunction``: ``ms_gru_recompute`` / ``ms_gru_backward_steps``).  ``rnn_train`` and ``lstm_train``
    keep refusing these cells -- earlier tests pin that -- so this entry is explicit, and ``RNN.forward(differentiable=True)``
    reaches it only with ``rnn.gru_backward = True``.  ValueError, before a device is needed: LSTM stacks (``rnn_train``
    serves them), ``HardLSTM``, inter-layer dropout in training mode, bad shapes or lengths."""
    if not isinstance(rnn, RNN):
        raise ValueError(f"gru_train serves RNN modules, not {type(rnn).__name__} (HardLSTM has no backward in this project)")
    if rnn.rnn_type == RNNType.LSTM:
        raise ValueError("gru_train serves GRU and tanh stacks; an LSTM stack goes through rnn_train")
    if rnn.training and rnn.rnn.dropout > 0 and rnn.rnn.num_layers > 1:
        raise ValueError("gru_train does not serve inter-layer dropout in training mode")
    lens_cpu = _checked_lens(rnn, x, lens, hx, single_state=True)
    _lib.require_gpu()
    max_len = int(lens_cpu[0])
    flat = [p for layer in rnn._layer_params() for d in layer for p in d]
    return _GRUStackFunction.apply(rnn, _lib.lens_i32(lens_cpu), max_len, bool(int(lens_cpu[-1]) < max_len), hx is not None, x, hx,
                                   *flat)
