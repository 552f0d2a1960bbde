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

Dropout (``model/dropout.py``; OWN specification: the comment on ``ms_dropout_forward`` in the header, restated by
tests/dropout_ref.py) is opt-in as well: with no ``DropoutGenerator`` attached every entry refuses ``Dropout(p > 0)`` and
inter-layer dropout in training mode exactly as before.  With one, ``linear_clamp_dropout_train`` is a clamped linear layer with
its dropout (forward: the product, then ``ms_dropout_forward``; backward: gate and mask in ONE ``ms_clamp_dropout_backward``),
``linear_stack_train`` serves a chain's ``Dropout`` modules, and the stack nodes drop the output of every layer but the last on
its way to the next layer.  A stack node saves each layer's UNDROPPED output (its own recurrence reads it as ``h_prev``) and
the backward remakes the dropped one into a scratch buffer for the next layer's recompute -- one memory-bound pass per layer
instead of a second saved ``[T, N, ndir H]`` tensor -- and passes the gradient handed down a layer through the same kernel.

``hard_lstm_train(rnn, x, hx)`` is the same for ``HardLSTM`` stacks of either kind (``_HardLSTMStackFunction``: per layer
``ms_hard_lstm_recompute`` per direction -- the gate plane holds the PRE-CLAMP values, formed with the reference's two roundings
-- ONE ``ms_hard_lstm_backward_steps`` and the batch products; OWN specification: the comment on ``ms_hard_lstm_recompute`` in
the header, restated by tests/hard_lstm_backward_ref.py).  No lengths (the cell ignores them) and no dropout (it has none).  It
is opt-in like ``gru_train``: ``rnn_train`` / ``gru_train`` keep refusing a ``HardLSTM``, and the models reach it only with
``HardLSTM.hard_backward = True``.

Out of scope, and refused with ValueError before a device is needed: dropout in training mode with no generator
attached (``lstm_train`` also refuses ``bidirectional=True``: ``rnn_train`` serves it; both refuse GRU and tanh cells:
``gru_train`` serves them), convolutions with ``groups > 1``.  There is no single-launch (persistent) backward recurrence and no
mixed-precision gradient.
"""
from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from myrtlespeech_amd import _lib
from myrtlespeech_amd.model.dropout import DropoutGenerator, apply_mask, dropout_call, dropout_train
from myrtlespeech_amd.model.hard_lstm import HardLSTM
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


def _linear_grads(ctx, dy, x, w):
    """(dx, dw, db) of y = x w^T + b from dy, for the inputs ``ctx.like`` = (x, w, b) that want one."""
    x_like, w_like, b_like = ctx.like
    need = ctx.needs_input_grad
    dx = _like(gemm_nt(dy, w.t()), x_like) if need[0] else None
    dy_t = dy.t().contiguous() if (need[1] or (b_like is not None and need[2])) else None
    dw = _like(gemm_nt(dy_t, x.t()), w_like) if need[1] else None
    db = None
    if b_like is not None and need[2]:
        ones = torch.ones((1, dy.shape[0]), dtype=torch.float32, device="cuda")
        db = _like(gemm_nt(ones, dy_t), b_like)
    return dx, dw, db


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
        return _linear_grads(ctx, _lib.f32c(dy), x, w)


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
        lo, hi = ctx.clamp
        dy = torch.where((y > lo) & (y < hi), _lib.f32c(dy), torch.zeros((), dtype=torch.float32, device="cuda"))
        return (*_linear_grads(ctx, dy, x, w), None, None)


def linear_clamp_train(x2d: torch.Tensor, lin: torch.nn.Linear, lo: float, hi: float) -> torch.Tensor:
    """``Hardtanh(lo, hi)(lin(x2d))`` for x2d [M, K] as one autograd node on the device."""
    if not lo < hi:
        raise ValueError(f"linear_clamp_train needs lo < hi, got [{lo}, {hi}]")
    return _LinearClampFunction.apply(x2d, lin.weight, lin.bias, lo, hi)


class _LinearClampDropoutFunction(torch.autograd.Function):
    """out = clamp(x w^T + b, lo, hi) * m: ``_LinearClampFunction``'s product into y (saved: the clamped PRE-dropout output),
    then ``ms_dropout_forward`` into out.  Backward: ``ms_clamp_dropout_backward`` -- dy * m where lo < y < hi strictly, 0
    elsewhere, the mask remade from ``call`` -- in one pass, then ``_LinearFunction``'s three products."""

    @staticmethod
    def forward(ctx, x2d, weight, bias, lo, hi, call):
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
        ctx.call = call
        return apply_mask(y, torch.empty_like(y), call)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        x, w, y = ctx.saved_tensors
        lo, hi = ctx.clamp
        thr, scale, seed, offset = ctx.call
        d_out = _lib.f32c(d_out)
        dy = torch.empty_like(y)
        _lib.check(_lib.load().ms_clamp_dropout_backward(_lib.ptr(d_out), _lib.ptr(y), _lib.ptr(dy), y.numel(), lo, hi, thr, scale,
                                                         seed, offset, _lib.stream_ptr()), "ms_clamp_dropout_backward")
        return (*_linear_grads(ctx, dy, x, w), None, None, None)


def linear_clamp_dropout_train(x2d: torch.Tensor, lin: torch.nn.Linear, lo: float, hi: float, p: float,
                               generator: DropoutGenerator) -> torch.Tensor:
    """``Dropout(p)(Hardtanh(lo, hi)(lin(x2d)))`` in training mode for x2d [M, K] as one autograd node on the device; the mask is
    indexed over the [M, N] output.  Consumes one offset of ``generator``."""
    if not lo < hi:
        raise ValueError(f"linear_clamp_dropout_train needs lo < hi, got [{lo}, {hi}]")
    return _LinearClampDropoutFunction.apply(x2d, lin.weight, lin.bias, lo, hi, dropout_call(p, generator))


def _dropout_steps(mods):
    """[[linear | None, fused clamp | None, dropout p | None], ...] of a Linear / activation / Dropout chain in training mode:
    a ``Dropout(p > 0)`` joins the layer in front of it, or stands alone (linear None) where there is none to join."""
    from myrtlespeech_amd.model.utils import activation_clamp
    steps = []
    for m in mods:
        if isinstance(m, torch.nn.Linear):
            steps.append([m, None, None])
        elif isinstance(m, torch.nn.Dropout):
            if m.p > 0:
                if steps and steps[-1][0] is not None and steps[-1][2] is None:
                    steps[-1][2] = m.p
                else:
                    steps.append([None, None, m.p])
        else:
            clamp = activation_clamp(m)
            if clamp is not None:
                if not steps or steps[-1][0] is None or steps[-1][1] is not None or steps[-1][2] is not None:
                    raise NotImplementedError("activation without a preceding Linear")
                steps[-1][1] = clamp
    return steps


def linear_stack_train(x2d: torch.Tensor, stack, training: bool = False, generator: Optional[DropoutGenerator] = None
                       ) -> torch.Tensor:
    """``run_linear_stack`` as a chain of autograd nodes: ``stack`` is ``linear_stack_plan``'s list, or the Linear / activation /
    Dropout chain itself (then ``training`` is the owning module's mode).  A layer with a clamp is ``linear_clamp_train``
    (``ReLU`` is the clamp (0, +inf)), one without ``linear_train``.  ``Dropout(p > 0)`` in training mode: with no ``generator``
    ValueError, before a device is needed (the rule a user can rely on: no source of randomness attached, no dropout); with
    one it is applied, fused with the clamp in front of it where there is one (``linear_clamp_dropout_train``) and through
    ``dropout_train`` otherwise, one offset per application in chain order.  A ``Dropout`` with p == 0, and any in eval mode,
    launches nothing and consumes no offset."""
    if isinstance(stack, torch.nn.Module):
        from myrtlespeech_amd.model.fully_connected import linear_stack_plan
        mods = [stack] if isinstance(stack, torch.nn.Linear) else list(stack)
        if training and any(isinstance(m, torch.nn.Dropout) and m.p > 0 for m in mods):
            if generator is None:
                raise ValueError("linear_stack_train does not serve dropout masks: train in .eval() or with dropout = 0")
            steps = _dropout_steps(mods)
            _lib.require_gpu()      # (before the first offset is taken: a call that cannot run consumes none)
            h = x2d
            for lin, clamp, p in steps:
                if lin is None:
                    h = dropout_train(h, p, generator)
                elif clamp is not None and p is not None:
                    h = linear_clamp_dropout_train(h, lin, clamp[0], clamp[1], p, generator)
                else:
                    h = linear_train(h, lin) if clamp is None else linear_clamp_train(h, lin, clamp[0], clamp[1])
                    if p is not None:
                        h = dropout_train(h, p, generator)
            return h
        stack = linear_stack_plan(stack, training)
    h = x2d
    for lin, clamp in stack:
        h = linear_train(h, lin) if clamp is None else linear_clamp_train(h, lin, clamp[0], clamp[1])
    return h


def embedding_train(table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """idx [...] int32 on the device -> [..., D], differentiable in ``table``."""
    return _EmbeddingFunction.apply(table, idx)


def _stack_forward(ctx, ndir, rnn, lens_dev, max_len, ragged, has_hx, drop, x, h0, c0, flat, cell=_lib.CELL_LSTM):
    """The forward of every stack node: ``run_layers`` one layer at a time, every layer's output kept for the backward.
    ``cell`` is the stack's own (``CELL_HARD_LSTM``: a ``HardLSTM``; ``CELL_GRU`` / ``CELL_RNN_TANH``: there is no ``c``, ``c0`` is None and ``(out, h_n)`` comes
    back), so the values are the default path's.  ``drop`` (``_stack_dropout``: one call per layer but the last, or None):
    layer l + 1 reads layer l's output through ``ms_dropout_forward``; what is KEPT is the undropped output."""
    lstm = cell in (_lib.CELL_LSTM, _lib.CELL_HARD_LSTM)      # the cells with a ``c``
    nl = rnn.rnn.num_layers
    hidden = rnn.rnn.hidden_size
    params = rnn._layer_params()
    xin = _lib.f32c(x.detach())
    h0d = _lib.f32c(h0.detach()) if has_hx else None
    c0d = _lib.f32c(c0.detach()) if (has_hx and lstm) else None
    layer_in, hns, cns = [xin], [], []
    cur = xin
    for layer in range(nl):
        sl = slice(ndir * layer, ndir * (layer + 1))
        out, hn, cn = run_layers(cell, cur, lens_dev, max_len, [params[layer]], [rnn._packed[layer]], hidden,
                                 None if h0d is None else h0d[sl], None if c0d is None else c0d[sl],
                                 rnn._workspace, rnn.check_status, ragged=ragged)
        cur = out.contiguous()
        layer_in.append(cur)
        if drop is not None and layer < nl - 1:
            cur = apply_mask(cur, torch.empty_like(cur), drop[layer])
        hns.append(hn)
        cns.append(cn)
    weights = [None if p is None else _lib.f32c(p.detach()) for p in flat]
    ctx.save_for_backward(*layer_in, *(([h0d, c0d] if lstm else [h0d]) if has_hx else []), *[w for w in weights if w is not None])
    ctx.meta = dict(nl=nl, hidden=hidden, lens_dev=lens_dev, max_len=max_len, has_hx=has_hx, lstm=lstm, drop=drop,
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
    """The backward's return value: gradients shaped and typed like the inputs they belong to, None where none is wanted.  A
    node's inputs are (rnn, lens_dev, max_len, ragged, has_hx, drop, x, h0[, c0], *flat): a GRU or tanh node has no ``c0`` slot."""
    m = ctx.meta
    x_like, h_like, c_like = m["like"][:3]
    need = ctx.needs_input_grad
    dx = _like(d_top, x_like) if need[6] else None
    states = [_like(d_h0, h_like) if (m["has_hx"] and need[7]) else None]
    if m["lstm"]:
        states.append(_like(d_c0, c_like) if (m["has_hx"] and need[8]) else None)
    first = 7 + len(states)
    flat = []
    for k, (g, like) in enumerate(zip(w_grads, m["like"][3:])):
        flat.append(None if (g is None or like is None or not need[first + k]) else _like(g, like))
    return (None, None, None, None, None, None, dx, *states, *flat)


def _empty(*shape):
    return torch.empty(shape, dtype=torch.float32, device="cuda")


def _layer_input(ctx_meta, layer_in, layer, scratch):
    """What layer ``layer`` read in the forward: the saved tensor, or (a stack with dropout, layer > 0) the layer below's saved
    output dropped again into ``scratch`` (one [T, N, ndir H] buffer for the whole backward)."""
    drop = ctx_meta["drop"]
    if drop is None or layer == 0:
        return layer_in[layer], scratch
    if scratch is None:
        scratch = torch.empty_like(layer_in[layer])
    return apply_mask(layer_in[layer], scratch, drop[layer - 1]), scratch


def _stack_dropout(rnn: RNN, generator: Optional[DropoutGenerator], what: str):
    """The inter-layer dropout of one forward of ``rnn``: None where there is none to apply (eval mode, ``dropout == 0``, one
    layer -- no offset is consumed), else one ``dropout_call`` per layer but the last, offsets in ascending layer order, from
    ``generator`` or ``rnn.dropout_generator``.  ValueError where dropout is due and neither generator is there."""
    if not (rnn.training and rnn.rnn.dropout > 0 and rnn.rnn.num_layers > 1):
        return None
    generator = generator if generator is not None else rnn.dropout_generator
    if generator is None:
        raise ValueError(f"{what} does not serve inter-layer dropout in training mode")
    return [dropout_call(rnn.rnn.dropout, generator) for _ in range(rnn.rnn.num_layers - 1)]


def _stack_masks(t, lens_dev, ndir):
    """(live, final), each [T, N, 1]: the rows that exist, and (bidirectional only) each sequence's last one."""
    steps = torch.arange(t, device="cuda")[:, None]
    live = (steps < lens_dev[None, :]).unsqueeze(-1)
    return live, ((steps == lens_dev[None, :] - 1).unsqueeze(-1) if ndir == 2 else None)


def _dir_outputs(out, hidden, ndir):
    """Each direction's [T, N, H] output, direction major (a unidirectional layer's is the output itself)."""
    return out[None] if ndir == 1 else torch.stack([out[..., :hidden], out[..., hidden:]], 0)


def _layer_products(xl, live, hs, h0l, final, d_gi, d_gh, w_ih, need_dx):
    """The batch products that finish a layer.  Per direction d: d_w_ih = dGi[d]^T x and d_w_hh = dGh[d]^T h_prev[d] (the
    LSTM's dGi and dGh are the one dG); and dx = sum over d of dGi[d] w_ih[d], [T, N, In], if ``need_dx`` (None otherwise).
    ``live`` is given for the stack's first layer only."""
    ndir, t, n, width = d_gi.shape
    rows, hidden, in_size = t * n, hs.shape[-1], xl.shape[2]
    zero = torch.zeros((), dtype=torch.float32, device="cuda")
    pad = torch.zeros((1, n, hidden), dtype=torch.float32, device="cuda")
    # (dGi is exactly 0 in the rows past a length and the layers' outputs are 0 there; what the CALLER left in those
    # rows of x may be anything, a NaN included, and must not reach the sum)
    x_rows = (xl if live is None else torch.where(live, xl, zero)).reshape(rows, in_size).t()
    # h_prev: direction 0 is h shifted down with h0[0] in row 0; the reverse direction is h shifted UP, and its
    # initial state sits at each sequence's last live row
    h_prev = [torch.cat([pad if h0l is None else h0l[0][None], hs[0][:-1]], 0)]
    if ndir == 2:
        h_prev.append(torch.where(final, zero if h0l is None else h0l[1][None], torch.cat([hs[1][1:], pad], 0)))
    d_w, dx = [], None
    for d in range(ndir):
        gi2 = d_gi[d].reshape(rows, width)
        g_t = gi2.t().contiguous()
        d_w_ih = gemm_nt(g_t, x_rows)
        if d_gh is not d_gi:
            g_t = None      # (the transposed planes are the backward's largest transients: one at a time)
            g_t = d_gh[d].reshape(rows, width).t().contiguous()
        d_w.append((d_w_ih, gemm_nt(g_t, h_prev[d].reshape(rows, hidden).t())))
        g_t = None
        if need_dx:
            part = gemm_nt(gi2, w_ih[d].t())
            dx = part if dx is None else dx + part
    return d_w, (dx.reshape(t, n, in_size) if need_dx else None)


class _LSTMStackFunction(torch.autograd.Function):
    """LSTM stacks of either kind.  Per layer, top down: the gates and c of each direction from the layer's own output
    (``ms_lstm_recompute``; bidirectional ``ms_lstm_recompute_dir`` into the halves of gates / c), ONE
    ``ms_lstm_backward_steps`` (bidirectional ``ms_lstm_backward_steps_bidir``: both recurrences in the same launches, the
    ``[T, N, 2H]`` output gradient read in place) and the batch products per direction.  ``flat`` holds four tensors per layer
    and direction: (w_ih, w_hh, b_ih, b_hh), direction 0 first, then the ``_reverse`` ones."""

    @staticmethod
    def forward(ctx, rnn, lens_dev, max_len, ragged, has_hx, drop, x, h0, c0, *flat):
        ctx.ndir = 2 if rnn.bidirectional else 1
        return _stack_forward(ctx, ctx.ndir, rnn, lens_dev, max_len, ragged, has_hx, drop, x, h0, c0, flat)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out, d_hn, d_cn):
        m, ndir = ctx.meta, ctx.ndir
        nl, hidden, lens_dev, max_len = m["nl"], m["hidden"], m["lens_dev"], m["max_len"]
        layer_in, h0, c0, weights = _stack_saved(ctx)
        t, n, _ = layer_in[0].shape
        live, final = _stack_masks(t, lens_dev, ndir)
        lib, ptr = _lib.load(), _lib.ptr
        ws = torch.empty(lib.ms_lstm_recompute_workspace_bytes(t, n, hidden), dtype=torch.uint8, device="cuda")      # transient
        gates, cells = _empty(ndir, t, n, 4 * hidden), _empty(ndir, t, n, hidden)
        d_top = _lib.f32c(d_out)
        d_hn = None if d_hn is None else _lib.f32c(d_hn)
        d_cn = None if d_cn is None else _lib.f32c(d_cn)
        d_h0s, d_c0s = [None] * nl, [None] * nl
        w_grads = [None] * (4 * ndir * nl)
        scratch = None
        for layer in range(nl - 1, -1, -1):
            lw = [weights[4 * (ndir * layer + d):4 * (ndir * layer + d) + 4] for d in range(ndir)]      # per direction
            xl, scratch = _layer_input(m, layer_in, layer, scratch)
            hs = _dir_outputs(layer_in[layer + 1], hidden, ndir)
            sl = slice(ndir * layer, ndir * (layer + 1))      # this layer's states of the stack's [num_layers * ndir, N, H]
            h0l = None if h0 is None else h0[sl].contiguous()
            c0l = None if c0 is None else c0[sl].contiguous()
            for d in range(ndir):
                w_ih, w_hh, b_ih, b_hh = lw[d]
                args = (ptr(xl), ptr(hs[d]), ptr(None if h0l is None else h0l[d]), ptr(None if c0l is None else c0l[d]),
                        ptr(lens_dev), ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), ptr(gates[d]), ptr(cells[d]), t, n, xl.shape[2],
                        hidden)
                if ndir == 1:
                    _lib.check(lib.ms_lstm_recompute(*args, ptr(ws), ws.numel(), _lib.stream_ptr()), "ms_lstm_recompute")
                else:
                    _lib.check(lib.ms_lstm_recompute_dir(*args, d, ptr(ws), ws.numel(), _lib.stream_ptr()), "ms_lstm_recompute_dir")
            d_g, d_b = _empty(ndir, t, n, 4 * hidden), _empty(ndir, 4 * hidden)
            d_h0, d_c0 = _empty(ndir, n, hidden), _empty(ndir, n, hidden)
            steps, name = ((lib.ms_lstm_backward_steps, "ms_lstm_backward_steps") if ndir == 1 else
                           (lib.ms_lstm_backward_steps_bidir, "ms_lstm_backward_steps_bidir"))
            _lib.check(steps(ptr(gates), ptr(cells), ptr(c0l), *(ptr(w[1]) for w in lw), ptr(d_top),
                             ptr(None if d_hn is None else d_hn[sl].contiguous()),
                             ptr(None if d_cn is None else d_cn[sl].contiguous()), ptr(lens_dev), max_len, ptr(d_g),
                             ptr(d_h0), ptr(d_c0), ptr(d_b), t, n, hidden, _lib.stream_ptr()), name)
            d_w, dx = _layer_products(xl, live if layer == 0 else None, hs, h0l, final, d_g, d_g, [w[0] for w in lw],
                                        layer > 0 or ctx.needs_input_grad[6])
            for d in range(ndir):
                base = 4 * (ndir * layer + d)
                w_grads[base], w_grads[base + 1] = d_w[d]
                w_grads[base + 2] = d_b[d] if lw[d][2] is not None else None
                w_grads[base + 3] = d_b[d] if lw[d][3] is not None else None
            d_h0s[layer], d_c0s[layer] = d_h0, d_c0
            if dx is not None:
                # (the gradient handed down a layer passes through the mask the forward put on that layer's output)
                d_top = dx if (m["drop"] is None or layer == 0) else apply_mask(dx, dx, m["drop"][layer - 1])
        return _stack_grads(ctx, d_top, torch.cat(d_h0s, 0), torch.cat(d_c0s, 0), w_grads)


class _GRUStackFunction(torch.autograd.Function):
    """GRU and tanh stacks of either kind.  Per layer, top down: ``ms_gru_recompute`` per direction (gates and q from the
    layer's own output), ONE ``ms_gru_backward_steps`` (both recurrences in the same launches, the ``[T, N, ndir H]`` output
    gradient read in place) and the batch products per direction through ``gemm_nt``.  ``flat`` holds four tensors per layer
    and direction: (w_ih, w_hh, b_ih, b_hh), direction 0 first.  A tanh layer runs on ``tanh_rnn_as_gru``'s parameters: with
    exact ``expf`` its r is exactly 1 and its z exactly 0, so da_r, da_z and the carried z dh are exact zeros, the layer's
    gradients are the n-block rows ``[2H:3H]`` of the GRU's, and dx / d_h0 are used as they are."""

    @staticmethod
    def forward(ctx, rnn, lens_dev, max_len, ragged, has_hx, drop, x, h0, *flat):
        ctx.tanh = rnn.rnn_type == RNNType.BASIC_RNN
        ctx.ndir = 2 if rnn.bidirectional else 1
        # (the GRU form of a tanh layer is the cached one the forward itself runs on where that width has a persistent kernel)
        ctx.as_gru = [pk.tanh_as_gru(lp) for pk, lp in zip(rnn._packed, rnn._layer_params())] if ctx.tanh else None
        return _stack_forward(ctx, ctx.ndir, rnn, lens_dev, max_len, ragged, has_hx, drop, x, h0, None, flat,
                              cell=_lib.CELL_RNN_TANH if ctx.tanh else _lib.CELL_GRU)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out, d_hn):
        m, ndir = ctx.meta, ctx.ndir
        nl, hidden, lens_dev, max_len = m["nl"], m["hidden"], m["lens_dev"], m["max_len"]
        layer_in, h0, c0, weights = _stack_saved(ctx)
        t, n, _ = layer_in[0].shape
        live, final = _stack_masks(t, lens_dev, ndir)
        lib, ptr = _lib.load(), _lib.ptr
        h3 = 3 * hidden
        ws = torch.empty(lib.ms_gru_recompute_workspace_bytes(t, n, hidden), dtype=torch.uint8, device="cuda")      # transient
        gates, q = _empty(ndir, t, n, h3), _empty(ndir, t, n, hidden)
        d_top = _lib.f32c(d_out)
        d_hn = None if d_hn is None else _lib.f32c(d_hn)
        d_h0s = [None] * nl
        w_grads = [None] * (4 * ndir * nl)
        scratch = None
        own_rows = slice(2 * hidden, h3) if ctx.tanh else slice(None)
        for layer in range(nl - 1, -1, -1):
            own = [tuple(weights[4 * (ndir * layer + d):4 * (ndir * layer + d) + 4]) for d in range(ndir)]
            lw = ctx.as_gru[layer] if ctx.tanh else own      # per direction (w_ih, w_hh, b_ih, b_hh) of the GRU
            xl, scratch = _layer_input(m, layer_in, layer, scratch)
            hs = _dir_outputs(layer_in[layer + 1], hidden, ndir)
            sl = slice(ndir * layer, ndir * (layer + 1))      # this layer's states of the stack's [num_layers * ndir, N, H]
            h0l = None if h0 is None else h0[sl].contiguous()
            for d in range(ndir):
                w_ih, w_hh, b_ih, b_hh = lw[d]
                _lib.check(lib.ms_gru_recompute(ptr(xl), ptr(hs[d]), ptr(None if h0l is None else h0l[d]), ptr(lens_dev), ptr(w_ih),
                                                ptr(w_hh), ptr(b_ih), ptr(b_hh), ptr(gates[d]), ptr(q[d]), t, n, xl.shape[2], hidden,
                                                d, ptr(ws), ws.numel(), _lib.stream_ptr()), "ms_gru_recompute")
            d_gi, d_gh = _empty(ndir, t, n, h3), _empty(ndir, t, n, h3)
            d_h0, d_bi, d_bh = _empty(ndir, n, hidden), _empty(ndir, h3), _empty(ndir, h3)
            _lib.check(lib.ms_gru_backward_steps(ptr(gates), ptr(q), ptr(hs), ptr(h0l), ptr(lw[0][1]),
                                                 ptr(lw[1][1] if ndir == 2 else None), ptr(d_top),
                                                 ptr(None if d_hn is None else d_hn[sl].contiguous()), ptr(lens_dev), max_len,
                                                 ptr(d_gi), ptr(d_gh), ptr(d_h0), ptr(d_bi), ptr(d_bh), t, n, hidden, ndir,
                                                 _lib.stream_ptr()), "ms_gru_backward_steps")
            d_w, dx = _layer_products(xl, live if layer == 0 else None, hs, h0l, final, d_gi, d_gh, [w[0] for w in lw],
                                        layer > 0 or ctx.needs_input_grad[6])
            for d in range(ndir):
                base = 4 * (ndir * layer + d)
                w_grads[base], w_grads[base + 1] = d_w[d][0][own_rows], d_w[d][1][own_rows]
                w_grads[base + 2] = d_bi[d][own_rows] if own[d][2] is not None else None
                w_grads[base + 3] = d_bh[d][own_rows] if own[d][3] is not None else None
            d_h0s[layer] = d_h0
            if dx is not None:
                # (the gradient handed down a layer passes through the mask the forward put on that layer's output)
                d_top = dx if (m["drop"] is None or layer == 0) else apply_mask(dx, dx, m["drop"][layer - 1])
        return _stack_grads(ctx, d_top, torch.cat(d_h0s, 0), None, w_grads)


class _HardLSTMStackFunction(torch.autograd.Function):
    """``HardLSTM`` stacks of either kind: ``_LSTMStackFunction``'s loop on the hard cell's two calls.  Per layer, top down:
    ``ms_hard_lstm_recompute`` per direction (the PRE-CLAMP gate values and c from the layer's own output), ONE
    ``ms_hard_lstm_backward_steps`` (both recurrences in the same launches, the ``[T, N, ndir H]`` output gradient read in
    place) and the batch products per direction.  No lengths: every sequence has T steps.  ``flat`` as in ``_LSTMStackFunction``."""

    @staticmethod
    def forward(ctx, rnn, lens_dev, max_len, ragged, has_hx, drop, x, h0, c0, *flat):
        ctx.ndir = 2 if rnn.bidirectional else 1
        res = _stack_forward(ctx, ctx.ndir, rnn, None, max_len, False, has_hx, None, x, h0, c0, flat, cell=_lib.CELL_HARD_LSTM)
        if rnn.num_layers == 1:
            return res
        # ``HardLSTM.forward`` runs a stack of several layers in ONE ``run_layers`` call, and a padded or chained stack hands
        # its layers' outputs on in another layout than the layer loop does: the same values in other bits.  The node returns
        # the default path's bits, so that call is made as well; the backward keeps the loop's per-layer outputs, which are
        # consistent with each other.  A one-layer stack (DeepSpeech1's) is one call either way.
        out, hn, cn = run_layers(_lib.CELL_HARD_LSTM, _lib.f32c(x.detach()), None, max_len, rnn._layer_params(), rnn._packed,
                                 rnn.hidden_size, _lib.f32c(h0.detach()) if has_hx else None,
                                 _lib.f32c(c0.detach()) if has_hx else None, rnn._workspace, rnn.check_status)
        return out, hn, cn

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out, d_hn, d_cn):
        m, ndir = ctx.meta, ctx.ndir
        nl, hidden = m["nl"], m["hidden"]
        layer_in, h0, c0, weights = _stack_saved(ctx)
        t, n, _ = layer_in[0].shape
        lib, ptr = _lib.load(), _lib.ptr
        ws = torch.empty(lib.ms_lstm_recompute_workspace_bytes(t, n, hidden), dtype=torch.uint8, device="cuda")      # transient
        gates, cells = _empty(ndir, t, n, 4 * hidden), _empty(ndir, t, n, hidden)
        # (every row is live; the reverse direction's initial state sits at the last step of every sequence)
        final = None if ndir == 1 else (torch.arange(t, device="cuda") == t - 1)[:, None, None].expand(t, n, 1)
        d_top = _lib.f32c(d_out)
        d_hn = None if d_hn is None else _lib.f32c(d_hn)
        d_cn = None if d_cn is None else _lib.f32c(d_cn)
        d_h0s, d_c0s = [None] * nl, [None] * nl
        w_grads = [None] * (4 * ndir * nl)
        for layer in range(nl - 1, -1, -1):
            lw = [weights[4 * (ndir * layer + d):4 * (ndir * layer + d) + 4] for d in range(ndir)]      # per direction
            xl = layer_in[layer]
            hs = _dir_outputs(layer_in[layer + 1], hidden, ndir)
            sl = slice(ndir * layer, ndir * (layer + 1))      # this layer's states of the stack's [num_layers * ndir, N, H]
            h0l = None if h0 is None else h0[sl].contiguous()
            c0l = None if c0 is None else c0[sl].contiguous()
            for d in range(ndir):
                w_ih, w_hh, b_ih, b_hh = lw[d]
                _lib.check(lib.ms_hard_lstm_recompute(ptr(xl), ptr(hs[d]), ptr(None if h0l is None else h0l[d]),
                                                      ptr(None if c0l is None else c0l[d]), ptr(w_ih), ptr(w_hh), ptr(b_ih),
                                                      ptr(b_hh), ptr(gates[d]), ptr(cells[d]), t, n, xl.shape[2], hidden, d, ptr(ws),
                                                      ws.numel(), _lib.stream_ptr()), "ms_hard_lstm_recompute")
            d_a, d_b = _empty(ndir, t, n, 4 * hidden), _empty(ndir, 4 * hidden)
            d_h0, d_c0 = _empty(ndir, n, hidden), _empty(ndir, n, hidden)
            _lib.check(lib.ms_hard_lstm_backward_steps(ptr(gates), ptr(cells), ptr(c0l), ptr(lw[0][1]),
                                                       ptr(lw[1][1] if ndir == 2 else None), ptr(d_top),
                                                       ptr(None if d_hn is None else d_hn[sl].contiguous()),
                                                       ptr(None if d_cn is None else d_cn[sl].contiguous()), ptr(d_a), ptr(d_h0),
                                                       ptr(d_c0), ptr(d_b), t, n, hidden, ndir, _lib.stream_ptr()),
                       "ms_hard_lstm_backward_steps")
            d_w, dx = _layer_products(xl, None, hs, h0l, final, d_a, d_a, [w[0] for w in lw], layer > 0 or ctx.needs_input_grad[6])
            for d in range(ndir):
                base = 4 * (ndir * layer + d)
                w_grads[base], w_grads[base + 1] = d_w[d]
                w_grads[base + 2] = d_b[d] if lw[d][2] is not None else None
                w_grads[base + 3] = d_b[d] if lw[d][3] is not None else None
            d_h0s[layer], d_c0s[layer] = d_h0, d_c0
            if dx is not None:
                d_top = dx
        return _stack_grads(ctx, d_top, torch.cat(d_h0s, 0), torch.cat(d_c0s, 0), w_grads)


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


def _stack_train(rnn: RNN, x: torch.Tensor, lens: torch.Tensor, hx, generator, what):
    """The autograd node of an LSTM stack the caller has vetted (``_LSTMStackFunction``)."""
    if _needs_generator(rnn, generator):
        raise ValueError(f"{what} does not serve inter-layer dropout in training mode")
    lens_cpu = _checked_lens(rnn, x, lens, hx)
    _lib.require_gpu()
    drop = _stack_dropout(rnn, generator, what)      # (after the device check: a call that cannot run consumes no offset)
    max_len = int(lens_cpu[0])
    flat = [p for layer in rnn._layer_params() for d in layer for p in d]
    h0, c0 = hx if hx is not None else (None, None)
    out, hn, cn = _LSTMStackFunction.apply(rnn, _lib.lens_i32(lens_cpu), max_len, bool(int(lens_cpu[-1]) < max_len), hx is not None,
                                           drop, x, h0, c0, *flat)
    return out, (hn, cn)


def _needs_generator(rnn: RNN, generator) -> bool:
    """Inter-layer dropout is due in this forward and there is no generator to draw its masks from."""
    return (rnn.training and rnn.rnn.dropout > 0 and rnn.rnn.num_layers > 1 and generator is None
            and rnn.dropout_generator is None)


def rnn_train(rnn: RNN, x: torch.Tensor, lens: torch.Tensor, hx: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
              generator: Optional[DropoutGenerator] = None) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """``lstm_train`` for LSTM stacks of either kind: x [T, N, In] TIME-MAJOR (whatever ``rnn.batch_first`` says:
    ``RNN.forward(differentiable=True)`` does the transposes), lens [N] sorted descending, hx = (h0, c0)
    [num_layers * ndir, N, H] or None (zeros) -> ``(out [T, N, ndir H], (h_n, c_n))`` with ``RNN.forward``'s values,
    differentiable in x, hx and every parameter, the ``_reverse`` ones included.  A unidirectional stack is ``lstm_train``'s
    node; a bidirectional one runs both directions' backward recurrences in the same launches.  Inter-layer dropout in training
    mode draws its masks from ``generator`` or ``rnn.dropout_generator`` (one offset per layer but the last) and is refused
    with ValueError where neither is there."""
    if not isinstance(rnn, RNN):
        raise ValueError(f"rnn_train serves RNN modules, not {type(rnn).__name__} (a HardLSTM goes through hard_lstm_train)")
    if rnn.rnn_type != RNNType.LSTM:
        raise ValueError("rnn_train serves LSTM stacks only (GRU and tanh cells have no backward in this project)")
    return _stack_train(rnn, x, lens, hx, generator, "rnn_train")


def lstm_train(rnn: RNN, x: torch.Tensor, lens: torch.Tensor, hx: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               generator: Optional[DropoutGenerator] = None) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """x [T, N, In] time-major, lens [N] sorted descending, hx = (h0, c0) [num_layers, N, H] or None (zeros) ->
    ``(out [T, N, H], (h_n, c_n))`` with ``RNN.forward``'s values (rows past a length are 0, the states are those at
    ``lens[n] - 1``), differentiable in x, hx and every parameter of the stack.  ``RNN.forward`` itself is untouched."""
    if not isinstance(rnn, RNN) or rnn.rnn_type != RNNType.LSTM:
        raise ValueError("lstm_train serves LSTM stacks only (GRU and tanh cells have no backward in this project)")
    if rnn.bidirectional:
        raise ValueError("lstm_train does not serve bidirectional=True (rnn_train does)")
    if _needs_generator(rnn, generator):
        raise ValueError("lstm_train does not serve inter-layer dropout in training mode")
    if rnn.batch_first:
        raise ValueError("lstm_train takes time-major input (batch_first=False)")
    return _stack_train(rnn, x, lens, hx, generator, "lstm_train")


def gru_train(rnn: RNN, x: torch.Tensor, lens: torch.Tensor, hx: Optional[torch.Tensor] = None,
              generator: Optional[DropoutGenerator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``rnn_train`` for GRU and tanh (``RNNType.BASIC_RNN``) stacks of either kind: x [T, N, In] TIME-MAJOR (whatever
    ``rnn.batch_first`` says), lens [N] sorted descending, hx ONE tensor [num_layers * ndir, N, H] or None (zeros) ->
    ``(out [T, N, ndir H], h_n)`` with ``RNN.forward``'s values, differentiable in x, hx and every parameter, the ``_reverse``
    ones included (``_GRUStackFunction``: ``ms_gru_recompute`` / ``ms_gru_backward_steps``).  ``rnn_train`` and ``lstm_train``
    keep refusing these cells -- earlier tests pin that -- so this entry is explicit, and ``RNN.forward(differentiable=True)``
    reaches it only with ``rnn.gru_backward = True``.  ValueError, before a device is needed: LSTM stacks (``rnn_train``
    serves them), ``HardLSTM``, inter-layer dropout in training mode with neither ``generator`` nor ``rnn.dropout_generator``,
    bad shapes or lengths."""
    if not isinstance(rnn, RNN):
        raise ValueError(f"gru_train serves RNN modules, not {type(rnn).__name__} (a HardLSTM goes through hard_lstm_train)")
    if rnn.rnn_type == RNNType.LSTM:
        raise ValueError("gru_train serves GRU and tanh stacks; an LSTM stack goes through rnn_train")
    if _needs_generator(rnn, generator):
        raise ValueError("gru_train does not serve inter-layer dropout in training mode")
    lens_cpu = _checked_lens(rnn, x, lens, hx, single_state=True)
    _lib.require_gpu()
    drop = _stack_dropout(rnn, generator, "gru_train")
    max_len = int(lens_cpu[0])
    flat = [p for layer in rnn._layer_params() for d in layer for p in d]
    return _GRUStackFunction.apply(rnn, _lib.lens_i32(lens_cpu), max_len, bool(int(lens_cpu[-1]) < max_len), hx is not None, drop, x,
                                   hx, *flat)


def hard_lstm_train(rnn: HardLSTM, x: torch.Tensor, hx: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
                    ) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """``rnn_train`` for ``HardLSTM`` stacks of either kind: x [T, N, In] TIME-MAJOR (whatever ``rnn.batch_first`` says:
    ``HardLSTM.forward(differentiable=True)`` does the transposes), hx = (h0, c0) [num_layers * ndir, N, H] or None (zeros) ->
    ``(out [T, N, ndir H], (h_n, c_n))`` with ``HardLSTM.forward``'s values, differentiable in x, hx and every ``weight_*`` /
    ``bias_*`` of ``rnn.rnn.layers[k](.fwd|.bwd).cell`` (``_HardLSTMStackFunction``: ``ms_hard_lstm_recompute`` /
    ``ms_hard_lstm_backward_steps``).  No lengths -- the cell ignores them -- and no dropout: the cell has none.  The derivative
    is the reference's under torch autograd: ``torch.clamp`` passes a gradient on the closed interval, ``Hardtanh`` on the open
    one.  ValueError, before a device is needed: a module that is no ``HardLSTM`` (``rnn_train`` / ``gru_train`` serve ``RNN``),
    bad shapes."""
    if not isinstance(rnn, HardLSTM):
        raise ValueError(f"hard_lstm_train serves HardLSTM modules, not {type(rnn).__name__} (rnn_train / gru_train serve RNN)")
    in_size = rnn.rnn.layers[0].fwd.cell.input_size if rnn.bidirectional else rnn.rnn.layers[0].cell.input_size
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[2] != in_size or min(x.shape) <= 0:
        raise ValueError(f"x must be [T, N, In] with In = {in_size}, got {tuple(getattr(x, 'shape', ()))}")
    t, n, _ = x.shape
    states, hidden = rnn.num_layers * (2 if rnn.bidirectional else 1), rnn.hidden_size
    if hx is not None:
        if (not isinstance(hx, (tuple, list)) or len(hx) != 2
                or any(not isinstance(s, torch.Tensor) or tuple(s.shape) != (states, n, hidden) for s in hx)):
            raise ValueError(f"hx must be (h0, c0), each [{states}, {n}, {hidden}]")
    _lib.require_gpu()
    flat = [p for layer in rnn._layer_params() for d in layer for p in d]
    h0, c0 = hx if hx is not None else (None, None)
    out, hn, cn = _HardLSTMStackFunction.apply(rnn, None, t, False, hx is not None, None, x, h0, c0, *flat)
    return out, (hn, cn)
