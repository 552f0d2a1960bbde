"""Transducer (RNN-T) loss -- this repository's OWN specification (the reference snapshot has no transducer, see
model/rnnt.py; parity unpinned).  The specification is the comment on ``ms_rnnt_loss_forward`` in include/ms_hotpath.h
(Graves 2012, section 2.4); tests/rnnt_loss_ref.py restates it in numpy.

``RNNTLoss(blank, reduction)`` is called like ``CTCLoss``: ``loss((logits[N, T, U + 1, V + 1], logit_lens), (y[N, U], y_lens))``
with the joint network's outputs (normalised or not: the loss applies its own log-softmax over the symbols) and returns
``nll[N] = -log P(y_n | logits_n)`` (``none``), its sum (``sum``) or the sum divided by the batch size N (``mean`` -- NOT the
CTC wrapper's mean over per-target-length-normalised losses).  The reduction is done with torch ops.  When the logits
require grad the loss is an autograd node whose backward is ``ms_rnnt_loss_backward``; the node saves the lattice (Z, alpha,
beta) the forward wrote, the module itself keeps no state and the workspace is transient.

With ``RNNT.joint_lattice`` the ``none`` reduction scores a transcript under a model.

``rnnt_score`` is the same -log P without the logits: it takes the joint network's two projected inputs and its output layer,
and ``ms_rnnt_score`` forms each cell's row inside one MFMA kernel, keeping only the two numbers per cell the recursion needs
(``RNNT.transcript_nll`` builds it from a model).  No gradient.

``rnnt_joint_loss`` / ``RNNTJointLoss`` is that scorer as a LOSS: the same forward value, and an autograd node whose backward
(``ms_rnnt_joint_loss_backward``) gives the gradients of enc_p, pred_p, w_out and b_out without a ``[N, T, U + 1, V + 1]``
tensor.  It differentiates the joint network's output layer and its two projected inputs.  ``RNNT.loss`` (model/rnnt.py)
carries those gradients on through the projections, the prediction network's LSTM (``model/rnn_autograd.py``) and its
embedding, and to the encoder frames it was given; the encoder modules themselves (convolutions, bidirectional stacks, GRU)
still have no backward in this project, so what trains is the predictor and the joint on a frozen encoder.
"""
from typing import Tuple

import torch
from torch.autograd.function import once_differentiable

from myrtlespeech_amd import _lib

_REDUCTIONS = ("none", "sum", "mean")
MAX_U1 = 1024       # the lattice pass runs one thread per u in one workgroup


class _RNNTLossFunction(torch.autograd.Function):
    """Forward = ``ms_rnnt_loss_forward`` (nll per utterance); backward = ``ms_rnnt_loss_backward`` (logits gradient only)."""

    @staticmethod
    def forward(ctx, x, run_forward, meta):
        nll, lattice = run_forward(x)
        ctx.save_for_backward(x, nll, lattice)
        ctx.meta = meta
        return nll

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, nll, lattice = ctx.saved_tensors
        m = ctx.meta
        n, t, u1, v1 = x.shape
        grad_nll = _lib.f32c(grad_out).reshape(n).contiguous()
        grad = torch.empty_like(x)
        _lib.check(_lib.load().ms_rnnt_loss_backward(_lib.ptr(x), _lib.ptr(m["xl_dev"]), _lib.ptr(m["y_dev"]),
                                                     _lib.ptr(m["yl_dev"]), _lib.ptr(nll), _lib.ptr(lattice),
                                                     _lib.ptr(grad_nll), _lib.ptr(grad), n, t, u1, v1, m["blank"],
                                                     _lib.stream_ptr()), "ms_rnnt_loss_backward")
        return grad, None, None


def _int_lens(lens: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(lens, torch.Tensor) or lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool:
        raise ValueError(f"{what} must be an integer tensor")
    return lens.detach().reshape(-1).to("cpu", torch.int64)


class RNNTLoss(torch.nn.Module):
    def __init__(self, blank: int, reduction: str = "mean"):
        super().__init__()
        if reduction not in _REDUCTIONS:
            raise ValueError(f"{reduction} is not a valid value for reduction")
        if int(blank) < 0:
            raise ValueError(f"blank={blank} must be >= 0")
        self.blank = int(blank)
        self.reduction = reduction

    def extra_repr(self) -> str:
        return f"blank={self.blank}, reduction={self.reduction}"

    def forward(self, inputs: Tuple[torch.Tensor, torch.Tensor], targets: Tuple[torch.Tensor, torch.Tensor]
                ) -> torch.Tensor:
        x, x_lens = inputs
        y, y_lens = targets
        # ---- validation: ValueError before a device is needed
        if x.dim() != 4:
            raise ValueError("logits must be [batch, max_seq_len, max_target_len + 1, symbols]")
        n, t, u1, v1 = x.shape
        if min(n, t, u1, v1) <= 0:
            raise ValueError(f"logits of shape {tuple(x.shape)} have an empty dimension")
        if u1 > MAX_U1:
            raise ValueError(f"max_target_len + 1 = {u1} exceeds the supported {MAX_U1}")
        if not 0 <= self.blank < v1:
            raise ValueError(f"blank={self.blank} must be in [0, {v1})")
        if y.dim() != 2 or y.shape[0] != n:
            raise ValueError(f"targets must be [batch = {n}, max_target_len], got {tuple(y.shape)}")
        if y.shape[1] != u1 - 1:
            raise ValueError(f"targets are padded to {y.shape[1]} labels, the logits hold {u1 - 1} + 1 rows per frame")
        if y.is_floating_point():
            raise ValueError("targets must be an integer tensor")
        xl, yl = _int_lens(x_lens, "logit lengths"), _int_lens(y_lens, "target lengths")
        if xl.numel() != n or yl.numel() != n:
            raise ValueError(f"lengths of batch {xl.numel()} / {yl.numel()} != logits batch {n}")
        if int(xl.min()) < 1 or int(xl.max()) > t:
            raise ValueError(f"logit lengths must be in [1, {t}]")
        if int(yl.min()) < 0 or int(yl.max()) > u1 - 1:
            raise ValueError(f"target lengths must be in [0, {u1 - 1}]")
        # (a label outside [0, V1) or equal to the blank is not looked for here -- the targets may live on the device; the
        # kernels index nothing with it and give that utterance nll = +inf and a zero gradient)
        _lib.require_gpu()
        lib = _lib.load()
        x = _lib.f32c(x)
        # ONE staged upload for what starts on the host (ctc_loss.py)
        host_parts = [xl.to(torch.int32), yl.to(torch.int32)]
        y_on_host = not y.is_cuda
        if y_on_host and y.numel():
            host_parts.append(y.detach().to(torch.int32).reshape(-1))
        packed = _lib.upload(torch.cat(host_parts))
        xl_dev, yl_dev = packed[:n], packed[n:2 * n]
        if not y.numel():
            y_dev = None                                   # U1 == 1: the ABI takes NULL
        elif y_on_host:
            y_dev = packed[2 * n:]
        else:
            y_dev = y.detach().to(dtype=torch.int32).contiguous().reshape(-1)
        blank = self.blank

        def run_forward(logits: torch.Tensor):
            nll = torch.empty(n, dtype=torch.float32, device="cuda")
            lattice = torch.empty(lib.ms_rnnt_loss_lattice_bytes(n, t, u1) // 4, dtype=torch.float32, device="cuda")
            nbytes = lib.ms_rnnt_loss_workspace_bytes(n, t, u1, v1)
            ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")     # transient: nothing outlives the call
            _lib.check(lib.ms_rnnt_loss_forward(_lib.ptr(logits), _lib.ptr(xl_dev), _lib.ptr(y_dev), _lib.ptr(yl_dev),
                                                _lib.ptr(nll), _lib.ptr(lattice), n, t, u1, v1, blank, _lib.ptr(ws),
                                                ws.numel(), _lib.stream_ptr()), "ms_rnnt_loss_forward")
            return nll, lattice

        if torch.is_grad_enabled() and x.requires_grad:
            meta = dict(blank=blank, xl_dev=xl_dev, yl_dev=yl_dev, y_dev=y_dev)
            nll = _RNNTLossFunction.apply(x, run_forward, meta)
        else:
            nll = run_forward(x)[0]
        if self.reduction == "none":
            return nll
        total = nll.sum()
        return total if self.reduction == "sum" else total / n


def check_score_shapes(t, n, u1, j, v1, in_lens, targets, target_lens, blank):
    """The validation of ``rnnt_score`` (that of ``RNNTLoss.forward``, for the fused scorer's arguments): ValueError before a
    device is needed.  Returns the host int64 lengths."""
    if min(t, n, u1, j, v1) <= 0:
        raise ValueError(f"shapes T={t}, N={n}, U+1={u1}, J={j}, symbols={v1} have an empty dimension")
    if u1 > MAX_U1:
        raise ValueError(f"max_target_len + 1 = {u1} exceeds the supported {MAX_U1}")
    if not 0 <= int(blank) < v1:
        raise ValueError(f"blank={blank} must be in [0, {v1})")
    if not isinstance(targets, torch.Tensor) or targets.dim() != 2 or targets.shape[0] != n:
        raise ValueError(f"targets must be [batch = {n}, max_target_len], got {tuple(getattr(targets, 'shape', ()))}")
    if targets.shape[1] != u1 - 1:
        raise ValueError(f"targets are padded to {targets.shape[1]} labels, pred_p holds {u1 - 1} + 1 rows")
    if targets.is_floating_point():
        raise ValueError("targets must be an integer tensor")
    xl, yl = _int_lens(in_lens, "input lengths"), _int_lens(target_lens, "target lengths")
    if xl.numel() != n or yl.numel() != n:
        raise ValueError(f"lengths of batch {xl.numel()} / {yl.numel()} != batch {n}")
    if int(xl.min()) < 1 or int(xl.max()) > t:
        raise ValueError(f"input lengths must be in [1, {t}]")
    if int(yl.min()) < 0 or int(yl.max()) > u1 - 1:
        raise ValueError(f"target lengths must be in [0, {u1 - 1}]")
    return xl, yl


def _score_inputs(enc_p, pred_p, w_out, b_out, in_lens, targets, target_lens, blank):
    """What ``rnnt_score`` and ``rnnt_joint_loss`` share: the validation (ValueError before a device is needed), the float32
    device tensors and ONE staged upload for what starts on the host (RNNTLoss.forward).  Returns the tensors as given
    to the kernels (detached) and the shape."""
    for name, x in (("enc_p", enc_p), ("pred_p", pred_p)):
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError(f"{name} must be [rows, batch, joint features]")
    if not isinstance(w_out, torch.Tensor) or w_out.dim() != 2:
        raise ValueError("w_out must be [symbols, joint features]")
    t, n, j = enc_p.shape
    u1 = pred_p.shape[0]
    v1 = w_out.shape[0]
    if pred_p.shape[1] != n or pred_p.shape[2] != j or w_out.shape[1] != j:
        raise ValueError(f"enc_p {tuple(enc_p.shape)}, pred_p {tuple(pred_p.shape)} and w_out {tuple(w_out.shape)} do not agree "
                         "in the batch or the joint features")
    if b_out is not None and tuple(b_out.shape) != (v1,):
        raise ValueError(f"b_out must be [{v1}], got {tuple(b_out.shape)}")
    xl, yl = check_score_shapes(t, n, u1, j, v1, in_lens, targets, target_lens, blank)
    _lib.require_gpu()
    enc_p, pred_p, w = _lib.f32c(enc_p.detach()), _lib.f32c(pred_p.detach()), _lib.f32c(w_out.detach())
    b = None if b_out is None else _lib.f32c(b_out.detach())
    host_parts = [xl.to(torch.int32), yl.to(torch.int32)]
    y_on_host = not targets.is_cuda
    if y_on_host and targets.numel():
        host_parts.append(targets.detach().to(torch.int32).reshape(-1))
    packed = _lib.upload(torch.cat(host_parts))
    xl_dev, yl_dev = packed[:n], packed[n:2 * n]
    if not targets.numel():
        y_dev = None                                       # U1 == 1: the ABI takes NULL
    elif y_on_host:
        y_dev = packed[2 * n:]
    else:
        y_dev = targets.detach().to(dtype=torch.int32).contiguous().reshape(-1)
    return (enc_p, pred_p, w, b, xl_dev, y_dev, yl_dev), (n, t, u1, j, v1)


def _run_score(args, shape, blank):
    """``ms_rnnt_score``: nll [N] and lattice [2, N, T, U + 1]."""
    enc_p, pred_p, w, b, xl_dev, y_dev, yl_dev = args
    n, t, u1, j, v1 = shape
    lib = _lib.load()
    nll = torch.empty(n, dtype=torch.float32, device="cuda")
    lattice = torch.empty((2, n, t, u1), dtype=torch.float32, device="cuda")
    nbytes = lib.ms_rnnt_score_workspace_bytes(n, t, u1, j, v1)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")             # transient: nothing outlives the call
    _lib.check(lib.ms_rnnt_score(_lib.ptr(enc_p), _lib.ptr(pred_p), _lib.ptr(w), _lib.ptr(b), _lib.ptr(xl_dev), _lib.ptr(y_dev),
                                 _lib.ptr(yl_dev), _lib.ptr(nll), _lib.ptr(lattice), n, t, u1, j, v1, int(blank), _lib.ptr(ws),
                                 ws.numel(), _lib.stream_ptr()), "ms_rnnt_score")
    return nll, lattice


def rnnt_score(enc_p: torch.Tensor, pred_p: torch.Tensor, w_out: torch.Tensor, b_out, in_lens: torch.Tensor,
               targets: torch.Tensor, target_lens: torch.Tensor, blank: int, return_lattice: bool = False):
    """``nll[N] = -log P(y_n | audio_n)`` from the joint network's inputs -- ``ms_rnnt_score`` (include/ms_hotpath.h).

    enc_p [T, N, J] projected encoder frames, pred_p [U + 1, N, J] projected predictor outputs (row u: after ``y_n[:u]``),
    w_out [V + 1, J] and b_out [V + 1] (or None) the joint's output layer, targets [N, U] padded labels.  The logits
    ``w_out . tanh(enc_p[t] + pred_p[u]) + b_out`` are never stored: memory is 8 bytes per cell plus the packed weights.
    Returns nll, or ``(nll, lattice)`` with lattice [2, N, T, U + 1] = alpha, beta (defined on existing cells only).
    Detached float32 device tensors; there is no backward."""
    args, shape = _score_inputs(enc_p, pred_p, w_out, b_out, in_lens, targets, target_lens, blank)
    nll, lattice = _run_score(args, shape, blank)
    return (nll, lattice) if return_lattice else nll


class _RNNTJointLossFunction(torch.autograd.Function):
    """Forward = ``ms_rnnt_joint_loss_forward`` (nll per utterance, the [3, N, T, U + 1] lattice saved); backward =
    ``ms_rnnt_joint_loss_backward`` with its preferred workspace, gradients for exactly the inputs that require one."""

    @staticmethod
    def forward(ctx, enc_p, pred_p, w_out, b_out, args, shape, blank):
        e, p, w, b, xl_dev, y_dev, yl_dev = args
        n, t, u1, j, v1 = shape
        lib = _lib.load()
        nll = torch.empty(n, dtype=torch.float32, device="cuda")
        lattice = torch.empty((3, n, t, u1), dtype=torch.float32, device="cuda")
        nbytes = lib.ms_rnnt_score_workspace_bytes(n, t, u1, j, v1)
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")         # transient: nothing outlives the call
        _lib.check(lib.ms_rnnt_joint_loss_forward(_lib.ptr(e), _lib.ptr(p), _lib.ptr(w), _lib.ptr(b), _lib.ptr(xl_dev),
                                                  _lib.ptr(y_dev), _lib.ptr(yl_dev), _lib.ptr(nll), _lib.ptr(lattice), n, t, u1, j,
                                                  v1, int(blank), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "ms_rnnt_joint_loss_forward")
        saved = [e, p, w, nll, lattice] + ([b] if b is not None else [])
        ctx.save_for_backward(*saved)
        ctx.meta = dict(shape=shape, blank=int(blank), xl_dev=xl_dev, y_dev=y_dev, yl_dev=yl_dev, has_bias=b is not None,
                        like=(enc_p, pred_p, w_out, b_out))
        return nll

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        e, p, w, nll, lattice = ctx.saved_tensors[:5]
        m = ctx.meta
        b = ctx.saved_tensors[5] if m["has_bias"] else None
        n, t, u1, j, v1 = m["shape"]
        lib = _lib.load()
        grad_nll = _lib.f32c(grad_out).reshape(n).contiguous()
        d_e, d_p, d_w = torch.empty_like(e), torch.empty_like(p), torch.empty_like(w)
        want_b = b is not None and ctx.needs_input_grad[3]
        d_b = torch.empty_like(b) if want_b else None
        nbytes = lib.ms_rnnt_joint_loss_backward_workspace_bytes(n, t, u1, j, v1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")                   # transient
        _lib.check(lib.ms_rnnt_joint_loss_backward(
            _lib.ptr(e), _lib.ptr(p), _lib.ptr(w), _lib.ptr(b), _lib.ptr(m["xl_dev"]), _lib.ptr(m["y_dev"]), _lib.ptr(m["yl_dev"]),
            _lib.ptr(nll), _lib.ptr(lattice), _lib.ptr(grad_nll), _lib.ptr(d_e), _lib.ptr(d_p), _lib.ptr(d_w), _lib.ptr(d_b),
            n, t, u1, j, v1, m["blank"], _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "ms_rnnt_joint_loss_backward")
        grads = []
        for k, (g, like) in enumerate(zip((d_e, d_p, d_w, d_b), m["like"])):
            if g is None or not ctx.needs_input_grad[k]:
                grads.append(None)
            else:
                grads.append(g.to(device=like.device, dtype=like.dtype).reshape(like.shape))
        return (*grads, None, None, None)


def rnnt_joint_loss(enc_p: torch.Tensor, pred_p: torch.Tensor, w_out: torch.Tensor, b_out, in_lens: torch.Tensor,
                    targets: torch.Tensor, target_lens: torch.Tensor, blank: int, reduction: str = "mean"):
    """The transducer loss from the joint network's INPUTS, differentiable: ``rnnt_score``'s value (its arguments, its
    validation, its staged upload) under ``RNNTLoss``'s reductions (``none``: nll [N]; ``sum``; ``mean``: the sum divided by
    the batch size N), as an autograd node over enc_p [T, N, J], pred_p [U + 1, N, J], w_out [V + 1, J] and b_out [V + 1]
    (or None).  The node saves the inputs, nll and the [3, N, T, U + 1] lattice (Z, alpha, beta) -- 12 bytes per cell; its
    backward is ``ms_rnnt_joint_loss_backward`` (include/ms_hotpath.h) with its preferred workspace and returns gradients
    for exactly the inputs that require one.  No ``[N, T, U + 1, V + 1]`` tensor exists at any point.  With grad disabled, or
    when no input requires grad, it makes ``rnnt_score``'s launches only.

    It differentiates the joint network's output layer and its two projected inputs; ``RNNT.loss`` chains it with the
    predictor's and the projections' backward.  The encoder modules have no backward in this project."""
    if reduction not in _REDUCTIONS:
        raise ValueError(f"{reduction} is not a valid value for reduction")
    args, shape = _score_inputs(enc_p, pred_p, w_out, b_out, in_lens, targets, target_lens, blank)
    inputs = (enc_p, pred_p, w_out) + (() if b_out is None else (b_out,))
    if torch.is_grad_enabled() and any(x.requires_grad for x in inputs):
        nll = _RNNTJointLossFunction.apply(enc_p, pred_p, w_out, b_out, args, shape, int(blank))
    else:
        nll = _run_score(args, shape, blank)[0]
    if reduction == "none":
        return nll
    total = nll.sum()
    return total if reduction == "sum" else total / shape[0]


class RNNTJointLoss(torch.nn.Module):
    """``rnnt_joint_loss`` as a module: ``loss((enc_p, in_lens), pred_p, w_out, b_out, (targets, target_lens))``."""

    def __init__(self, blank: int, reduction: str = "mean"):
        super().__init__()
        if reduction not in _REDUCTIONS:
            raise ValueError(f"{reduction} is not a valid value for reduction")
        if int(blank) < 0:
            raise ValueError(f"blank={blank} must be >= 0")
        self.blank = int(blank)
        self.reduction = reduction

    def extra_repr(self) -> str:
        return f"blank={self.blank}, reduction={self.reduction}"

    def forward(self, inputs: Tuple[torch.Tensor, torch.Tensor], pred_p: torch.Tensor, w_out: torch.Tensor, b_out,
                targets: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        enc_p, in_lens = inputs
        y, y_lens = targets
        return rnnt_joint_loss(enc_p, pred_p, w_out, b_out, in_lens, y, y_lens, self.blank, self.reduction)
