"""Training pieces for DeepSpeech2's front end and lookahead -- this repository's OWN specification (the comment on
``ms_maskconv_backward_data`` in include/ms_hotpath.h; tests/conv_backward_cases.py restates it in numpy).

``maskconv_train(module, (acts, lens), clamp)`` is ``MaskConv1d`` / ``MaskConv2d`` (+ the clamp that follows it) as one autograd
node.  The forward is ``cnn._conv_forward`` exactly as the default path calls it -- the same routes, so the same bits as
``module(x, fused_activation=clamp)`` -- with one difference: the caller's tensor is NOT masked in place (an in-place write
under autograd is a trap, and the kernels' load predicates already read the frames past a length as 0).  It saves x, the
OUTPUT y and w; the backward gates dy on y (dy passes where y is strictly inside the clamp: ``_LinearClampFunction``'s rule) and
makes two calls, ``ms_maskconv_backward_data`` (skipped when the input needs no gradient: DS2's first convolution reads data)
and ``ms_maskconv_backward_weight`` (dw and db in one pass), both float32 MFMA without atomics.

``lookahead_train(module, x_tnf, clamp)`` follows ``lookahead_apply(..., out_layout="ntf")``: the recurrent stack's ``[T, N, F]``
output in, ``[N, T, F]`` out, and the gradient comes back ``[T, N, F]``, ready for ``rnn_train``'s backward.

Out of scope, refused with ValueError before a device is needed: ``groups != 1``.
"""
from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from myrtlespeech_amd import _lib
from myrtlespeech_amd.model.cnn import MaskConv1d, MaskConv2d, PaddingMode, _conv_forward, _geometry, _pair
from myrtlespeech_amd.model.lookahead import Lookahead, lookahead_apply


def _act_args(clamp):
    return (_lib.ACT_NONE, 0.0, 0.0) if clamp is None else (_lib.ACT_CLAMP, float(clamp[0]), float(clamp[1]))


class _MaskConvFunction(torch.autograd.Function):
    """(x4 [N, Cin, Fin, Tin], weight4 [Cout, Cin, KF, KT], bias) -> (y [N, Cout, Fout, Tout], the new lengths)."""

    @staticmethod
    def forward(ctx, module, seq_lens, stride, dilation, clamp, x4, weight4, bias):
        x = _lib.f32c(x4.detach())
        w = weight4.detach()
        same = module._padding_mode == PaddingMode.SAME
        y, new_lens = _conv_forward(x, seq_lens, w, bias, module._packed, stride, dilation, 1, same, clamp)
        pf, pt, _, _ = _geometry(x.shape, w, stride, dilation, same)
        ctx.save_for_backward(x, _lib.f32c(w), y)
        ctx.meta = dict(lens=_lib.lens_i32(seq_lens), stride=stride, dilation=dilation, pads=(pf[0], pt[0]), clamp=clamp,
                        like=(x4, weight4, bias))
        ctx.mark_non_differentiable(new_lens)
        return y, new_lens

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, _d_lens):
        x, w, y = ctx.saved_tensors
        m = ctx.meta
        x_like, w_like, b_like = m["like"]
        lib = _lib.load()
        n, cin, fin, tin = x.shape
        cout, _, kf, kt = w.shape
        _, _, fout, tout = y.shape
        (sf, st), (df, dt), (pf, pt) = m["stride"], m["dilation"], m["pads"]
        a, lo, hi = _act_args(m["clamp"])
        dy = _lib.f32c(dy)
        geom = (n, cin, fin, tin, cout, fout, tout, kf, kt, sf, st, df, dt, pf, pt, a, lo, hi)
        need = ctx.needs_input_grad
        dx = dw = db = None
        if need[5]:
            dx = torch.empty_like(x)
            _lib.check(lib.ms_maskconv_backward_data(_lib.ptr(w), _lib.ptr(y), _lib.ptr(dy), _lib.ptr(m["lens"]), _lib.ptr(dx),
                                                     *geom, _lib.stream_ptr()), "ms_maskconv_backward_data")
            dx = dx.to(x_like.dtype).reshape(x_like.shape)
        want_db = b_like is not None and need[7]
        if need[6] or want_db:
            dw = torch.empty_like(w)
            db = torch.empty(cout, dtype=torch.float32, device="cuda") if want_db else None
            nbytes = lib.ms_maskconv_backward_workspace_bytes(n, cin, cout, fout, tout, kf, kt)
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")                      # transient
            _lib.check(lib.ms_maskconv_backward_weight(_lib.ptr(x), _lib.ptr(y), _lib.ptr(dy), _lib.ptr(m["lens"]), _lib.ptr(dw),
                                                       _lib.ptr(db), *geom, _lib.ptr(ws), nbytes, _lib.stream_ptr()),
                       "ms_maskconv_backward_weight")
            dw = dw.to(w_like.dtype).reshape(w_like.shape) if need[6] else None
            db = db.to(b_like.dtype).reshape(b_like.shape) if want_db else None
        return None, None, None, None, None, dx, dw, db


def maskconv_train(module, x: Tuple[torch.Tensor, torch.Tensor], clamp: Optional[Tuple[float, float]] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``module((acts, lens), fused_activation=clamp)`` for a ``MaskConv1d`` / ``MaskConv2d`` as an autograd node on the device:
    the same output bits, differentiable in acts, weight and bias; acts is left as the caller gave it."""
    if not isinstance(module, (MaskConv1d, MaskConv2d)):
        raise ValueError(f"maskconv_train serves MaskConv1d / MaskConv2d, not {type(module).__name__}")
    if module.groups != 1:
        raise ValueError("maskconv_train does not serve groups != 1 (grouped convolutions have no backward in this project)")
    if clamp is not None and not clamp[0] < clamp[1]:
        raise ValueError(f"maskconv_train needs lo < hi, got {clamp}")
    acts, seq_lens = x
    one_d = isinstance(module, MaskConv1d)
    if acts.dim() != (3 if one_d else 4) or acts.shape[1] != module.in_channels or min(acts.shape) <= 0:
        raise ValueError(f"the input must be [batch, {module.in_channels}, {'' if one_d else 'features, '}seq_len], got "
                         f"{tuple(acts.shape)}")
    _lib.require_gpu()
    if one_d:
        y, new_lens = _MaskConvFunction.apply(module, seq_lens, (1, module.stride[0]), (1, module.dilation[0]), clamp,
                                              acts.unsqueeze(2), module.weight.unsqueeze(2), module.bias)
        return y.squeeze(2), new_lens
    return _MaskConvFunction.apply(module, seq_lens, _pair(module.stride), _pair(module.dilation), clamp, acts, module.weight,
                                   module.bias)


class _LookaheadFunction(torch.autograd.Function):
    """(x [T, N, F], weight [F, 1, ctx]) -> y [N, T, F] = clamp(lookahead(x))."""

    @staticmethod
    def forward(ctx, clamp, x_tnf, weight):
        x = _lib.f32c(x_tnf.detach())
        t, n, f = x.shape
        w = _lib.f32c(weight.detach()).reshape(f, -1)
        y = lookahead_apply(x, w, (f, 1, n * f), n, f, t, out_layout="ntf", clamp=clamp)
        ctx.save_for_backward(x, w, y)
        ctx.clamp = clamp
        ctx.like = (x_tnf, weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        x_like, w_like = ctx.like
        t, n, f = x.shape
        a, lo, hi = _act_args(ctx.clamp)
        dy = _lib.f32c(dy)
        dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[2] else None
        if dx is not None or dw is not None:
            _lib.check(_lib.load().ms_lookahead_backward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(y), _lib.ptr(dy), _lib.ptr(dx),
                                                         _lib.ptr(dw), n, f, t, w.shape[1], f, 1, n * f, t * f, 1, f, a, lo, hi,
                                                         _lib.stream_ptr()), "ms_lookahead_backward")
        return (None, None if dx is None else dx.to(x_like.dtype).reshape(x_like.shape),
                None if dw is None else dw.to(w_like.dtype).reshape(w_like.shape))


def lookahead_train(module: Lookahead, x_tnf: torch.Tensor, clamp: Optional[Tuple[float, float]] = None) -> torch.Tensor:
    """x_tnf [T, N, F] (the recurrent stack's output) -> ``[N, T, F]`` = clamp(lookahead(x)), ``lookahead_apply(...,
    out_layout="ntf")``'s bits, differentiable in x_tnf and ``module.weight``."""
    if not isinstance(module, Lookahead):
        raise ValueError(f"lookahead_train serves Lookahead, not {type(module).__name__}")
    if x_tnf.dim() != 3 or x_tnf.shape[2] != module.in_features or min(x_tnf.shape) <= 0:
        raise ValueError(f"the input must be [seq_len, batch, {module.in_features}], got {tuple(x_tnf.shape)}")
    if clamp is not None and not clamp[0] < clamp[1]:
        raise ValueError(f"lookahead_train needs lo < hi, got {clamp}")
    _lib.require_gpu()
    return _LookaheadFunction.apply(clamp, x_tnf, module.weight)
