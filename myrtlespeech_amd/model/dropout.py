"""Dropout on the device -- this repository's OWN specification (the comment on ``ms_dropout_forward`` in include/ms_hotpath.h;
tests/dropout_ref.py restates it in numpy).

A mask is a pure function of ``(seed, offset, element index, p)``: Philox4x32-10 keyed on the seed, counted by the element's
quad and the call's offset, an element kept iff its 32-bit word is at or above ``ceil(p * 2^32)``.  Nothing is stored and the
device holds no generator state: a backward calls the same kernel with the same four numbers.  What a model needs from the host
is therefore two integers, and ``DropoutGenerator`` is exactly that: ``(seed, offset)``, one offset handed out per dropout
application.

Opt-in: every differentiable entry keeps refusing ``Dropout(p > 0)`` in training mode (earlier tests pin those refusals) unless
a generator is attached -- ``attach(seq_to_seq.model, DropoutGenerator(seed))`` is the one line in front of ``fit()``.  No
builder attaches one.  The state is no ``Module``, parameter or buffer: model ``state_dict`` keys stay as they are, and a
checkpoint that wants the mask stream stores ``generator.state_dict()`` beside the model's.
"""
import ctypes
import math
from fractions import Fraction
from typing import Dict, Tuple

import torch
from torch.autograd.function import once_differentiable

from myrtlespeech_amd import _lib

_U64 = (1 << 64) - 1

# (thr, scale, seed, offset): everything a kernel needs to remake one application's mask
DropoutCall = Tuple[int, float, int, int]


def threshold(p: float) -> int:
    """``ceil(p * 2^32)`` in exact integer arithmetic from the float ``p`` (0 < p <= 1): an element is kept iff its word >= this."""
    p = float(p)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"dropout probability must be in (0, 1], got {p}")
    return math.ceil(Fraction(p) * (1 << 32))


def scale_of(p: float) -> float:
    """``float32(1 / (1 - p))``, formed in double and rounded once; 0 for p == 1 (nothing is kept)."""
    p = float(p)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"dropout probability must be in (0, 1], got {p}")
    return 0.0 if p == 1.0 else ctypes.c_float(1.0 / (1.0 - p)).value


class DropoutGenerator:
    """Host-side ``(seed, offset)``.  ``next_offset()`` returns the current offset and advances it by 1: one offset per dropout
    application, so two applications never share a counter whatever their sizes."""

    def __init__(self, seed: int = 0):
        self.manual_seed(seed)

    def manual_seed(self, seed: int) -> "DropoutGenerator":
        self.seed = int(seed) & _U64
        self.offset = 0
        return self

    def next_offset(self) -> int:
        offset = self.offset
        self.offset = (offset + 1) & _U64
        return offset

    def state_dict(self) -> Dict[str, int]:
        return {"seed": self.seed, "offset": self.offset}

    def load_state_dict(self, state: Dict[str, int]) -> None:
        self.seed = int(state["seed"]) & _U64
        self.offset = int(state["offset"]) & _U64

    def __repr__(self):
        return f"DropoutGenerator(seed={self.seed}, offset={self.offset})"


def dropout_call(p: float, generator: DropoutGenerator) -> DropoutCall:
    """The numbers of the NEXT application of ``Dropout(p)``: consumes one offset of ``generator``."""
    if not isinstance(generator, DropoutGenerator):
        raise ValueError(f"a DropoutGenerator is needed, got {type(generator).__name__}")
    thr, scale = threshold(p), scale_of(p)
    return thr, scale, generator.seed, generator.next_offset()


def attach(module: torch.nn.Module, generator: DropoutGenerator) -> torch.nn.Module:
    """Sets ``dropout_generator`` on every ``DeepSpeech1``, ``DeepSpeech2``, ``RNN`` and ``FullyConnected`` under ``module`` (itself
    included); ``None`` detaches.  Returns ``module``."""
    from myrtlespeech_amd.model.deep_speech_1 import DeepSpeech1
    from myrtlespeech_amd.model.deep_speech_2 import DeepSpeech2
    from myrtlespeech_amd.model.fully_connected import FullyConnected
    from myrtlespeech_amd.model.rnn import RNN
    if generator is not None and not isinstance(generator, DropoutGenerator):
        raise ValueError(f"a DropoutGenerator is needed, got {type(generator).__name__}")
    for m in module.modules():
        if isinstance(m, (DeepSpeech1, DeepSpeech2, RNN, FullyConnected)):
            m.dropout_generator = generator
    return module


def apply_mask(src: torch.Tensor, dst: torch.Tensor, call: DropoutCall) -> torch.Tensor:
    """``dst = src * m(call)`` on the device (``ms_dropout_forward``); both float32, contiguous, of one size; dst may be src."""
    thr, scale, seed, offset = call
    _lib.check(_lib.load().ms_dropout_forward(_lib.ptr(src), _lib.ptr(dst), src.numel(), thr, scale, seed, offset, _lib.stream_ptr()),
               "ms_dropout_forward")
    return dst


class _DropoutFunction(torch.autograd.Function):
    """out = x * m; backward dx = dy * m through the same kernel.  Saves the call's four numbers and no tensor."""

    @staticmethod
    def forward(ctx, x, call):
        ctx.call = call
        ctx.like = x
        xd = _lib.f32c(x.detach())
        return apply_mask(xd, torch.empty_like(xd), call)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dy = _lib.f32c(dy)
        dx = apply_mask(dy, torch.empty_like(dy), ctx.call)
        return dx.to(device=ctx.like.device, dtype=ctx.like.dtype).reshape(ctx.like.shape), None


def dropout_train(x: torch.Tensor, p: float, generator: DropoutGenerator) -> torch.Tensor:
    """``Dropout(p)`` in training mode on ``x`` (any shape; the mask is indexed over the contiguous array) as an autograd node on
    the device.  Consumes one offset.  ValueError, before a device is needed, for p outside (0, 1] or a missing generator."""
    threshold(p)
    if not isinstance(generator, DropoutGenerator):
        raise ValueError(f"a DropoutGenerator is needed, got {type(generator).__name__}")
    _lib.require_gpu()      # (before the offset is taken: a call that cannot run consumes none)
    return _DropoutFunction.apply(x, dropout_call(p, generator))
