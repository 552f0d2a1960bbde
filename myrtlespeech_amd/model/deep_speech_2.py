"""Deep Speech 2 composition: mirror of myrtlespeech/model/deep_speech_2.py.

``DeepSpeech2(cnn, rnn, lookahead, fully_connected)`` takes the same sub-modules
the reference's builder assembles (builders/deep_speech_2.py:105-221) and returns
``((logits[T,N,V], lens), hid)``.  The forward pass keeps every tensor on the GPU
and fuses what the reference does as separate torch ops:

* ``MaskConv -> SeqLenWrapper(Hardtanh/ReLU)`` pairs run as one conv kernel with
  the clamp in its epilogue;
* ``(N,C,F,T) -> (T,N,C*F)`` is one tiled transpose kernel;
* the fully connected stack consumes the RNN output in its native ``[T,N,F]``
  order (rows are independent), so neither ``transpose(0, 1)`` is materialised;
* the lookahead kernel reads ``[T,N,F]`` through strides.
"""
from typing import Optional, Tuple

import torch

from myrtlespeech_amd import _lib
from myrtlespeech_amd.model.cnn import Conv1dTo2d, Conv2dTo1d, MaskConv1d, MaskConv2d, conv_pair_forward
from myrtlespeech_amd.model.fully_connected import FullyConnected, linear_stack_plan, run_linear_stack
from myrtlespeech_amd.model.lookahead import Lookahead, lookahead_apply
from myrtlespeech_amd.model.rnn import RNNState
from myrtlespeech_amd.model.seq_len_wrapper import SeqLenWrapper
from myrtlespeech_amd.model.utils import activation_clamp


def _is_plain_activation(m) -> bool:
    return (isinstance(m, SeqLenWrapper) and isinstance(m.module, (torch.nn.Hardtanh, torch.nn.ReLU, torch.nn.Identity))
            and isinstance(m.seq_lens_fn, torch.nn.Identity))


def _is_plain_clamp(m) -> bool:
    return _is_plain_activation(m) and isinstance(m.module, (torch.nn.Hardtanh, torch.nn.ReLU))


class DeepSpeech2(torch.nn.Module):
    """`Deep Speech 2 <http://proceedings.mlr.press/v48/amodei16.pdf>`_
    (deep_speech_2.py:8-172); argument contract as in the reference."""

    dropout_generator = None      # opt-in (model/dropout.py: attach); no Module, parameter or buffer; no builder sets it

    def __init__(self, cnn: Optional[torch.nn.Module], rnn: torch.nn.Module, lookahead: Optional[torch.nn.Module],
                 fully_connected: torch.nn.Module):
        super().__init__()
        self.cnn = cnn
        self.rnn = rnn
        self.lookahead = lookahead
        self.fully_connected = fully_connected
        self.use_cuda = torch.cuda.is_available()
        if self.use_cuda:
            self.cuda()

    # ------------------------------------------------------------------ stages
    def _run_cnn(self, h):
        mods = list(self.cnn) if isinstance(self.cnn, torch.nn.Sequential) else [self.cnn]
        i = 0
        while i < len(mods):
            m = mods[i]
            if (isinstance(m, MaskConv2d) and i + 2 < len(mods) and _is_plain_clamp(mods[i + 1])
                    and isinstance(mods[i + 2], MaskConv2d)):
                # conv -> clamp -> conv (DS2's front end): the first hands the second its operand planes where the kernels allow
                act2 = i + 3 < len(mods) and _is_plain_activation(mods[i + 3])
                out = conv_pair_forward(m, activation_clamp(mods[i + 1].module), mods[i + 2],
                                        activation_clamp(mods[i + 3].module) if act2 else None, h)
                if out is not None:
                    h = out
                    i += 4 if act2 else 3
                    continue
            if isinstance(m, (MaskConv1d, MaskConv2d)) and i + 1 < len(mods) and _is_plain_activation(mods[i + 1]):
                h = m(h, fused_activation=activation_clamp(mods[i + 1].module))
                i += 2
            else:
                h = m(h)
                i += 1
        return h

    @staticmethod
    def _conv_to_rnn_size(x: torch.Tensor) -> torch.Tensor:
        """(batch, chnls, feature, seq_len) -> (seq_len, batch, chnls*feature), deep_speech_2.py:114-117."""
        n, c, f, t = x.shape
        x = _lib.f32c(x)
        y = torch.empty((t, n, c * f), dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().ms_nct_to_tnc(_lib.ptr(x), _lib.ptr(y), n, c * f, t, _lib.stream_ptr()), "ms_nct_to_tnc")
        return y

    def _run_lookahead_ntf(self, h_tnf: torch.Tensor):
        """[T,N,F] RNN output -> lookahead (+activation) -> [N,T,F], or None if the
        lookahead module is not the builder's Sequential(Lookahead, SeqLenWrapper(act))."""
        la = self.lookahead
        mods = list(la) if isinstance(la, torch.nn.Sequential) else [la]
        if not isinstance(mods[0], Lookahead) or len(mods) > 2:
            return None
        clamp = None
        if len(mods) == 2:
            if not _is_plain_activation(mods[1]):
                return None
            clamp = activation_clamp(mods[1].module)
        t, n, f = h_tnf.shape
        return lookahead_apply(h_tnf, mods[0].weight, (f, 1, n * f), n, f, t, out_layout="ntf", clamp=clamp)

    # ------------------------------------------------------------------ forward
    def forward(self, x: Tuple[torch.Tensor, torch.Tensor], hx: Optional[RNNState] = None, differentiable: bool = False
                ) -> Tuple[Tuple[torch.Tensor, torch.Tensor], RNNState]:
        """``differentiable=True``: the same chain as autograd nodes on the device (``model/conv_autograd.py``,
        ``model/rnn_autograd.py``), so ``CTCLoss()((out, lens), (y, y_lens)).backward()`` fills the gradient of every parameter
        and of ``hx``; the input features are data and get none.  ValueError, before a device is needed, for what has no
        backward here: ``HardLSTM`` stacks unless ``self.rnn.hard_backward = True``, GRU / tanh stacks unless
        ``self.rnn.gru_backward = True`` (the opt-in switch of ``RNN``: fine-tuning the shipped GRU configuration is that one line), dropout in training mode with no ``DropoutGenerator``
        attached (``model/dropout.py``: ``attach(model, generator)`` sets ``self.dropout_generator``, which serves the
        ``FullyConnected``'s ``Dropout`` modules, and ``self.rnn.dropout_generator``, which serves the inter-layer dropout; the
        recurrent stack takes its offsets first), ``groups > 1``, and a ``cnn`` or ``lookahead`` holding modules other than the
        builder's own.  The default path is untouched."""
        if differentiable:
            return self._forward_train(x, hx)
        return self.back(self.front(x), hx)

    def _train_plan(self):
        """The differentiable chain, vetted without a device: ([(conv, clamp) | view module, ...], (Lookahead, clamp) | None)."""
        from myrtlespeech_amd.model.hard_lstm import HardLSTM
        from myrtlespeech_amd.model.rnn import RNN, RNNType
        what = "DeepSpeech2.forward(differentiable=True)"
        rnn, fc = self.rnn, self.fully_connected
        # (GRU and tanh stacks pass with the stack's opt-in switch on: RNN.forward then sends them to gru_train; a HardLSTM
        # with its own, ``hard_backward``: HardLSTM.forward sends it to hard_lstm_train -- it has no dropout to vet)
        hard = isinstance(rnn, HardLSTM) and rnn.hard_backward
        if not hard and (not isinstance(rnn, RNN) or (rnn.rnn_type != RNNType.LSTM and not rnn.gru_backward)):
            raise ValueError(f"{what} serves LSTM stacks only (GRU and tanh cells and HardLSTM have no backward in this project)")
        if rnn.batch_first:
            raise ValueError(f"{what} takes a time-major recurrent stack (batch_first=False), as the builder makes it")
        # (dropout is opt-in: served where a DropoutGenerator is attached -- model/dropout.py -- and refused as ever where not)
        if not hard and rnn.training and rnn.rnn.dropout > 0 and rnn.rnn.num_layers > 1 and rnn.dropout_generator is None:
            raise ValueError(f"{what} does not serve inter-layer dropout in training mode")
        if not isinstance(fc, FullyConnected):
            raise ValueError(f"{what} serves the builder's FullyConnected, not {type(fc).__name__}")
        fc_mods = [fc.fully_connected] if isinstance(fc.fully_connected, torch.nn.Linear) else list(fc.fully_connected)
        if (fc.training and any(isinstance(m, torch.nn.Dropout) and m.p > 0 for m in fc_mods)
                and self.dropout_generator is None):
            raise ValueError(f"{what} does not serve dropout masks: train in .eval() or with dropout = 0")
        front = []
        mods = [] if self.cnn is None else (list(self.cnn) if isinstance(self.cnn, torch.nn.Sequential) else [self.cnn])
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, (MaskConv1d, MaskConv2d)):
                if m.groups != 1:
                    raise ValueError(f"{what} does not serve convolutions with groups != 1")
                fused = i + 1 < len(mods) and _is_plain_activation(mods[i + 1])
                front.append((m, activation_clamp(mods[i + 1].module) if fused else None))
                i += 2 if fused else 1
            elif _is_plain_activation(m) and isinstance(m.module, torch.nn.Identity):
                i += 1
            elif isinstance(m, (Conv1dTo2d, Conv2dTo1d)) and m.seq_len_support:
                front.append(m)
                i += 1
            else:
                raise ValueError(f"{what} serves a cnn of MaskConv1d / MaskConv2d, each optionally followed by SeqLenWrapper of "
                                 f"Hardtanh / ReLU / Identity, Conv1dTo2d and Conv2dTo1d; found {type(m).__name__} at {i}")
        la = None
        if self.lookahead is not None:
            lmods = list(self.lookahead) if isinstance(self.lookahead, torch.nn.Sequential) else [self.lookahead]
            if not (1 <= len(lmods) <= 2 and isinstance(lmods[0], Lookahead) and all(_is_plain_activation(m) for m in lmods[1:])):
                raise ValueError(f"{what} serves a lookahead of Lookahead or Sequential(Lookahead, SeqLenWrapper(activation))")
            la = (lmods[0], activation_clamp(lmods[1].module) if len(lmods) == 2 else None)
        return front, la

    def _forward_train(self, x: Tuple[torch.Tensor, torch.Tensor], hx: Optional[RNNState]):
        """``forward`` as a chain of autograd nodes: one node per convolution with its clamp fused (no planes hand-over pair),
        the (N,C,F,T) -> (T,N,C*F) re-layout as torch ops autograd sees, ``rnn_train``, ``lookahead_train`` and
        ``linear_stack_train``."""
        from myrtlespeech_amd.model.conv_autograd import lookahead_train, maskconv_train
        from myrtlespeech_amd.model.rnn_autograd import linear_stack_train
        front, la = self._train_plan()
        acts, lens = x
        if acts.dim() not in (3, 4) or min(acts.shape) <= 0:
            raise ValueError(f"the input must be [batch, channels, features, seq_len], got {tuple(acts.shape)}")
        _lib.require_gpu()
        h = (_lib.f32c(acts.detach()), lens)
        for step in front:
            h = maskconv_train(step[0], h, step[1]) if isinstance(step, tuple) else step(h)
        seq, lens = h
        if seq.dim() != 4:
            raise ValueError(f"the cnn must end on [batch, channels, features, seq_len], got {tuple(seq.shape)}")
        n, c, f, t = seq.shape
        seq = seq.reshape(n, c * f, t).permute(2, 0, 1).contiguous()
        (seq, lens), hid = self.rnn((seq, lens), hx, differentiable=True)
        t, n, f = seq.shape
        fc, gen = self.fully_connected, self.dropout_generator
        if la is not None:
            ntf = lookahead_train(la[0], seq.contiguous(), la[1])
            out = linear_stack_train(ntf.reshape(n * t, f), fc.fully_connected, fc.training, gen).reshape(n, t, -1).transpose(0, 1)
        else:
            out = linear_stack_train(seq.reshape(t * n, f), fc.fully_connected, fc.training, gen).reshape(t, n, -1)
        return (out, _lib.lens_to_device(lens)), hid

    def front(self, x: Tuple[torch.Tensor, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        """The part of ``forward`` that depends on the input only: convolutions and the (N,C,F,T) -> (T,N,C*F) re-layout
        (deep_speech_2.py:150-157).  ``forward(x, hx) == back(front(x), hx)``; a pipeline may run ``front`` of a later batch
        on another stream while an earlier batch is in its recurrent layers (``pipeline.BatchesInFlight``)."""
        _lib.require_gpu()
        h = (x[0].cuda() if not x[0].is_cuda else x[0], x[1])
        if self.cnn is not None:
            h = self._run_cnn(h)
        return self._conv_to_rnn_size(h[0]), h[1]

    def back(self, h: Tuple[torch.Tensor, torch.Tensor], hx: Optional[RNNState] = None
             ) -> Tuple[Tuple[torch.Tensor, torch.Tensor], RNNState]:
        """Recurrent layers, lookahead and fully-connected layers on the output of ``front`` (deep_speech_2.py:158-172)."""
        return self.output(*self.recurrent(h, hx))

    def recurrent(self, h: Tuple[torch.Tensor, torch.Tensor], hx: Optional[RNNState] = None):
        """The recurrent stack on the output of ``front``: ``(seq [T, N, D*H], lens, hid)``."""
        _lib.at_issue_point()
        h, hid = self.rnn(h, hx=hx)
        _lib.at_issue_point()
        return h[0], h[1], hid

    def output(self, seq: torch.Tensor, lens: torch.Tensor, hid: RNNState
               ) -> Tuple[Tuple[torch.Tensor, torch.Tensor], RNNState]:
        """Lookahead and fully-connected layers on the recurrent stack's output (the part of ``forward`` that a pipeline may
        issue late: nothing of the NEXT batch depends on it)."""
        fc = self.fully_connected
        fused_fc = isinstance(fc, FullyConnected)
        if self.lookahead is not None:
            ntf = self._run_lookahead_ntf(seq) if seq.is_contiguous() else None
            if ntf is None:  # foreign lookahead module: follow the reference's permutes literally
                la_out, lens = self.lookahead((seq.permute(1, 2, 0), lens))
                ntf = la_out.transpose(1, 2)
            out, lens = fc((ntf, lens))
            return (out.transpose(0, 1), lens), hid
        if fused_fc:
            t, n, f = seq.shape
            y = run_linear_stack(_lib.f32c(seq).reshape(t * n, f), linear_stack_plan(fc.fully_connected, fc.training))
            return (y.reshape(t, n, -1), _lib.lens_to_device(lens)), hid
        out, lens = fc((seq.transpose(0, 1), lens))
        return (out.transpose(0, 1), lens), hid
