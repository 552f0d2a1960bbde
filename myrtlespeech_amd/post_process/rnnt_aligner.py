"""Transducer (RNN-T) forced alignment: at which frame each label of a KNOWN transcript is emitted.

``RNNTForcedAligner(blank)((logits[N, T, U + 1, V + 1], logit_lens), (y[N, U], y_lens))`` is called like ``RNNTLoss`` and runs
``ms_rnnt_align`` (the Viterbi form of the transducer recursion, back-trace and read-out on the device; the specification is
the comment on ``ms_rnnt_align`` in include/ms_hotpath.h).  It returns one :class:`RNNTAlignment` per utterance, ``None`` where
the transcript cannot be aligned.  ``RNNT.align`` (model/rnnt.py) gives the same for a model without the logit lattice
(``ms_rnnt_align_joint``).  Tokens are ``ctc_aligner.TokenSpan(label, frame, frame + 1, log_prob)`` -- a transducer emits a
label AT a frame -- so ``ctc_aligner.words`` groups them into timed words unchanged.  The reference has no aligner.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from myrtlespeech_amd import _lib
from myrtlespeech_amd.post_process.ctc_aligner import TokenSpan

MS_RNNT_LOG_PROBS_IN = 2
# include/ms_hotpath.h MS_RNNT_ALIGN_BP_LDS_BYTES: the back-pointer rows of a launch stay in LDS up to this size
BACKPOINTER_LDS_BYTES = 96 * 1024


def backpointer_bytes(seq_len: int, u1: int) -> int:
    """Bytes of one utterance's back-pointers: one 64-bit word per 64 values of u and anti-diagonal t + u."""
    return (seq_len + u1 - 1) * ((u1 + 63) // 64) * 8


def backpointers_in_lds(seq_len: int, u1: int) -> bool:
    """Where a launch of ``ms_rnnt_align`` / ``ms_rnnt_align_joint`` keeps its back-pointers: LDS (True) or the workspace."""
    return backpointer_bytes(seq_len, u1) <= BACKPOINTER_LDS_BYTES


@dataclass
class RNNTAlignment:
    score: float                                                 # log-probability of the best path
    tokens: List[TokenSpan] = field(default_factory=list)        # label u: emitted at frame ``start`` (``end`` = start + 1)
    frame_labels: List[List[int]] = field(default_factory=list)  # the labels emitted at each frame, in order
    frame_log_probs: List[float] = field(default_factory=list)   # each frame's blank log-probability on the path


def validate_labels(targets: torch.Tensor, yl: torch.Tensor, symbols: int, blank: int) -> List[List[int]]:
    """The labels of every utterance as host lists; a label outside [0, symbols) or equal to the blank is the caller's mistake
    (the kernel would report "no alignment", which would hide it)."""
    y_host = targets.detach().to("cpu", torch.int64)
    labels = [y_host[n, :int(l)].tolist() for n, l in enumerate(yl.tolist())]
    for n, lab in enumerate(labels):
        for v in lab:
            if not 0 <= v < symbols or v == blank:
                raise ValueError(f"utterance {n}: target label {v} must be in [0, {symbols}) and differ from the blank ({blank})")
    return labels


def output_buffer(n: int, t: int, u1: int):
    """Every result in one buffer, so that one copy reads it back: score [N] | token_frame, token_logp [N, U] | frame_u,
    frame_logp [N, T].  Returns the buffer, its five views and their sizes."""
    sizes = [n, n * (u1 - 1), n * (u1 - 1), n * t, n * t]
    out = torch.empty(sum(sizes), dtype=torch.int32, device="cuda")
    return out, torch.split(out, sizes), sizes


def read_back(out: torch.Tensor, sizes, labels, xl_list, n: int, t: int, u1: int, who: str) -> List[Optional[RNNTAlignment]]:
    """ONE device -> host copy, then the per-utterance records."""
    host = out.cpu().numpy()
    starts = [sum(sizes[:i]) for i in range(len(sizes))]
    h_score, h_tf, h_tl, h_fu, h_fl = (host[a:a + s] for a, s in zip(starts, sizes))
    h_score = h_score.view("float32")
    h_tf, h_tl = h_tf.reshape(n, u1 - 1), h_tl.view("float32").reshape(n, u1 - 1)
    h_fu, h_fl = h_fu.reshape(n, t), h_fl.view("float32").reshape(n, t)
    result: List[Optional[RNNTAlignment]] = []
    for i, lab in enumerate(labels):
        sc = float(h_score[i])
        if math.isnan(sc):
            raise RuntimeError(f"{who}: utterance {i} has a non-finite value in one of its {xl_list[i]} x {len(lab) + 1} cells "
                               "(a NaN or +inf input, or a cell whose log-softmax normaliser is not finite)")
        if sc == -math.inf:
            result.append(None)
            continue
        tn = xl_list[i]
        tokens = [TokenSpan(v, int(h_tf[i, u]), int(h_tf[i, u]) + 1, float(h_tl[i, u])) for u, v in enumerate(lab)]
        counts = h_fu[i, :tn].tolist()
        frame_labels = [lab[(counts[f - 1] if f else 0):counts[f]] for f in range(tn)]
        result.append(RNNTAlignment(sc, tokens, frame_labels, h_fl[i, :tn].tolist()))
    return result


class RNNTForcedAligner(torch.nn.Module):
    """Best path of a given transcript through a transducer's lattice.

    ``logits`` [N, T, U + 1, V + 1] holds the joint network's outputs (the device applies its log-softmax over the symbols)
    or, with ``log_probs=True``, log-probabilities that are used exactly as given (``-inf`` = impossible).  One staged upload
    of the host-side integers, two launches, one read-back."""

    def __init__(self, blank: int, log_probs: bool = False):
        super().__init__()
        if int(blank) < 0:
            raise ValueError(f"blank={blank} must be >= 0")
        self.blank = int(blank)
        self.log_probs = bool(log_probs)
        self._workspace = _lib.Workspace()

    def extra_repr(self) -> str:
        return f"blank={self.blank}, log_probs={self.log_probs}"

    def forward(self, inputs: Tuple[torch.Tensor, torch.Tensor], targets: Tuple[torch.Tensor, torch.Tensor]
                ) -> List[Optional[RNNTAlignment]]:
        from myrtlespeech_amd.loss.rnnt_loss import check_score_shapes
        x, x_lens = inputs
        y, y_lens = targets
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise ValueError("logits must be [batch, max_seq_len, max_target_len + 1, symbols]")
        n, t, u1, v1 = x.shape
        blank = self.blank
        xl, yl = check_score_shapes(t, n, u1, 1, v1, x_lens, y, y_lens, blank)   # (1: there are no joint features to check)
        labels = validate_labels(y, yl, v1, blank)
        _lib.require_gpu()
        lib = _lib.load()
        xd = _lib.f32c(x.detach())
        # ONE staged upload for what starts on the host (RNNTLoss.forward)
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
        out, (score, t_frame, t_logp, f_u, f_logp), sizes = output_buffer(n, t, u1)
        nbytes = lib.ms_rnnt_align_workspace_bytes(n, t, u1, v1)
        ws = self._workspace.get(nbytes, zero=False)
        has_tokens = u1 > 1
        _lib.check(lib.ms_rnnt_align(_lib.ptr(xd), _lib.ptr(xl_dev), _lib.ptr(y_dev), _lib.ptr(yl_dev), _lib.ptr(score),
                                     _lib.ptr(t_frame if has_tokens else None), _lib.ptr(t_logp if has_tokens else None),
                                     _lib.ptr(f_u), _lib.ptr(f_logp), n, t, u1, v1, blank,
                                     MS_RNNT_LOG_PROBS_IN if self.log_probs else 0, _lib.ptr(ws), ws.numel(),
                                     _lib.stream_ptr()), "ms_rnnt_align")
        return read_back(out, sizes, labels, xl.tolist(), n, t, u1, "RNNTForcedAligner")
