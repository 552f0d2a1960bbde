"""CTC forced alignment: where each label -- and each word -- of a KNOWN transcript lies in the audio.

``CTCForcedAligner(blank)(x[T,N,V], lengths, targets, target_lengths)`` runs ``ms_ctc_align`` (the Viterbi form of the CTC
recursion, back-trace and token spans on the device; the specification is the comment on ``ms_ctc_align`` in
include/ms_hotpath.h) and returns one :class:`Alignment` per utterance, ``None`` where the transcript cannot be aligned.
``words`` groups an alignment's tokens into words.  The reference has no aligner.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from myrtlespeech_amd import _lib
from myrtlespeech_amd.post_process._common import check_decoder_args

MS_CTC_LOG_PROBS_IN = 2
# include/ms_hotpath.h MS_CTC_ALIGN_BP_LDS_BYTES: the back-pointer rows of a launch stay in LDS up to this size
BACKPOINTER_LDS_BYTES = 96 * 1024


def backpointer_row_bytes(max_target_length: int) -> int:
    """Bytes of one frame's back-pointers: two 64-bit planes per 64 of the 2 L_max + 1 states."""
    return 16 * ((2 * max_target_length + 1 + 63) // 64)


def backpointers_in_lds(seq_len: int, max_target_length: int) -> bool:
    """Where a launch of ``ms_ctc_align`` keeps its back-pointers: LDS (True) or the global workspace."""
    return seq_len * backpointer_row_bytes(max_target_length) <= BACKPOINTER_LDS_BYTES


@dataclass
class TokenSpan:
    """One label of the transcript: frames ``start .. end - 1`` and the sum of its log-probabilities over them."""
    label: int
    start: int
    end: int
    log_prob: float

    @property
    def confidence(self) -> float:
        """Geometric mean of the label's per-frame probabilities."""
        return math.exp(self.log_prob / (self.end - self.start))


@dataclass
class Alignment:
    score: float                 # log-probability of the best path
    frames: List[int]            # the label of every frame, blank included
    tokens: List[TokenSpan] = field(default_factory=list)


@dataclass
class WordSpan:
    """A maximal run of non-separator tokens: ``start`` is its first token's, ``end`` its last token's (exclusive)."""
    labels: List[int]
    start: int
    end: int
    log_prob: float              # the sum of its tokens', in float64
    confidence: float            # exp(log_prob / frames its tokens occupy)
    start_s: Optional[float] = None
    end_s: Optional[float] = None


def words(alignment: Alignment, separator_index: int, frame_seconds: Optional[float] = None) -> List[WordSpan]:
    """Words of an alignment: maximal runs of tokens other than ``separator_index`` (separators belong to no word).
    ``frame_seconds`` -- the duration of one frame of ``x``, i.e. the caller's knowledge of the stride of their
    convolution stack -- adds ``start_s`` / ``end_s``."""
    out, run = [], []

    def close():
        if not run:
            return
        log_prob = math.fsum(float(tok.log_prob) for tok in run)
        n_frames = sum(tok.end - tok.start for tok in run)
        w = WordSpan([tok.label for tok in run], run[0].start, run[-1].end, log_prob, math.exp(log_prob / n_frames))
        if frame_seconds is not None:
            w.start_s, w.end_s = w.start * frame_seconds, w.end * frame_seconds
        out.append(w)
        run.clear()

    for tok in alignment.tokens:
        if tok.label == separator_index:
            close()
        else:
            run.append(tok)
    close()
    return out


class CTCForcedAligner(torch.nn.Module):
    """Best path of a given transcript through CTC scores.

    ``x`` [T, N, V] holds logits (the device applies its log-softmax over the symbols) or, with ``log_probs=True``,
    log-probabilities that are used exactly as given (``-inf`` = impossible).  ``targets`` is padded [N, S] or 1-D
    concatenated, as ``CTCLoss`` takes them.  One staged upload of the host-side integers, two launches, one read-back."""

    def __init__(self, blank_index: int, log_probs: bool = False):
        super().__init__()
        if blank_index < 0:
            raise ValueError(f"blank_index={blank_index} must be >= 0")
        self.blank_index = blank_index
        self.log_probs = bool(log_probs)
        self._workspace = _lib.Workspace()

    def forward(self, x: torch.Tensor, lengths: torch.Tensor, targets: torch.Tensor, target_lengths: torch.Tensor
                ) -> List[Optional[Alignment]]:
        if x.dim() != 3:
            raise ValueError("x must be [seq_len, batch, symbols]")
        seq_len, batch, symbols = check_decoder_args(x, lengths)
        blank = self.blank_index
        if blank >= symbols:
            raise ValueError(f"blank_index={blank} must be less than the number of symbols ({symbols})")
        if targets.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
            raise ValueError(f"targets.dtype={targets.dtype} must be an integer type")
        if target_lengths.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
            raise ValueError(f"target_lengths.dtype={target_lengths.dtype} must be an integer type")
        xl = _lib.host_lens(lengths)
        yl = target_lengths.detach().to("cpu", torch.int64)
        if yl.numel() != batch:
            raise ValueError(f"batch size of x ({batch}) and target_lengths {yl.numel()} must be equal")
        if batch and (int(xl.min()) < 0 or int(yl.min()) < 0):
            raise ValueError("lengths must not be negative")
        # labels are validated on the host (one small copy if they live on the device): the kernel treats a bad label as
        # "no alignment", which would hide the caller's mistake
        y_host = targets.detach().to("cpu", torch.int64)
        if y_host.dim() == 2:
            if y_host.shape[0] != batch:
                raise ValueError(f"batch size of x ({batch}) and targets {y_host.shape[0]} must be equal")
            if batch and int(yl.max()) > y_host.shape[1]:
                raise ValueError("target length exceeds the padded target width")
            offsets = torch.arange(batch, dtype=torch.int64) * y_host.shape[1]
        elif y_host.dim() == 1:
            offsets = torch.cumsum(yl, 0) - yl
            if int(yl.sum()) > y_host.numel():
                raise ValueError("sum(target_lengths) exceeds the number of targets")
        else:
            raise ValueError("targets must be [batch, max_target_len] or 1-D")
        flat = y_host.reshape(-1)
        labels = [flat[o:o + l].tolist() for o, l in zip(offsets.tolist(), yl.tolist())]
        for n, lab in enumerate(labels):
            for v in lab:
                if not 0 <= v < symbols or v == blank:
                    raise ValueError(f"utterance {n}: target label {v} must be in [0, {symbols}) and differ from the blank ({blank})")
        _lib.require_gpu()
        xl_list = xl.tolist()
        if seq_len == 0 or batch == 0:
            # no frames at all: an empty transcript has the empty path (score 0), any other has none
            return [Alignment(0.0, [], []) if not lab else None for lab in labels]
        lib = _lib.load()
        l_max = max(len(lab) for lab in labels)
        xd = _lib.f32c(x)
        # ONE staged upload for everything that starts on the host (CTCLoss.forward does the same)
        host_parts = [xl.to(torch.int32), offsets.to(torch.int32), yl.to(torch.int32)]
        y_on_host = not targets.is_cuda
        if y_on_host and flat.numel():
            host_parts.append(flat.to(torch.int32))
        packed = _lib.upload(torch.cat(host_parts))
        xl_dev, off_dev, yl_dev = packed[:batch], packed[batch:2 * batch], packed[2 * batch:3 * batch]
        if y_on_host and flat.numel():
            y_dev = packed[3 * batch:]
        elif flat.numel():
            y_dev = targets.detach().to(dtype=torch.int32).contiguous().reshape(-1)
        else:
            y_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
        # every result in one buffer: score [N] | frame_state [N, T] | token_start, token_end, token_logp [N, L_max]
        sizes = [batch, batch * seq_len, batch * l_max, batch * l_max, batch * l_max]
        out = torch.empty(sum(sizes), dtype=torch.int32, device="cuda")
        score, frame_state, t_start, t_end, t_logp = torch.split(out, sizes)
        nbytes = lib.ms_ctc_align_workspace_bytes(seq_len, batch, symbols, 2 * l_max + 1)
        ws = self._workspace.get(nbytes, zero=False)
        _lib.check(lib.ms_ctc_align(_lib.ptr(xd), _lib.ptr(xl_dev), _lib.ptr(y_dev), _lib.ptr(off_dev), _lib.ptr(yl_dev),
                                    _lib.ptr(score), _lib.ptr(frame_state), _lib.ptr(t_start), _lib.ptr(t_end),
                                    _lib.ptr(t_logp), seq_len, batch, symbols, l_max, blank,
                                    MS_CTC_LOG_PROBS_IN if self.log_probs else 0, _lib.ptr(ws), ws.numel(),
                                    _lib.stream_ptr()), "ms_ctc_align")
        host = out.cpu().numpy()
        h_score, h_state, h_start, h_end, h_logp = (host[a:a + s] for a, s in zip(_starts(sizes), sizes))
        h_score = h_score.view("float32")
        h_state = h_state.reshape(batch, seq_len)
        h_start, h_end = h_start.reshape(batch, l_max), h_end.reshape(batch, l_max)
        h_logp = h_logp.view("float32").reshape(batch, l_max)
        result: List[Optional[Alignment]] = []
        for n, lab in enumerate(labels):
            sc = float(h_score[n])
            if math.isnan(sc):
                raise RuntimeError(f"CTCForcedAligner: utterance {n} has a non-finite score in one of its {xl_list[n]} frames "
                                   "(a NaN or +inf input, or a frame whose log-softmax normaliser is not finite)")
            if sc == -math.inf:
                result.append(None)
                continue
            states = h_state[n, :xl_list[n]].tolist()
            frames = [lab[s >> 1] if s & 1 else blank for s in states]
            tokens = [TokenSpan(v, int(h_start[n, i]), int(h_end[n, i]), float(h_logp[n, i])) for i, v in enumerate(lab)]
            result.append(Alignment(sc, frames, tokens))
        return result

    def extra_repr(self) -> str:
        return f"blank_index={self.blank_index}, log_probs={self.log_probs}"


def _starts(sizes):
    a = 0
    for s in sizes:
        yield a
        a += s
