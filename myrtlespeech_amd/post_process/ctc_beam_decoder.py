"""CTC prefix beam search: mirror of myrtlespeech/post_process/ctc_beam_decoder.py.

Same constructor checks and ``forward(x, lengths) -> List[List[int]]`` as the
reference.  The search itself (Hannun et al. 2014 prefix beam search in linear
float32 arithmetic, ctc_beam_decoder.py:175-258) runs on the GPU, one workgroup
per utterance, and reproduces the reference's beam bit for bit (visiting order,
Counter merge order, stable sort, float32 rounding).

A ``language_model`` is a host callable, so with one set the kernel is advanced a
frame at a time and the host supplies, per beam entry, the factor
``float32(lm(prefix + (separator,)) ** lm_weight)`` the reference multiplies in at
ctc_beam_decoder.py:222-228; without one the whole utterance is a single launch.

An ``NGramLanguageModel`` (myrtlespeech_amd/language_model.py) is the exception: its table lives in device memory and
the kernel looks the factor up itself, so the decode is a single launch with a model as well.

``range_safe=True`` is the same search with an unbounded exponent (``ms_ctc_beam_decode_ex``): when a frame's best stored
probability falls below 2^-32 every stored probability of the frame is multiplied by one power of two, which is exact and
changes no comparison, and the exponent is kept per utterance.  The transcripts are the reference's wherever its float32
search stays in range, and the beam does not run empty (``[]``) where it underflows.  ``decode_nbest`` returns the whole
final beam with log-probabilities, in either mode.
"""
import ctypes
import math
from typing import Callable, List, NamedTuple, Optional, Tuple

import torch

from myrtlespeech_amd import _lib
from myrtlespeech_amd.language_model import NGramLanguageModel
from myrtlespeech_amd.post_process._common import check_decoder_args, ragged_to_lists


def check_device_language_model(lm: NGramLanguageModel, separator_index: Optional[int], symbols: Optional[int]) -> None:
    """The model's separator and alphabet must be the decoder's / the input's."""
    if separator_index is not None and lm.separator_index != separator_index:
        raise ValueError(f"language_model.separator_index={lm.separator_index} and separator_index={separator_index} differ")
    if symbols is not None and len(lm.alphabet) != symbols:
        raise ValueError(f"language_model has an alphabet of {len(lm.alphabet)} symbols, the input has {symbols}")


class BeamHypothesis(NamedTuple):
    """One entry of the final beam: its symbols and ln P (prefix probability Pb + Pnb, without the word-count factor that
    orders the beam)."""
    indices: List[int]
    log_prob: float


def read_nbest(beam_len, beam_idx, beam_plen, score, scale, n: int) -> List[List[BeamHypothesis]]:
    """The device's beam read-out (ms_ctc_beam_decode_ex) as lists of hypotheses, at most ``n`` per utterance."""
    bl, bp = beam_len.cpu().tolist(), beam_plen.cpu()
    longest = int(bp.max()) if bp.numel() else 0
    bi = beam_idx[:, :, :max(longest, 1)].cpu()
    bp, sc, sl = bp.tolist(), score.cpu().double().tolist(), scale.cpu().tolist()
    ln2 = math.log(2.0)
    return [[BeamHypothesis(bi[u, k, :bp[u][k]].tolist(), math.log(sc[u][k]) + sl[u] * ln2) for k in range(min(bl[u], n))]
            for u in range(len(bl))]


class CTCBeamDecoder(torch.nn.Module):
    """ctc_beam_decoder.py:10-273; ``range_safe`` and ``decode_nbest`` have no counterpart in the reference."""

    def __init__(self, blank_index: int, beam_width: int, prune_threshold: float = 0.001,
                 language_model: Optional[Callable[[Tuple[int, ...]], float]] = None,
                 lm_weight: Optional[float] = None, separator_index: Optional[int] = None, word_weight: float = 1.0,
                 range_safe: bool = False):
        if not isinstance(range_safe, bool):
            raise ValueError(f"range_safe={range_safe!r} must be a bool")
        if blank_index < 0:
            raise ValueError(f"blank_index={blank_index} must be >= 0")
        if beam_width <= 0:
            raise ValueError(f"beam_width={beam_width} must be > 0")
        if prune_threshold < 0.0 or prune_threshold > 1.0:
            raise ValueError(f"prune_threshold={prune_threshold} not in [0.0, 1.0]")
        if language_model is not None and lm_weight is None:
            raise ValueError("lm_weight must be set when using language_model")
        if separator_index is not None and separator_index < 0:
            raise ValueError(f"separator_index={separator_index} must be >= 0")
        if isinstance(language_model, NGramLanguageModel):
            check_device_language_model(language_model, separator_index, None)
        super().__init__()
        self.blank_index = blank_index
        self.beam_width = beam_width
        self.prune_threshold = prune_threshold
        self.language_model = language_model
        self.lm_weight = lm_weight
        self.separator_index = separator_index
        self.word_weight = word_weight
        self.range_safe = range_safe
        self._workspace = _lib.Workspace()

    def _word_factor(self, seq_len: int) -> Optional[torch.Tensor]:
        """float32((1 + n_words) ** word_weight), n_words = 0..seq_len+1, evaluated
        on the host exactly like the sort key at ctc_beam_decoder.py:248-253."""
        if self.separator_index is None:
            return None
        vals = [float((1 + n) ** self.word_weight) for n in range(seq_len + 2)]
        return torch.tensor(vals, dtype=torch.float64).to(torch.float32).cuda()

    def forward(self, x: torch.Tensor, lengths: torch.Tensor) -> List[List[int]]:
        if self.range_safe:
            return self._decode_ex(x, lengths, None)
        seq_len, batch, symbols = check_decoder_args(x, lengths)
        _lib.require_gpu()
        if seq_len == 0 or batch == 0:
            return [[] for _ in range(batch)]
        lib = _lib.load()
        xd = _lib.f32c(x)
        lens_dev = _lib.lens_i32(lengths)
        w = self.beam_width
        out_idx = torch.empty((batch, seq_len), dtype=torch.int32, device="cuda")
        out_len = torch.empty(batch, dtype=torch.int32, device="cuda")
        ws = self._workspace.get(lib.ms_ctc_beam_workspace_bytes(seq_len, batch, symbols, w))
        sep = -1 if self.separator_index is None else int(self.separator_index)
        wf = self._word_factor(seq_len)
        use_lm = self.language_model is not None and self.separator_index is not None

        def call(t0, t1, lm_factor, finish, beam_len=None, beam_idx=None, beam_plen=None):
            _lib.check(lib.ms_ctc_beam_decode(_lib.ptr(xd), _lib.ptr(lens_dev), _lib.ptr(out_idx), _lib.ptr(out_len),
                                              seq_len, batch, symbols, self.blank_index, w,
                                              float(self.prune_threshold), sep, _lib.ptr(wf), t0, t1,
                                              _lib.ptr(lm_factor), finish, _lib.ptr(beam_len), _lib.ptr(beam_idx),
                                              _lib.ptr(beam_plen), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "ms_ctc_beam_decode")

        if not use_lm:
            call(0, seq_len, None, 1)
            return ragged_to_lists(out_idx, out_len)

        if isinstance(self.language_model, NGramLanguageModel):
            # the model is a table in device memory: one launch, nothing read back, no host call per beam entry
            lm = self.language_model
            check_device_language_model(lm, self.separator_index, symbols)
            table, blob = lm.device_table(self.lm_weight)
            ws = self._workspace.get(lib.ms_ctc_beam_lm_workspace_bytes(seq_len, batch, symbols, w, lm.order))
            _lib.check(lib.ms_ctc_beam_decode_lm(_lib.ptr(xd), _lib.ptr(lens_dev), _lib.ptr(out_idx), _lib.ptr(out_len),
                                                 seq_len, batch, symbols, self.blank_index, w, float(self.prune_threshold),
                                                 sep, _lib.ptr(wf), 0, seq_len, 0, seq_len, _lib.ptr(table),
                                                 ctypes.c_void_p(blob.ctypes.data), blob.size, 1, None, None, None,
                                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "ms_ctc_beam_decode_lm")
            return ragged_to_lists(out_idx, out_len)

        self._advance_with_host_model(call, xd, lengths, seq_len, batch, sep)
        return ragged_to_lists(out_idx, out_len)

    def decode_nbest(self, x: torch.Tensor, lengths: torch.Tensor, n: Optional[int] = None) -> List[List[BeamHypothesis]]:
        """The final beam of every utterance, best first (the order ``forward`` takes its transcript from): at most
        ``min(n, beam_width)`` hypotheses, none where the beam ran empty.  ``log_prob`` = ln(stored Pb + Pnb) + scale_log2 *
        ln 2, evaluated on the host in double; without ``range_safe`` scale_log2 is 0."""
        if n is None:
            n = self.beam_width
        if isinstance(n, bool) or not isinstance(n, int) or n <= 0:
            raise ValueError(f"n={n!r} must be an int > 0")
        return self._decode_ex(x, lengths, n)

    def _decode_ex(self, x, lengths, nbest: Optional[int]):
        """ms_ctc_beam_decode_ex: model-free, device model or host callable; transcripts (nbest None) or the scored beam."""
        seq_len, batch, symbols = check_decoder_args(x, lengths)
        _lib.require_gpu()
        if seq_len == 0 or batch == 0:      # no frame: the beam is the empty prefix with probability 1
            return [[] if nbest is None else [BeamHypothesis([], 0.0)] for _ in range(batch)]
        lib = _lib.load()
        xd = _lib.f32c(x)
        lens_dev = _lib.lens_i32(lengths)
        w = self.beam_width
        out_idx = torch.empty((batch, seq_len), dtype=torch.int32, device="cuda")
        out_len = torch.empty(batch, dtype=torch.int32, device="cuda")
        sep = -1 if self.separator_index is None else int(self.separator_index)
        wf = self._word_factor(seq_len)
        lm = self.language_model if self.separator_index is not None else None
        table = blob = None
        if isinstance(lm, NGramLanguageModel):
            check_device_language_model(lm, self.separator_index, symbols)
            table, blob = lm.device_table(self.lm_weight)
            ws = self._workspace.get(lib.ms_ctc_beam_lm_workspace_bytes(seq_len, batch, symbols, w, lm.order))
        else:
            ws = self._workspace.get(lib.ms_ctc_beam_workspace_bytes(seq_len, batch, symbols, w))
        host_model = lm is not None and table is None
        beam_len = beam_idx = beam_plen = score = scale = None
        if nbest is not None:
            beam_len = torch.empty(batch, dtype=torch.int32, device="cuda")
            beam_idx = torch.empty((batch, w, seq_len), dtype=torch.int32, device="cuda")
            beam_plen = torch.empty((batch, w), dtype=torch.int32, device="cuda")
        if nbest is not None:
            score = torch.empty((batch, w), dtype=torch.float32, device="cuda")
            scale = torch.empty(batch, dtype=torch.int32, device="cuda")

        def call(t0, t1, lm_factor, finish, b_len=None, b_idx=None, b_plen=None, b_score=None, b_scale=None):
            _lib.check(lib.ms_ctc_beam_decode_ex(
                _lib.ptr(xd), _lib.ptr(lens_dev), _lib.ptr(out_idx), _lib.ptr(out_len), seq_len, batch, symbols,
                self.blank_index, w, float(self.prune_threshold), sep, _lib.ptr(wf), t0, t1, 0, seq_len, _lib.ptr(lm_factor),
                finish, _lib.ptr(b_len), _lib.ptr(b_idx), _lib.ptr(b_plen), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(),
                _lib.ptr(table), ctypes.c_void_p(blob.ctypes.data if blob is not None else 0),
                blob.size if blob is not None else 0, 1 if self.range_safe else 0, _lib.ptr(b_score), _lib.ptr(b_scale)),
                "ms_ctc_beam_decode_ex")

        if host_model:
            self._advance_with_host_model(call, xd, lengths, seq_len, batch, sep)
            if nbest is not None:      # a read-out behind the last frame: no frame is processed (t_begin == t_end)
                t_end = int(_lib.host_lens(lengths).max())
                call(t_end, t_end, None, 1, beam_len, beam_idx, beam_plen, score, scale)
        else:
            call(0, seq_len, None, 1, beam_len, beam_idx, beam_plen, score, scale)
        if nbest is None:
            return ragged_to_lists(out_idx, out_len)
        return read_nbest(beam_len, beam_idx, beam_plen, score, scale, nbest)

    def _advance_with_host_model(self, call, xd, lengths, seq_len, batch, sep) -> None:
        """``call(t0, t1, lm_factor, finish, beam_len, beam_idx, beam_plen)`` advances the search; the best prefixes are
        written by the last call."""
        w = self.beam_width
        # host language model.  The reference consults it for beam entry l at frame t only when the separator extension of l
        # survives the pruning test -- float32 p[t, n, sep] > prune_threshold, ctc_beam_decoder.py:198 -- and multiplies the
        # separator extension by float32(lm(l + (sep,)) ** lm_weight) (:214-230).  So the host reads the separator's column of
        # the posteriors ONCE, advances the kernel over every run of frames in which no utterance's separator survives in one
        # launch (no factor is read there), and stops only at the frames that need the model: there it reads back the live
        # beam -- prefix lengths first, then only the first max(prefix length) columns of the prefix table instead of all T
        # (round 5 copied [batch, width, T] int32 every frame: 513 KB at T = 501, batch 32, width 8) -- and calls the model for
        # the entries of the utterances whose separator survives, as the reference does.
        beam_len = torch.empty(batch, dtype=torch.int32, device="cuda")
        beam_idx = torch.empty((batch, w, seq_len), dtype=torch.int32, device="cuda")
        beam_plen = torch.empty((batch, w), dtype=torch.int32, device="cuda")
        lens_h = _lib.host_lens(lengths)
        max_len = int(lens_h.max())
        thr = torch.tensor(float(self.prune_threshold), dtype=torch.float32)
        # [T, N] bool: the separator extension of utterance n is visited at frame t (float32 compare, as in the reference)
        # (the reference SKIPS when p <= thr: a NaN probability is visited, so the test is "not (p <= thr)")
        need = ~(xd[:max_len, :, sep].cpu() <= thr) & (torch.arange(max_len)[:, None] < lens_h[None, :].to(torch.int64))
        need_t = need.any(dim=1).tolist()
        self.lm_calls = self.lm_frames = 0
        call(0, 0, None, 0, beam_len, beam_idx, beam_plen)  # initialise: beam = [()]
        t = 0
        while t < max_len:
            if not need_t[t]:
                t1 = t + 1
                while t1 < max_len and not need_t[t1]:
                    t1 += 1
                call(t, t1, None, 1 if t1 == max_len else 0, beam_len, beam_idx, beam_plen)
                t = t1
                continue
            bl, bp = beam_len.cpu().tolist(), beam_plen.cpu()
            longest = int(bp.max()) if bp.numel() else 0
            bi = beam_idx[:, :, :max(longest, 1)].cpu() if longest else None
            bp = bp.tolist()
            fac = torch.ones((batch, w), dtype=torch.float32)
            row = need[t].tolist()
            for n in range(batch):
                if not row[n]:
                    continue
                for k in range(bl[n]):
                    pre = tuple(bi[n, k, :bp[n][k]].tolist()) if bp[n][k] else ()
                    if pre and pre[-1] == sep:
                        continue        # a repeated separator takes the repeat-character branch (:210-213): no model there
                    prefix = pre + (sep,)
                    fac[n, k] = float(self.language_model(prefix) ** self.lm_weight)
                    self.lm_calls += 1
            self.lm_frames += 1
            call(t, t + 1, fac.cuda(), 1 if t == max_len - 1 else 0, beam_len, beam_idx, beam_plen)
            t += 1
        if max_len == 0:
            call(0, 0, None, 1)

    def extra_repr(self) -> str:
        return ",\n".join([f"blank_index={self.blank_index}", f"beam_width={self.beam_width}",
                           f"prune_threshold={self.prune_threshold}", f"language_model={self.language_model}",
                           f"lm_weight={self.lm_weight}", f"separator_index={self.separator_index}",
                           f"word_weight={self.word_weight}"] + (["range_safe=True"] if self.range_safe else []))
