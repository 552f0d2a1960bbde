"""CTC decoders that are advanced one chunk of logit rows at a time.

The reference decodes whole utterances (post_process/ctc_greedy_decoder.py:74-92, ctc_beam_decoder.py:175-258); a
caller who streams audio through ``ChunkedDeepSpeech2`` gets a few rows per push and wants to know what they add.
Decoding every chunk on its own and stitching the lists is wrong whenever a run of one symbol spans a chunk boundary
(the repeat is emitted twice) and impossible for the beam search, so both decoders here keep their state on the device
between pushes and end with exactly the transcript the whole-clip decoder gives:

* ``StreamingCTCGreedyDecoder``: one ``ms_ctc_greedy_stream_step`` launch per push; the symbol of each stream's last
  row, its label count and its rows seen are carried in a small device buffer, the labels a push adds come back in ONE
  small device-to-host copy (``PendingLabels``), the greedy prefix never changes once emitted.
* ``StreamingCTCBeamDecoder``: ``ms_ctc_beam_decode_rows`` over the rows of the push; the search state lives in the
  kernel's workspace as it does between the frames of ``CTCBeamDecoder``'s host-language-model path.  ``best()`` is the
  current best prefix and may change as audio arrives.  A host ``language_model`` is refused: the callback stays with
  ``CTCBeamDecoder``.  An ``NGramLanguageModel`` is taken: its table is in device memory and every prefix's model state
  in the workspace, so ``ms_ctc_beam_decode_lm`` advances over a push exactly as the model-free search does.
  ``range_safe=True`` is ``CTCBeamDecoder``'s: the search with an unbounded exponent (``ms_ctc_beam_decode_ex``), its scale
  carried in the workspace from push to push; ``nbest()`` is the scored beam beside ``best()``.
"""
import ctypes
from typing import List, Optional

import torch

from myrtlespeech_amd import _lib
from myrtlespeech_amd.language_model import NGramLanguageModel
from myrtlespeech_amd.post_process._common import SUPPORTED_LENGTH_DTYPES, check_decoder_args, ragged_to_lists
from myrtlespeech_amd.post_process.ctc_beam_decoder import BeamHypothesis, read_nbest

# layout of ms_ctc_greedy_stream_step's state (include/ms_hotpath.h): int32 words, a header and four words per stream
_HDR_INTS, _STREAM_INTS = 16, 4
_COUNT = 1          # a stream's label count among its four words


class PendingLabels:
    """The labels one push added, on their way to the host."""

    def __init__(self, host, done, batch, keep=None):
        self._host, self._done, self._batch, self._keep = host, done, batch, keep

    def result(self) -> List[List[int]]:
        if self._host is None:
            return [[] for _ in range(self._batch)]
        self._done.synchronize()
        packed = self._host.numpy()
        self._keep = None
        return [packed[n, 1:1 + int(packed[n, 0])].tolist() for n in range(packed.shape[0])]


class StreamingCTCGreedyDecoder:
    """Best-path decoding (ctc_greedy_decoder.py:74-92) of a batch of streams, chunk by chunk."""

    def __init__(self, blank_index: int):
        self.blank_index = blank_index
        self._batch = None

    def begin(self, batch: int, max_labels: int, total_lens: Optional[torch.Tensor] = None) -> None:
        """Start ``batch`` streams with room for ``max_labels`` labels each (a clip's output frames always suffice).
        ``total_lens [batch]``: the streams' total output lengths -- every push then carries all streams and a stream's
        rows past its length are ignored (the carried-context mode); without it every push names its rows' lengths
        (``chunk_lens``, the slice-by-slice mode)."""
        if batch <= 0:
            raise ValueError(f"batch={batch} must be > 0")
        if max_labels <= 0:
            raise ValueError(f"max_labels={max_labels} must be > 0")
        if total_lens is not None:
            if total_lens.dtype not in SUPPORTED_LENGTH_DTYPES:
                raise ValueError(f"total_lens.dtype={total_lens.dtype} must be in {SUPPORTED_LENGTH_DTYPES}")
            if len(total_lens) != batch:
                raise ValueError(f"batch ({batch}) and total_lens {len(total_lens)} must be equal")
        _lib.require_gpu()
        lib = _lib.load()
        self._state = torch.empty(lib.ms_ctc_greedy_stream_state_bytes(batch) // 4, dtype=torch.int32, device="cuda")
        self._labels = torch.empty((batch, max_labels), dtype=torch.int32, device="cuda")
        self._frames = torch.empty((batch, max_labels), dtype=torch.int32, device="cuda")
        self._total = None if total_lens is None else _lib.lens_i32(total_lens)
        _lib.check(lib.ms_ctc_greedy_stream_begin(_lib.ptr(self._state), batch, _lib.stream_ptr()), "ms_ctc_greedy_stream_begin")
        self._batch, self._cap = batch, max_labels

    def _started(self):
        if self._batch is None:
            raise RuntimeError("call begin(batch, max_labels) first")

    def step(self, rows: torch.Tensor, chunk_lens: Optional[torch.Tensor] = None, fresh: Optional[torch.Tensor] = None) -> None:
        """Enqueue the decode of ``rows [r, n <= batch, V]`` (float32, on the device) on the current stream and nothing
        else: no copy, no allocation, no synchronisation, so steps with a fixed ``r`` can be captured into a HIP graph.
        ``chunk_lens``: int32 device tensor ``[n]``; ``fresh``: int32 device tensor ``[batch, 1 + r]`` for the news."""
        self._started()
        r, n, symbols = rows.shape
        if not 0 < n <= self._batch:
            raise ValueError(f"rows hold {n} streams, the batch has {self._batch}")
        if (chunk_lens is None) == (self._total is None):
            raise ValueError("chunk_lens goes with begin(..., total_lens=None), and only with it")
        if chunk_lens is not None and (chunk_lens.dtype != torch.int32 or chunk_lens.numel() != n):
            raise ValueError(f"step: chunk_lens must be int32 [{n}]")
        if fresh is not None and (fresh.dtype != torch.int32 or tuple(fresh.shape) != (self._batch, 1 + r)):
            raise ValueError(f"step: fresh must be int32 [{self._batch}, {1 + r}]")
        if rows.dtype != torch.float32:
            raise ValueError("step: rows must be float32")
        _lib.check(_lib.load().ms_ctc_greedy_stream_step(
            _lib.ptr(rows), r, n, symbols, self.blank_index, _lib.ptr(self._total), _lib.ptr(chunk_lens),
            _lib.ptr(self._labels), _lib.ptr(self._frames), self._cap, _lib.ptr(fresh), _lib.ptr(self._state), self._batch,
            _lib.stream_ptr()), "ms_ctc_greedy_stream_step")

    def push(self, rows: Optional[torch.Tensor], chunk_lens: Optional[torch.Tensor] = None) -> PendingLabels:
        """Decode the next rows ``[r, n, V]`` of the first ``n <= batch`` streams and start the copy of the labels they
        add to pinned host memory WITHOUT waiting for it; ``.result()`` waits and builds the lists (one per stream of the
        batch).  ``rows`` may be None or hold no rows: nothing new."""
        self._started()
        if rows is None or rows.shape[0] == 0 or rows.shape[1] == 0:
            return PendingLabels(None, None, self._batch)
        if chunk_lens is not None:
            check_decoder_args(rows, chunk_lens)
            chunk_lens = _lib.lens_i32(chunk_lens)
        xd = _lib.f32c(rows)
        fresh = torch.empty((self._batch, 1 + xd.shape[0]), dtype=torch.int32, device="cuda")
        self.step(xd, chunk_lens, fresh)
        host = torch.empty(fresh.shape, dtype=torch.int32, pin_memory=True)
        host.copy_(fresh, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        return PendingLabels(host, done, self._batch, keep=(fresh, xd, chunk_lens))

    def _read(self, table: torch.Tensor):
        """Per-stream words of the state and ``table`` in ONE read-back; raises if a stream ran out of label room."""
        per_stream = self._state[_HDR_INTS:].view(self._batch, _STREAM_INTS)
        packed = torch.cat([per_stream, table], dim=1).cpu().numpy()
        counts = packed[:, _COUNT]
        if bool((counts > self._cap).any()):
            raise RuntimeError(f"streaming greedy decode: a stream has {int(counts.max())} labels, max_labels={self._cap}")
        return [packed[n, _STREAM_INTS:_STREAM_INTS + int(counts[n])].tolist() for n in range(self._batch)]

    def transcripts(self) -> List[List[int]]:
        """Every label so far, per stream."""
        self._started()
        return self._read(self._labels)

    def timestamps(self) -> List[List[int]]:
        """For every label the 0-based output frame of its stream at which the label's run began."""
        self._started()
        return self._read(self._frames)

    def check_status(self) -> None:
        """Raises if a stream had more labels than ``max_labels`` (the labels beyond it were counted, not kept)."""
        self._started()
        if int(self._state[0].item()) != 0:
            raise RuntimeError(f"streaming greedy decode: a stream has more labels than max_labels={self._cap}")


class StreamingCTCBeamDecoder:
    """Prefix beam search (ctc_beam_decoder.py:175-258) of a batch of streams, advanced over the rows of each push."""

    def __init__(self, blank_index: int, beam_width: int, prune_threshold: float = 0.001,
                 separator_index: Optional[int] = None, word_weight: float = 1.0, language_model=None, lm_weight=None,
                 range_safe: bool = False):
        if not isinstance(range_safe, bool):
            raise ValueError(f"range_safe={range_safe!r} must be a bool")
        if blank_index < 0:
            raise ValueError(f"blank_index={blank_index} must be >= 0")
        if beam_width <= 0:
            raise ValueError(f"beam_width={beam_width} must be > 0")
        if prune_threshold < 0.0 or prune_threshold > 1.0:
            raise ValueError(f"prune_threshold={prune_threshold} not in [0.0, 1.0]")
        if separator_index is not None and separator_index < 0:
            raise ValueError(f"separator_index={separator_index} must be >= 0")
        if isinstance(language_model, NGramLanguageModel):
            if lm_weight is None:
                raise ValueError("lm_weight must be set when using language_model")
            if separator_index is not None and language_model.separator_index != separator_index:
                raise ValueError(f"language_model.separator_index={language_model.separator_index} and "
                                 f"separator_index={separator_index} differ")
        elif language_model is not None or lm_weight is not None:
            raise ValueError("the streaming beam decoder takes no host language_model (only an NGramLanguageModel, whose "
                             "table is in device memory): the host callback is CTCBeamDecoder's")
        self.blank_index = blank_index
        self.beam_width = beam_width
        self.prune_threshold = prune_threshold
        self.separator_index = separator_index
        self.word_weight = word_weight
        # as in the reference, a model without a separator is never consulted
        self.language_model = language_model if separator_index is not None else None
        self.lm_weight = lm_weight
        self.range_safe = range_safe
        self._lens = None

    def begin(self, lens: torch.Tensor, total_frames: int) -> None:
        """``lens [N]``: the streams' total output lengths; ``total_frames``: the clip's output frames (it sizes the
        search's trie, so it has to be known up front: ``ChunkedDeepSpeech2.total_out``)."""
        if lens.dtype not in SUPPORTED_LENGTH_DTYPES:
            raise ValueError(f"lengths.dtype={lens.dtype} must be in {SUPPORTED_LENGTH_DTYPES}")
        if total_frames <= 0:
            raise ValueError(f"total_frames={total_frames} must be > 0")
        if len(lens) == 0:
            raise ValueError("lens is empty")
        if not bool((_lib.host_lens(lens) <= total_frames).all()):
            raise ValueError("length values must be less than or equal to total_frames")
        _lib.require_gpu()
        n, t = len(lens), int(total_frames)
        self._lens = _lib.lens_i32(lens)
        self._n, self._total, self._t, self._symbols = n, t, 0, None
        self._out_idx = torch.empty((n, t), dtype=torch.int32, device="cuda")
        self._out_len = torch.empty(n, dtype=torch.int32, device="cuda")
        self._wf = None
        if self.separator_index is not None:          # CTCBeamDecoder._word_factor
            vals = [float((1 + k) ** self.word_weight) for k in range(t + 2)]
            self._wf = torch.tensor(vals, dtype=torch.float64).to(torch.float32).cuda()
        self._ws = self._window = None

    def _started(self):
        if self._lens is None:
            raise RuntimeError("call begin(lens, total_frames) first")

    def _call(self, window, t0, t1, row0, finish, beam=None):
        """``beam``: (beam_len, beam_idx, beam_plen, beam_score, scale_log2) for the scored read-out."""
        sep = -1 if self.separator_index is None else int(self.separator_index)
        if self.range_safe or beam is not None:
            table = blob = None
            if self.language_model is not None:
                table, blob = self.language_model.device_table(self.lm_weight)
            b = beam if beam is not None else (None,) * 5
            _lib.check(_lib.load().ms_ctc_beam_decode_ex(
                _lib.ptr(window), _lib.ptr(self._lens), _lib.ptr(self._out_idx), _lib.ptr(self._out_len), self._total,
                self._n, self._symbols, self.blank_index, self.beam_width, float(self.prune_threshold), sep,
                _lib.ptr(self._wf), t0, t1, row0, window.shape[0], None, finish, _lib.ptr(b[0]), _lib.ptr(b[1]),
                _lib.ptr(b[2]), _lib.ptr(self._ws), self._ws.numel(), _lib.stream_ptr(), _lib.ptr(table),
                ctypes.c_void_p(blob.ctypes.data if blob is not None else 0), blob.size if blob is not None else 0,
                1 if self.range_safe else 0, _lib.ptr(b[3]), _lib.ptr(b[4])), "ms_ctc_beam_decode_ex")
            return
        if self.language_model is not None:
            table, blob = self.language_model.device_table(self.lm_weight)
            _lib.check(_lib.load().ms_ctc_beam_decode_lm(
                _lib.ptr(window), _lib.ptr(self._lens), _lib.ptr(self._out_idx), _lib.ptr(self._out_len), self._total,
                self._n, self._symbols, self.blank_index, self.beam_width, float(self.prune_threshold), sep,
                _lib.ptr(self._wf), t0, t1, row0, window.shape[0], _lib.ptr(table), ctypes.c_void_p(blob.ctypes.data),
                blob.size, finish, None, None, None, _lib.ptr(self._ws), self._ws.numel(), _lib.stream_ptr()),
                "ms_ctc_beam_decode_lm")
            return
        _lib.check(_lib.load().ms_ctc_beam_decode_rows(
            _lib.ptr(window), _lib.ptr(self._lens), _lib.ptr(self._out_idx), _lib.ptr(self._out_len), self._total, self._n,
            self._symbols, self.blank_index, self.beam_width, float(self.prune_threshold), sep, _lib.ptr(self._wf), t0, t1,
            row0, window.shape[0], None, finish, None, None, None, _lib.ptr(self._ws), self._ws.numel(),
            _lib.stream_ptr()), "ms_ctc_beam_decode_rows")

    def push(self, probs_rows: Optional[torch.Tensor]) -> None:
        """Advance the search of every stream over the next rows ``[r, N, V]`` of normalised probabilities."""
        self._started()
        if probs_rows is None or probs_rows.shape[0] == 0:
            return
        r, n, symbols = probs_rows.shape
        if n != self._n:
            raise ValueError(f"batch size of probs_rows ({n}) and lengths {self._n} must be equal")
        if self._t + r > self._total:
            raise ValueError(f"{self._t + r} rows pushed, total_frames={self._total}")
        if self._symbols is None:
            self._symbols = symbols
            if self.language_model is not None:
                if len(self.language_model.alphabet) != symbols:
                    raise ValueError(f"language_model has an alphabet of {len(self.language_model.alphabet)} symbols, "
                                     f"probs_rows has {symbols}")
                nbytes = _lib.load().ms_ctc_beam_lm_workspace_bytes(self._total, n, symbols, self.beam_width,
                                                                    self.language_model.order)
            else:
                nbytes = _lib.load().ms_ctc_beam_workspace_bytes(self._total, n, symbols, self.beam_width)
            self._ws = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")
        elif symbols != self._symbols:
            raise ValueError(f"probs_rows has {symbols} symbols, earlier pushes had {self._symbols}")
        self._window = _lib.f32c(probs_rows)
        self._call(self._window, self._t, self._t + r, self._t, 0)
        self._t += r

    def best(self) -> List[List[int]]:
        """The best prefix of every stream after the rows pushed so far (it may change as audio arrives)."""
        self._started()
        if self._symbols is None:
            return [[] for _ in range(self._n)]
        # a read-out: no frame is processed (t_begin == t_end), the last window (it ends at row _t) is not read
        self._call(self._window, self._t, self._t, self._t - self._window.shape[0], 1)
        return ragged_to_lists(self._out_idx, self._out_len)

    def nbest(self, n: Optional[int] = None) -> List[List[BeamHypothesis]]:
        """The beam of every stream after the rows pushed so far, best first, at most ``min(n, beam_width)`` hypotheses
        each (``CTCBeamDecoder.decode_nbest``)."""
        self._started()
        if n is None:
            n = self.beam_width
        if isinstance(n, bool) or not isinstance(n, int) or n <= 0:
            raise ValueError(f"n={n!r} must be an int > 0")
        if self._symbols is None:      # no row yet: the empty prefix with probability 1
            return [[BeamHypothesis([], 0.0)] for _ in range(self._n)]
        w = self.beam_width
        beam = (torch.empty(self._n, dtype=torch.int32, device="cuda"),
                torch.empty((self._n, w, self._total), dtype=torch.int32, device="cuda"),
                torch.empty((self._n, w), dtype=torch.int32, device="cuda"),
                torch.empty((self._n, w), dtype=torch.float32, device="cuda"),
                torch.empty(self._n, dtype=torch.int32, device="cuda"))
        self._call(self._window, self._t, self._t, self._t - self._window.shape[0], 1, beam)
        return read_nbest(*beam, n)

    def result(self) -> List[List[int]]:
        """The transcripts: ``best()`` once every row has been pushed."""
        return self.best()
