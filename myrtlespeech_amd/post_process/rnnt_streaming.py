"""The RNN-T greedy decode advanced one chunk of encoder rows at a time -- OWN specification (model/rnnt.py,
oracle/rnnt_oracle.py::greedy_decode; the reference has no transducer).

``RNNTGreedyDecoder`` takes a whole clip and starts the prediction network from the start symbol on every call, so
decoding chunk by chunk and stitching would make every chunk start from "nothing said yet".  Here the predictor's LSTM
state, the projected prediction and the label and frame counts of every stream stay on the device between pushes
(``ms_rnnt_greedy_stream_begin`` / ``_step``), and the decode ends with exactly the transcript the whole-clip decoder
gives, whichever way the clip is cut.  ``timestamps()`` has, per label, the encoder frame that emitted it.

A push blocks the host like ``RNNTGreedyDecoder`` does: the number of iterations depends on the labels, so the library
polls a device counter a few iterations behind its launch queue.  A push can therefore not be captured into a HIP graph.
"""
import ctypes
from typing import List, Optional

import torch

from myrtlespeech_amd import _lib
from myrtlespeech_amd.model.rnnt import RNNTJoint, RNNTPredictor
from myrtlespeech_amd.post_process._common import SUPPORTED_LENGTH_DTYPES
from myrtlespeech_amd.post_process.streaming import PendingLabels

# layout of ms_rnnt_greedy_stream_step's state (include/ms_hotpath.h): int32 words, a header and four words per stream
_HDR_INTS, _STREAM_INTS = 16, 4
_COUNT = 0          # a stream's label count among its four words


class StreamingRNNTGreedyDecoder:
    """Greedy transducer decoding (``RNNTGreedyDecoder``) of a batch of streams, chunk by chunk."""

    def __init__(self, predictor: RNNTPredictor, joint: RNNTJoint, max_symbols: int = 4):
        if max_symbols <= 0:
            raise ValueError(f"max_symbols={max_symbols} must be > 0")
        self.predictor, self.joint, self.max_symbols = predictor, joint, max_symbols
        self._ws = _lib.Workspace()
        self._batch = None

    def _network(self):
        """The C-ABI arguments of the prediction and joint networks, and what keeps them alive."""
        p, j = self.predictor, self.joint
        rnn = p.rnn.rnn                                          # torch.nn.LSTM used as the parameter container
        layers = p.num_layers
        keep = []

        def col(name: str):
            ts = [getattr(rnn, f"{name}_l{l}", None) for l in range(layers)]
            ts = [None if t is None else _lib.f32c(t.detach()) for t in ts]
            arr = (ctypes.c_void_p * layers)(*[None if t is None else t.data_ptr() for t in ts])
            keep.extend((ts, arr))
            return ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))

        emb = _lib.f32c(p.embedding.weight.detach())
        w_pred = _lib.f32c(j.pred_proj.weight.detach())
        w_out = _lib.f32c(j.out.weight.detach())
        b_out = None if j.out.bias is None else _lib.f32c(j.out.bias.detach())
        keep.extend((emb, w_pred, w_out, b_out))
        args = (_lib.ptr(emb), col("weight_ih"), col("weight_hh"), col("bias_ih"), col("bias_hh"), _lib.ptr(w_pred),
                _lib.ptr(w_out), _lib.ptr(b_out))
        dims = (p.vocab_size, emb.shape[1], p.hidden_size, layers, w_out.shape[1])     # V, D, H, L, J
        return args, dims, keep

    def begin(self, batch: int, max_labels: int, total_lens: Optional[torch.Tensor] = None) -> None:
        """Start ``batch`` streams with room for ``max_labels`` labels each (``max_symbols`` times a clip's encoder frames
        always suffice).  ``total_lens [batch]``: the streams' total encoder lengths -- every push then carries all streams
        and a stream's rows past its length are ignored; without it every push names its rows' lengths (``chunk_lens``)."""
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
        args, dims, keep = self._network()
        v, d, h, layers, j = dims
        nbytes = lib.ms_rnnt_greedy_stream_workspace_bytes(batch, v, d, h, layers, j)
        if nbytes == 0:
            raise ValueError("unsupported RNN-T decode shape")
        ws = self._ws.get(nbytes)
        self._state = torch.empty(lib.ms_rnnt_greedy_stream_state_bytes(batch, h, layers, j) // 4, dtype=torch.int32,
                                  device="cuda")
        self._labels = torch.empty((batch, max_labels), dtype=torch.int32, device="cuda")
        self._frames = torch.empty((batch, max_labels), dtype=torch.int32, device="cuda")
        self._total = None if total_lens is None else _lib.lens_i32(total_lens)
        _lib.check(lib.ms_rnnt_greedy_stream_begin(_lib.ptr(self._state), batch, *args, v, d, h, layers, j, _lib.ptr(ws),
                                                   ws.numel(), _lib.stream_ptr()), "ms_rnnt_greedy_stream_begin")
        self._batch, self._cap = batch, max_labels
        del keep

    def _started(self):
        if self._batch is None:
            raise RuntimeError("call begin(batch, max_labels) first")

    def step(self, enc_p: torch.Tensor, rows: int, n: int, chunk_lens: Optional[torch.Tensor] = None,
             fresh: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
             label_frames: Optional[torch.Tensor] = None) -> None:
        """The raw ``ms_rnnt_greedy_stream_step`` on projected rows ``enc_p [rows * n, J]`` (float32, on the device).
        ``fresh``: int32 device tensor ``[batch, 1 + rows * max_symbols]``; ``labels`` / ``label_frames``: int32 device
        tensors ``[batch, cap]`` to append to instead of the decoder's own."""
        self._started()
        if not 0 < n <= self._batch:
            raise ValueError(f"rows hold {n} streams, the batch has {self._batch}")
        if (chunk_lens is None) == (self._total is None):
            raise ValueError("chunk_lens goes with begin(..., total_lens=None), and only with it")
        if chunk_lens is not None and (chunk_lens.dtype != torch.int32 or chunk_lens.numel() != n):
            raise ValueError(f"step: chunk_lens must be int32 [{n}]")
        news = (self._batch, 1 + rows * self.max_symbols)
        if fresh is not None and (fresh.dtype != torch.int32 or tuple(fresh.shape) != news):
            raise ValueError(f"step: fresh must be int32 {list(news)}")
        if enc_p.dtype != torch.float32 or enc_p.dim() != 2 or enc_p.shape[0] != rows * n:
            raise ValueError(f"step: enc_p must be float32 [{rows * n}, J]")
        labels = self._labels if labels is None else labels
        label_frames = self._frames if label_frames is None else label_frames
        for t in (labels, label_frames):
            if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != self._batch:
                raise ValueError(f"step: labels and label_frames must be int32 [{self._batch}, cap]")
        if labels.shape != label_frames.shape:
            raise ValueError("step: labels and label_frames must have one shape")
        args, dims, keep = self._network()
        v, d, h, layers, j = dims
        if enc_p.shape[1] != j:
            raise ValueError(f"step: enc_p has {enc_p.shape[1]} joint features, the joint network {j}")
        lib = _lib.load()
        ws = self._ws.get(lib.ms_rnnt_greedy_stream_workspace_bytes(self._batch, v, d, h, layers, j))
        _lib.check(lib.ms_rnnt_greedy_stream_step(
            _lib.ptr(enc_p), rows, n, _lib.ptr(self._total), _lib.ptr(chunk_lens), *args, _lib.ptr(labels),
            _lib.ptr(label_frames), labels.shape[1], _lib.ptr(fresh), _lib.ptr(self._state), self._batch, v, d, h, layers, j,
            self.max_symbols, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "ms_rnnt_greedy_stream_step")
        del keep

    def push(self, enc_rows: Optional[torch.Tensor], chunk_lens: Optional[torch.Tensor] = None) -> PendingLabels:
        """Decode the next encoder rows ``[r, n, E]`` of the first ``n <= batch`` streams (projected here through
        ``joint.project_encoder``) and start the copy of the labels they add to pinned host memory; ``.result()`` waits
        for it and builds the lists (one per stream of the batch).  ``enc_rows`` may be None or hold no rows: nothing new."""
        self._started()
        if enc_rows is None or enc_rows.shape[0] == 0 or enc_rows.shape[1] == 0:
            return PendingLabels(None, None, self._batch)
        if enc_rows.dim() != 3:
            raise ValueError(f"enc_rows must be [r, n, E], got {tuple(enc_rows.shape)}")
        r, n, _ = enc_rows.shape
        if not 0 < n <= self._batch:
            raise ValueError(f"rows hold {n} streams, the batch has {self._batch}")
        if (chunk_lens is None) == (self._total is None):
            raise ValueError("chunk_lens goes with begin(..., total_lens=None), and only with it")
        if chunk_lens is not None:
            if chunk_lens.dtype not in SUPPORTED_LENGTH_DTYPES:
                raise ValueError(f"chunk_lens.dtype={chunk_lens.dtype} must be in {SUPPORTED_LENGTH_DTYPES}")
            if chunk_lens.numel() != n:
                raise ValueError(f"batch size of enc_rows ({n}) and chunk_lens {chunk_lens.numel()} must be equal")
            chunk_lens = _lib.lens_i32(chunk_lens)
        enc_p = self.joint.project_encoder(enc_rows)              # [r * n, J], row r n + i
        fresh = torch.empty((self._batch, 1 + r * self.max_symbols), dtype=torch.int32, device="cuda")
        self.step(enc_p, r, n, chunk_lens, fresh)
        host = torch.empty(fresh.shape, dtype=torch.int32, pin_memory=True)
        host.copy_(fresh, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        return PendingLabels(host, done, self._batch, keep=(fresh, enc_p, chunk_lens))

    def _read(self, table: torch.Tensor):
        """Per-stream words of the state and ``table`` in ONE read-back; raises if a stream ran out of label room."""
        per_stream = self._state[_HDR_INTS:_HDR_INTS + self._batch * _STREAM_INTS].view(self._batch, _STREAM_INTS)
        packed = torch.cat([per_stream, table], dim=1).cpu().numpy()
        counts = packed[:, _COUNT]
        if bool((counts > self._cap).any()):
            raise RuntimeError(f"streaming RNN-T greedy decode: a stream has {int(counts.max())} labels, max_labels={self._cap}")
        return [packed[n, _STREAM_INTS:_STREAM_INTS + int(counts[n])].tolist() for n in range(self._batch)]

    def transcripts(self) -> List[List[int]]:
        """Every label so far, per stream."""
        self._started()
        return self._read(self._labels)

    def timestamps(self) -> List[List[int]]:
        """For every label the 0-based encoder frame of its stream that emitted it."""
        self._started()
        return self._read(self._frames)

    def iterations(self) -> int:
        """Iterations (score + predictor step) the library has launched since ``begin``: a record for tools."""
        self._started()
        return int(self._state[1].item())

    def check_status(self) -> None:
        """Raises if a stream had more labels than ``max_labels`` (the labels beyond it were counted, not kept)."""
        self._started()
        if int(self._state[0].item()) != 0:
            raise RuntimeError(f"streaming RNN-T greedy decode: a stream has more labels than max_labels={self._cap}")
