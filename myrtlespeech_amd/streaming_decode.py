"""Streaming transcripts: audio chunks in, labels out.

``StreamingTranscriber`` couples ``ChunkedDeepSpeech2(carry_context=True)`` -- whose concatenated chunk outputs are the
full-utterance logits -- with one of the chunk-by-chunk decoders of ``post_process/streaming.py``: every push feeds the
audio chunk, hands the logit rows that became computable to the decoder and returns what the decoder has to say about
them.  The transcript at the end is the whole-clip decoder's on the whole-clip logits.

``StreamingRNNTTranscriber`` does the same for a transducer: the encoder of an ``RNNT`` streamed through
``ChunkedDeepSpeech2(carry_context=True)``, its rows handed to ``StreamingRNNTGreedyDecoder``, whose prediction network keeps
its state on the device across the pushes.
"""
from typing import List, Optional

import torch

from myrtlespeech_amd.post_process.rnnt_streaming import StreamingRNNTGreedyDecoder
from myrtlespeech_amd.post_process.streaming import PendingLabels, StreamingCTCBeamDecoder, StreamingCTCGreedyDecoder
from myrtlespeech_amd.streaming import ChunkedDeepSpeech2


class StreamingTranscriber:
    def __init__(self, model, decoder, chunk_frames: int, use_graph: Optional[bool] = None):
        if not isinstance(decoder, (StreamingCTCGreedyDecoder, StreamingCTCBeamDecoder)):
            raise TypeError("decoder must be a StreamingCTCGreedyDecoder or a StreamingCTCBeamDecoder, "
                            f"got {type(decoder).__name__}")
        self.chunked = ChunkedDeepSpeech2(model, chunk_frames, carry_context=True, use_graph=use_graph)
        self.decoder = decoder
        self._greedy = isinstance(decoder, StreamingCTCGreedyDecoder)
        self._begun = False

    def begin(self, lens: torch.Tensor, total_frames: Optional[int] = None, hx=None) -> None:
        """As ``ChunkedDeepSpeech2.begin``: ``lens [N]`` sorted in decreasing order, ``total_frames`` the batch's padded
        length (default ``lens[0]``), ``hx`` the recurrent stack's initial state."""
        self.chunked.begin(lens, total_frames, hx)
        out_lens, total_out = self.chunked.out_lens, max(self.chunked.total_out, 1)
        if self._greedy:
            self.decoder.begin(len(out_lens), total_out, total_lens=out_lens)
        else:
            self.decoder.begin(out_lens, total_out)
        self._begun = True

    def push(self, chunk: Optional[torch.Tensor], final: bool = False):
        """Feed the next input frames ``[N, C, F, frames]`` (``final=True`` flushes the held-back context; chunk may then
        be None).  Greedy decoder: returns the ``PendingLabels`` of the rows that came out (empty news while the
        latency is being filled).  Beam decoder: advances the search over ``softmax`` of those rows and returns None;
        ``decoder.best()`` has the current best prefixes."""
        if not self._begun:
            raise RuntimeError("call begin(lens) first")
        rows = self.chunked.push(chunk, final)
        if self._greedy:
            return self.decoder.push(rows)
        return self.decoder.push(None if rows is None else torch.softmax(rows, -1))

    def result(self) -> List[List[int]]:
        """The transcripts of everything pushed so far."""
        if not self._begun:
            raise RuntimeError("call begin(lens) first")
        return self.decoder.transcripts() if self._greedy else self.decoder.result()


class StreamingRNNTTranscriber:
    """Audio chunks in, transducer labels out: ``rnnt.encoder`` (a unidirectional ``DeepSpeech2``) chunk by chunk, greedy
    decoding of the rows that come out.  ``result()`` is ``RNNTGreedyDecoder`` on the whole clip's encoder output."""

    def __init__(self, rnnt, chunk_frames: int, max_symbols: int = 4, use_graph: Optional[bool] = None):
        self.chunked = ChunkedDeepSpeech2(rnnt.encoder, chunk_frames, carry_context=True, use_graph=use_graph)
        self.decoder = StreamingRNNTGreedyDecoder(rnnt.predictor, rnnt.joint, max_symbols)
        self._begun = False

    def begin(self, lens: torch.Tensor, total_frames: Optional[int] = None, hx=None) -> None:
        """As ``ChunkedDeepSpeech2.begin`` (which refuses a bidirectional encoder): ``lens [N]`` sorted in decreasing order,
        ``total_frames`` the batch's padded length (default ``lens[0]``), ``hx`` the recurrent stack's initial state."""
        self.chunked.begin(lens, total_frames, hx)
        out_lens, total_out = self.chunked.out_lens, max(self.chunked.total_out, 1)
        self.decoder.begin(len(out_lens), total_out * self.decoder.max_symbols, total_lens=out_lens)
        self._begun = True

    def push(self, chunk: Optional[torch.Tensor], final: bool = False) -> PendingLabels:
        """Feed the next input frames ``[N, C, F, frames]`` (``final=True`` flushes the held-back context; chunk may then
        be None) and return the ``PendingLabels`` of the encoder rows that came out (empty news while the latency is
        being filled)."""
        if not self._begun:
            raise RuntimeError("call begin(lens) first")
        return self.decoder.push(self.chunked.push(chunk, final))

    def result(self) -> List[List[int]]:
        """The transcripts of everything pushed so far."""
        if not self._begun:
            raise RuntimeError("call begin(lens) first")
        return self.decoder.transcripts()

    def timestamps(self) -> List[List[int]]:
        """Per label the encoder frame that emitted it."""
        if not self._begun:
            raise RuntimeError("call begin(lens) first")
        return self.decoder.timestamps()
