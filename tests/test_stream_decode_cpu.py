"""Streaming CTC decoders, the part that needs no GPU: the new entry points exist on every side of the C ABI, the numpy
restatement of the greedy step's specification (tests/stream_decode_ref.py) fed chunk by chunk gives the whole-clip
decode -- which pins the specification the kernel is then held to (tests/test_stream_decode_gpu.py) --, the shared inputs
do contain runs that span chunk boundaries, and the argument errors raised before any GPU call."""
import numpy as np
import pytest
import torch

from oracle import ds_oracle as O
from util import Golden, unragged

NEW_SYMBOLS = ["ms_ctc_greedy_stream_state_bytes", "ms_ctc_greedy_stream_begin", "ms_ctc_greedy_stream_step",
               "ms_ctc_beam_decode_rows"]
CHUNKS = (1, 7, 16, 64)


def test_new_entry_points_are_exported_declared_and_bound(lib):
    from myrtlespeech_amd import _lib
    declared = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the window entry point = ms_ctc_beam_decode's arguments + row0, rows_held
    assert len(_lib.SIGNATURES["ms_ctc_beam_decode_rows"][1]) == len(_lib.SIGNATURES["ms_ctc_beam_decode"][1]) + 2
    sizes = [lib.ms_ctc_greedy_stream_state_bytes(n) for n in (1, 2, 6, 32, 33, 1000)]
    assert all(s > 0 for s in sizes)
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert lib.ms_ctc_greedy_stream_state_bytes(0) == 0
    assert lib.ms_ctc_greedy_stream_state_bytes(-3) == 0
    # the state's layout is part of the header's contract: 16 header words + 4 per stream
    assert lib.ms_ctc_greedy_stream_state_bytes(32) == (16 + 4 * 32) * 4


def _check_frames(ref, x, lens):
    for n, (labs, frames) in enumerate(zip(ref.labels, ref.frames)):
        assert len(labs) == len(frames)
        assert all(a < b for a, b in zip(frames, frames[1:]))
        assert all(0 <= f < int(lens[n]) for f in frames)
        assert [int(x[f, n].argmax()) for f in frames] == labs


def test_restated_step_chunk_by_chunk_equals_the_recorded_reference_output_on_ties():
    import stream_decode_ref as R
    g = Golden("greedy_ties")
    x, lens = g["in/x"], g["in/lens"].astype(np.int64)
    for b in g.cfg["blanks"]:
        want = unragged(g[f"out/flat_b{b}"], g[f"out/lens_b{b}"])
        assert O.ctc_greedy_decode(x, lens, b) == want
        for chunk in CHUNKS + (x.shape[0],):
            ref = R.run_chunked(x, lens, b, chunk)
            assert ref.labels == want, (b, chunk)
            assert not ref.overflow
            _check_frames(ref, x, lens)


def test_restated_step_on_inputs_whose_runs_span_the_chunk_boundaries():
    import stream_decode_ref as R
    x, lens, blank = R.boundary_inputs()
    T = x.shape[0]
    want = O.ctc_greedy_decode(x, lens, blank)
    assert [len(w) for w in want] == [66, 62, 47, 34, 5, 0]
    for chunk in CHUNKS + (T,):
        if chunk < T:
            # a condition on the INPUT: without such runs a decoder that forgets the carried symbol would pass
            assert R.spanning_runs(x, lens, blank, chunk) >= 1, chunk
            assert R.stitched_stateless(x, lens, blank, chunk, O.ctc_greedy_decode) != want, chunk
        ref = R.run_chunked(x, lens, blank, chunk)
        assert ref.labels == want, chunk
        _check_frames(ref, x, lens)
    # the news of the steps, joined, are the labels; a live prefix that shrinks (chunk_lens addressing) gives the same
    ref = R.GreedyStreamRef(len(lens), blank, T)
    news = [[] for _ in lens]
    for t0 in range(0, T, 16):
        cl = np.clip(lens - t0, 0, min(16, T - t0))
        alive = int((cl > 0).sum())
        if alive:
            for n, lab in enumerate(ref.step(x[t0:t0 + 16, :alive], cl[:alive])):
                news[n] += lab
    assert news == ref.labels == want


def test_restated_step_capacity_stops_appending_and_keeps_counting():
    import stream_decode_ref as R
    x, lens, blank = R.boundary_inputs()
    want = O.ctc_greedy_decode(x, lens, blank)
    ref = R.run_chunked(x, lens, blank, 16, cap=40)
    assert ref.overflow
    assert ref.labels == [w[:40] for w in want]
    assert ref.count == [len(w) for w in want]


def test_streaming_decoder_argument_errors_before_any_gpu_call():
    from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder, StreamingCTCGreedyDecoder
    with pytest.raises(ValueError):
        StreamingCTCBeamDecoder(-1, 2)
    with pytest.raises(ValueError):
        StreamingCTCBeamDecoder(0, 0)
    with pytest.raises(ValueError):
        StreamingCTCBeamDecoder(0, 2, prune_threshold=-0.1)
    with pytest.raises(ValueError):
        StreamingCTCBeamDecoder(0, 2, prune_threshold=1.1)
    with pytest.raises(ValueError):
        StreamingCTCBeamDecoder(0, 2, separator_index=-1)
    with pytest.raises(ValueError, match="language_model"):
        StreamingCTCBeamDecoder(0, 2, language_model=lambda p: 1.0, lm_weight=1.0)
    rows = torch.zeros(4, 2, 5)
    g = StreamingCTCGreedyDecoder(4)
    for call in (lambda: g.push(rows), g.transcripts, g.timestamps, g.check_status, lambda: g.step(rows)):
        with pytest.raises(RuntimeError, match="begin"):
            call()
    b = StreamingCTCBeamDecoder(4, 2)
    for call in (lambda: b.push(rows), b.best, b.result):
        with pytest.raises(RuntimeError, match="begin"):
            call()
    with pytest.raises(ValueError):
        g.begin(0, 10)
    with pytest.raises(ValueError):
        g.begin(2, 0)
    with pytest.raises(ValueError):
        g.begin(2, 10, total_lens=torch.tensor([4.0, 3.0]))       # float lengths
    with pytest.raises(ValueError):
        g.begin(2, 10, total_lens=torch.tensor([4]))              # batch mismatch
    with pytest.raises(ValueError):
        b.begin(torch.tensor([4.0, 3.0]), 4)
    with pytest.raises(ValueError):
        b.begin(torch.tensor([5, 3]), 4)                          # a length beyond the clip
    with pytest.raises(ValueError):
        b.begin(torch.tensor([4, 3]), 0)


def test_streaming_transcriber_checks_its_decoder_and_call_order():
    from myrtlespeech_amd.post_process.ctc_greedy_decoder import CTCGreedyDecoder
    from myrtlespeech_amd.post_process.streaming import StreamingCTCGreedyDecoder
    from myrtlespeech_amd.streaming_decode import StreamingTranscriber
    model = torch.nn.Identity()
    with pytest.raises(TypeError):
        StreamingTranscriber(model, CTCGreedyDecoder(0), 8)       # a whole-clip decoder cannot be advanced
    with pytest.raises(ValueError):
        StreamingTranscriber(model, StreamingCTCGreedyDecoder(0), 0)
    tr = StreamingTranscriber(model, StreamingCTCGreedyDecoder(0), 8)
    with pytest.raises(RuntimeError, match="begin"):
        tr.push(torch.zeros(1, 1, 4, 8))
    with pytest.raises(RuntimeError, match="begin"):
        tr.result()
