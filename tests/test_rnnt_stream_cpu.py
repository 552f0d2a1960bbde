"""The streaming RNN-T greedy decode without a GPU: the numpy restatement (tests/rnnt_stream_ref.py) against the oracle's
whole-clip loop for every chunking, the margins of the shared cases, the library's new entry points and the Python
argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnnt_stream_ref as R  # noqa: E402
from oracle import rnnt_oracle as RO  # noqa: E402

NEW_SYMBOLS = ["ms_rnnt_greedy_stream_state_bytes", "ms_rnnt_greedy_stream_workspace_bytes", "ms_rnnt_greedy_stream_begin",
               "ms_rnnt_greedy_stream_step"]


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_equals_the_oracle_for_every_chunking(name):
    pred, joint, enc, lens, case = R.build_case(name)
    V, _, _, P, _, _, _, _, ms, _, _ = case
    psd, jsd = R.state_dicts(pred, joint)
    want = RO.greedy_decode(enc, lens, psd, jsd, P, R.LAYERS, V, ms)
    assert [len(w) for w in want] == R.LABEL_COUNTS[name]
    ref = R.RNNTGreedyStreamRef(psd, jsd, P, R.LAYERS, V, ms)
    frames = None
    for chunk in R.CHUNKS:
        news = R.run_chunked(ref, enc, lens, chunk)
        print(name, chunk, "margin", ref.margin, "iterations", ref.iterations)
        assert ref.labels == want and news == want, chunk
        assert ref.margin >= R.MARGIN_FLOOR, (chunk, ref.margin)
        assert ref.seen == [int(v) for v in lens] and not ref.overflow
        for f in ref.frames:
            assert f == sorted(f)
            assert all(f.count(v) <= ms for v in set(f))
        assert frames is None or frames == ref.frames, chunk          # the emission frames do not depend on the cut
        frames = ref.frames


def test_restatement_chunk_lengths_mode_and_capacity():
    pred, joint, enc, lens, case = R.build_case("A4")
    V, _, _, P, _, _, _, _, ms, _, _ = case
    psd, jsd = R.state_dicts(pred, joint)
    ref = R.RNNTGreedyStreamRef(psd, jsd, P, R.LAYERS, V, ms)
    want = R.run_chunked(ref, enc, lens, None)
    ref.begin(len(lens), None)
    for t0 in range(0, enc.shape[0], 16):
        left = np.clip(lens - t0, 0, 16)
        n = max(int((left > 0).sum()), 1)
        ref.push(enc[t0:t0 + 16, :n], left[:n])
    assert ref.labels == want
    capped = R.RNNTGreedyStreamRef(psd, jsd, P, R.LAYERS, V, ms)
    news = R.run_chunked(capped, enc, lens, 7, cap=20)
    assert capped.overflow and capped.labels == [w[:20] for w in want] and news == capped.labels
    assert capped.count == [len(w) for w in want]


def test_device_iterations_counts_labels_plus_blank_blocks():
    assert R.device_iterations(0, [], 3) == 0
    assert R.device_iterations(100, [], 3) == 4                  # blocks of 32 blanks
    assert R.device_iterations(40, [5], 3) == 1 + 1 + 1          # the label, the rest of its block re-scored, the tail
    assert R.device_iterations(3, [0, 0, 1], 2) == 3 + 1         # quota reached on frame 0; frame 2 is scored once more
    assert R.device_iterations(1, [0, 0], 2) == 2                # the quota ends the last frame: nothing is left


def test_library_exports_the_streaming_entry_points():
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in declared and hasattr(lib, name), name
    assert lib.ms_abi_version() == 4


def test_state_bytes_is_host_arithmetic():
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    for bad in ((0, 64, 2, 32), (-1, 64, 2, 32), (4, 0, 2, 32), (4, 64, 0, 32), (4, 64, 2, 0)):
        assert lib.ms_rnnt_greedy_stream_state_bytes(*bad) == 0, bad
    sizes = [lib.ms_rnnt_greedy_stream_state_bytes(n, 64, 2, 32) for n in (1, 2, 16, 64)]
    assert sizes == sorted(set(sizes)) and sizes[0] >= (16 + 4) * 4 + (2 * 2 * 64 + 32) * 4
    assert lib.ms_rnnt_greedy_stream_workspace_bytes(0, 9, 8, 64, 2, 32) == 0
    assert lib.ms_rnnt_greedy_stream_workspace_bytes(4, 9, 8, 64, 2, 32) > 0


def _decoder(max_symbols=3):
    from myrtlespeech_amd.model.rnnt import RNNTJoint, RNNTPredictor
    from myrtlespeech_amd.post_process import StreamingRNNTGreedyDecoder
    torch.manual_seed(0)
    return StreamingRNNTGreedyDecoder(RNNTPredictor(9, 8, 64, num_layers=2), RNNTJoint(24, 64, 32, 9), max_symbols)


def test_argument_checks_raise_before_anything_touches_the_gpu():
    from myrtlespeech_amd.model.rnnt import RNNTJoint, RNNTPredictor
    from myrtlespeech_amd.post_process.rnnt_streaming import StreamingRNNTGreedyDecoder
    with pytest.raises(ValueError, match="max_symbols"):
        StreamingRNNTGreedyDecoder(RNNTPredictor(9, 8, 64), RNNTJoint(24, 64, 32, 9), 0)
    dec = _decoder()
    rows = torch.zeros(4, 2, 24)
    for call in (lambda: dec.push(rows), dec.transcripts, dec.timestamps, dec.check_status):
        with pytest.raises(RuntimeError, match="begin"):
            call()
    with pytest.raises(ValueError, match="batch"):
        dec.begin(0, 10)
    with pytest.raises(ValueError, match="max_labels"):
        dec.begin(2, 0)
    with pytest.raises(ValueError, match="dtype"):
        dec.begin(2, 10, total_lens=torch.tensor([4.0, 2.0]))
    with pytest.raises(ValueError, match="must be equal"):
        dec.begin(2, 10, total_lens=torch.tensor([4, 2, 1]))
    # the checks of push, on a decoder that looks begun (begin itself needs the device)
    dec._batch, dec._cap, dec._total = 2, 10, None
    with pytest.raises(ValueError, match="3 streams"):
        dec.push(torch.zeros(4, 3, 24), torch.tensor([4, 4, 4]))
    with pytest.raises(ValueError, match="chunk_lens"):
        dec.push(rows)                                              # slice-by-slice mode needs chunk_lens
    with pytest.raises(ValueError, match="must be equal"):
        dec.push(rows, torch.tensor([4, 4, 4]))
    with pytest.raises(ValueError, match="dtype"):
        dec.push(rows, torch.tensor([4.0, 4.0]))
    dec._total = torch.tensor([4, 2], dtype=torch.int32)
    with pytest.raises(ValueError, match="chunk_lens"):
        dec.push(rows, torch.tensor([4, 2]))                        # total-lengths mode takes none
    assert dec.push(None).result() == [[], []] and dec.push(rows[:0]).result() == [[], []]


def test_transcriber_is_a_class_of_its_own():
    from myrtlespeech_amd import streaming_decode as SD
    from myrtlespeech_amd.post_process.streaming import PendingLabels
    dec = _decoder()
    with pytest.raises(TypeError):                                  # StreamingTranscriber stays the CTC decoders'
        SD.StreamingTranscriber(torch.nn.Identity(), dec, 8)
    assert hasattr(SD, "StreamingRNNTTranscriber") and PendingLabels is SD.PendingLabels
