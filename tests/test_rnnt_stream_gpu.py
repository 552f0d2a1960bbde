"""The streaming RNN-T greedy decode on the device (ms_rnnt_greedy_stream_begin / _step, StreamingRNNTGreedyDecoder,
StreamingRNNTTranscriber) against the float64 restatement of tests/rnnt_stream_ref.py and the whole-clip decoder.

A float32 / f16x3 device can be held to a float64 arg max only away from ties: every comparison with the restatement first
ASSERTS that the case's margin (smallest gap between best and second-best logit over every decision) is at least 1e-4, the
project's tolerance on the joint's log-probabilities.  The comparisons between chunkings carry no such condition: equal
bits for every way of cutting a clip is the entry point's determinism clause."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnnt_stream_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _join(news_per_push, batch):
    out = [[] for _ in range(batch)]
    for news in news_per_push:
        assert len(news) == batch
        for n, lab in enumerate(news):
            out[n] += lab
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's modules and inputs, and the restatement's answer (computed once, shared, never changed)."""
    pred, joint, enc, lens, case = R.build_case(name)
    V, _, _, P, _, _, _, _, ms, _, _ = case
    ref = R.RNNTGreedyStreamRef(*R.state_dicts(pred, joint), P, R.LAYERS, V, ms)
    R.run_chunked(ref, enc, lens, None)
    want = dict(labels=[list(v) for v in ref.labels], frames=[list(v) for v in ref.frames], margin=float(ref.margin))
    return pred, joint, enc, lens, ms, want


def _stream(pred, joint, ms, enc_d, lens, chunk, cap=None):
    """Total-lengths mode, `chunk` rows per push (None: the whole clip); returns (decoder, joined news)."""
    from myrtlespeech_amd.post_process import StreamingRNNTGreedyDecoder
    steps, N, _ = enc_d.shape
    dec = StreamingRNNTGreedyDecoder(pred, joint, max_symbols=ms)
    dec.begin(N, cap or steps * ms, total_lens=T(lens))
    news = []
    for t0 in range(0, steps, chunk or steps):
        news.append(dec.push(enc_d[t0:t0 + (chunk or steps)]).result())
    return dec, _join(news, N)


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_chunking_gives_the_whole_clip_transcripts_and_frames(name):
    from myrtlespeech_amd.post_process.rnnt_decoder import RNNTGreedyDecoder
    pred, joint, enc, lens, ms, want = _case(name)
    print(name, "margin", want["margin"])
    assert want["margin"] >= R.MARGIN_FLOOR
    assert [len(v) for v in want["labels"]] == R.LABEL_COUNTS[name]
    enc_d = T(enc).cuda()
    whole = RNNTGreedyDecoder(pred, joint, max_symbols=ms)(enc_d, T(lens))
    results = {}
    for chunk in R.CHUNKS:
        dec, joined = _stream(pred, joint, ms, enc_d, lens, chunk)
        dec.check_status()
        got, frames = dec.transcripts(), dec.timestamps()
        results[chunk] = (got, frames)
        assert joined == got, chunk
        assert got == want["labels"], chunk
        assert got == whole, chunk
        assert frames == want["frames"], chunk
        for f in frames:
            assert f == sorted(f), chunk
            assert all(f.count(v) <= ms for v in set(f)), chunk
    # exact chunking invariance (no margin condition: the determinism clause)
    first = results[R.CHUNKS[0]]
    assert all(results[c] == first for c in R.CHUNKS)


def test_chunk_lengths_mode_with_streams_leaving_as_a_suffix():
    from myrtlespeech_amd.post_process import StreamingRNNTGreedyDecoder
    pred, joint, enc, lens, ms, want = _case("A4")
    assert want["margin"] >= R.MARGIN_FLOOR
    enc_d = T(enc).cuda()
    steps, N, _ = enc.shape
    dec = StreamingRNNTGreedyDecoder(pred, joint, max_symbols=ms)
    dec.begin(N, steps * ms)
    news, ns, zero_rows = [], [], False
    for t0 in range(0, steps, 16):
        left = np.clip(lens - t0, 0, 16)
        n = max(int((left > 0).sum()), 1)
        if t0 == 0:
            n = N                                   # the empty stream is part of the first push: zero rows for it
        zero_rows |= bool((left[:n] == 0).any())
        ns.append(n)
        news.append(dec.push(enc_d[t0:t0 + 16, :n].contiguous(), T(left[:n])).result())
    assert zero_rows and ns == sorted(ns, reverse=True) and ns[0] > ns[-1]
    dec.check_status()
    assert dec.transcripts() == want["labels"] == _join(news, N)
    assert dec.timestamps() == want["frames"]


def test_capacity_overflow_is_reported_and_nothing_is_written_past_it():
    from myrtlespeech_amd.post_process import StreamingRNNTGreedyDecoder
    pred, joint, enc, lens, ms, want = _case("A2")
    assert want["margin"] >= R.MARGIN_FLOOR
    enc_d = T(enc).cuda()
    steps, N, _ = enc.shape
    cap, guard = 50, 8
    dec, joined = _stream(pred, joint, ms, enc_d, lens, 33, cap=cap)
    with pytest.raises(RuntimeError, match="max_labels"):
        dec.check_status()
    with pytest.raises(RuntimeError, match="max_labels"):
        dec.transcripts()
    assert joined == [w[:cap] for w in want["labels"]]
    # guard columns through the raw step: labels [N, cap] and label_frames [N, cap] are the first halves of wider rows
    dec = StreamingRNNTGreedyDecoder(pred, joint, max_symbols=ms)
    dec.begin(N, cap, total_lens=T(lens))
    # (the entry point takes dense [N, cap] tables, so column cap of stream i is column 0 of stream i + 1, whose labels are
    # checked below; the guard words stand behind the LAST row of each table)
    tables = torch.full((2, N * cap + guard), -7, dtype=torch.int32, device="cuda")
    labels, frames = tables[0, :N * cap].view(N, cap), tables[1, :N * cap].view(N, cap)
    for t0 in range(0, steps, 33):
        rows = enc_d[t0:t0 + 33]
        dec.step(joint.project_encoder(rows), rows.shape[0], N, labels=labels, label_frames=frames)
    got = tables.cpu().numpy()
    assert (got[:, N * cap:] == -7).all()
    counts = dec._state[16:16 + 4 * N].view(N, 4)[:, 0].cpu().tolist()
    assert counts == [len(w) for w in want["labels"]]               # it kept counting, and its predictor kept stepping
    for i, w in enumerate(want["labels"]):
        k = min(len(w), cap)
        assert got[0, i * cap:i * cap + k].tolist() == w[:k]
        assert (got[0, i * cap + k:(i + 1) * cap] == -7).all()      # a stream's unused places are untouched
        assert got[1, i * cap:i * cap + k].tolist() == want["frames"][i][:k]
    # a second begin with enough room decodes correctly in the same object
    dec.begin(N, steps * ms, total_lens=T(lens))
    for t0 in range(0, steps, 33):
        dec.push(enc_d[t0:t0 + 33])
    dec.check_status()
    assert dec.transcripts() == want["labels"] and dec.timestamps() == want["frames"]


def test_a_nan_stream_leaves_the_others_alone():
    pred, joint, enc, lens, ms, want = _case("A4")
    assert want["margin"] >= R.MARGIN_FLOOR
    bad = enc.copy()
    bad[32:64, 1] = np.nan                          # stream 1's rows of the second push of 32
    dec, _ = _stream(pred, joint, ms, T(bad).cuda(), lens, 32)
    got = dec.transcripts()                         # the call returned
    for i in range(len(lens)):
        if i != 1:
            assert got[i] == want["labels"][i], i
    assert all(0 <= v < 9 for v in got[1])          # unspecified, but labels
    before = sum(f < 32 for f in want["frames"][1])
    assert got[1][:before] == want["labels"][1][:before]      # what it said before the bad push stands


# ---- the transcriber: a tiny unidirectional DS2 encoder (the construction of
# test_streaming_transcriber_greedy_equals_the_whole_clip_transcripts) + a family-A predictor and joint
TRANSCRIBER_FIXTURE = "ds2_tiny_gru_lookahead"
# Model seed of the predictor and the joint, blank bias, scale of enc_proj.weight (the fixture's encoder rows are within
# +-0.35: unscaled, every frame decides alike); max_symbols 2.  Chosen on the CPU with the oracle's forward of the fixture:
# margin 1.64e-3, stream 0 emits on frames [1, 13, 13, 14, 14] -- blank runs, single labels and a used-up quota.
TRANSCRIBER_SEED, TRANSCRIBER_BIAS, TRANSCRIBER_SCALE = 13, 0.5, 32.0


def _transcriber_parts():
    from test_gpu_parity import build_ds2, load_sd
    from util import Golden
    from myrtlespeech_amd.model.rnnt import RNNT, RNNTJoint, RNNTPredictor
    g = Golden(TRANSCRIBER_FIXTURE)
    encoder = load_sd(build_ds2(g.cfg), g.sd())
    x, lens = T(g["in/x"]).cuda(), T(g["in/lens"])
    hx = T(g["in/h0"]) if g.has("in/h0") else None
    with torch.no_grad():
        (y, out_lens), _ = encoder((x.clone(), lens), hx)
    E, V = y.shape[-1], 9
    torch.manual_seed(TRANSCRIBER_SEED)
    pred = RNNTPredictor(V, 8, 64, num_layers=R.LAYERS).eval()
    joint = RNNTJoint(E, 64, 32, V).eval()
    with torch.no_grad():
        joint.out.bias[V] += TRANSCRIBER_BIAS
        joint.enc_proj.weight *= TRANSCRIBER_SCALE
    return RNNT(encoder, pred, joint), x, lens, hx, y, out_lens


def test_transcriber_equals_the_decoder_on_the_whole_clip_rows():
    from myrtlespeech_amd.post_process.rnnt_decoder import RNNTGreedyDecoder
    from myrtlespeech_amd.streaming import ChunkedDeepSpeech2
    from myrtlespeech_amd.streaming_decode import StreamingRNNTTranscriber
    rnnt, x, lens, hx, y, out_lens = _transcriber_parts()
    ms, V = 2, 9
    total, N = x.shape[-1], x.shape[0]
    # the margin of the whole-clip decode, from the read-back whole-clip rows
    ref = R.RNNTGreedyStreamRef(*R.state_dicts(rnnt.predictor, rnnt.joint), 64, R.LAYERS, V, ms)
    host_lens = out_lens.cpu().numpy().astype(np.int64)
    R.run_chunked(ref, y.cpu().numpy(), host_lens, None)
    print("transcriber margin", ref.margin, "labels", [len(v) for v in ref.labels])
    assert ref.margin >= R.MARGIN_FLOOR
    assert sum(len(v) for v in ref.labels) >= 4
    whole = RNNTGreedyDecoder(rnnt.predictor, rnnt.joint, max_symbols=ms)(y, out_lens)
    assert whole == ref.labels
    for chunk in (4, 13, total):
        tr = StreamingRNNTTranscriber(rnnt, chunk, max_symbols=ms)
        tr.begin(lens, total, hx)
        news = [tr.push(x[..., t0:t0 + chunk], final=(t0 + chunk >= total)).result() for t0 in range(0, total, chunk)]
        got = tr.result()
        tr.decoder.check_status()
        assert _join(news, N) == got, chunk
        assert got == whole, chunk
        assert tr.timestamps() == ref.frames, chunk
        # the decoder alone, pushed with the whole-clip encoder's output rows cut where the chunked encoder cut its own
        c = ChunkedDeepSpeech2(rnnt.encoder, chunk, carry_context=True)
        c.begin(lens, total, hx)
        cuts = []
        for t0 in range(0, total, chunk):
            rows = c.push(x[..., t0:t0 + chunk], final=(t0 + chunk >= total))
            cuts.append(0 if rows is None else rows.shape[0])
        from myrtlespeech_amd.post_process import StreamingRNNTGreedyDecoder
        dec = StreamingRNNTGreedyDecoder(rnnt.predictor, rnnt.joint, max_symbols=ms)
        dec.begin(N, max(y.shape[0], 1) * ms, total_lens=out_lens)
        r0 = 0
        for cnt in cuts:
            dec.push(y[r0:r0 + cnt] if cnt else None)
            r0 += cnt
        assert r0 == y.shape[0]
        assert dec.transcripts() == got and dec.timestamps() == tr.timestamps(), chunk


def test_transcriber_refuses_a_bidirectional_encoder():
    from test_gpu_parity import build_ds2, load_sd
    from util import Golden
    from myrtlespeech_amd.model.rnnt import RNNT, RNNTJoint, RNNTPredictor
    from myrtlespeech_amd.streaming_decode import StreamingRNNTTranscriber
    g = Golden("ds2_tiny_bilstm")
    rnnt = RNNT(load_sd(build_ds2(g.cfg), g.sd()), RNNTPredictor(9, 8, 64), RNNTJoint(29, 64, 32, 9))
    tr = StreamingRNNTTranscriber(rnnt, 8)
    with pytest.raises(ValueError, match="bidirectional"):
        tr.begin(T(g["in/lens"]))
    with pytest.raises(RuntimeError, match="begin"):
        tr.push(None)
