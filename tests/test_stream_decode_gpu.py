"""Streaming CTC decoders on the GPU: advanced chunk by chunk they end with exactly what the whole-clip decoders give.
Every comparison is exact (integer labels); the expectations are the whole-clip decoders, the numpy oracle, the numpy
restatement of the step's specification (tests/stream_decode_ref.py, pinned in tests/test_stream_decode_cpu.py) and
outputs recorded from the reference.  Needs a real MI355X: -m gpu."""
import numpy as np
import pytest
import torch

from oracle import ds_oracle as O
from util import Golden, unragged

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


def _greedy_case(name):
    import stream_decode_ref as R
    if name == "boundary":
        return R.boundary_inputs()
    Tn, N, V = {"config": (501, 32, 29), "wide": (120, 5, 5000)}[name]
    rng = np.random.default_rng(Tn + N + V)
    # (seeds for which a run spans a boundary of every chunk size used below: asserted there, from the inputs)
    seed = {"config": 21061, "wide": 5601}[name]
    return R.boundary_inputs(seed=seed, T=Tn, N=N, V=V, lens=R.ragged_sorted_lens(rng, Tn, N))


def _stream_greedy(xd, lens, blank, chunk, shrink, cap=None):
    """Feed xd [T, N, V] (device) chunk by chunk; returns (decoder, the pushes' news joined)."""
    from myrtlespeech_amd.post_process.streaming import StreamingCTCGreedyDecoder
    Tn, N, _ = xd.shape
    dec = StreamingCTCGreedyDecoder(blank)
    dec.begin(N, cap or Tn, total_lens=None if shrink else T(lens))
    pending = []
    for t0 in range(0, Tn, chunk):
        rows = xd[t0:t0 + chunk]
        if shrink:          # the slice-by-slice mode: the slice's own lengths, streams that have ended leave as a suffix
            cl = np.clip(lens - t0, 0, rows.shape[0])
            alive = int((cl > 0).sum())
            pending.append(dec.push(rows[:, :alive] if alive else None, T(cl[:alive]) if alive else None))
        else:
            pending.append(dec.push(rows))
    return dec, _join([p.result() for p in pending], N)


@pytest.mark.parametrize("name", ["boundary", "config", "wide"])
def test_greedy_steps_equal_the_whole_clip_decoder(name):
    """Every chunk size, both ways of saying which rows exist: the pushes' news joined == transcripts() ==
    CTCGreedyDecoder on the whole tensor == the oracle; timestamps() == the restated specification's."""
    import stream_decode_ref as R
    from myrtlespeech_amd.post_process.ctc_greedy_decoder import CTCGreedyDecoder
    x, lens, blank = _greedy_case(name)
    Tn, N, _ = x.shape
    assert int(lens.min()) == 0 and int(lens.max()) == Tn and bool((np.diff(lens) <= 0).all())
    xd = T(x).cuda()
    want = CTCGreedyDecoder(blank)(xd, T(lens))
    assert want == O.ctc_greedy_decode(x, lens, blank)
    ref = R.run_chunked(x, lens, blank, 16)
    assert ref.labels == want
    for chunk in (1, 7, 16, 64, 100, Tn):
        if chunk < Tn:
            assert R.spanning_runs(x, lens, blank, chunk) >= 1, chunk
        for shrink in (False, True):
            dec, news = _stream_greedy(xd, lens, blank, chunk, shrink)
            dec.check_status()
            assert news == want, (chunk, shrink)
            assert dec.transcripts() == want, (chunk, shrink)
            assert dec.timestamps() == ref.frames, (chunk, shrink)


def test_greedy_steps_on_ties_equal_the_recorded_reference_output():
    g = Golden("greedy_ties")
    x, lens = g["in/x"], g["in/lens"].astype(np.int64)
    order = np.argsort(-lens, kind="stable")           # the shrinking live prefix wants sorted lengths
    xd = T(x).cuda()
    for b in g.cfg["blanks"]:
        want = unragged(g[f"out/flat_b{b}"], g[f"out/lens_b{b}"])
        for chunk in (1, 7, 16, 64, x.shape[0]):
            dec, news = _stream_greedy(xd, lens, b, chunk, shrink=False)
            assert news == want and dec.transcripts() == want, (b, chunk)
            dec, news = _stream_greedy(T(x[:, order]).cuda(), lens[order], b, chunk, shrink=True)
            assert news == [want[i] for i in order] and dec.transcripts() == news, (b, chunk)


@pytest.mark.parametrize("V", [29, 100])
def test_greedy_steps_count_nan_as_the_maximum(V):
    """tests/test_gpu_parity.py::test_greedy_counts_nan_as_the_maximum_like_torch_argmax, chunked."""
    from myrtlespeech_amd.post_process.ctc_greedy_decoder import CTCGreedyDecoder
    rng = np.random.default_rng(V)
    x = rng.normal(size=(90, 4, V)).astype(np.float32)
    for t, n, v in [(3, 0, V - 2), (3, 0, 5), (10, 1, 0), (40, 2, V - 1), (41, 2, 70 % V), (41, 2, 7), (89, 3, 1)]:
        x[t, n, v] = np.nan
    lens = np.array([90, 80, 90, 90], dtype=np.int64)
    want = [torch.unique_consecutive(torch.from_numpy(x[:l, n]).argmax(-1)).tolist() for n, l in enumerate(lens)]
    want = [[v for v in w if v != V - 1] for w in want]
    xd = T(x).cuda()
    assert CTCGreedyDecoder(V - 1)(xd, T(lens)) == want
    for chunk in (1, 7, 16, 41, 64, 90):
        dec, news = _stream_greedy(xd, lens, V - 1, chunk, shrink=False)
        assert news == want and dec.transcripts() == want, chunk


def test_greedy_capacity_is_reported_and_never_exceeded():
    """max_labels below the label count: check_status() and transcripts() raise; at the C ABI, with canaries in the slabs
    of silent streams that FOLLOW the talkative ones and behind every buffer, nothing is written past `cap`."""
    import stream_decode_ref as R
    from myrtlespeech_amd import _lib
    x, lens, blank = R.boundary_inputs()
    want = O.ctc_greedy_decode(x, lens, blank)
    cap = 40
    assert len(want[0]) > cap and len(want[1]) > cap > len(want[3])      # some streams overflow, some do not
    dec, news = _stream_greedy(T(x).cuda(), lens, blank, 16, shrink=False, cap=cap)
    assert news == [w[:cap] for w in want]               # the news stop where the appending stops
    with pytest.raises(RuntimeError, match="max_labels"):
        dec.check_status()
    with pytest.raises(RuntimeError, match="max_labels"):
        dec.transcripts()

    lib = _lib.load()
    N, rows, CANARY = 4, 16, -77
    xs = np.ascontiguousarray(np.stack([x[:, 0], x[:, 5], x[:, 1], x[:, 5]], axis=1))      # talkative, silent, talkative, silent
    total = torch.tensor([203, 0, 203, 0], dtype=torch.int32, device="cuda")
    xd = T(xs).cuda()
    pad = 64
    labels = torch.full((N * cap + pad,), CANARY, dtype=torch.int32, device="cuda")
    frames = torch.full((N * cap + pad,), CANARY, dtype=torch.int32, device="cuda")
    fresh = torch.full((N * (1 + rows) + pad,), CANARY, dtype=torch.int32, device="cuda")
    state = torch.full((lib.ms_ctc_greedy_stream_state_bytes(N) // 4 + pad,), CANARY, dtype=torch.int32, device="cuda")
    _lib.check(lib.ms_ctc_greedy_stream_begin(_lib.ptr(state), N, _lib.stream_ptr()), "begin")
    for t0 in range(0, xs.shape[0], rows):
        chunk = xd[t0:t0 + rows].contiguous()
        fresh.fill_(CANARY)
        _lib.check(lib.ms_ctc_greedy_stream_step(_lib.ptr(chunk), chunk.shape[0], N, xs.shape[2], blank, _lib.ptr(total), None,
                                                 _lib.ptr(labels), _lib.ptr(frames), cap, _lib.ptr(fresh), _lib.ptr(state), N,
                                                 _lib.stream_ptr()), "step")
        f = fresh.cpu().numpy()
        assert (f[N * (1 + chunk.shape[0]):] == CANARY).all()
        news = f[:N * (1 + chunk.shape[0])].reshape(N, 1 + chunk.shape[0])
        assert news[1, 0] == 0 and news[3, 0] == 0 and (news[:, 0] <= chunk.shape[0]).all()
    lab, frm, st = labels.cpu().numpy(), frames.cpu().numpy(), state.cpu().numpy()
    for buf in (lab, frm):
        slabs = buf[:N * cap].reshape(N, cap)
        assert (slabs[1] == CANARY).all() and (slabs[3] == CANARY).all()
        assert (buf[N * cap:] == CANARY).all()
    assert lab[:cap].tolist() == want[0][:cap] and lab[2 * cap:3 * cap].tolist() == want[1][:cap]
    assert st[0] == 1                                                     # the sticky overflow word
    per_stream = st[16:16 + 4 * N].reshape(N, 4)
    assert per_stream[:, 1].tolist() == [len(want[0]), 0, len(want[1]), 0]   # it kept counting
    assert per_stream[:, 2].tolist() == [203, 0, 203, 0]
    assert (st[16 + 4 * N:] == CANARY).all()


def test_greedy_steps_replayed_from_a_captured_graph_equal_the_eager_steps():
    """step() reads and writes its counts on the device and allocates nothing: one capture of a 16-row step on one
    stream, replayed over the full chunks of a clip (the short last chunk runs eagerly), gives the eager pushes' news and
    transcripts."""
    import stream_decode_ref as R
    from myrtlespeech_amd.post_process.streaming import StreamingCTCGreedyDecoder
    x, lens, blank = R.boundary_inputs()
    Tn, N, V = x.shape
    rows = 16
    xd = T(x).cuda()
    eager, eager_news = _stream_greedy(xd, lens, blank, rows, shrink=False)
    want = eager.transcripts()
    assert want == O.ctc_greedy_decode(x, lens, blank)

    dec = StreamingCTCGreedyDecoder(blank)
    xs = torch.zeros((rows, N, V), dtype=torch.float32, device="cuda")
    fs = torch.zeros((N, 1 + rows), dtype=torch.int32, device="cuda")
    dec.begin(N, Tn, total_lens=T(lens))
    dec.step(xs, fresh=fs)                      # warm-up: the code object is loaded outside the capture
    torch.cuda.synchronize()
    dec.begin(N, Tn, total_lens=T(lens))        # ... and the state starts again
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        dec.step(xs, fresh=fs)
    news = []
    t0 = 0
    while t0 + rows <= Tn:
        xs.copy_(xd[t0:t0 + rows])
        graph.replay()
        f = fs.cpu().numpy()
        news.append([f[n, 1:1 + int(f[n, 0])].tolist() for n in range(N)])
        t0 += rows
    assert t0 < Tn
    news.append(dec.push(xd[t0:]).result())
    dec.check_status()
    assert _join(news, N) == eager_news == want
    assert dec.transcripts() == want
    assert dec.timestamps() == eager.timestamps()


def test_streaming_decoders_refuse_what_the_kernels_cannot_read():
    """step() hands its tensors to the kernel as they are: host or strided ones are refused (``_lib.ptr``), and so are a
    chunk_lens in the wrong mode and more streams than the batch has -- all before any launch."""
    from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder, StreamingCTCGreedyDecoder
    dec = StreamingCTCGreedyDecoder(4)
    dec.begin(2, 8, total_lens=torch.tensor([8, 5]))
    rows = torch.zeros((4, 2, 5), device="cuda")
    with pytest.raises(ValueError):
        dec.step(torch.zeros(4, 2, 5))                                     # a host tensor
    with pytest.raises(ValueError):
        dec.step(torch.zeros((4, 5, 2), device="cuda").transpose(1, 2))    # a strided view
    with pytest.raises(ValueError):
        dec.push(rows, chunk_lens=torch.tensor([4, 4]))                    # begun with total_lens
    with pytest.raises(ValueError):
        dec.push(torch.zeros((4, 3, 5), device="cuda"))                    # three streams in a batch of two
    dec.begin(2, 8)
    with pytest.raises(ValueError):
        dec.push(rows)                                                     # begun without total_lens: chunk_lens is needed
    with pytest.raises(ValueError):
        dec.push(rows, chunk_lens=torch.tensor([5, 4]))                    # a length beyond the rows
    assert dec.push(rows, chunk_lens=torch.tensor([4, 2])).result() == [[0], [0]]
    assert dec.push(None).result() == [[], []] and dec.push(rows[:0]).result() == [[], []]
    assert dec.transcripts() == [[0], [0]] and dec.timestamps() == [[0], [0]]
    beam = StreamingCTCBeamDecoder(4, 2)
    beam.begin(torch.tensor([8, 5]), 8)
    beam.push(None)
    assert beam.best() == [[], []]
    beam.push(torch.softmax(rows, -1))
    with pytest.raises(ValueError):
        beam.push(torch.softmax(torch.zeros((4, 2, 6), device="cuda"), -1))   # another alphabet
    beam.push(torch.softmax(rows, -1))
    with pytest.raises(ValueError):
        beam.push(torch.softmax(rows, -1))                                    # more rows than total_frames


def _beam_case(name):
    if name == "split":       # the shapes of test_beam_call_split_between_frames_equals_one_call
        rng = np.random.default_rng(77)
        z = rng.normal(size=(50, 5, 9)) * 0.8
        x = np.exp(z - z.max(-1, keepdims=True))
        x = (x / x.sum(-1, keepdims=True)).astype(np.float32)
        return x, np.array([50, 50, 37, 20, 0], dtype=np.int64), 5, 0.0
    torch.manual_seed(5)
    x = torch.softmax(torch.randn(501, 4, 29) * 12, dim=2).numpy()
    return x, np.array([501, 300, 120, 40], dtype=np.int64), 8, 0.001


@pytest.mark.parametrize("sep", [None, 0])
@pytest.mark.parametrize("name", ["split", "config"])
def test_beam_over_row_windows_equals_the_whole_clip_decoder(name, sep):
    from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
    from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder
    x, lens, W, thr = _beam_case(name)
    Tn, N, V = x.shape
    xd = T(x).cuda()
    kw = dict(separator_index=sep, word_weight=1.7) if sep is not None else {}
    whole = CTCBeamDecoder(V - 1, W, thr, **kw)
    want = whole(xd, T(lens))
    assert want == O.ctc_beam_decode(x, lens, V - 1, W, thr, **kw)
    for window in (1, 7, 16, Tn):
        dec = StreamingCTCBeamDecoder(V - 1, W, thr, **kw)
        dec.begin(T(lens), Tn)
        assert dec.best() == [[] for _ in range(N)]
        pushes = 0
        for t0 in range(0, Tn, window):
            dec.push(xd[t0:t0 + window])
            pushes += 1
            k = min(t0 + window, Tn)
            if window == 7 and (name == "split" or pushes % 9 == 0):
                # the read-out after k rows = the whole-clip decoder on the first k rows; it does not disturb the search
                assert dec.best() == whole(xd[:k].contiguous(), T(np.minimum(lens, k))), k
        assert dec.result() == want, window
        assert dec.best() == want, window
    with pytest.raises(ValueError):
        dec.push(xd[:1])                                     # more rows than total_frames
    with pytest.raises(ValueError):
        dec.begin(T(lens), Tn)
        dec.push(xd[:4, :N - 1].contiguous())                # every window carries all streams


def test_beam_windows_on_the_reference_known_answers_without_language_model():
    from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder
    g = Golden("beam_kats")
    al = dict(zip("deouw_ ", range(7)))
    cases = [(g["kat2x2/x"], 2, dict(blank_index=1, beam_width=2, prune_threshold=0.0), g["kat2x2/out"].tolist()),
             (g["katlm/x"], 4, dict(blank_index=al["_"], beam_width=20), g["katlm/out_nolm"].tolist())]
    assert cases[0][3] == [0] and cases[1][3] == [al[c] for c in "do"]
    for x, n_frames, kw, want in cases:
        xd = T(x).cuda()
        for window in (1, n_frames):
            dec = StreamingCTCBeamDecoder(**kw)
            dec.begin(torch.tensor([n_frames], dtype=torch.int8), n_frames)
            for t0 in range(0, n_frames, window):
                dec.push(xd[t0:t0 + window])
            assert dec.result() == [want]


# ----------------------------------------------------------------------------- end to end
FIXTURES = ["ds2_tiny_gru_lookahead", "ds2_tiny_ctx_lstm_even_kernel", "ds2_tiny_ctx_gru_lookahead_act"]
# seed and scale of the normal values that replace the last Linear's weight, chosen on the CPU with the oracle's forward so
# that the longest stream's whole-clip greedy transcript has at least four labels (asserted below)
TALKATIVE = {"ds2_tiny_gru_lookahead": (1, 1.0), "ds2_tiny_ctx_lstm_even_kernel": (212, 64.0),
             "ds2_tiny_ctx_gru_lookahead_act": (1, 1.0)}


def _models(name):
    """(fixture, its model, a talkative copy of it)."""
    from test_gpu_parity import build_ds2, load_sd
    g = Golden(name)
    sd = g.sd()
    last = [k for k in sd if k.startswith("fully_connected.") and k.endswith("weight")][-1]
    seed, scale = TALKATIVE[name]
    sd2 = dict(sd)
    sd2[last] = (np.random.default_rng(seed).normal(size=sd[last].shape) * scale).astype(np.float32)
    hx = g["in/h0"] if g.has("in/h0") else None
    y, nl, _ = O.deep_speech_2_forward(g["in/x"], g["in/lens"], g.cfg, sd2, hx)
    assert len(O.ctc_greedy_decode(y, nl, g.cfg["blank"])[0]) >= 4        # a condition on the input
    return g, load_sd(build_ds2(g.cfg), sd), load_sd(build_ds2(g.cfg), sd2)


def _chunked_rows(model, x, lens, hx, chunk):
    """A plain ChunkedDeepSpeech2 run with the same chunking: the rows of every push, and the output lengths."""
    from myrtlespeech_amd.streaming import ChunkedDeepSpeech2
    total = x.shape[-1]
    c = ChunkedDeepSpeech2(model, chunk, carry_context=True)
    c.begin(lens, total, hx)
    rows = []
    for t0 in range(0, total, chunk):
        y = c.push(x[..., t0:t0 + chunk], final=(t0 + chunk >= total))
        rows.append(None if y is None else y.clone())
    return rows, c.out_lens


@pytest.mark.parametrize("name", FIXTURES)
def test_streaming_transcriber_greedy_equals_the_whole_clip_transcripts(name):
    from myrtlespeech_amd.post_process.ctc_greedy_decoder import CTCGreedyDecoder
    from myrtlespeech_amd.post_process.streaming import StreamingCTCGreedyDecoder
    from myrtlespeech_amd.streaming_decode import StreamingTranscriber
    g, plain, talkative = _models(name)
    blank = g.cfg["blank"]
    x, lens = T(g["in/x"]).cuda(), T(g["in/lens"])
    hx = T(g["in/h0"]) if g.has("in/h0") else None
    total, N = x.shape[-1], x.shape[0]
    for model, recorded in ((plain, g.has("out/greedy_flat")), (talkative, False)):
        for chunk in (1, 4, 13, total):
            tr = StreamingTranscriber(model, StreamingCTCGreedyDecoder(blank), chunk)
            tr.begin(lens, total, hx)
            lat = tr.chunked.latency_frames(total)
            news = []
            for t0 in range(0, total, chunk):
                pend = tr.push(x[..., t0:t0 + chunk], final=(t0 + chunk >= total))
                news.append(pend.result())
                if t0 + chunk < lat and t0 + chunk < total:
                    assert news[-1] == [[] for _ in range(N)], (t0, lat)
            got = tr.result()
            tr.decoder.check_status()
            assert _join(news, N) == got, chunk
            rows, out_lens = _chunked_rows(model, x, lens, hx, chunk)
            logits = torch.cat([r for r in rows if r is not None], 0)
            assert got == CTCGreedyDecoder(blank)(logits, out_lens), chunk
            if recorded:
                assert got == unragged(g["out/greedy_flat"], g["out/greedy_lens"]), chunk
            if model is talkative:
                assert len(got[0]) >= 4


@pytest.mark.parametrize("name", FIXTURES)
def test_streaming_transcriber_beam_equals_the_whole_clip_decoder_on_the_same_softmax_rows(name):
    from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
    from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder
    from myrtlespeech_amd.streaming_decode import StreamingTranscriber
    g, plain, talkative = _models(name)
    blank = g.cfg["blank"]
    x, lens = T(g["in/x"]).cuda(), T(g["in/lens"])
    hx = T(g["in/h0"]) if g.has("in/h0") else None
    total = x.shape[-1]
    for model in (plain, talkative):
        for chunk in (1, 4, 13, total):
            tr = StreamingTranscriber(model, StreamingCTCBeamDecoder(blank, 8), chunk)
            tr.begin(lens, total, hx)
            for t0 in range(0, total, chunk):
                tr.push(x[..., t0:t0 + chunk], final=(t0 + chunk >= total))
            got = tr.result()
            rows, out_lens = _chunked_rows(model, x, lens, hx, chunk)
            probs = torch.cat([torch.softmax(r, -1) for r in rows if r is not None], 0)
            assert got == CTCBeamDecoder(blank, 8)(probs, out_lens), chunk
            assert got == tr.decoder.best()


def test_streaming_transcriber_refuses_a_bidirectional_model():
    from test_gpu_parity import build_ds2, load_sd
    from myrtlespeech_amd.post_process.streaming import StreamingCTCGreedyDecoder
    from myrtlespeech_amd.streaming_decode import StreamingTranscriber
    g = Golden("ds2_tiny_bilstm")
    tr = StreamingTranscriber(load_sd(build_ds2(g.cfg), g.sd()), StreamingCTCGreedyDecoder(g.cfg["blank"]), 8)
    with pytest.raises(ValueError, match="bidirectional"):
        tr.begin(T(g["in/lens"]))
