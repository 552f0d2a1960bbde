"""The range-safe CTC prefix beam search on the device (ms_ctc_beam_decode_ex, CTCBeamDecoder(range_safe=True),
decode_nbest, StreamingCTCBeamDecoder.nbest) against the numpy restatement tests/beam_range_ref.py.  Every comparison is
an equality: transcripts, n-best prefixes, float32 score bits, scale_log2 and (host doubles from equal inputs) ln P.
Needs a real MI355X: -m gpu."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import beam_range_ref as R
from ngram_lm_cases import BLANK, SEP, decoder_model, sentence_posteriors

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def posteriors(scale, frames, N, V, seed=0):
    torch.manual_seed(seed)
    return torch.softmax(scale * torch.randn(frames, N, V), dim=2).numpy()


@functools.lru_cache(maxsize=None)
def clip(name):
    """(x, lens, blank, width, prune, separator, word_weight) of the named case -- built once, never modified."""
    if name == "generic":          # 8 symbols: the generic kernel; ~1e-118 per path in utterance 0
        return posteriors(0.3, 160, 3, 8), (160, 40, 0), 7, 4, 0.0, None, 1.0
    if name == "const":            # 29 x 8: the constant-shape kernel
        return posteriors(4, 200, 3, 29), (200, 200, 200), 28, 8, 1e-3, None, 1.0
    if name == "const_words":
        return posteriors(4, 200, 3, 29), (200, 200, 200), 28, 8, 1e-3, 0, 1.7
    if name == "big":              # 100 x 30 candidates do not fit the LDS: the working arrays are in the workspace
        return posteriors(0.3, 40, 2, 29), (40, 40), 28, 100, 1e-3, None, 1.0
    if name == "short":            # peaky and short: the rule never fires
        return posteriors(12, 40, 2, 29), (40, 31), 28, 8, 1e-3, None, 1.0
    if name == "generic_short":    # the first 48 frames of "generic": two rescales, every split affordable
        return posteriors(0.3, 160, 3, 8)[:48], (48, 20, 0), 7, 4, 0.0, None, 1.0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def want(name, range_safe=True):
    x, lens, blank, width, prune, sep, ww = clip(name)
    return R.decode(x, lens, blank, width, prune_threshold=prune, separator_index=sep, word_weight=ww, range_safe=range_safe)


LM_WEIGHT, LM_WORD_WEIGHT, LM_FRAMES = 1.3, 1.2, 210


@functools.lru_cache(maxsize=None)
def lm_clip():
    """The sentence-shaped posteriors of the device-model tests, tiled past 200 frames: the default search dies at ~150."""
    x, lens = sentence_posteriors(tile_to=LM_FRAMES)
    return x, tuple(int(v) for v in lens)


@functools.lru_cache(maxsize=None)
def lm_want():
    x, lens = lm_clip()
    return R.decode(x, lens, BLANK, 8, prune_threshold=1e-3, language_model=decoder_model(3).weighted_callable(LM_WEIGHT),
                    lm_weight=1.0, separator_index=SEP, word_weight=LM_WORD_WEIGHT, range_safe=True)


def abi_ex(x, lens, blank, width, prune, sep, word_weight, range_safe, pieces=None, lm=None, lm_weight=None):
    """ms_ctc_beam_decode_ex over the frame ranges `pieces` (default: one call), the read-out with the last:
    (transcripts, beams, score arrays, scale_log2 list)."""
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    xd, ld = _lib.f32c(T(x)), T(np.asarray(lens)).to(torch.int32).cuda()
    Tn, N, V = xd.shape
    out_idx = torch.zeros((N, Tn), dtype=torch.int32, device="cuda")
    out_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    beam_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    beam_idx = torch.zeros((N, width, Tn), dtype=torch.int32, device="cuda")
    beam_plen = torch.zeros((N, width), dtype=torch.int32, device="cuda")
    score = torch.zeros((N, width), dtype=torch.float32, device="cuda")
    scale = torch.full((N,), 12345, dtype=torch.int32, device="cuda")
    table = blob = wf = None
    if lm is not None:
        table, blob = lm.device_table(lm_weight)
        nbytes = lib.ms_ctc_beam_lm_workspace_bytes(Tn, N, V, width, lm.order)
    else:
        nbytes = lib.ms_ctc_beam_workspace_bytes(Tn, N, V, width)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ws.view(torch.int32).view(N, -1)[:, 14] = 12345      # a stale scale word: t_begin = 0 has to initialise it
    if sep is not None:
        vals = [float((1 + n) ** word_weight) for n in range(Tn + 2)]
        wf = torch.tensor(vals, dtype=torch.float64).to(torch.float32).cuda()
    pieces = pieces or [(0, Tn)]
    for k, (t0, t1) in enumerate(pieces):
        last = k == len(pieces) - 1
        _lib.check(lib.ms_ctc_beam_decode_ex(
            _lib.ptr(xd), _lib.ptr(ld), _lib.ptr(out_idx), _lib.ptr(out_len), Tn, N, V, blank, width, float(prune),
            -1 if sep is None else sep, _lib.ptr(wf), t0, t1, 0, Tn, None, 1 if last else 0,
            _lib.ptr(beam_len) if last else None, _lib.ptr(beam_idx) if last else None, _lib.ptr(beam_plen) if last else None,
            _lib.ptr(ws), ws.numel(), _lib.stream_ptr(), _lib.ptr(table),
            ctypes.c_void_p(blob.ctypes.data if blob is not None else 0), blob.size if blob is not None else 0,
            1 if range_safe else 0, _lib.ptr(score) if last else None, _lib.ptr(scale) if last else None),
            "ms_ctc_beam_decode_ex")
    bl, bi, bp = beam_len.cpu().tolist(), beam_idx.cpu().numpy(), beam_plen.cpu().numpy()
    oi, ol, sc = out_idx.cpu().numpy(), out_len.cpu().tolist(), score.cpu().numpy()
    beams = [[tuple(int(s) for s in bi[n, k, :bp[n, k]]) for k in range(bl[n])] for n in range(N)]
    return ([[int(s) for s in oi[n, :ol[n]]] for n in range(N)], beams, [sc[n, :bl[n]] for n in range(N)],
            scale.cpu().tolist())


def assert_equals_restatement(got, ref):
    outs, beams, scores, scales = got
    assert outs == R.transcripts(ref)
    assert beams == [r.beam for r in ref]
    assert scales == [r.scale_log2 for r in ref]
    for s, r in zip(scores, ref):
        np.testing.assert_array_equal(s.view(np.uint32), r.scores.astype(np.float32).view(np.uint32))


def assert_nbest_equals_restatement(hyps, ref, n=None):
    assert len(hyps) == len(ref)
    for h, r in zip(hyps, ref):
        k = len(r.beam) if n is None else min(n, len(r.beam))
        assert [tuple(v.indices) for v in h] == r.beam[:k]
        assert [v.log_prob for v in h] == R.log_probs(r)[:k]


def decoder(name, **kw):
    from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
    _, _, blank, width, prune, sep, ww = clip(name)
    return CTCBeamDecoder(blank, width, prune, separator_index=sep, word_weight=ww, **kw)


# ----------------------------------------------------------------------------- the kernels
def test_generic_kernel_survives_where_the_default_search_runs_empty():
    """Lengths 160 / 40 / 0: utterance 0 rescales eight times, utterance 1 twice (0.3 * randn over 8 symbols loses 2^-32 in
    ~19 frames, so 40 frames cannot go without; the clip that never rescales is test_short_peaky_clip_never_rescales), the
    third has no frame.  THE case that fails without the feature: the default decoder returns [] for utterance 0."""
    x, lens, blank, width, prune, sep, ww = clip("generic")
    ref = want("generic")
    assert [len(r.rescaled_at) for r in ref] == [8, 2, 0] and ref[0].scale_log2 < -250
    assert_equals_restatement(abi_ex(x, lens, blank, width, prune, sep, ww, True), ref)
    plain, safe = decoder("generic"), decoder("generic", range_safe=True)
    got_plain, got_safe = plain(T(x), T(np.asarray(lens))), safe(T(x), T(np.asarray(lens)))
    assert got_plain[0] == [] and len(got_safe[0]) > 60
    assert got_safe == R.transcripts(ref)
    assert got_plain[1:] == got_safe[1:]                      # float32 survives 40 frames: the same decoder there
    assert_nbest_equals_restatement(safe.decode_nbest(T(x), T(np.asarray(lens))), ref)
    assert_nbest_equals_restatement(safe.decode_nbest(T(x), T(np.asarray(lens)), n=2), ref, n=2)
    assert plain.decode_nbest(T(x), T(np.asarray(lens)))[0] == []      # an empty beam: no hypothesis


@pytest.mark.parametrize("name", ["const", "const_words"])
def test_constant_shape_kernel(name):
    x, lens, blank, width, prune, sep, ww = clip(name)
    ref = want(name)
    assert all(len(r.rescaled_at) >= 3 for r in ref)
    assert_equals_restatement(abi_ex(x, lens, blank, width, prune, sep, ww, True), ref)
    dec = decoder(name, range_safe=True)
    assert dec(T(x), T(np.asarray(lens))) == R.transcripts(ref)
    assert_nbest_equals_restatement(dec.decode_nbest(T(x), T(np.asarray(lens))), ref)


def test_working_arrays_in_the_workspace():
    x, lens, blank, width, prune, sep, ww = clip("big")
    ref = want("big")
    assert all(len(r.rescaled_at) == 4 and len(r.beam) == 100 for r in ref)
    assert_equals_restatement(abi_ex(x, lens, blank, width, prune, sep, ww, True), ref)
    assert_nbest_equals_restatement(decoder("big", range_safe=True).decode_nbest(T(x), T(np.asarray(lens)), n=5), ref, n=5)


def test_short_peaky_clip_never_rescales():
    x, lens, blank, width, prune, sep, ww = clip("short")
    ref = want("short")
    assert all(r.rescaled_at == [] and r.scale_log2 == 0 for r in ref)
    got = abi_ex(x, lens, blank, width, prune, sep, ww, True)
    assert_equals_restatement(got, ref)
    assert got[0] == decoder("short")(T(x), T(np.asarray(lens)))


def test_no_frames_at_all():
    from myrtlespeech_amd.post_process import BeamHypothesis
    dec = decoder("short", range_safe=True)
    assert dec(torch.zeros(0, 2, 29), torch.tensor([0, 0])) == [[], []]
    assert dec.decode_nbest(torch.zeros(0, 2, 29), torch.tensor([0, 0])) == [[BeamHypothesis([], 0.0)]] * 2
    # frames, but none of them this utterance's: the beam is the empty prefix with probability 1
    assert dec.decode_nbest(torch.full((3, 1, 29), 1 / 29), torch.tensor([0])) == [[BeamHypothesis([], 0.0)]]


# ----------------------------------------------------------------------------- the language model
def test_device_model_and_host_callable_past_200_frames():
    from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
    x, lens = lm_clip()
    ref = lm_want()
    lm = decoder_model(3)
    assert x.shape[0] > 200 and all(len(r.rescaled_at) >= 3 and len(r.beam) == 8 for r in ref)
    assert_equals_restatement(abi_ex(x, lens, BLANK, 8, 1e-3, SEP, LM_WORD_WEIGHT, True, lm=lm, lm_weight=LM_WEIGHT), ref)
    xt, lt = T(x), T(np.asarray(lens))
    kw = dict(separator_index=SEP, word_weight=LM_WORD_WEIGHT)
    dev = CTCBeamDecoder(BLANK, 8, 1e-3, language_model=lm, lm_weight=LM_WEIGHT, range_safe=True, **kw)
    host = CTCBeamDecoder(BLANK, 8, 1e-3, language_model=lm.weighted_callable(LM_WEIGHT), lm_weight=1.0, range_safe=True, **kw)
    assert dev(xt, lt) == host(xt, lt) == R.transcripts(ref)
    assert all(len(v) > 70 for v in R.transcripts(ref))       # (22 characters per ~57 frames: 77 .. 86 labels)
    assert_nbest_equals_restatement(dev.decode_nbest(xt, lt), ref)
    assert_nbest_equals_restatement(host.decode_nbest(xt, lt, n=3), ref, n=3)
    # what the default search makes of the same clip: float32 underflow to empty beams
    default = CTCBeamDecoder(BLANK, 8, 1e-3, language_model=lm, lm_weight=LM_WEIGHT, **kw)(xt, lt)
    assert sum(v == [] for v in default) >= 3


# ----------------------------------------------------------------------------- persisted state
def test_every_split_into_two_calls_equals_one_call():
    x, lens, blank, width, prune, sep, ww = clip("generic_short")
    ref = want("generic_short")
    whole = abi_ex(x, lens, blank, width, prune, sep, ww, True)
    assert_equals_restatement(whole, ref)
    assert ref[0].rescaled_at == [17, 37]                     # the splits at 18 and 38 follow a frame that rescales
    for cut in range(0, 49):
        got = abi_ex(x, lens, blank, width, prune, sep, ww, True, pieces=[(0, cut), (cut, 48)])
        assert_equals_restatement(got, ref)


@pytest.mark.parametrize("name", ["const_words", "big"])
def test_splits_behind_a_rescaling_frame_on_the_other_kernels(name):
    x, lens, blank, width, prune, sep, ww = clip(name)
    ref = want(name)
    Tn = x.shape[0]
    t = ref[0].rescaled_at[1]
    for cut in (t, t + 1, t + 2):
        if cut < Tn:
            assert_equals_restatement(abi_ex(x, lens, blank, width, prune, sep, ww, True, pieces=[(0, cut), (cut, Tn)]), ref)
    assert_equals_restatement(abi_ex(x, lens, blank, width, prune, sep, ww, True,
                                     pieces=[(0, 1), (1, t + 1), (t + 1, t + 1), (t + 1, Tn)]), ref)


def test_splits_with_the_device_model():
    x, lens = lm_clip()
    ref = lm_want()
    t = ref[0].rescaled_at[0]
    for cut in (t + 1, 150):
        got = abi_ex(x, lens, BLANK, 8, 1e-3, SEP, LM_WORD_WEIGHT, True, pieces=[(0, cut), (cut, x.shape[0])],
                     lm=decoder_model(3), lm_weight=LM_WEIGHT)
        assert_equals_restatement(got, ref)


@pytest.mark.parametrize("rows", [1, 7, 32])
def test_streaming_decoder_pushed_in_chunks(rows):
    from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder
    x, lens, blank, width, prune, sep, ww = clip("const_words")
    ref = want("const_words")
    dec = StreamingCTCBeamDecoder(blank, width, prune, separator_index=sep, word_weight=ww, range_safe=True)
    dec.begin(T(np.asarray(lens)), x.shape[0])
    xd = T(x).cuda()
    for t in range(0, x.shape[0], rows):
        dec.push(xd[t:t + rows])
    assert dec.result() == R.transcripts(ref)
    assert_nbest_equals_restatement(dec.nbest(), ref)
    assert_nbest_equals_restatement(dec.nbest(3), ref, n=3)
    assert dec.best() == R.transcripts(ref)                   # the read-outs do not disturb the search


def test_streaming_decoder_with_the_device_model():
    from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder
    x, lens = lm_clip()
    ref = lm_want()
    dec = StreamingCTCBeamDecoder(BLANK, 8, 1e-3, separator_index=SEP, word_weight=LM_WORD_WEIGHT,
                                  language_model=decoder_model(3), lm_weight=LM_WEIGHT, range_safe=True)
    dec.begin(T(np.asarray(lens)), x.shape[0])
    xd = T(x).cuda()
    for t in range(0, x.shape[0], 32):
        dec.push(xd[t:t + 32])
    assert dec.result() == R.transcripts(ref)
    assert_nbest_equals_restatement(dec.nbest(), ref)


# ----------------------------------------------------------------------------- range_safe=False
@pytest.mark.parametrize("name", ["short", "generic_short", "const_words"])
def test_nbest_of_the_default_search(name):
    """The kernels of the existing entry points and the workspace read-out: scale_log2 is 0, the scores are the plain
    restatement's, the first hypothesis is forward's transcript."""
    x, lens, blank, width, prune, sep, ww = clip(name)
    if name == "const_words":
        x, lens = x[:60], (60, 33, 0)
        ref = R.decode(x, lens, blank, width, prune_threshold=prune, separator_index=sep, word_weight=ww)
    else:
        ref = want(name, range_safe=False)
    assert all(r.scale_log2 == 0 and r.beam for r in ref)
    got = abi_ex(x, lens, blank, width, prune, sep, ww, False)
    assert got[3] == [0] * len(lens)
    assert_equals_restatement(got, ref)
    assert_equals_restatement(abi_ex(x, lens, blank, width, prune, sep, ww, False, pieces=[(0, 9), (9, x.shape[0])]), ref)
    dec = decoder(name)
    hyps = dec.decode_nbest(T(x), T(np.asarray(lens)))
    assert [h[0].indices for h in hyps] == dec(T(x), T(np.asarray(lens)))
    assert_nbest_equals_restatement(hyps, ref)


def test_nbest_of_the_default_search_with_the_device_model_and_streaming():
    from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
    from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder
    x, lens = sentence_posteriors()
    lm = decoder_model(3)
    ref = R.decode(x, lens, BLANK, 8, prune_threshold=1e-3, language_model=lm.weighted_callable(LM_WEIGHT), lm_weight=1.0,
                   separator_index=SEP, word_weight=LM_WORD_WEIGHT)
    kw = dict(separator_index=SEP, word_weight=LM_WORD_WEIGHT, language_model=lm, lm_weight=LM_WEIGHT)
    dec = CTCBeamDecoder(BLANK, 8, 1e-3, **kw)
    hyps = dec.decode_nbest(T(x), T(lens))
    assert_nbest_equals_restatement(hyps, ref)
    assert [h[0].indices for h in hyps] == dec(T(x), T(lens))
    host = CTCBeamDecoder(BLANK, 8, 1e-3, separator_index=SEP, word_weight=LM_WORD_WEIGHT,
                          language_model=lm.weighted_callable(LM_WEIGHT), lm_weight=1.0)
    assert_nbest_equals_restatement(host.decode_nbest(T(x), T(lens)), ref)
    stream = StreamingCTCBeamDecoder(BLANK, 8, 1e-3, **kw)
    stream.begin(T(lens), x.shape[0])
    xd = T(x).cuda()
    for t in range(0, x.shape[0], 16):
        stream.push(xd[t:t + 16])
    assert_nbest_equals_restatement(stream.nbest(), ref)
    assert stream.result() == R.transcripts(ref)
