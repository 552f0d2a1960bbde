"""CTC prefix beam search with the n-gram language model resident on the device (ms_ctc_beam_decode_lm).  Every
comparison is equality of integer transcripts or of float32 bit patterns.  The yardsticks: (1) the numpy oracle given
``lm.weighted_callable(a)`` and lm_weight 1.0, (2) this package's host-model path (ms_ctc_beam_decode fed lm_factor per
frame) given the same callable.  Needs a real MI355X: -m gpu."""
import ctypes
import io

import numpy as np
import pytest
import torch

from ngram_lm_cases import (ALPHABET, ARPA_TRIGRAM, BLANK, SEP, decoder_model, prefix_set, sentence_posteriors)
from oracle import ds_oracle as O
from util import Golden

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _word_factor(seq_len, word_weight):
    vals = [float((1 + n) ** word_weight) for n in range(seq_len + 2)]
    return torch.tensor(vals, dtype=torch.float64).to(torch.float32).cuda()


def _read_beam(beam_len, beam_idx, beam_plen):
    bl, bi, bp = beam_len.cpu().tolist(), beam_idx.cpu().numpy(), beam_plen.cpu().numpy()
    return [[tuple(int(s) for s in bi[n, k, :bp[n, k]]) for k in range(bl[n])] for n in range(len(bl))]


def _outputs(out_idx, out_len):
    oi, ol = out_idx.cpu().numpy(), out_len.cpu().tolist()
    return [[int(s) for s in oi[n, :ol[n]]] for n in range(len(ol))]


def abi_decode_lm(x, lens, lm, a, width, thr, word_weight, pieces=None, blank=BLANK):
    """ms_ctc_beam_decode_lm over the frame ranges `pieces` (default: one call): (transcripts, whole final beam, counters)."""
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    xd, ld = _lib.f32c(T(x)), T(np.asarray(lens)).to(torch.int32).cuda()
    Tn, N, V = xd.shape
    out_idx = torch.zeros((N, Tn), dtype=torch.int32, device="cuda")
    out_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    beam_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    beam_idx = torch.zeros((N, width, Tn), dtype=torch.int32, device="cuda")
    beam_plen = torch.zeros((N, width), dtype=torch.int32, device="cuda")
    per_utt = lib.ms_ctc_beam_lm_workspace_bytes(Tn, 1, V, width, lm.order)
    ws = torch.zeros(lib.ms_ctc_beam_lm_workspace_bytes(Tn, N, V, width, lm.order), dtype=torch.uint8, device="cuda")
    assert ws.numel() == per_utt * N
    table, blob = lm.device_table(a)
    wf = _word_factor(Tn, word_weight)
    pieces = pieces or [(0, Tn)]
    for k, (t0, t1) in enumerate(pieces):
        _lib.check(lib.ms_ctc_beam_decode_lm(
            _lib.ptr(xd), _lib.ptr(ld), _lib.ptr(out_idx), _lib.ptr(out_len), Tn, N, V, blank, width, float(thr), SEP,
            _lib.ptr(wf), t0, t1, 0, Tn, _lib.ptr(table), ctypes.c_void_p(blob.ctypes.data), blob.size,
            1 if k == len(pieces) - 1 else 0, _lib.ptr(beam_len), _lib.ptr(beam_idx), _lib.ptr(beam_plen), _lib.ptr(ws),
            ws.numel(), _lib.stream_ptr()), "ms_ctc_beam_decode_lm")
    hdr = ws.view(torch.int32).view(N, per_utt // 4)[:, :16].cpu().numpy()
    return _outputs(out_idx, out_len), _read_beam(beam_len, beam_idx, beam_plen), dict(nodes=int(hdr[:, 0].sum()),
                                                                                     factors=int(hdr[:, 13].sum()))


def abi_decode_host_factors(x, lens, fn, width, thr, word_weight, blank=BLANK):
    """Yardstick 2 through the ABI: ms_ctc_beam_decode advanced a frame at a time, lm_factor[n, w] =
    float32(fn(entry + (separator,))) for every beam entry that does not end in the separator (the kernel reads it only
    for a separator extension that survives pruning): (transcripts, whole final beam, factors applied that are not 1)."""
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    xd, ld = _lib.f32c(T(x)), T(np.asarray(lens)).to(torch.int32).cuda()
    Tn, N, V = xd.shape
    out_idx = torch.zeros((N, Tn), dtype=torch.int32, device="cuda")
    out_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    beam_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    beam_idx = torch.zeros((N, width, Tn), dtype=torch.int32, device="cuda")
    beam_plen = torch.zeros((N, width), dtype=torch.int32, device="cuda")
    ws = torch.zeros(lib.ms_ctc_beam_workspace_bytes(Tn, N, V, width), dtype=torch.uint8, device="cuda")
    wf = _word_factor(Tn, word_weight)

    def call(t0, t1, fac, finish):
        _lib.check(lib.ms_ctc_beam_decode(_lib.ptr(xd), _lib.ptr(ld), _lib.ptr(out_idx), _lib.ptr(out_len), Tn, N, V, blank,
                                          width, float(thr), SEP, _lib.ptr(wf), t0, t1, _lib.ptr(fac), finish,
                                          _lib.ptr(beam_len), _lib.ptr(beam_idx), _lib.ptr(beam_plen), _lib.ptr(ws),
                                          ws.numel(), _lib.stream_ptr()), "ms_ctc_beam_decode")

    call(0, 0, None, 0)
    not_one = 0
    sep_col = np.asarray(x)[:, :, SEP]
    for t in range(Tn):
        beam = _read_beam(beam_len, beam_idx, beam_plen)
        fac = np.ones((N, width), dtype=np.float32)
        for n in range(N):
            for k, pre in enumerate(beam[n]):
                if not (pre and pre[-1] == SEP):
                    fac[n, k] = np.float32(fn(pre + (SEP,)))
                    if t < lens[n] and not (sep_col[t, n] <= np.float32(thr)) and fac[n, k] != 1.0:
                        not_one += 1
        call(t, t + 1, torch.from_numpy(fac).cuda(), 1 if t == Tn - 1 else 0)
    return _outputs(out_idx, out_len), _read_beam(beam_len, beam_idx, beam_plen), not_one


def decoder(width, thr, lm=None, a=None, word_weight=1.0, blank=BLANK, sep=SEP):
    from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
    return CTCBeamDecoder(blank, width, thr, language_model=lm, lm_weight=a, separator_index=sep, word_weight=word_weight)


# ----------------------------------------------------------------------------- the look-ups alone
@pytest.mark.parametrize("weight", [0.5, 1.0, 1.7])
def test_score_kernel_bit_equal_to_the_host_walk(weight):
    from myrtlespeech_amd.language_model import NGramLanguageModel
    lm = NGramLanguageModel.from_arpa(io.StringIO(ARPA_TRIGRAM), ALPHABET, SEP)
    prefixes = prefix_set()
    for model in (lm, decoder_model(2), decoder_model(3)):
        got = model.score_on_device(prefixes, weight)
        want = np.asarray([model.factor(p, weight) for p in prefixes], dtype=np.float32)
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        assert bad.size == 0, (model, [(prefixes[i], got[i], want[i]) for i in bad[:5]])
        assert (want != 1.0).sum() > len(prefixes) // 2


def test_score_kernel_five_gram_and_no_bos():
    from myrtlespeech_amd.language_model import NGramLanguageModel
    grams = {("<unk>",): (-2.0, -0.1), ("a",): (-0.5, -0.2), ("b",): (-0.7, -0.3), ("a", "b"): (-0.3, -0.15),
             ("b", "a", "b"): (-0.25, -0.1), ("a", "b", "a", "b"): (-0.2, -0.05), ("a", "b", "a", "b", "a"): (-0.1, None),
             ("b", "a"): (-0.35, -0.2), ("a", "b", "a"): (-0.22, None), ("b", "a", "b", "a"): (-0.21, None)}
    lm = NGramLanguageModel(grams, ALPHABET, SEP)
    assert lm.order == 5 and lm.bos_id == -1
    rng = np.random.default_rng(3)
    prefixes = []
    for _ in range(2000):
        words = ["ab"[int(k)] if k < 2 else "c" for k in rng.integers(0, 3, size=int(rng.integers(1, 9)))]
        prefixes.append(tuple(ALPHABET.index(ch) for ch in " ".join(words)) + (SEP,))
    got = lm.score_on_device(prefixes, 1.3)
    want = np.asarray([lm.factor(p, 1.3) for p in prefixes], dtype=np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


# ----------------------------------------------------------------------------- inputs on which the model matters
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("a", [0.7, 1.3])
def test_sentences_equal_the_oracle_and_the_host_path(order, a):
    lm = decoder_model(order)
    x, lens = sentence_posteriors()
    assert len(set(lens.tolist())) > 1                      # ragged
    width, thr, b = 8, 1e-3, 1.2
    got = decoder(width, thr, lm, a, b)(T(x), T(lens))
    # yardstick 1: the oracle
    want = O.ctc_beam_decode(x, lens, BLANK, width, thr, language_model=lm.weighted_callable(a), lm_weight=1.0,
                             separator_index=SEP, word_weight=b)
    assert got == want
    # yardstick 2: the host-model path, as a decoder and through the ABI (whole beam)
    assert decoder(width, thr, lm.weighted_callable(a), 1.0, b)(T(x), T(lens)) == want
    out_h, beam_h, not_one = abi_decode_host_factors(x, lens, lm.weighted_callable(a), width, thr, b)
    out_d, beam_d, counters = abi_decode_lm(x, lens, lm, a, width, thr, b)
    assert out_d == out_h == want
    assert beam_d == beam_h and all(len(bm) == width for bm in beam_d)
    # the model matters here: a decoder that ignores the table cannot pass
    plain = decoder(width, thr, None, None, b)(T(x), T(lens))
    assert sum(p != q for p, q in zip(plain, got)) >= 1
    assert not_one >= 1 and counters["factors"] >= 1
    print(f"order {order}, lm_weight {a}: {sum(p != q for p, q in zip(plain, got))} of {len(got)} transcripts change with "
          f"the model; {counters['nodes']} nodes, {counters['factors']} factors computed, {not_one} factors != 1 applied")


# ----------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("width", [1, 4, 8, 16, 32, 96])
def test_widths_at_29_symbols(width):
    """1: the generic kernel; 4 .. 32: the constant-shape twins; 96: the working arrays do not fit the LDS (BIG)."""
    lm = decoder_model(3)
    x, lens = sentence_posteriors(seed=11 + width)
    if width == 96:
        x, lens = x[:30], np.minimum(lens, 30)
    a, b, thr = 1.3, 1.2, 1e-3
    want = decoder(width, thr, lm.weighted_callable(a), 1.0, b)(T(x), T(lens))
    assert decoder(width, thr, lm, a, b)(T(x), T(lens)) == want
    if width <= 8:
        assert want == O.ctc_beam_decode(x, lens, BLANK, width, thr, language_model=lm.weighted_callable(a), lm_weight=1.0,
                                         separator_index=SEP, word_weight=b)


def test_another_alphabet_takes_the_generic_kernel():
    from myrtlespeech_amd.language_model import NGramLanguageModel
    alphabet = [" "] + list("abcdefghij") + ["_"]         # 12 symbols, separator 0, blank 11
    grams = {("<s>",): (-99, -0.2), ("<unk>",): (-1.5, None), ("ab",): (-0.6, -0.3), ("ba",): (-0.8, -0.2), ("cab",): (-1.0, None),
             ("a",): (-0.9, -0.1), ("<s>", "ab"): (-0.2, None), ("ab", "ba"): (-0.25, None), ("ba", "a"): (-0.3, None)}
    lm = NGramLanguageModel(grams, alphabet, 0)
    torch.manual_seed(2)
    x = torch.softmax(torch.randn(80, 5, 12) * 2.5, dim=2)
    x[:, :, :4] *= 3                                       # separators and a / b / c often: words of the vocabulary appear
    x = x / x.sum(dim=2, keepdim=True)
    lens = torch.tensor([80, 61, 33, 0, 7])
    a, b = 0.8, 1.1
    want = decoder(8, 1e-3, lm.weighted_callable(a), 1.0, b, blank=11, sep=0)(x, lens)
    assert decoder(8, 1e-3, lm, a, b, blank=11, sep=0)(x, lens) == want
    assert want == O.ctc_beam_decode(x.numpy(), lens.numpy(), 11, 8, 1e-3, language_model=lm.weighted_callable(a),
                                     lm_weight=1.0, separator_index=0, word_weight=b)
    assert want[3] == []                                   # an utterance of length 0
    with pytest.raises(ValueError, match="alphabet"):
        decoder(8, 1e-3, decoder_model(2), a, b, blank=11, sep=0)(x, lens)


@pytest.mark.parametrize("batch", [1, 32])
def test_batches_and_prune_threshold_zero(batch):
    """prune threshold 0: every frame consults the model."""
    lm = decoder_model(2)
    xs, ls = zip(*(sentence_posteriors(seed=100 + k) for k in range(batch // 4 + 1)))
    Tn = min(v.shape[0] for v in xs)
    x = np.concatenate([v[:Tn] for v in xs], axis=1)[:, :batch]
    lens = np.minimum(np.concatenate(ls)[:batch], Tn)
    if batch > 1:
        lens[5] = 0
    a, b = 0.7, 1.2
    for thr in (0.0, 1e-3):
        want = decoder(4, thr, lm.weighted_callable(a), 1.0, b)(T(x), T(lens))
        assert decoder(4, thr, lm, a, b)(T(x), T(lens)) == want


# ----------------------------------------------------------------------------- the decode size of the configuration
def test_config_size_against_the_oracle():
    """T = 501, 4 ragged utterances of peaky random posteriors (tests/golden/beam_cfg2.npz's, regenerated from its seed):
    mostly out-of-vocabulary words, the <unk> / back-off walk at length."""
    g = Golden("beam_cfg2")
    c = g.cfg
    torch.manual_seed(c["seed"])
    x = torch.softmax(torch.randn(c["T"], c["N"], c["V"]) * c["scale"], dim=2)
    np.testing.assert_array_equal(x[::50, :, ::7].numpy(), g["in/x_probe"])
    lens = T(g["in/lens"])
    assert c["sep"] == SEP and c["T"] == 501 and c["N"] == 4
    lm, a = decoder_model(3, unk_log10_p=-0.05), 1.3
    got = decoder(c["beam_width"], c["prune"], lm, a, c["word_weight"])(x, lens)
    want = O.ctc_beam_decode(x.numpy(), lens.numpy(), 28, c["beam_width"], c["prune"], language_model=lm.weighted_callable(a),
                             lm_weight=1.0, separator_index=SEP, word_weight=c["word_weight"])
    assert got == want
    assert got != decoder(c["beam_width"], c["prune"], None, None, c["word_weight"])(x, lens)
    assert all(len(v) > 20 for v in got)                   # the search survived (no float32 underflow to empty beams)


def test_config_size_batch_of_32_against_the_host_path():
    torch.manual_seed(5)
    x = torch.softmax(torch.randn(501, 32, 29) * 12, dim=2)
    lens = torch.sort(torch.randint(100, 502, (32,)), descending=True).values
    lens[0] = 501
    lm, a, b = decoder_model(3, unk_log10_p=-0.05), 0.7, 1.2
    host = decoder(8, 1e-3, lm.weighted_callable(a), 1.0, b)
    want = host(x, lens)
    assert decoder(8, 1e-3, lm, a, b)(x, lens) == want
    assert all(len(v) > 20 for v in want)                  # no beam ran empty
    assert want != decoder(8, 1e-3, None, None, b)(x, lens)
    assert host.lm_calls > 1000


# ----------------------------------------------------------------------------- in pieces
def test_decode_advanced_in_pieces_equals_one_call():
    lm, a, b = decoder_model(3, unk_log10_p=-0.05), 1.3, 1.2
    # two utterances of peaky random posteriors at the configuration's length, two of sentences (120 frames: the linear float32
    # search underflows to an empty beam on longer ones once a factor below 1 per word comes on top of the acoustics)
    torch.manual_seed(9)
    x = torch.softmax(torch.randn(501, 4, 29) * 12, dim=2).numpy()
    x[:120, 2:] = sentence_posteriors(tile_to=120)[0][:, :2]
    lens = np.asarray([501, 350, 7, 120])
    whole = abi_decode_lm(x, lens, lm, a, 8, 1e-3, b)
    cuts = [0, 7, 8, 200, 201, 350, 501]
    parts = abi_decode_lm(x, lens, lm, a, 8, 1e-3, b, pieces=list(zip(cuts[:-1], cuts[1:])))
    assert parts == whole
    assert whole[0] == decoder(8, 1e-3, lm, a, b)(T(x), T(lens))
    assert whole[2]["factors"] <= whole[2]["nodes"]        # a factor is computed at most once per node
    assert all(len(v) > 0 for v in whole[0])               # no beam ran empty


def test_streaming_decoder_with_the_model():
    from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder
    lm, a, b = decoder_model(2), 1.3, 1.2
    x, lens = sentence_posteriors(seed=21)
    Tn = x.shape[0]
    whole = decoder(8, 1e-3, lm, a, b)
    want = whole(T(x), T(lens))
    dec = StreamingCTCBeamDecoder(BLANK, 8, 1e-3, separator_index=SEP, word_weight=b, language_model=lm, lm_weight=a)
    dec.begin(T(lens), Tn)
    xd = T(x).cuda()
    t = 0
    for r in [1, 7, 2, 16, 5, 64]:
        rows = xd[t:t + r]
        if rows.shape[0] == 0:
            break
        dec.push(rows)
        t += rows.shape[0]
        assert dec.best() == whole(T(x[:t]), T(np.minimum(lens, t))), t
    assert t == Tn
    assert dec.result() == want
    assert want != decoder(8, 1e-3, None, None, b)(T(x), T(lens))
