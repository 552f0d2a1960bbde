"""NGramLanguageModel without a GPU: the ARPA text parses to the values typed in here, the packed table agrees with the
model's meaning to the derived float32 bound, the blob keeps its invariants and ms_ngram_lm_table_check refuses damaged
ones, and the decoders' argument errors."""
import io

import numpy as np
import pytest

from ngram_lm_cases import ALPHABET, ARPA_TRIGRAM, SEP, ask, prefix_set, spell

from myrtlespeech_amd.language_model import HEADER_BYTES, MAGIC, NGramLanguageModel, _fin, _step


@pytest.fixture(scope="module")
def lm():
    return NGramLanguageModel.from_arpa(io.StringIO(ARPA_TRIGRAM), ALPHABET, SEP)


def test_arpa_text_parses_to_the_values_on_its_lines(lm, tmp_path):
    path = tmp_path / "toy.arpa"
    path.write_text(ARPA_TRIGRAM)
    from_file = NGramLanguageModel.from_arpa(str(path), ALPHABET, SEP)
    assert lm.order == from_file.order == 3
    cases = [
        (ask("the cat sat"), -0.15),                          # a stored trigram
        (ask("the cat"), -0.10),                              # ... with <s> in its context
        (ask("sat on the cat"), -0.15 - 0.30),                # back-off(on the), bigram the cat
        (ask("cat sat on cat"), -0.20 - 0.45 - 1.10),         # back-off(sat on), back-off(on), unigram
        (ask("cap map the"), -0.10 - 0.70),                   # "cap map" is not stored: back-off(map), unigram
        (ask("the dog"), -0.20 - 0.40 - 1.20),                # out of vocabulary: back-off(<s> the), back-off(the), <unk>
        (ask("dog cat"), -1.10),                              # <unk> in the context, nothing stored about it
        (ask("the"), -0.25),                                  # a word after <s> only
        (ask("a"), -0.90),
        (ask("zzz"), -0.30 - 1.20),                           # back-off(<s>), <unk>
        (ask("the  cat"), -0.10),                             # runs of separators
        (ask("  the   cat  sat"), -0.15),
        (ask(" the"), -0.25),
        (spell("the cat sat"), -0.15),                        # without the trailing separator: the same word is scored
    ]
    for prefix, log10_sum in cases:
        assert lm(prefix) == pytest.approx(10 ** log10_sum, rel=1e-12), prefix
        assert from_file(prefix) == lm(prefix)
    for empty in [(), (SEP,), ask("the "), (SEP, SEP)]:       # the empty word: exactly 1
        assert lm(empty) == 1.0
        assert lm.factor(empty, 1.3) == np.float32(1.0)


@pytest.mark.parametrize("weight", [0.5, 1.0, 1.7])
def test_packed_table_against_the_meaning(lm, weight):
    """factor() walks the packed bytes; lm() the dictionaries in double.  One float32 rounding per stored factor and one
    per multiply, at most order back-offs + one probability: relative error <= (2 * order + 1) * 2^-24."""
    prefixes = prefix_set()
    assert len(prefixes) >= 2000
    bound = (2 * lm.order + 1) * 2.0 ** -24
    worst = 0.0
    for p in prefixes:
        want = lm(p) ** weight
        got = lm.factor(p, weight)
        assert got.dtype == np.float32
        worst = max(worst, abs(float(got) - want) / want)
    print(f"lm_weight {weight}: worst relative error {worst / 2.0 ** -24:.2f} x 2^-24, bound {2 * lm.order + 1} x 2^-24")
    assert worst <= bound
    if weight == 1.0:
        f = lm.weighted_callable(1.0)
        assert all(np.float32(f(p) ** 1.0) == lm.factor(p, 1.0) for p in prefixes[:500])


def _tables(blob):
    hdr = blob[:HEADER_BYTES].view(np.uint32)
    v = blob[hdr[12]:hdr[12] + 16 * (1 << int(hdr[2]))]
    n = blob[hdr[13]:hdr[13] + 16 * (1 << int(hdr[3]))]
    return hdr, v.view(np.uint64).reshape(-1, 2)[:, 0], n.view(np.uint64).reshape(-1, 2)[:, 0]


def test_blob_invariants(lm):
    blob = lm.packed(1.3)
    assert blob is lm.packed(1.3) and blob.dtype == np.uint8          # cached per weight
    hdr, vkeys, nkeys = _tables(blob)
    assert hdr[0] == MAGIC and hdr[1] == 3 and hdr[14] == blob.size
    for keys, probes, count in ((vkeys, int(hdr[10]), len(lm._spelling)), (nkeys, int(hdr[11]), len(lm._prob))):
        slots = len(keys)
        assert slots & (slots - 1) == 0
        stored = [int(k) for k in keys if k != 0]
        assert len(stored) == count and len(set(stored)) == count and count <= slots // 2
        # the recorded probe bound is the true maximum: the farthest a stored key sits from its home slot, + 1
        far = max((s - (int(k) & (slots - 1))) % slots + 1 for s, k in enumerate(keys) if k != 0)
        assert far == probes
    # the hash is the documented one
    the = int(hdr[4]) | (int(hdr[5]) << 32)
    for s in spell("the"):
        the = _step(the, s)
    assert _fin(the) in set(int(k) for k in vkeys)
    # a factor that underflows float32's normal range is stored as 0, a missing back-off as 1
    n = blob[hdr[13]:].view(np.float32).reshape(-1, 4)
    assert (n[nkeys != 0][:, 2:] >= 0).all() and (n[nkeys != 0][:, 2] == 0).sum() == 1           # <s>'s 10 ** -99
    assert (n[nkeys != 0][:, 3] == 1).sum() >= 8


def test_table_check_accepts_the_blob_and_refuses_damage(lm, lib):
    import ctypes
    blob = lm.packed(1.0)

    def rc(b, size=None):
        b = np.ascontiguousarray(b)
        return lib.ms_ngram_lm_table_check(ctypes.c_void_p(b.ctypes.data), b.size if size is None else size)

    assert rc(blob) == 0
    lm.check_packed(blob)
    assert rc(blob[:-16].copy()) != 0                      # truncated
    assert rc(blob[:32].copy()) != 0                       # shorter than the header

    def damaged(word, value):
        b = blob.copy()
        b[:HEADER_BYTES].view(np.uint32)[word] = value
        return b

    assert rc(damaged(0, 0x12345678)) != 0                 # wrong magic
    assert rc(damaged(1, 0)) != 0 and rc(damaged(1, 6)) != 0          # order 0 / 6
    assert rc(damaged(13, blob.size)) != 0                 # an offset past the end
    assert rc(damaged(12, blob.size - 16)) != 0
    slots = 1 << int(blob[:HEADER_BYTES].view(np.uint32)[3])
    assert rc(damaged(11, slots + 1)) != 0                 # a probe bound larger than the table
    assert rc(damaged(10, 1 << 20)) != 0
    assert rc(damaged(2, 40)) != 0                         # slot count
    with pytest.raises(ValueError, match="magic"):
        lm.check_packed(damaged(0, 1))
    assert b"magic" in lib.ms_last_error()


def test_constructor_errors():
    uni = {("<unk>",): (-1.0, None), ("the",): (-0.5, -0.1)}
    NGramLanguageModel(uni, ALPHABET, SEP)
    with pytest.raises(ValueError, match="unk_log10_p"):
        NGramLanguageModel({("the",): (-0.5, None)}, ALPHABET, SEP)
    no_unk = NGramLanguageModel({("the",): (-0.5, None)}, ALPHABET, SEP, unk_log10_p=-3.0)
    assert no_unk(ask("qq")) == pytest.approx(1e-3)
    with pytest.raises(ValueError, match="café"):
        NGramLanguageModel({**uni, **{("café",): (-1.0, None)}}, ALPHABET, SEP)
    with pytest.raises(ValueError, match="order"):
        NGramLanguageModel({**uni, **{("the",) * 6: (-1.0, None)}}, ALPHABET, SEP)
    with pytest.raises(ValueError):
        NGramLanguageModel({}, ALPHABET, SEP)
    with pytest.raises(ValueError, match="separator_index"):
        NGramLanguageModel(uni, ALPHABET, 29)
    with pytest.raises(ValueError, match="order"):
        NGramLanguageModel.from_arpa(io.StringIO("\\data\\\nngram 6=1\n\n\\6-grams:\n-1 a a a a a a\n\\end\\\n"), ALPHABET, SEP)
    five = NGramLanguageModel({**uni, **{("the",) * 5: (-0.2, None), ("the",) * 2: (-0.3, -0.1)}}, ALPHABET, SEP)
    assert five.order == 5
    assert five(ask("the the the the the")) == pytest.approx(10 ** -0.2)
    assert float(five.factor(ask("the the the the the"), 1.0)) == pytest.approx(10 ** -0.2, rel=1e-6)
    # </s> entries are read and ignored
    eos = NGramLanguageModel({**uni, **{("the", "</s>"): (-0.1, None), ("</s>",): (-1.0, None)}}, ALPHABET, SEP)
    assert eos.order == 1


def test_decoder_argument_errors(lm):
    from myrtlespeech_amd.post_process import NGramLanguageModel as exported
    from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
    from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder
    assert exported is NGramLanguageModel
    with pytest.raises(ValueError, match="lm_weight"):
        CTCBeamDecoder(28, 8, language_model=lm, separator_index=SEP)
    with pytest.raises(ValueError, match="separator_index"):
        CTCBeamDecoder(28, 8, language_model=lm, lm_weight=1.0, separator_index=3)
    CTCBeamDecoder(28, 8, language_model=lm, lm_weight=1.0, separator_index=SEP)
    CTCBeamDecoder(28, 8, language_model=lm, lm_weight=1.0)               # no separator: never consulted, as the reference
    with pytest.raises(ValueError, match="language_model"):
        StreamingCTCBeamDecoder(0, 2, language_model=lambda p: 1.0, lm_weight=1.0)
    with pytest.raises(ValueError, match="lm_weight"):
        StreamingCTCBeamDecoder(28, 8, separator_index=SEP, language_model=lm)
    with pytest.raises(ValueError, match="separator_index"):
        StreamingCTCBeamDecoder(28, 8, separator_index=3, language_model=lm, lm_weight=1.0)
    StreamingCTCBeamDecoder(28, 8, separator_index=SEP, language_model=lm, lm_weight=1.0)


def test_workspace_size_queries(lib):
    base = lib.ms_ctc_beam_workspace_bytes(501, 4, 29, 8)
    with_lm = lib.ms_ctc_beam_lm_workspace_bytes(501, 4, 29, 8, 3)
    assert with_lm > base > 0
    assert lib.ms_ctc_beam_lm_workspace_bytes(501, 4, 29, 8, 0) == 0 == lib.ms_ctc_beam_lm_workspace_bytes(501, 4, 29, 8, 6)
