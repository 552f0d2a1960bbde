"""The restatement of ``ms_edit_distance``'s specification (tests/edit_distance_ref.py) against what the project and the
reference already compute on the host, on every case of tests/edit_distance_cases.py and on random draws; and the argument
checks of ``post_process.edit_distance`` / ``wer.DeviceWordErrorRate`` that need no device.  Integer equality throughout."""
import numpy as np
import pytest
import torch

import edit_distance_cases as C
import edit_distance_ref as R
from myrtlespeech_amd.data.alphabet import Alphabet
from myrtlespeech_amd.post_process import EditCounts, edit_distance
from myrtlespeech_amd.post_process.utils import levenshtein
from myrtlespeech_amd.wer import DeviceWordErrorRate, WordErrorRate, WordSegmentor
from oracle.ds_oracle import levenshtein as oracle_levenshtein


def host_words(labels, separator, n_symbols):
    """The reference's pipeline, mapped back to labels: Alphabet.get_symbols -> WordSegmentor -> tuples of indices."""
    alphabet = Alphabet([chr(ord("a") + k) for k in range(n_symbols)])
    sep = alphabet.get_symbol(separator) if separator >= 0 else "#"
    assert sep is not None
    words = WordSegmentor(sep)(alphabet.get_symbols([int(v) for v in labels]))
    return [tuple(alphabet.get_index(ch) for ch in w) for w in words]


def check_pair(hyp, ref, mode, separator, n_symbols, row):
    a, b = R.units(hyp, mode, separator, n_symbols), R.units(ref, mode, separator, n_symbols)
    if mode == R.WORDS:
        assert a == host_words(hyp, separator, n_symbols) and b == host_words(ref, separator, n_symbols)
    dist, s, d, i, m, n = (int(v) for v in row)
    assert (m, n) == (len(a), len(b))
    assert dist == levenshtein(a, b) == oracle_levenshtein(a, b)
    assert s + d + i == dist
    assert m - i == n - d
    matches, in_b = m - i - s, set(b)
    assert matches >= 0 and sum(1 for u in a if u in in_b) >= matches


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_restatement_on_the_cases(case):
    want = C.expected(case.name)
    assert want.shape == (len(case.hyp), 6)
    for hyp, ref, row in zip(case.hyp, case.ref, want):
        check_pair(hyp, ref, case.mode, case.separator, case.n_symbols, row)


def test_restatement_on_random_draws():
    rng = np.random.default_rng(7)
    for _ in range(400):
        mode = int(rng.integers(0, 2))
        n_symbols = int(rng.integers(2, 5))
        separator = int(rng.integers(-1, n_symbols))
        lo, hi = (-1, n_symbols + 2) if mode == R.WORDS else (0, 3)
        hyp = rng.integers(lo, hi, size=int(rng.integers(0, 25))).tolist()
        ref = rng.integers(lo, hi, size=int(rng.integers(0, 25))).tolist()
        row = R.edit_distance([hyp], [ref], mode, separator, n_symbols)[0]
        check_pair(hyp, ref, mode, separator, n_symbols, row)


def test_known_counts_and_tie_order():
    # kitten -> sitting: two substitutions and one deletion (the reference has one unit more)
    assert R.counts("kitten", "sitting") == (3, 2, 1, 0, 6, 7)
    # "ab" against "ba", cost 2 three ways: the diagonal is tried first, so two substitutions
    assert R.counts("ab", "ba") == (2, 2, 0, 0, 2, 2)
    assert R.counts("", "abc") == (3, 0, 3, 0, 0, 3) and R.counts("abc", "") == (3, 0, 0, 3, 3, 0)
    # a dropped label joins its neighbours: "a", blank, "b" is the word "ab"
    assert R.units([0, 3, 1, 2, 2, 7, 1], R.WORDS, 2, 3) == [(0, 1), (1,)]
    assert R.units([0, 2, 1], R.WORDS, -1, 3) == [(0, 2, 1)]


def test_value_errors_need_no_device():
    ok = dict(hyp=[[1, 2]], hyp_lens=None, ref=[[1]], ref_lens=None)
    bad = [
        dict(ok, hyp=torch.zeros(1, 2), hyp_lens=torch.tensor([2])),                              # float labels
        dict(ok, ref=torch.zeros(1, 2, dtype=torch.int32), ref_lens=torch.tensor([2.0])),        # float lengths
        dict(ok, hyp=torch.zeros(3, dtype=torch.int32), hyp_lens=torch.tensor([2])),             # rows not 2-D
        dict(ok, hyp=torch.zeros(1, 2, dtype=torch.int32)),                                      # a tensor without lengths
        dict(ok, ref=[[1], [2]]),                                                                # batch mismatch between sides
        dict(ok, hyp_lens=torch.tensor([2, 2])),                                                 # ... between rows and lengths
        dict(ok, hyp_lens=torch.tensor([3])),                                                    # a length beyond its row
        dict(ok, ref=torch.zeros(1, 4, dtype=torch.int64), ref_lens=torch.tensor([5])),
        dict(ok, ref_lens=torch.tensor([-1])),                                                   # a negative length
        dict(ok, hyp=[[0] * 4097]),                                                              # above the limit
        dict(ok, hyp="ab"),
    ]
    for kwargs in bad:
        with pytest.raises(ValueError):
            edit_distance(kwargs["hyp"], kwargs["hyp_lens"], kwargs["ref"], kwargs["ref_lens"])
    with pytest.raises(ValueError):
        edit_distance([[1]], None, [[1]], None, separator_index=0)                               # word mode without n_symbols
    with pytest.raises(ValueError):
        edit_distance([[1]], None, [[1]], None, totals=torch.zeros(6, dtype=torch.int32))
    with pytest.raises(ValueError):
        edit_distance([[1]], None, [[1]], None, totals=torch.zeros(5, dtype=torch.int64))
    assert EditCounts(*range(6)).ref_units == 5


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("needs a CPU-only box")
    from myrtlespeech_amd.post_process.ctc_greedy_decoder import CTCGreedyDecoder
    with pytest.raises(RuntimeError, match="HIP device"):
        edit_distance([[1, 2]], None, [[1]], None)
    with pytest.raises(RuntimeError, match="HIP device"):
        DeviceWordErrorRate(Alphabet(list("ab ")), WordSegmentor(" ")).update([[0, 1]], torch.tensor([[0, 2, 1]]), torch.tensor([3]))
    with pytest.raises(RuntimeError, match="HIP device"):
        CTCGreedyDecoder(0).launch_device(torch.zeros(3, 1, 2), torch.tensor([3]))
    with pytest.raises(ValueError):
        CTCGreedyDecoder(0).launch_device(torch.zeros(3, 1, 2), torch.tensor([4]))


def test_device_word_error_rate_refuses_what_it_cannot_reproduce():
    class OtherSegmentor(WordSegmentor):
        def __call__(self, sentence):
            return ["".join(sentence)]

    plain = Alphabet(list("ab '"))
    assert DeviceWordErrorRate(plain, WordSegmentor(" ")).separator_index == 2
    assert DeviceWordErrorRate(plain, WordSegmentor("#")).separator_index == -1      # one character, not a symbol: no separator
    assert DeviceWordErrorRate(plain, WordSegmentor("ab"), unit="token").separator_index is None
    for alphabet, segmentor in [(Alphabet(["a", "th", " "]), WordSegmentor(" ")),         # "t","h" and "th" would join alike
                                (Alphabet(["a", "", " "]), WordSegmentor(" ")),
                                (plain, OtherSegmentor(" ")),
                                (plain, lambda s: s),
                                (plain, WordSegmentor("  ")),
                                (plain, WordSegmentor(""))]:
        with pytest.raises(ValueError):
            DeviceWordErrorRate(alphabet, segmentor)
    with pytest.raises(ValueError):
        DeviceWordErrorRate(plain, WordSegmentor(" "), unit="char")
    # with nothing accumulated the rate is the reference's 0 / 0
    with pytest.raises(ZeroDivisionError):
        DeviceWordErrorRate(plain, WordSegmentor(" ")).value()
    with pytest.raises(ZeroDivisionError):
        WordErrorRate(plain, WordSegmentor(" ")).value()


def test_size_query_without_gpu(lib):
    assert lib.ms_edit_distance_workspace_bytes(0, 10, 10) == 0
    small, large = lib.ms_edit_distance_workspace_bytes(3, 10, 10), lib.ms_edit_distance_workspace_bytes(3, 4096, 4096)
    assert 0 < small < large
    assert large >= 3 * (2 + 2048 + 2048) * 4
