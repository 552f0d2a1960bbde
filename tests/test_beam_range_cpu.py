"""The range-safe prefix beam search on the CPU: the numpy restatement (tests/beam_range_ref.py) against the oracle, against
itself without the rule, and against its float64 twin; argument validation of the new options.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import beam_range_ref as R
from oracle import ds_oracle as O

# ln P of the float32 search against the float64 twin: the largest difference the restatement shows over every beam entry
# of the seeds below is 9.94e-7 (float32 rounding of ~200 frames' sums and products, not the rescaling, which is exact);
# four times that is allowed for other platforms' libm (log) and numpy builds
MEASURED_LN_P_DIFF = 9.94e-7
LN_P_TOL = 4 * MEASURED_LN_P_DIFF


def posteriors(scale, T, N, V, seed=0):
    torch.manual_seed(seed)
    return torch.softmax(scale * torch.randn(T, N, V), dim=2).numpy()


@functools.lru_cache(maxsize=None)
def runs(scale, T, N, V, width, prune, sep=None, word_weight=1.0):
    """(posteriors, plain float32, range-safe float32, plain float64) -- computed once, shared, never modified."""
    x = posteriors(scale, T, N, V)
    kw = dict(prune_threshold=prune, separator_index=sep, word_weight=word_weight)
    lens = [T] * N
    return (x, R.decode(x, lens, V - 1, width, **kw), R.decode(x, lens, V - 1, width, range_safe=True, **kw),
            R.decode(x, lens, V - 1, width, dtype=np.float64, **kw))


@pytest.mark.parametrize("kw", [dict(), dict(separator_index=0, word_weight=1.7),
                                dict(separator_index=0, word_weight=0.5, language_model=O.toy_language_model, lm_weight=1.3)])
def test_without_the_rule_the_restatement_is_the_oracle(kw):
    for scale, T, N, V, width, prune in [(12, 60, 3, 29, 8, 1e-3), (2, 40, 2, 6, 3, 0.0), (4, 50, 2, 29, 2, 1e-2)]:
        x = posteriors(scale, T, N, V, seed=3)
        lens = [T, T // 2, 0][:N]
        if kw.get("language_model") is not None and V != 29:
            continue
        want = O.ctc_beam_decode(x, lens, V - 1, width, prune, **kw)
        got = R.decode(x, lens, V - 1, width, prune_threshold=prune, **kw)
        assert R.transcripts(got) == want
        assert all(r.scale_log2 == 0 and r.rescaled_at == [] for r in got)


@pytest.mark.parametrize("sep,word_weight", [(None, 1.0), (0, 1.7)])
def test_peaky_posteriors_rescale_and_equal_the_plain_search(sep, word_weight):
    """softmax(12 * randn(200, 3, 29)): float32 survives, so the whole beam and its TRUE scores must not change."""
    _, plain, safe, _ = runs(12, 200, 3, 29, 8, 1e-3, sep, word_weight)
    for p, s in zip(plain, safe):
        assert len(p.beam[0]) > 150
        assert s.beam == p.beam
        assert len(s.rescaled_at) >= 1 and s.scale_log2 < -32 and p.scale_log2 == 0
        # the stored scores differ by exactly 2^scale: the rescaling rounds nothing
        np.testing.assert_array_equal(np.ldexp(s.scores.astype(np.float64), s.scale_log2), p.scores.astype(np.float64))


def test_flatter_posteriors_equal_the_float64_search():
    """softmax(4 * randn(200, 3, 29)): three to four rescales; on these seeds the plain float32 search still agrees too."""
    _, plain, safe, twin = runs(4, 200, 3, 29, 8, 1e-3)
    for p, s, d in zip(plain, safe, twin):
        assert len(s.rescaled_at) >= 3
        assert s.beam == d.beam and s.beam[0] == p.beam[0]


def test_where_float32_underflows_the_range_safe_search_is_the_float64_one():
    """softmax(0.3 * randn(200, 2, 8)), width 4: about 1e-147 per path."""
    _, plain, safe, twin = runs(0.3, 200, 2, 8, 4, 1e-3)
    for p, s, d in zip(plain, safe, twin):
        assert p.beam == []                                # the reference's failure mode
        assert len(s.beam) == 4 and len(s.beam[0]) > 100
        assert s.beam == d.beam
        assert len(s.rescaled_at) == 10 and s.scale_log2 < -300
        assert s.scores[0] >= 2.0 ** -32                   # what the rule guarantees for the best entry


def test_log_prob_against_the_float64_twin():
    """Measured on these seeds: 9.94e-7 at most (MEASURED_LN_P_DIFF); asserted at four times that."""
    worst = 0.0
    for args in [(12, 200, 3, 29, 8, 1e-3), (12, 200, 3, 29, 8, 1e-3, 0, 1.7), (4, 200, 3, 29, 8, 1e-3), (0.3, 200, 2, 8, 4, 1e-3)]:
        _, _, safe, twin = runs(*args)
        for s, d in zip(safe, twin):
            assert s.beam == d.beam
            diff = np.abs(np.asarray(R.log_probs(s)) - np.asarray(R.log_probs(d)))
            worst = max(worst, float(diff.max()))
    print(f"largest |ln p (float32, range-safe) - ln p (float64)| = {worst:.3e}")
    assert worst <= LN_P_TOL


def test_subnormal_best_entry_takes_the_smallest_exponent():
    """A frame of probabilities 1e-40 takes a rescaled beam (best entry in [1, 2)) into float32's subnormals: e is -126,
    the exponent IEEE gives a subnormal, so the factor 2^126 still fits an exponent field.  The subnormal product kept
    ~16 bits (1e-40 / 2^-149 = 7e4), hence ln p agrees with the float64 twin to 2^-16 = 1.5e-5 per entry, not to LN_P_TOL."""
    x = np.asarray([[0.5, 0.25, 0.25], [1e-20] * 3, [1e-40] * 3, [0.3, 0.3, 0.4]], dtype=np.float32)
    r = R.search(x, 4, 2, 2, prune_threshold=0.0, range_safe=True)
    assert r.rescaled_at == [1, 2]
    e1 = int(np.frexp(R.search(x, 2, 2, 2, prune_threshold=0.0).scores[0])[1]) - 1
    assert -70 < e1 < -60 and r.scale_log2 == e1 - 126
    twin = R.search(x, 4, 2, 2, prune_threshold=0.0, dtype=np.float64)
    assert r.beam == twin.beam and len(r.beam) == 2
    assert R.search(x, 4, 2, 2, prune_threshold=0.0).beam == []
    assert np.abs(np.asarray(R.log_probs(r)) - np.asarray(R.log_probs(twin))).max() < 2 * 2.0 ** -16


def test_constructor_and_argument_validation():
    from myrtlespeech_amd.post_process import BeamHypothesis
    from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
    from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder
    assert CTCBeamDecoder(0, 2).range_safe is False and StreamingCTCBeamDecoder(0, 2).range_safe is False
    assert CTCBeamDecoder(0, 2, range_safe=True).range_safe is True
    assert "range_safe" not in repr(CTCBeamDecoder(0, 2)) and "range_safe=True" in repr(CTCBeamDecoder(0, 2, range_safe=True))
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="range_safe"):
            CTCBeamDecoder(0, 2, range_safe=bad)
        with pytest.raises(ValueError, match="range_safe"):
            StreamingCTCBeamDecoder(0, 2, range_safe=bad)
    h = BeamHypothesis([1, 2], -0.5)
    assert h.indices == [1, 2] and h.log_prob == -0.5 and tuple(h) == ([1, 2], -0.5)
    x = torch.zeros(5, 2, 4)
    for dec in (CTCBeamDecoder(0, 2), CTCBeamDecoder(0, 2, range_safe=True)):
        for bad in (0, -1, 1.5, True):
            with pytest.raises(ValueError, match="n="):
                dec.decode_nbest(x, torch.tensor([5, 3]), n=bad)
        with pytest.raises(ValueError):
            dec.decode_nbest(x, torch.tensor([5.0, 3.0]))          # float lengths
        with pytest.raises(ValueError):
            dec.decode_nbest(x, torch.tensor([5]))                 # batch mismatch
        with pytest.raises(ValueError):
            dec.decode_nbest(x, torch.tensor([6, 1]))              # length > seq_len
    with pytest.raises(RuntimeError, match="begin"):
        StreamingCTCBeamDecoder(0, 2).nbest()


def test_the_entry_point_is_declared_and_bound(lib):
    from myrtlespeech_amd import _lib
    assert "ms_ctc_beam_decode_ex" in _lib.header_symbols()
    res, args = _lib.SIGNATURES["ms_ctc_beam_decode_ex"]
    rows = _lib.SIGNATURES["ms_ctc_beam_decode_rows"][1]
    assert args[:len(rows)] == rows and len(args) == len(rows) + 6
    assert hasattr(lib, "ms_ctc_beam_decode_ex")
