"""CTC forced alignment, the parts that need no GPU: the two ABI entries, the numpy restatement of the specification pinned
against brute force and against known answers (the tie rule), the aligner's argument checks, ``words`` and the absence of
a CPU fallback."""
import itertools
import math

import numpy as np
import pytest
import torch

import ctc_align_ref as R
from myrtlespeech_amd import _lib


def test_abi_entries_in_header_binding_and_library(lib):
    declared = _lib.header_symbols()
    for name in ("ms_ctc_align_workspace_bytes", "ms_ctc_align"):
        assert name in declared
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES["ms_ctc_align"][1]) == 19


def test_workspace_query_is_host_arithmetic(lib):
    q = lib.ms_ctc_align_workspace_bytes
    assert q(501, 0, 29, 241) == 0 and q(501, -3, 29, 241) == 0
    assert q(501, 32, 29, 241) >= 501 * 32 * 4            # the per-frame normalisers
    prev = 0
    for t in (1, 2, 63, 64, 500, 501, 700, 1024, 4096, 8192):
        cur = q(t, 4, 29, 601)
        assert cur >= prev
        prev = cur
    prev = 0
    for s_max in (1, 3, 63, 65, 241, 255, 257, 601, 1025, 2001, 2047):
        cur = q(700, 4, 29, s_max)
        assert cur >= prev
        prev = cur


def test_backpointer_placement_matches_the_size_query(lib):
    """The workspace grows by the back-pointer rows exactly when they leave the LDS (the documented budget)."""
    from myrtlespeech_amd.post_process import ctc_aligner as A
    assert A.BACKPOINTER_LDS_BYTES == 96 * 1024
    with open(_lib.HEADER_PATH) as f:
        assert f"#define MS_CTC_ALIGN_BP_LDS_BYTES {A.BACKPOINTER_LDS_BYTES}" in f.read()
    for t, l_max, n in ((501, 120, 32), (700, 300, 2), (4096, 1000, 1), (6144, 1, 3), (6145, 1, 3), (64, 1023, 2)):
        base = -(-t * n * 4 // 256) * 256
        rows = -(-n * t * A.backpointer_row_bytes(l_max) // 256) * 256
        want = base if A.backpointers_in_lds(t, l_max) else base + rows
        assert lib.ms_ctc_align_workspace_bytes(t, n, 29, 2 * l_max + 1) == want
    assert A.backpointers_in_lds(501, 120) and not A.backpointers_in_lds(700, 300)


def _targets(L, V, blank):
    labels = [v for v in range(V) if v != blank]
    return [list(p) for p in itertools.product(labels, repeat=L)]


@pytest.mark.parametrize("blank", [0, 2])
def test_restatement_against_brute_force(blank):
    """Every T <= 6, V = 3, L <= 3 (repeated labels included): the restatement's score is the maximum over all state paths
    in float64, its path attains it, and "no alignment" agrees."""
    rng = np.random.default_rng(7 + blank)
    V = 3
    for T in range(0, 7):
        for L in range(0, 4):
            for target in _targets(L, V, blank):
                lp = np.log(rng.dirichlet(np.ones(V), size=T)) if T else np.zeros((0, V))
                if T and rng.random() < 0.3:
                    lp[rng.integers(T), rng.integers(V)] = -np.inf
                ext = R.extended(target, blank)
                got = R.align(lp, target, blank, log_probs=True, dtype=np.float64)
                scores = [R.rescore(p, lp, ext) for p in R.all_paths(T, ext, blank)]
                best = max(scores) if scores else -np.inf
                if T == 0 and L == 0:
                    assert got.score == 0 and len(got.states) == 0
                    continue
                if best == -np.inf:
                    assert got.states is None and got.score == -np.inf, (T, target)
                    continue
                assert R.is_valid_path(got.states, ext, blank)
                assert R.collapse(got.states, ext, blank) == target
                assert abs(got.score - best) <= 1e-12 * max(1.0, abs(best)), (T, target)
                assert abs(R.rescore(got.states, lp, ext) - best) <= 1e-12 * max(1.0, abs(best))
                assert T >= L + sum(a == b for a, b in zip(target[1:], target[:-1]))    # a path: the length is feasible


def test_tie_rule_known_answers():
    zeros = lambda t: np.zeros((t, 5), dtype=np.float32)   # noqa: E731
    r = R.align(zeros(6), [1, 1, 2], 4)
    assert r.states.tolist() == [1, 2, 3, 5, 6, 6] and r.score == 0
    assert r.start.tolist() == [0, 2, 3] and r.end.tolist() == [1, 3, 4]
    assert R.align(zeros(4), [0, 0, 1], 4).states.tolist() == [1, 2, 3, 5]      # the minimal feasible length
    r = R.align(zeros(3), [0, 0, 1], 4)
    assert r.states is None and r.score == -np.inf and r.logp.tolist() == [-np.inf] * 3
    assert R.align(zeros(5), [], 4).states.tolist() == [0] * 5
    # non-finite input: NaN score, no path
    bad = zeros(4)
    bad[2, 0] = np.nan
    r = R.align(bad, [1], 4)
    assert math.isnan(r.score) and r.states is None and np.isnan(r.logp).all()
    bad[2, 0] = np.inf
    assert math.isnan(R.align(bad, [1], 4).score)
    assert math.isnan(R.align(np.full((2, 3), -np.inf, dtype=np.float32), [1], 0, log_probs=False).score)


def test_argument_validation_needs_no_device():
    from myrtlespeech_amd.post_process import CTCForcedAligner
    with pytest.raises(ValueError):
        CTCForcedAligner(-1)
    al = CTCForcedAligner(0)
    x = torch.zeros(5, 2, 4)
    lens = torch.tensor([5, 3])
    y, yl = torch.tensor([[1, 2], [3, 0]]), torch.tensor([2, 1])
    with pytest.raises(ValueError):
        al(x, torch.tensor([5.0, 3.0]), y, yl)                        # float lengths
    with pytest.raises(ValueError):
        al(x, torch.tensor([5]), y, yl)                               # batch mismatch
    with pytest.raises(ValueError):
        al(x, torch.tensor([6, 1]), y, yl)                            # length > seq_len
    with pytest.raises(ValueError):
        al(x, lens, y.float(), yl)                                    # float targets
    with pytest.raises(ValueError):
        al(x, lens, y, torch.tensor([2]))                             # target_lengths batch mismatch
    with pytest.raises(ValueError):
        al(x, lens, y, torch.tensor([3, 1]))                          # longer than the padded width
    with pytest.raises(ValueError):
        al(x, lens, torch.tensor([1, 2]), torch.tensor([2, 1]))       # concatenated: too few labels
    with pytest.raises(ValueError, match="utterance 1"):
        al(x, lens, torch.tensor([[1, 2], [4, 0]]), yl)               # label >= V
    with pytest.raises(ValueError, match="utterance 0"):
        al(x, lens, torch.tensor([[1, 0], [3, 0]]), yl)               # the blank inside a target
    with pytest.raises(ValueError):
        al(x, lens, torch.tensor([[1, -1], [3, 0]]), yl)              # negative label
    with pytest.raises(ValueError):
        CTCForcedAligner(4)(x, lens, y, yl)                           # blank outside the alphabet
    with pytest.raises(ValueError):
        al(x, lens, torch.zeros(1, 2, 2, dtype=torch.int64), yl)      # 3-D targets


def _alignment(labels_and_spans, score=-1.0):
    from myrtlespeech_amd.post_process import Alignment, TokenSpan
    toks = [TokenSpan(*t) for t in labels_and_spans]
    return Alignment(score, [], toks)


def test_words():
    from myrtlespeech_amd.post_process import TokenSpan, words
    SEP = 9
    assert TokenSpan(3, 4, 6, -1.0).confidence == pytest.approx(math.exp(-0.5))
    assert words(_alignment([]), SEP) == []
    # no separator: one word
    w = words(_alignment([(1, 0, 2, -0.5), (2, 3, 4, -0.25)]), SEP)
    assert len(w) == 1 and w[0].labels == [1, 2] and (w[0].start, w[0].end) == (0, 4)
    assert w[0].log_prob == -0.75 and w[0].confidence == pytest.approx(math.exp(-0.75 / 3))
    assert w[0].start_s is None and w[0].end_s is None
    # leading, doubled and trailing separators belong to no word
    toks = [(SEP, 0, 1, -0.1), (1, 1, 3, -0.5), (SEP, 4, 5, -0.1), (SEP, 5, 6, -0.1), (2, 7, 8, -1.0), (3, 8, 10, -2.0),
            (SEP, 11, 12, -0.1)]
    w = words(_alignment(toks), SEP, frame_seconds=0.02)
    assert [x.labels for x in w] == [[1], [2, 3]]
    assert [(x.start, x.end) for x in w] == [(1, 3), (7, 10)]
    assert w[1].log_prob == -3.0 and w[1].confidence == pytest.approx(math.exp(-1.0))
    assert w[1].start_s == pytest.approx(0.14) and w[1].end_s == pytest.approx(0.20)
    # only separators: no words
    assert words(_alignment([(SEP, 0, 1, -0.1), (SEP, 1, 2, -0.1)]), SEP) == []


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("needs a CPU-only box")
    from myrtlespeech_amd.post_process import CTCForcedAligner
    with pytest.raises(RuntimeError, match="HIP device"):
        CTCForcedAligner(0)(torch.zeros(3, 1, 4), torch.tensor([3]), torch.tensor([[1, 2]]), torch.tensor([2]))
