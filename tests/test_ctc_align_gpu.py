"""CTC forced alignment on the device (``ms_ctc_align``, ``CTCForcedAligner``) against the numpy restatement of its
specification (tests/ctc_align_ref.py).

Log-probability mode is held to EXACT equality with the float32 restatement: the recursion is additions and strict
comparisons only.  On the grid inputs (multiples of 1/8) every partial sum is exact, so every tie is a real tie and the tie
rule decides it.  Logits mode is held to the derived bound B = 8 T 2^-24 max(1, |S*|) against the float64 restatement (two
paths compared, each accumulating T roundings of at most 2^-24 |S|, the per-frame log-softmax error of the same order, a
factor 4 for the hardware exp / log forms); T is the utterance's own frame count.  The numpy float32 restatement's worst ratios over the
cases below are 0.000 (optimum gap), 0.010 (score) and 0.003 (token log-probability); the device's are printed by the test
and recorded by tools/ctc_align_time.py -- not measured yet."""
import math

import numpy as np
import pytest
import torch

import ctc_align_ref as R
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

LOG_PROBS_IN = 2
paths_taken = set()       # {"lds", "global"}: where the launches of this module kept their back-pointers


def run_abi(x, in_lens, targets, blank, log_probs, form="padded", pad_width=None, pad_value=None):
    """One ``ms_ctc_align`` call on the current stream.  x [T, N, V] numpy, or a float32 tensor on the device; targets a
    list of label lists.  Returns the five outputs as numpy arrays, exactly as the device wrote them."""
    from myrtlespeech_amd.post_process import ctc_aligner as A
    lib = _lib.load()
    xd = torch.as_tensor(np.asarray(x), dtype=torch.float32).cuda().contiguous() if not torch.is_tensor(x) else x
    T, N, V = xd.shape
    lens = [len(t) for t in targets]
    l_max = max(lens) if lens else 0
    if form == "padded":
        width = max(l_max, 1) if pad_width is None else pad_width
        y = np.full((N, width), blank if pad_value is None else pad_value, dtype=np.int32)
        for n, t in enumerate(targets):
            y[n, :len(t)] = t
        offsets = np.arange(N, dtype=np.int32) * width
    else:
        y = np.asarray([v for t in targets for v in t] or [0], dtype=np.int32)
        offsets = (np.cumsum(lens) - np.asarray(lens)).astype(np.int32)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a).reshape(-1), dtype=torch.int32).cuda()   # noqa: E731
    y_dev, off_dev, yl_dev, xl_dev = dev(y), dev(offsets), dev(np.asarray(lens)), dev(np.asarray(in_lens))
    score = torch.full((N,), 123.0, dtype=torch.float32, device="cuda")
    frame_state = torch.full((N, T), -77, dtype=torch.int32, device="cuda")
    t_start = torch.full((N, max(l_max, 1)), -77, dtype=torch.int32, device="cuda")[:, :l_max].contiguous()
    t_end, t_logp = t_start.clone(), t_start.to(torch.float32)
    nbytes = lib.ms_ctc_align_workspace_bytes(T, N, V, 2 * l_max + 1)
    in_lds = A.backpointers_in_lds(T, l_max)
    assert (nbytes > -(-T * N * 4 // 256) * 256) == (not in_lds)      # the size query says where the back-pointers live
    paths_taken.add("lds" if in_lds else "global")
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")
    _lib.check(lib.ms_ctc_align(_lib.ptr(xd), _lib.ptr(xl_dev), _lib.ptr(y_dev), _lib.ptr(off_dev), _lib.ptr(yl_dev),
                                _lib.ptr(score), _lib.ptr(frame_state), _lib.ptr(t_start), _lib.ptr(t_end), _lib.ptr(t_logp),
                                T, N, V, l_max, blank, LOG_PROBS_IN if log_probs else 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "ms_ctc_align")
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (score, frame_state, t_start, t_end, t_logp))


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def assert_exact(x, in_lens, targets, blank, out):
    """Every output equal to the float32 restatement, element for element (log-probability mode)."""
    score, frame_state, t_start, t_end, t_logp = out
    x = np.asarray(x, dtype=np.float32)
    T = x.shape[0]
    l_max = t_start.shape[1]
    n_paths = 0
    for n, tgt in enumerate(targets):
        Tn, L = int(in_lens[n]), len(tgt)
        ref = R.align(x[:Tn, n], tgt, blank, log_probs=True, dtype=np.float32)
        assert same_bits(score[n], ref.score), (n, score[n], ref.score)
        want = np.full(T, -1, dtype=np.int64)
        if ref.states is not None:
            want[:Tn] = ref.states
            n_paths += 1
        assert frame_state[n].tolist() == want.tolist(), n
        assert t_start[n, :L].tolist() == ref.start.tolist() and t_end[n, :L].tolist() == ref.end.tolist(), n
        assert same_bits(t_logp[n, :L], ref.logp), n
        assert (t_start[n, L:] == -1).all() and (t_end[n, L:] == -1).all() and (t_logp[n, L:] == 0).all()
        assert l_max >= L
    return n_paths


def grid_table(rng, T, N, V, p_inf=0.01):
    """lp = -k / 8, k an integer in [0, 64), plus sprinkled -inf."""
    x = -(rng.integers(0, 64, size=(T, N, V)).astype(np.float32)) / 8
    x[rng.random((T, N, V)) < p_inf] = -np.inf
    return x


def random_target(rng, L, V, blank):
    labels = [v for v in range(V) if v != blank]
    return [int(labels[i]) for i in rng.integers(0, len(labels), size=L)]


def min_frames(tgt):
    return len(tgt) + sum(a == b for a, b in zip(tgt[1:], tgt[:-1]))


# (name, T, V, blank, [(T_n, L) per utterance], form, padded width) -- the smallest shapes that reach each path
GRID_CASES = [
    ("S63", 80, 5, 0, [(80, 31), (71, 31)], "padded", None),
    ("S65", 80, 5, 4, [(80, 32), (66, 32)], "concat", None),
    ("S67", 80, 5, 0, [(80, 33), (70, 33)], "padded", 40),
    ("S255", 300, 7, 0, [(300, 127), (290, 127)], "padded", None),
    ("S257", 300, 7, 6, [(300, 128), (280, 128)], "concat", None),
    ("S601_global", 700, 9, 0, [(700, 300), (650, 299)], "padded", 310),
    ("T1", 1, 4, 0, [(1, 0), (1, 1), (1, 2), (0, 0), (0, 1)], "padded", 3),
    ("L0", 9, 4, 3, [(9, 0), (5, 0), (0, 0)], "padded", None),
    ("ragged_V3", 60, 3, 0, [(60, 20), (0, 3), (17, 1), (44, 9), (60, 0), (31, 12), (2, 2)], "padded", 25),
    ("ragged_V3_blank_last", 60, 3, 2, [(60, 20), (0, 3), (17, 1), (44, 9), (60, 0), (31, 12), (2, 2)], "concat", None),
    ("V300", 90, 300, 299, [(90, 30), (75, 12), (90, 40)], "padded", 64),
    ("V300_blank0", 90, 300, 0, [(90, 30), (75, 12), (90, 40)], "concat", None),
]


@pytest.mark.parametrize("case", GRID_CASES, ids=[c[0] for c in GRID_CASES])
def test_log_prob_mode_grid_is_bit_exact(case):
    name, T, V, blank, shape, form, width = case
    rng = np.random.default_rng(sum(map(ord, name)))
    N = len(shape)
    x = grid_table(rng, T, N, V, p_inf=0.01 if V <= 9 else 0.05)
    in_lens = [tn for tn, _ in shape]
    targets = [random_target(rng, L, V, blank) for _, L in shape]
    # a padded form wider than any length holds out-of-range values in its padding: they must never be read as labels
    out = run_abi(x, in_lens, targets, blank, True, form=form, pad_width=width, pad_value=-5)
    n_paths = assert_exact(x, in_lens, targets, blank, out)
    if name.startswith("S"):
        assert n_paths >= 1          # the case is about the recursion, not about "no alignment"


def test_both_backpointer_placements_are_exercised():
    from myrtlespeech_amd.post_process import ctc_aligner as A
    assert A.backpointers_in_lds(300, 128) and not A.backpointers_in_lds(700, 300)
    rng = np.random.default_rng(5)
    for T, L in ((300, 128), (700, 300)):
        x = grid_table(rng, T, 1, 6, p_inf=0.0)
        tgt = [random_target(rng, L, 6, 0)]
        assert assert_exact(x, [T], tgt, 0, run_abi(x, [T], tgt, 0, True)) == 1
    assert paths_taken >= {"lds", "global"}


def test_minimal_feasible_length_and_one_less():
    rng = np.random.default_rng(11)
    tgt = [1, 1, 2, 2, 2, 3, 1, 1]
    m = min_frames(tgt)
    assert m == 12
    x = grid_table(rng, m + 2, 3, 4, p_inf=0.0)
    out = run_abi(x, [m, m - 1, m + 2], [tgt, tgt, tgt], 0, True)
    assert assert_exact(x, [m, m - 1, m + 2], [tgt, tgt, tgt], 0, out) == 2
    assert out[0][1] == -np.inf and (out[1][1] == -1).all() and (out[4][1] == -np.inf).all()
    # the known answers of the tie rule, on the device
    zeros = np.zeros((6, 4, 5), dtype=np.float32)
    s, fs, a, b, lp = run_abi(zeros, [6, 4, 3, 6], [[1, 1, 2], [0, 0, 1], [0, 0, 1], []], 4, True)
    assert fs[0].tolist() == [1, 2, 3, 5, 6, 6] and fs[1].tolist() == [1, 2, 3, 5, -1, -1]
    assert fs[2].tolist() == [-1] * 6 and s[2] == -np.inf and fs[3].tolist() == [0] * 6
    assert s[0] == 0 and a[0].tolist() == [0, 2, 3] and b[0].tolist() == [1, 3, 4]


def test_all_equal_table_every_decision_is_a_tie():
    for blank, form in ((0, "padded"), (5, "concat")):
        rng = np.random.default_rng(3 + blank)
        T, V = 150, 6
        shape = [(150, 40), (97, 33), (150, 74), (64, 0)]
        x = np.full((T, len(shape), V), -0.5, dtype=np.float32)
        targets = [random_target(rng, L, V, blank) for _, L in shape]
        in_lens = [tn for tn, _ in shape]
        out = run_abi(x, in_lens, targets, blank, True, form=form)
        assert assert_exact(x, in_lens, targets, blank, out) >= 3


@pytest.mark.parametrize("scale", [1.0, 4.0, 12.0])
def test_log_prob_mode_continuous_values_are_bit_exact(scale):
    rng = np.random.default_rng(int(scale))
    T, V, blank = 150, 30, 0
    shape = [(150, 20), (150, 70), (90, 33), (40, 40), (150, 5)]
    x = torch.log_softmax(torch.as_tensor(rng.standard_normal((T, len(shape), V)) * scale, dtype=torch.float32), -1).numpy()
    targets = [random_target(rng, L, V, blank) for _, L in shape]
    in_lens = [tn for tn, _ in shape]
    out = run_abi(x, in_lens, targets, blank, True, form="concat")
    assert assert_exact(x, in_lens, targets, blank, out) >= 4


worst = {"gap": 0.0, "score": 0.0, "logp": 0.0}


@pytest.mark.parametrize("scale", [1.0, 4.0, 12.0])
def test_logits_mode_within_the_derived_bound(scale):
    rng = np.random.default_rng(100 + int(scale))
    T, V, blank, N = 120, 30, 29, 16
    x = (rng.standard_normal((T, N, V)) * scale).astype(np.float32)
    in_lens = [int(v) for v in rng.integers(40, T + 1, size=N)]
    in_lens[0] = T
    targets = [random_target(rng, int(rng.integers(1, tn // 2)), V, blank) for tn in in_lens]
    score, frame_state, t_start, t_end, t_logp = run_abi(x, in_lens, targets, blank, False)
    for n, tgt in enumerate(targets):
        Tn, L = in_lens[n], len(tgt)
        ext = R.extended(tgt, blank)
        lp64, _ = R.log_softmax(x[:Tn, n].astype(np.float64), np.float64)
        best = R.align(lp64, tgt, blank, log_probs=True, dtype=np.float64)
        assert best.states is not None
        bound = 8 * Tn * 2.0 ** -24 * max(1.0, abs(float(best.score)))
        states = frame_state[n, :Tn]
        assert (frame_state[n, Tn:] == -1).all()
        assert R.is_valid_path(states, ext, blank) and R.collapse(states, ext, blank) == tgt          # (i)
        rescored = R.rescore(states, lp64, ext)
        gap, err = float(best.score) - rescored, abs(float(score[n]) - rescored)
        start, end, logp64 = R.spans(states, lp64, ext, np.float64)                                  # (iv) spans are exact
        assert t_start[n, :L].tolist() == start.tolist() and t_end[n, :L].tolist() == end.tolist()
        lerr = float(np.max(np.abs(t_logp[n, :L].astype(np.float64) - logp64)))
        worst["gap"], worst["score"], worst["logp"] = (max(worst["gap"], gap / bound), max(worst["score"], err / bound),
                                                       max(worst["logp"], lerr / bound))
        print(f"scale {scale} n {n}: T_n {Tn} L {L} S* {float(best.score):.4f} gap/B {gap / bound:.4f} "
              f"|score-R|/B {err / bound:.4f} logp/B {lerr / bound:.4f}")
        assert gap <= bound                                                                          # (ii)
        assert err <= bound                                                                          # (iii)
        assert lerr <= bound
    print("worst ratios so far", worst)


def test_against_the_loss_and_no_alignment_where_the_loss_is_infinite():
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    from myrtlespeech_amd.post_process import CTCForcedAligner
    rng = np.random.default_rng(21)
    T, V, blank, N = 100, 29, 28, 12
    x = torch.as_tensor(rng.standard_normal((T, N, V)) * 3, dtype=torch.float32)
    in_lens = [int(v) for v in rng.integers(20, T + 1, size=N)]
    targets = [random_target(rng, int(rng.integers(1, 15)), V, blank) for _ in range(N)]
    targets[3], in_lens[3] = [1, 1, 2, 2, 3], 6            # one frame short: no alignment
    targets[7], in_lens[7] = random_target(rng, 30, V, blank), 25
    targets[9], in_lens[9] = [4, 5], 0
    width = max(len(t) for t in targets)
    y = torch.zeros((N, width), dtype=torch.int64)
    for n, t in enumerate(targets):
        y[n, :len(t)] = torch.tensor(t)
    yl, xl = torch.tensor([len(t) for t in targets]), torch.tensor(in_lens)
    nll = CTCLoss(blank=blank, reduction="none")((x.cuda(), xl), (y, yl)).cpu().numpy()
    got = CTCForcedAligner(blank)(x.cuda(), xl, y.cuda(), yl)         # targets on the device: validated through one copy
    assert [g is None for g in got] == np.isinf(nll).tolist()
    assert got[3] is None and got[7] is None and got[9] is None and sum(g is not None for g in got) >= 6
    for n, g in enumerate(got):
        if g is None:
            continue
        bound = 8 * in_lens[n] * 2.0 ** -24 * max(1.0, abs(g.score))
        assert g.score <= -nll[n] + 2e-5 * abs(nll[n]) + bound, (n, g.score, nll[n])     # the best path cannot beat the sum
        assert len(g.frames) == in_lens[n] and [t.label for t in g.tokens] == targets[n]
        assert all(0 < t.confidence <= 1 and t.end > t.start for t in g.tokens)
        assert math.fsum(t.log_prob for t in g.tokens) >= g.score - bound                # the blanks' frames only lower it


def test_peaked_logits_reproduce_the_greedy_decoders():
    from myrtlespeech_amd.post_process import CTCForcedAligner
    from myrtlespeech_amd.post_process.ctc_greedy_decoder import CTCGreedyDecoder
    from myrtlespeech_amd.post_process.streaming import StreamingCTCGreedyDecoder
    rng = np.random.default_rng(33)
    T, V, blank, N = 300, 12, 0, 4
    x = rng.standard_normal((T, N, V)).astype(np.float32)
    x[..., blank] += 1.5                                      # blanks between the labels, as a trained model has
    top = x.argmax(-1)
    np.put_along_axis(x, top[..., None], np.take_along_axis(x, top[..., None], -1) + 1.0, -1)
    srt = np.sort(x, -1)
    assert (srt[..., -1] - srt[..., -2] >= 1.0).all()         # top-1 / top-2 gap: the optimum is unique
    lens = torch.tensor([300, 257, 300, 64])
    xd = torch.as_tensor(x).cuda()
    transcripts = CTCGreedyDecoder(blank)(xd, lens)
    assert all(len(t) > 0 for t in transcripts)
    stream = StreamingCTCGreedyDecoder(blank)
    stream.begin(N, T, total_lens=lens)
    stream.push(xd).result()
    stamps = stream.timestamps()
    assert stream.transcripts() == transcripts
    flat = torch.tensor([v for t in transcripts for v in t], dtype=torch.int32)            # concatenated, on the host
    got = CTCForcedAligner(blank)(xd, lens, flat, torch.tensor([len(t) for t in transcripts]))
    for n, g in enumerate(got):
        assert g is not None
        assert g.frames == top[:int(lens[n]), n].tolist()
        assert [t.start for t in g.tokens] == stamps[n]
        assert [t.label for t in g.tokens] == transcripts[n]


def test_non_finite_input():
    from myrtlespeech_amd.post_process import CTCForcedAligner
    rng = np.random.default_rng(44)
    T, V, N = 40, 8, 3
    x = torch.as_tensor(rng.standard_normal((T, N, V)), dtype=torch.float32).cuda()
    lens, y, yl = torch.tensor([40, 30, 40]), torch.tensor([[1, 2, 3], [4, 4, 5], [6, 1, 0]]), torch.tensor([3, 3, 2])
    al = CTCForcedAligner(0)
    clean = al(x, lens, y, yl)
    padded = x.clone()
    padded[35, 1, 2] = float("nan")                           # a padding row of utterance 1: changes nothing
    assert al(padded, lens, y, yl) == clean
    poisoned = x.clone()
    poisoned[29, 1, 7] = float("nan")                         # its last existing row, a symbol the target does not even use
    with pytest.raises(RuntimeError, match="utterance 1"):
        al(poisoned, lens, y, yl)
    # the raw outputs of the poisoned utterance, in both modes: NaN score, no path, NaN token log-probabilities
    for log_probs, bad in ((False, float("inf")), (True, float("nan")), (True, float("inf"))):
        src = torch.log_softmax(x, -1) if log_probs else x.clone()
        src[3, 1, 6] = bad
        s, fs, a, b, lp = run_abi(src, [40, 30, 40], [[1, 2, 3], [4, 4, 5], [6, 1]], 0, log_probs)
        assert np.isnan(s[1]) and (fs[1] == -1).all() and (a[1] == -1).all() and (b[1] == -1).all() and np.isnan(lp[1]).all()
        assert np.isfinite(s[[0, 2]]).all() and lp[2, 2] == 0
    src = torch.log_softmax(x, -1)
    src[3, 1, 6] = float("-inf")                              # "impossible", not poison
    assert np.isfinite(run_abi(src, [40, 30, 40], [[1, 2, 3], [4, 4, 5], [6, 1]], 0, True)[0]).all()


def test_out_of_range_labels_at_the_abi_are_no_alignment():
    """The Python layer refuses them; the kernel must not index a row with one."""
    rng = np.random.default_rng(55)
    x = grid_table(rng, 20, 4, 6, p_inf=0.0)
    targets = [[1, 2], [1, 6], [3, -1, 2], [2, 0, 1]]         # label == V, negative, the blank
    s, fs, a, b, lp = run_abi(x, [20] * 4, targets, 0, True)
    assert np.isfinite(s[0]) and (s[1:] == -np.inf).all() and (fs[1:] == -1).all()
    assert (a[1:] == -1).all() and (lp[1, :2] == -np.inf).all() and lp[1, 2] == 0


def test_non_default_stream_gives_the_same_bits():
    rng = np.random.default_rng(66)
    x = grid_table(rng, 90, 3, 7)
    in_lens, targets = [90, 45, 77], [random_target(rng, L, 7, 0) for L in (30, 9, 21)]
    ref = run_abi(x, in_lens, targets, 0, True)
    side = torch.cuda.Stream()
    xd = torch.as_tensor(x).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side and side != torch.cuda.default_stream()
        got = run_abi(xd, in_lens, targets, 0, True)
    for r, g in zip(ref, got):
        assert same_bits(r, g) if r.dtype == np.float32 else (r == g).all()


def test_two_aligners_back_to_back_do_not_share_workspace_state():
    from myrtlespeech_amd.post_process import CTCForcedAligner
    rng = np.random.default_rng(77)
    a1, a2 = CTCForcedAligner(0), CTCForcedAligner(0, log_probs=True)
    x1 = torch.as_tensor(rng.standard_normal((80, 3, 9)), dtype=torch.float32).cuda()
    x2 = torch.log_softmax(torch.as_tensor(rng.standard_normal((50, 2, 9)), dtype=torch.float32), -1).cuda()
    l1, y1, yl1 = torch.tensor([80, 61, 80]), torch.tensor([[1, 2, 2, 3], [4, 5, 0, 0], [6, 7, 8, 1]]), torch.tensor([4, 2, 4])
    l2, y2, yl2 = torch.tensor([50, 33]), torch.tensor([3, 3, 3, 1, 2]), torch.tensor([3, 2])
    first1, first2 = a1(x1, l1, y1, yl1), a2(x2, l2, y2, yl2)
    assert a1._workspace.buf is not a2._workspace.buf
    # interleaved, without a synchronisation between the launches: each aligner's results are what they were alone
    again1, again2, third1 = a1(x1, l1, y1, yl1), a2(x2, l2, y2, yl2), a1(x1, l1, y1, yl1)
    assert again1 == first1 and third1 == first1 and again2 == first2
    assert CTCForcedAligner(0)(x1, l1, y1, yl1) == first1
    ref = R.align(x2[:50, 0].cpu().numpy(), [3, 3, 3], 0, log_probs=True, dtype=np.float32)
    assert first2[0].score == float(ref.score) and [t.start for t in first2[0].tokens] == ref.start.tolist()
