"""The transducer forced-alignment specification on the host: the numpy restatement (tests/rnnt_align_ref.py) against brute
force over all monotone paths, its own invariants and edge cases, and the C ABI's declarations.  No GPU.

Why the float32 restatement can be held to brute force BIT FOR BIT: float32 addition is monotone (a >= b gives fl(a + c) >=
fl(b + c)), so the maximum over paths of the in-order float32 sum is the maximum over the last step of fl(best prefix + term):
exactly the recursion.
"""
import ctypes
import re

import numpy as np
import pytest

import rnnt_align_ref as A
import rnnt_loss_ref as R
from myrtlespeech_amd import _lib

NEW_SYMBOLS = ("ms_rnnt_align_workspace_bytes", "ms_rnnt_align", "ms_rnnt_align_joint_workspace_bytes", "ms_rnnt_align_joint")


def tiny_tables(rng, Tn, Un, grid, p_inf=0.0):
    x = A.grid_table(rng, 1, Tn, Un + 1, 4, p_inf) if grid else A.continuous_table(rng, 1, Tn, Un + 1, 4, p_inf)
    y = R.random_targets(rng, 1, Un, 4, 3)[0].tolist()
    b, e = A.cell_tables(x[0], Tn, y, 3, True, np.float32)
    return x, y, b, e


@pytest.mark.parametrize("grid", [True, False])
def test_restatement_equals_brute_force_on_tiny_lattices(grid):
    rng = np.random.default_rng(7 if grid else 8)
    checked = unique = 0
    for Tn in range(1, 5):
        for Un in range(0, 5):
            for rep in range(3):
                x, y, b, e = tiny_tables(rng, Tn, Un, grid, p_inf=0.15 if rep == 2 else 0.0)
                sc, tf, fu = A.align_planes(b, e, np.float32)
                best, arg = A.brute_force(b, e, np.float32)
                assert np.float32(sc).tobytes() == np.float32(best).tobytes(), (Tn, Un, sc, best)
                if sc == -np.inf:
                    assert tf is None and fu is None
                    continue
                assert (tf, fu) in arg                       # the traced path reaches the maximum ...
                assert A.path_score(b, e, tf, fu).tobytes() == np.float32(sc).tobytes()
                if len(arg) == 1:
                    unique += 1                              # ... and is THE path when the maximum is unique
                checked += 1
    assert checked > 40 and unique > 10


def test_score_is_the_in_order_sum_of_its_outputs_and_below_the_loss():
    rng = np.random.default_rng(11)
    N, T, U1, V1, blank = 4, 9, 7, 5, 4
    x = (rng.standard_normal((N, T, U1, V1)) * 3).astype(np.float32)
    in_lens, tgt_lens = A.ragged_lengths(rng, N, T, U1)
    y = R.pad_targets(R.random_targets(rng, N, U1 - 1, V1, blank), tgt_lens, blank)
    for dtype in (np.float32, np.float64):
        res = A.rnnt_align(x, in_lens, y, tgt_lens, blank, log_probs=False, dtype=dtype)
        loss = R.rnnt_loss(x, in_lens, y, tgt_lens, blank, dtype=np.float64)
        assert np.isfinite(res.score).all()
        # the best path is one term of the sum over all paths
        assert (res.score.astype(np.float64) <= -loss.nll + 1e-4).all()
        if dtype is np.float32:
            A.check_consistent(res, in_lens, tgt_lens)
    # float32 and float64 agree on these well-separated tables
    r32 = A.rnnt_align(x, in_lens, y, tgt_lens, blank, log_probs=False, dtype=np.float32)
    r64 = A.rnnt_align(x, in_lens, y, tgt_lens, blank, log_probs=False, dtype=np.float64)
    np.testing.assert_allclose(r32.score, r64.score, rtol=0, atol=1e-4)
    # a path with one label has T_n alignments: the score is the largest, the loss their log-sum
    x1 = np.log(np.full((1, 3, 2, 2), 0.5, dtype=np.float32))
    res = A.rnnt_align(x1, [3], np.array([[0]]), [1], 1, log_probs=True)
    assert res.score[0] == np.float32(4 * np.log(np.float32(0.5)))


def test_a_tie_takes_the_blank_predecessor():
    """All-equal table: every decision is a tie, so every cell with a blank predecessor takes it: walking back from (T-1, U)
    the path goes up to frame 0 first -- every label is emitted in frame 0."""
    Tn, Un = 5, 4
    x = np.full((1, Tn, Un + 1, 3), -1.0, dtype=np.float32)
    res = A.rnnt_align(x, [Tn], np.array([[0, 1, 0, 1]]), [Un], 2, log_probs=True)
    assert res.token_frame[0].tolist() == [0] * Un
    assert res.frame_u[0].tolist() == [Un] * Tn
    assert res.score[0] == np.float32(-(Tn + Un))
    A.check_consistent(res, [Tn], [Un])


def test_edge_cases():
    rng = np.random.default_rng(13)
    N, T, U1, V1, blank = 5, 4, 4, 4, 3
    x = A.grid_table(rng, N, T, U1, V1, p_inf=0.0)
    y = R.random_targets(rng, N, U1 - 1, V1, blank)
    in_lens, tgt_lens = np.array([4, 4, 3, 4, 2]), np.array([3, 2, 3, 1, 0])
    clean = A.rnnt_align(x, in_lens, y, tgt_lens, blank)
    assert np.isfinite(clean.score).all()
    A.check_consistent(clean, in_lens, tgt_lens)
    # impossible transcript: the only way out of (T_n-1, U_n) is its blank
    xi = x.copy()
    xi[0, 3, 3, blank] = -np.inf
    # a NaN / +inf in an existing b or e poisons its own utterance only, on or off the best path
    xi[1, 0, 2, blank] = np.nan
    xi[2, 2, 1, y[2, 1]] = np.inf
    # ... but not in a symbol the recursion does not read, nor in a cell that does not exist
    other = next(v for v in range(V1) if v not in (blank, y[3, 0]))
    xi[3, 1, 0, other] = np.nan
    xi[3, :, 2:, :] = np.nan
    xi[4, 2:, :, :] = np.inf
    res = A.rnnt_align(xi, in_lens, y, tgt_lens, blank)
    A.check_consistent(res, in_lens, tgt_lens)
    assert res.score[0] == -np.inf and (res.token_logp[0] == -np.inf).all() and (res.frame_u[0] == -1).all()
    assert np.isnan(res.score[1]) and np.isnan(res.token_logp[1, :2]).all() and res.token_logp[1, 2] == 0
    assert np.isnan(res.score[2]) and np.isnan(res.frame_logp[2, :3]).all() and res.frame_logp[2, 3] == 0
    for n in (3, 4):
        for got, want in zip(res, clean):
            assert got[n].tobytes() == want[n].tobytes()
    # the caller's errors: lengths out of range, a label out of range or equal to the blank
    yb = y.copy()
    yb[1, 0], yb[3, 0] = blank, V1
    res = A.rnnt_align(x, [0, 4, 5, 4, 2], yb, [3, 2, 3, 1, -1], blank)
    A.check_consistent(res, [0, 4, 5, 4, 2], [3, 2, 3, 1, -1])
    assert (res.score == -np.inf).all() and (res.token_frame == -1).all() and (res.frame_u == -1).all()
    # padding of the targets changes nothing
    yp = y.copy()
    for n in range(N):
        yp[n, tgt_lens[n]:] = -99
    res = A.rnnt_align(x, in_lens, yp, tgt_lens, blank)
    for got, want in zip(res, clean):
        assert got.tobytes() == want.tobytes()
    # logits mode: a row of -inf only has no finite normaliser
    xl = (rng.standard_normal((1, 2, 2, 3))).astype(np.float32)
    xl[0, 1, 0, :] = -np.inf
    assert np.isnan(A.rnnt_align(xl, [2], np.array([[0]]), [1], 2, log_probs=False).score[0])


C_TYPES = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}


def test_header_prototypes_match_the_binding(lib):
    with open(_lib.HEADER_PATH) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        m = re.search(r"\b(size_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert res is C_TYPES[m.group(1)]
        want = []
        for arg in m.group(2).split(","):
            arg = " ".join(arg.split())
            want.append(ctypes.c_void_p if "*" in arg else C_TYPES[arg.rsplit(" ", 1)[0]])
        assert args == want, (name, args, want)
    assert "#define MS_RNNT_LOG_PROBS_IN 2" in raw
    assert int(re.search(r"#define MS_ABI_VERSION (\d+)", raw).group(1)) == 4


def test_workspace_queries_are_host_arithmetic(lib):
    from myrtlespeech_amd.post_process import rnnt_aligner as P
    with open(_lib.HEADER_PATH) as f:
        assert f"#define MS_RNNT_ALIGN_BP_LDS_BYTES {P.BACKPOINTER_LDS_BYTES}" in f.read()
    assert P.MS_RNNT_LOG_PROBS_IN == 2
    assert P.backpointers_in_lds(300, 200) and not P.backpointers_in_lds(3100, 200)

    def up(v):
        return -(-v // 256) * 256

    for n, t, u1 in ((1, 300, 200), (1, 3100, 200), (16, 250, 121), (3, 12288, 1), (3, 12289, 1), (2, 70, 1024), (2, 700, 1024)):
        plane = up(n * (t + u1 - 1) * u1 * 4)
        rows = 0 if P.backpointers_in_lds(t, u1) else up(n * P.backpointer_bytes(t, u1))
        assert lib.ms_rnnt_align_workspace_bytes(n, t, u1, 29) == 2 * plane + up(n * t * u1 * 4) + rows
        assert lib.ms_rnnt_align_workspace_bytes(n, t, u1, 5000) == lib.ms_rnnt_align_workspace_bytes(n, t, u1, 29)
        assert lib.ms_rnnt_align_joint_workspace_bytes(n, t, u1, 64, 29) == up(lib.ms_rnnt_score_workspace_bytes(n, t, u1, 64, 29)) + rows
    assert lib.ms_rnnt_align_workspace_bytes(0, 5, 5, 5) == 0 and lib.ms_rnnt_align_joint_workspace_bytes(2, 5, 5, 0, 5) == 0


def test_python_layer_validates_on_the_host():
    import torch
    from myrtlespeech_amd.post_process import RNNTAlignment, RNNTForcedAligner, TokenSpan, words
    al = RNNTForcedAligner(3, log_probs=True)
    x = torch.zeros(2, 4, 3, 4)
    with pytest.raises(ValueError):
        RNNTForcedAligner(-1)
    with pytest.raises(ValueError):
        al((x[0], torch.tensor([4])), (torch.zeros(2, 2, dtype=torch.int64), torch.tensor([2, 2])))
    with pytest.raises(ValueError):
        al((x, torch.tensor([4, 5])), (torch.zeros(2, 2, dtype=torch.int64), torch.tensor([2, 2])))
    with pytest.raises(ValueError):
        al((x, torch.tensor([4, 4])), (torch.zeros(2, 2, dtype=torch.int64), torch.tensor([2, 3])))
    with pytest.raises(ValueError, match="utterance 1: target label 3"):
        al((x, torch.tensor([4, 4])), (torch.tensor([[0, 1], [3, 9]]), torch.tensor([2, 1])))
    # tokens are spans of one frame: ``words`` groups them unchanged
    a = RNNTAlignment(-3.0, [TokenSpan(0, 1, 2, -0.5), TokenSpan(1, 1, 2, -0.25), TokenSpan(2, 2, 3, -0.1), TokenSpan(0, 5, 6, -1.0)],
                      [[], [0, 1], [2], [], [], [0]], [-0.1] * 6)
    w = words(a, separator_index=2, frame_seconds=0.04)
    assert [(s.labels, s.start, s.end) for s in w] == [([0, 1], 1, 2), ([0], 5, 6)]
    assert w[0].start_s == pytest.approx(0.04) and w[1].end_s == pytest.approx(0.24)
