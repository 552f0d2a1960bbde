"""Transducer forced alignment on the device (``ms_rnnt_align``, ``ms_rnnt_align_joint``, ``RNNTForcedAligner``,
``RNNT.align``) against the numpy restatement of its specification (tests/rnnt_align_ref.py).

Log-probability mode computes nothing but the recursion's additions: every output is held to the float32 restatement BIT
FOR BIT.

The other two modes form b and e on the device with an error; they are held to the float64 restatement within a bound that is
derived, not fitted.  Let delta_n bound the error of one cell's b / e.  A path has T_n + U_n terms; summed in float32 in path
order, every partial sum is bounded by the final one (every lp is <= 0), so each addition rounds by at most
2^-24 max(1, |score|).  Any fixed path's device sum is therefore within

  A_n = (T_n + U_n) (delta_n + 2^-24 max(1, |score_ref|))

of its exact sum under the exact b / e.  The device's score is the maximum over paths of the device sums (float32 addition is
monotone, tests/test_rnnt_align_cpu.py), the reference's the maximum of the exact sums, and two maxima of functions that differ
by at most A_n pointwise differ by at most A_n:  |score - score_ref| <= A_n.  The device's PATH, rescored under the float64
b / e, is within A_n of the device's score, hence >= score_ref - 2 A_n: near-optimal, whichever of two near-tied paths it took.

  fused entry   delta_n = rnnt_score_ref.delta(max_v eps_v, max |Z| over the utterance's cells): the per-cell bound derived in
                tests/test_rnnt_score_gpu.py (the picked logit and Z each off by eps; 16 * 2^-24 max(1, |Z|) for Z itself).
  logits mode   delta_n = 8 * 2^-24 max(1, |score_ref|): the per-step term of rnnt_loss_ref.bound (B_n = 8 (T_n + U_n) 2^-24
                max(1, |nll_n|)), with the path's own magnitude in place of nll.  It covers a cell of the path: b = (x - m) - lse
                with x - m <= 0 <= lse, so both magnitudes are at most |b| <= |score|; the subtraction x - m, the precise logf
                and the final subtraction round by 2^-24 |b| each, and the sum of V1 hardware exps (relative errors weighted by
                the softmax itself) moves lse by a few 2^-24 absolute -- inside the factor 8.

The worst ratio of error to bound is printed by every such test.
"""
import numpy as np
import pytest
import torch

import rnnt_align_ref as A
import rnnt_loss_ref as R
import rnnt_score_ref as S
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
LOG_PROBS_IN = 2
U24 = 2.0 ** -24
CASES = S.cases()
placements = set()
worst = {"fused": 0.0, "logits": 0.0}


def f32(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda().contiguous()


def i32(a):
    return torch.as_tensor(np.ascontiguousarray(a).reshape(-1), dtype=torch.int32).cuda()


def outputs(N, T, U1):
    """The five outputs pre-filled with a sentinel: the device must write all of them."""
    return (torch.full((N,), SENTINEL, dtype=torch.float32, device="cuda"),
            torch.full((N, U1 - 1), -777, dtype=torch.int32, device="cuda"),
            torch.full((N, U1 - 1), SENTINEL, dtype=torch.float32, device="cuda"),
            torch.full((N, T), -777, dtype=torch.int32, device="cuda"),
            torch.full((N, T), SENTINEL, dtype=torch.float32, device="cuda"))


def fetch(out):
    torch.cuda.synchronize()
    res = A.Result(*(o.cpu().numpy() for o in out))
    assert not (res.score == SENTINEL).any() and not (res.token_logp == SENTINEL).any() and not (res.frame_logp == SENTINEL).any()
    assert not (res.token_frame == -777).any() and not (res.frame_u == -777).any()
    return res


def note_placement(lib, T, U1, nbytes, base):
    """The size query says where the back-pointers live; the Python helper must agree."""
    from myrtlespeech_amd.post_process import rnnt_aligner as P
    in_lds = P.backpointers_in_lds(T, U1)
    assert (nbytes > base) == (not in_lds)
    placements.add("lds" if in_lds else "global")
    return in_lds


def run_align(x, in_lens, targets, tgt_lens, blank, log_probs):
    """One ``ms_rnnt_align`` call on the current stream; the workspace filled with NaN bytes.  x numpy or a device tensor."""
    lib = _lib.load()
    xd = x if torch.is_tensor(x) else f32(x)
    N, T, U1, V1 = xd.shape
    xl, yl = i32(in_lens), i32(tgt_lens)
    y = i32(targets) if U1 > 1 else None
    out = outputs(N, T, U1)
    nbytes = lib.ms_rnnt_align_workspace_bytes(N, T, U1, V1)
    up = lambda v: -(-v // 256) * 256                                       # noqa: E731
    note_placement(lib, T, U1, nbytes, 2 * up(N * (T + U1 - 1) * U1 * 4) + up(N * T * U1 * 4))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    tok = U1 > 1
    _lib.check(lib.ms_rnnt_align(_lib.ptr(xd), _lib.ptr(xl), _lib.ptr(y), _lib.ptr(yl), _lib.ptr(out[0]),
                                 _lib.ptr(out[1] if tok else None), _lib.ptr(out[2] if tok else None), _lib.ptr(out[3]),
                                 _lib.ptr(out[4]), N, T, U1, V1, blank, LOG_PROBS_IN if log_probs else 0, _lib.ptr(ws), nbytes,
                                 _lib.stream_ptr()), "ms_rnnt_align")
    return fetch(out)


def run_joint(c, **change):
    """One ``ms_rnnt_align_joint`` call on a case of rnnt_score_ref."""
    c = dict(c, **change)
    lib = _lib.load()
    T, N, J = c["enc_p"].shape
    U1, V1 = c["pred_p"].shape[0], c["w_out"].shape[0]
    e, p, w = f32(c["enc_p"]), f32(c["pred_p"]), f32(c["w_out"])
    b = None if c["b_out"] is None else f32(c["b_out"])
    xl, yl = i32(c["in_lens"]), i32(c["tgt_lens"])
    y = i32(c["targets"]) if U1 > 1 else None
    out = outputs(N, T, U1)
    nbytes = lib.ms_rnnt_align_joint_workspace_bytes(N, T, U1, J, V1)
    note_placement(lib, T, U1, nbytes, -(-lib.ms_rnnt_score_workspace_bytes(N, T, U1, J, V1) // 256) * 256)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    tok = U1 > 1
    _lib.check(lib.ms_rnnt_align_joint(_lib.ptr(e), _lib.ptr(p), _lib.ptr(w), _lib.ptr(b), _lib.ptr(xl), _lib.ptr(y), _lib.ptr(yl),
                                       _lib.ptr(out[0]), _lib.ptr(out[1] if tok else None), _lib.ptr(out[2] if tok else None),
                                       _lib.ptr(out[3]), _lib.ptr(out[4]), N, T, U1, J, V1, c["blank"], _lib.ptr(ws), nbytes,
                                       _lib.stream_ptr()), "ms_rnnt_align_joint")
    return fetch(out)


def materialise(c):
    """The dense [N, T, U1, V1] log-probabilities of a case ON THE DEVICE: ms_rnnt_joint_forward over all N T U1 cells."""
    lib = _lib.load()
    T, N, J = c["enc_p"].shape
    U1, V1 = c["pred_p"].shape[0], c["w_out"].shape[0]
    n, t, u = np.meshgrid(np.arange(N), np.arange(T), np.arange(U1), indexing="ij")
    enc_rows = i32(t * N + n)
    pred_rows = f32(c["pred_p"].reshape(U1 * N, J)[(u * N + n).reshape(-1)])
    e, w, b = f32(c["enc_p"]), f32(c["w_out"]), f32(c["b_out"])
    logp = torch.empty((N, T, U1, V1), dtype=torch.float32, device="cuda")
    _lib.check(lib.ms_rnnt_joint_forward(_lib.ptr(e), _lib.ptr(enc_rows), _lib.ptr(pred_rows), _lib.ptr(w), _lib.ptr(b),
                                         _lib.ptr(logp), N * T * U1, J, V1, _lib.stream_ptr()), "ms_rnnt_joint_forward")
    return logp


def same_result(a, b, rows=None):
    for x, y in zip(a, b):
        if rows is not None:
            x, y = x[rows], y[rows]
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def assert_bit_exact(x, in_lens, y, tgt_lens, blank):
    got = run_align(x, in_lens, y, tgt_lens, blank, log_probs=True)
    want = A.rnnt_align(x, in_lens, y, tgt_lens, blank, log_probs=True, dtype=np.float32)
    for name, g, w in zip(A.Result._fields, got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, g, w)
    A.check_consistent(got, in_lens, tgt_lens)
    return got


SHAPES = [(3, 1, 1), (3, 5, 1), (2, 1, 6), (4, 9, 7), (3, 20, 64), (3, 20, 65), (2, 12, 129), (2, 70, 200)]


@pytest.mark.parametrize("grid", [True, False], ids=["grid", "continuous"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_log_prob_mode_is_bit_exact(shape, grid):
    """U1 = 1 (no labels at all), T = 1, one wave exactly, the first lane of a second wave, three and four waves; ragged
    lengths with U_n = 0 and T_n = 1 inside the batch; a 1 % sprinkle of -inf."""
    N, T, U1 = shape
    rng = np.random.default_rng(1000 * T + U1 + (500 if grid else 0))
    x = (A.grid_table if grid else A.continuous_table)(rng, N, T, U1, 4, p_inf=0.01)
    in_lens, tgt_lens = A.ragged_lengths(rng, N, T, U1)
    y = R.pad_targets(R.random_targets(rng, N, U1 - 1, 4, 3), tgt_lens, 3)
    got = assert_bit_exact(x, in_lens, y, tgt_lens, 3)
    print(f"{shape} scores {got.score.tolist()}")
    # the same tables without the -inf: every utterance has a path
    x = np.where(np.isinf(x), np.float32(-9.0), x)
    got = assert_bit_exact(x, in_lens, y, tgt_lens, 3)
    assert np.isfinite(got.score).all()


def test_all_equal_table_every_decision_is_a_tie():
    N, T, U1 = 2, 30, 70
    x = np.full((N, T, U1, 4), -0.5, dtype=np.float32)
    rng = np.random.default_rng(3)
    y = R.random_targets(rng, N, U1 - 1, 4, 0)
    got = assert_bit_exact(x, [30, 17], y, [69, 40], 0)
    # a tie takes the blank predecessor: walking back, the path climbs to frame 0 first -- every label is emitted there
    assert (got.token_frame[0] == 0).all() and (got.token_frame[1, :40] == 0).all()
    assert (got.frame_u[0] == 69).all() and (got.frame_u[1, :17] == 40).all()


def test_both_backpointer_placements_are_exercised():
    from myrtlespeech_amd.post_process import rnnt_aligner as P
    assert P.backpointers_in_lds(300, 200) and not P.backpointers_in_lds(3100, 200)
    rng = np.random.default_rng(5)
    placements.clear()
    for T in (300, 3100):
        x = A.grid_table(rng, 1, T, 200, 4, p_inf=0.0)
        y = R.random_targets(rng, 1, 199, 4, 3)
        got = assert_bit_exact(x, [T], y, [199], 3)
        assert np.isfinite(got.score[0])
    assert placements == {"lds", "global"}


# ---- the modes whose b / e carry an error: the float64 restatement and the derived bounds

_ref64 = {}


def ref64(name, dense=False):
    """(float64 Result, the utterances' float64 (b, e) tables, delta_n per utterance) of a case: computed once, never edited.
    ``dense``: the reference of the logits mode, on the case's logits rounded to float32 (what the device is handed)."""
    key = (name, dense)
    if key not in _ref64:
        c = CASES[name]
        x = S.joint_logits(c["enc_p"], c["pred_p"], c["w_out"], c["b_out"])
        if dense:
            x = x.astype(np.float32)
        tables = []
        res = A.rnnt_align(x.astype(np.float64), c["in_lens"], c["targets"], c["tgt_lens"], c["blank"], log_probs=False,
                           dtype=np.float64, tables=tables)
        if dense:
            deltas = [8.0 * U24 * max(1.0, abs(float(s))) for s in res.score]
        else:
            loss, eps, _ = S.reference(name)
            deltas = [S.delta(float(np.max(eps)), float(np.max(np.abs(loss.Z[n][loss.exists[n]])))) for n in range(len(res.score))]
        _ref64[key] = (res, tables, deltas, x if dense else None)
    return _ref64[key]


def bounds_of(res, deltas, in_lens, tgt_lens):
    return np.array([(int(in_lens[n]) + int(tgt_lens[n])) * (deltas[n] + U24 * max(1.0, abs(float(res.score[n]))))
                     for n in range(len(deltas))])


def check_within(got, name, dense, mode):
    c = CASES[name]
    res, tables, deltas, _ = ref64(name, dense)
    bounds = bounds_of(res, deltas, c["in_lens"], c["tgt_lens"])
    A.check_consistent(got, c["in_lens"], c["tgt_lens"])
    assert np.isfinite(res.score).all() and np.isfinite(got.score).all()
    err = np.abs(got.score.astype(np.float64) - res.score)
    rescored = np.array([float(A.path_score(tables[n][0], tables[n][1], got.token_frame[n, :c["tgt_lens"][n]].tolist(),
                                            got.frame_u[n, :c["in_lens"][n]].tolist(), np.float64)) for n in range(len(err))])
    gap = res.score - rescored
    ratio = float(np.max(err / bounds))
    worst[mode] = max(worst[mode], ratio)
    print(f"{name} ({mode}): score {got.score.tolist()} ref {res.score.tolist()} |error| / A_n {(err / bounds).tolist()} "
          f"(ref - rescored path) / 2 A_n {(gap / (2 * bounds)).tolist()}  A_n {[float(f'{b:.3g}') for b in bounds]}")
    print("worst ratios of error to bound so far", {k: round(v, 4) for k, v in worst.items()})
    assert (err <= bounds).all(), (name, err, bounds)
    assert (gap >= -1e-9 * np.abs(res.score)).all()               # no path beats the float64 optimum
    assert (rescored >= res.score - 2 * bounds).all(), (name, gap, bounds)
    return bounds


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_entry_within_the_derived_bound(name):
    check_within(run_joint(CASES[name]), name, False, "fused")


@pytest.mark.parametrize("name", sorted(CASES))
def test_logits_mode_within_the_derived_bound(name):
    c = CASES[name]
    x = ref64(name, True)[3]
    check_within(run_align(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"], log_probs=False), name, True, "logits")


def test_peaked_case_every_route_finds_the_same_path():
    """The model of case d knows the transcript: the best path leads by far more than any bound, so the fused entry, the logits
    mode on the lattice materialised on the device, and the restatement must agree on it."""
    name = "d_peaked"
    c = CASES[name]
    res, _, deltas, _ = ref64(name, False)
    fused = run_joint(c)
    dense = run_align(materialise(c), c["in_lens"], c["targets"], c["tgt_lens"], c["blank"], log_probs=False)
    A.check_consistent(dense, c["in_lens"], c["tgt_lens"])
    assert fused.token_frame.tobytes() == dense.token_frame.tobytes() == res.token_frame.tobytes()
    assert fused.frame_u.tobytes() == dense.frame_u.tobytes() == res.frame_u.tobytes()
    # the materialised lattice holds log-probabilities inside the same per-cell bound (tests/test_rnnt_score_gpu.py) and the
    # logits mode adds its own per-cell term on top: the two scores differ by at most the sum of the two bounds
    a_fused = bounds_of(res, deltas, c["in_lens"], c["tgt_lens"])
    a_dense = bounds_of(res, [d + 8.0 * U24 * max(1.0, abs(float(sc))) for d, sc in zip(deltas, res.score)], c["in_lens"],
                        c["tgt_lens"])
    diff = np.abs(fused.score.astype(np.float64) - dense.score)
    print(f"fused {fused.score.tolist()} materialised {dense.score.tolist()} |difference| / (sum of the two bounds) "
          f"{(diff / (a_fused + a_dense)).tolist()}")
    assert (diff <= a_fused + a_dense).all()


@pytest.mark.parametrize("name", ["a_ragged", "b_tiles", "d_peaked"])
def test_best_path_is_below_the_sum_over_all_paths(name):
    """score <= -nll of ms_rnnt_score on the same inputs, up to the two bounds."""
    import test_rnnt_score_gpu as G
    c = CASES[name]
    res, _, deltas, _ = ref64(name, False)
    got = run_joint(c)
    nll = G.run_case(c)[0]
    slack = bounds_of(res, deltas, c["in_lens"], c["tgt_lens"]) + S.reference(name)[2]
    print(f"{name}: score {got.score.tolist()} -nll {(-nll).tolist()} slack {slack.tolist()}")
    assert (got.score.astype(np.float64) <= -nll.astype(np.float64) + slack).all()


# ---- edge cases

def test_nan_poisons_its_own_utterance_only():
    name = "b_tiles"
    c = CASES[name]
    clean = run_joint(c)
    enc = c["enc_p"].copy()
    enc[11, 0, 40] = np.nan                                       # an existing frame of utterance 0
    got = run_joint(c, enc_p=enc)
    A.check_consistent(got, c["in_lens"], c["tgt_lens"])
    assert np.isnan(got.score[0]) and (got.token_frame[0] == -1).all() and np.isnan(got.frame_logp[0, :19]).all()
    same_result(got, clean, rows=slice(1, 2))
    # log-probability mode: a NaN / +inf in a b or e of an existing cell, off the best path as well; not in a symbol the
    # recursion does not read
    rng = np.random.default_rng(17)
    x = A.grid_table(rng, 4, 9, 7, 5, p_inf=0.0)
    in_lens, tgt_lens = [9, 9, 6, 9], [6, 4, 6, 3]
    y = R.pad_targets(R.random_targets(rng, 4, 6, 5, 4), tgt_lens, 4)
    clean = assert_bit_exact(x, in_lens, y, tgt_lens, 4)
    x[0, 8, 0, 4] = np.nan                                        # b of a corner cell no good path visits
    x[1, 2, 1, y[1, 1]] = np.inf
    x[3, 4, 2, next(v for v in range(4) if v != y[3, 2])] = np.nan
    got = assert_bit_exact(x, in_lens, y, tgt_lens, 4)
    assert np.isnan(got.score[:2]).all()
    same_result(got, clean, rows=slice(2, 4))


def test_minus_inf_bias_on_a_target_label_means_no_alignment():
    c = CASES["a_ragged"]
    clean = run_joint(c)
    needed = next(int(v) for v in c["targets"][0, :c["tgt_lens"][0]]
                  if not any((c["targets"][n, :c["tgt_lens"][n]] == v).any() for n in (1, 2)))
    b = c["b_out"].copy()
    b[needed] = -np.inf
    got = run_joint(c, b_out=b)
    A.check_consistent(got, c["in_lens"], c["tgt_lens"])
    assert got.score[0] == -np.inf and (got.frame_u[0] == -1).all() and (got.token_logp[0, :3] == -np.inf).all()
    assert np.isfinite(got.score[1:]).all()
    assert got.token_frame[1:].tobytes() == clean.token_frame[1:].tobytes()      # (Z moved a little: the path did not)


def test_the_callers_errors_and_the_supported_shapes():
    rng = np.random.default_rng(19)
    x = A.grid_table(rng, 4, 9, 7, 5, p_inf=0.0)
    y = R.random_targets(rng, 4, 6, 5, 4)
    clean = assert_bit_exact(x, [9, 9, 9, 9], y, [6, 6, 6, 6], 4)
    yb = y.copy()
    yb[0, 2], yb[1, 0] = 10 ** 6, 4                                # a label past V1, a label equal to the blank
    got = assert_bit_exact(x, [9, 9, 0, 10], yb, [6, 6, 6, 6], 4)
    assert (got.score == -np.inf).all()
    got = assert_bit_exact(x, [9, 9, 9, 9], y, [6, -1, 7, 6], 4)
    assert (got.score[1:3] == -np.inf).all()
    same_result(got, clean, rows=[0, 3])
    c = CASES["a_ragged"]
    got = run_joint(c, in_lens=[5, 0, 3], tgt_lens=[3, 2, 4])
    assert (got.score[1:] == -np.inf).all() and np.isfinite(got.score[0])
    # past the supported shapes: MS_ERR_UNSUPPORTED, nothing launched; a short workspace: MS_ERR_WORKSPACE
    lib = _lib.load()
    z = torch.zeros((1025 * 2,), device="cuda")
    out = outputs(1, 1, 1025)
    one, yy = i32([1]), i32(np.zeros(1024))
    nbytes = lib.ms_rnnt_align_workspace_bytes(1, 1, 1025, 2)
    ws = torch.empty(nbytes + lib.ms_rnnt_align_joint_workspace_bytes(1, 1, 1025, 2, 2), dtype=torch.uint8, device="cuda")
    for flags in (0, LOG_PROBS_IN):
        rc = lib.ms_rnnt_align(_lib.ptr(z), _lib.ptr(one), _lib.ptr(yy), _lib.ptr(one), *(_lib.ptr(o) for o in out), 1, 1, 1025, 2,
                               1, flags, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        assert _lib.ERR_NAMES[rc] == "MS_ERR_UNSUPPORTED"
    rc = lib.ms_rnnt_align_joint(_lib.ptr(z), _lib.ptr(z), _lib.ptr(z), None, _lib.ptr(one), _lib.ptr(yy), _lib.ptr(one),
                                 *(_lib.ptr(o) for o in out), 1, 1, 1025, 2, 2, 1, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert _lib.ERR_NAMES[rc] == "MS_ERR_UNSUPPORTED"
    rc = lib.ms_rnnt_align(_lib.ptr(z), _lib.ptr(one), _lib.ptr(yy), _lib.ptr(one), *(_lib.ptr(o) for o in out), 1, 1, 4, 2, 1, 0,
                           _lib.ptr(ws), 16, _lib.stream_ptr())
    assert _lib.ERR_NAMES[rc] == "MS_ERR_WORKSPACE"
    rc = lib.ms_rnnt_align(_lib.ptr(z), _lib.ptr(one), _lib.ptr(yy), _lib.ptr(one), *(_lib.ptr(o) for o in out), 1, 1, 4, 2, 1, 1,
                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert _lib.ERR_NAMES[rc] == "MS_ERR_INVALID"                  # flags takes 0 or MS_RNNT_LOG_PROBS_IN
    torch.cuda.synchronize()
    assert float(out[0][0]) == SENTINEL and bool((out[3] == -777).all()) and bool((out[2] == SENTINEL).all())


@pytest.mark.parametrize("name", ["a_ragged", "b_tiles"])
def test_padding_changes_no_bit_and_runs_repeat(name):
    c = CASES[name]
    clean = run_joint(c)
    same_result(clean, run_joint(c))
    enc, pred, y = c["enc_p"].copy(), c["pred_p"].copy(), c["targets"].copy()
    junk = np.array([np.nan, np.inf, 3e38, -np.inf, -3e38], dtype=np.float32)
    for n, (Tn, Un) in enumerate(zip(c["in_lens"], c["tgt_lens"])):
        enc[Tn:, n] = np.resize(junk, enc[Tn:, n].shape)
        pred[Un + 1:, n] = np.resize(junk[::-1], pred[Un + 1:, n].shape)
        y[n, Un:] = [(-7, 1 << 30, c["blank"], 10 ** 6)[(n + k) % 4] for k in range(y.shape[1] - Un)]
    assert np.isnan(enc).any() and np.isnan(pred).any()
    same_result(run_joint(c, enc_p=enc, pred_p=pred, targets=y), clean)
    # the dense modes: junk in the cells that do not exist
    x = ref64(name, True)[3].copy()
    for log_probs in (False, True):
        clean = run_align(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"], log_probs)
        same_result(clean, run_align(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"], log_probs))
        xd = x.copy()
        for n, (Tn, Un) in enumerate(zip(c["in_lens"], c["tgt_lens"])):
            xd[n, Tn:] = np.resize(junk, xd[n, Tn:].shape)
            xd[n, :, Un + 1:] = np.resize(junk, xd[n, :, Un + 1:].shape)
        same_result(run_align(xd, c["in_lens"], y, c["tgt_lens"], c["blank"], log_probs), clean)


def test_non_default_stream_gives_the_same_bits():
    c = CASES["b_tiles"]
    x = ref64("b_tiles", True)[3]
    want_j = run_joint(c)
    want_l = run_align(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"], False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got_j = run_joint(c)
        got_l = run_align(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"], False)
    torch.cuda.current_stream().wait_stream(s)
    same_result(got_j, want_j)
    same_result(got_l, want_l)


# ---- the Python layer

def alignment_matches(al, res, n, labels, Tn):
    assert al.score == float(res.score[n])
    assert [t.label for t in al.tokens] == labels
    assert [t.start for t in al.tokens] == res.token_frame[n, :len(labels)].tolist()
    assert all(t.end == t.start + 1 for t in al.tokens)
    assert [t.log_prob for t in al.tokens] == res.token_logp[n, :len(labels)].tolist()
    assert al.frame_log_probs == res.frame_logp[n, :Tn].tolist()
    assert len(al.frame_labels) == Tn and [v for f in al.frame_labels for v in f] == labels
    for f, labs in enumerate(al.frame_labels):
        assert len(labs) == int((res.token_frame[n, :len(labels)] == f).sum())


def test_two_aligners_back_to_back_share_no_workspace_state():
    from myrtlespeech_amd.post_process import RNNTForcedAligner
    rng = np.random.default_rng(23)
    a1, a2 = RNNTForcedAligner(4), RNNTForcedAligner(4, log_probs=True)
    big = A.grid_table(rng, 2, 40, 30, 5, p_inf=0.0)
    small = A.grid_table(rng, 3, 9, 7, 5)
    yb, ys = R.random_targets(rng, 2, 29, 5, 4), R.random_targets(rng, 3, 6, 5, 4)
    lb, ls = ([40, 31], [29, 11]), ([9, 1, 5], [6, 0, 4])
    want_b = A.rnnt_align(big, lb[0], yb, lb[1], 4)
    want_s = A.rnnt_align(small, ls[0], ys, ls[1], 4)

    def call(al, x, y, lens):
        return al((torch.as_tensor(x), torch.tensor(lens[0])), (torch.as_tensor(y.astype(np.int64)), torch.tensor(lens[1])))

    first = call(a2, big, yb, lb)
    logits_first = call(a1, big, yb, lb)          # (another aligner, another mode, in between)
    second = call(a2, small, ys, ls)              # a smaller problem in the grown workspace
    third = call(a2, big, yb, lb)
    for outs, want, y, lens in ((first, want_b, yb, lb), (second, want_s, ys, ls), (third, want_b, yb, lb)):
        for n, al in enumerate(outs):
            if want.score[n] == -np.inf:
                assert al is None
            else:
                alignment_matches(al, want, n, y[n, :lens[1][n]].tolist(), lens[0][n])
    assert all(al is not None and al.score <= 0 for al in logits_first)
    bad = big.copy()
    bad[1, 3, 2, 4] = np.nan
    with pytest.raises(RuntimeError, match="utterance 1"):
        call(a2, bad, yb, lb)


def test_model_align_agrees_with_the_aligner_on_the_joint_lattice():
    import test_rnnt_score_gpu as G
    from myrtlespeech_amd.post_process import RNNTForcedAligner, words
    model, pred, joint, enc, lens = G._tiny()
    rng = np.random.default_rng(3)
    y = torch.as_tensor(rng.integers(0, 8, size=(3, 6)))
    y_lens = torch.tensor([6, 3, 0])
    y_pad = y.clone()
    y_pad[1, 3:], y_pad[2, :] = -3, 99                            # the padding is never a label
    lattice = model.joint_lattice(enc.cuda(), lens, y_pad, y_lens)
    dense = RNNTForcedAligner(8)((lattice, lens), (y_pad, y_lens))
    fused = model.align(enc.cuda(), lens, y_pad, y_lens)
    assert len(fused) == len(dense) == 3 and all(a is not None for a in fused + dense)
    # the yardstick is the float64 optimum ON the materialised lattice (what ``dense`` was handed): the logits mode is within its
    # own A_n of it; the fused path and the lattice's cells are each within the fused delta of the exact values
    # (tests/test_rnnt_score_gpu.py bounds the model's weights the same way), so ``fused`` is within the sum of the two
    w, b = joint.out.weight.detach().cpu().numpy(), joint.out.bias.detach().cpu().numpy()
    delta = S.delta(float(np.max(S.eps_v(w, b, w.shape[1]))), float(np.max(np.abs(w).sum(-1) + np.abs(b))) + 2.2)
    tables = []
    ref = A.rnnt_align(lattice.cpu().numpy().astype(np.float64), lens.numpy(), y_pad.numpy(), y_lens.numpy(), 8,
                       log_probs=False, dtype=np.float64, tables=tables)
    for n in range(3):
        Tn, Un = int(lens[n]), int(y_lens[n])
        mag = U24 * max(1.0, abs(float(ref.score[n])))
        a_dense = (Tn + Un) * (8.0 * mag + mag)
        a_fused = 2 * (Tn + Un) * (delta + mag)
        print(f"utterance {n}: fused {fused[n].score:.6f} dense {dense[n].score:.6f} ref {ref.score[n]:.6f} bounds {a_fused:.3g} "
              f"{a_dense:.3g} frames fused {[t.start for t in fused[n].tokens]} dense {[t.start for t in dense[n].tokens]}")
        for al, bound in ((fused[n], a_fused), (dense[n], a_dense)):
            assert abs(al.score - ref.score[n]) <= bound
            assert [t.label for t in al.tokens] == y[n, :Un].tolist() and len(al.frame_labels) == Tn
            rescored = float(A.path_score(tables[n][0], tables[n][1], [t.start for t in al.tokens],
                                          np.cumsum([len(f) for f in al.frame_labels]).tolist(), np.float64))
            assert rescored >= ref.score[n] - 2 * bound
    # words() on a transducer alignment: label 7 as the separator, spans of one frame per label
    al = fused[0]
    spans = words(al, separator_index=7, frame_seconds=0.02)
    runs, cur = [], []
    for t in al.tokens:
        if t.label == 7:
            if cur:
                runs.append(cur)
            cur = []
        else:
            cur.append(t)
    if cur:
        runs.append(cur)
    assert [(s.labels, s.start, s.end) for s in spans] == [([t.label for t in r], r[0].start, r[-1].start + 1) for r in runs]
    assert all(s.start_s == s.start * 0.02 and s.end_s == s.end * 0.02 for s in spans)
