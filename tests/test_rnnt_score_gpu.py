"""The fused transducer scorer on the device (``ms_rnnt_score``, ``rnnt_score``, ``RNNT.transcript_nll``) against the float64
numpy reference: dense logits from tests/rnnt_score_ref.py handed to the loss's restatement tests/rnnt_loss_ref.py.

The bounds, derived (not fitted).  With |tanh| <= 1 a logit x[v] = sum_j w[v, j] tanh(enc_p + pred_p) + b[v] is off by at most

  eps_v = 2^-24 ((J + 16) sum_j |w_out[v, j]| + |b_out[v]|)

in units of 2^-24 |w[v, j]| per product:
  J    the float32 roundings of the accumulation: every partial sum is at most sum_j |w| (1 + 2^-10), and the 3 J / 16 MFMA
       instructions of a row round it at most ~5 times each (the 16 products of an instruction are summed in hardware);
  16   the dropped lo.lo term (2^-11 * 2^-11 = 4 units), the rounding of the two lo planes (2^-11 of a value below 2^-11 of
       its operand: up to 4 units each, which cannot all peak with the lo.lo term since a large lo.lo needs both lo planes
       near the middle of an fp16 step), the rounding of enc_p + pred_p (below 1 unit: |x| sech^2 x <= 0.45), the tanh built
       from the hardware exp and reciprocal (~4 units absolute), and fp16 lo planes that flush below 2^-24
  |b|  one rounding of the sum with the bias.
It is stated for weights of magnitude within [2^-10, 2^10] (above, the fp16 planes clamp; far below, the lo plane is gone);
the cases draw their weights inside that range.  A symbol whose bias is -inf is exactly -inf: no error.

A cell's b = x[blank] - Z and e = x[y_u] - Z are then off by at most

  delta = 2 max_v eps_v + 16 * 2^-24 max(1, |Z|)

(the picked logit and Z each move by at most max eps; 16 * 2^-24 max(1, |Z|) is what the loss's tests allow its own Z for
the hardware exp in the sums, the precise logf and the roundings of max + log(sum) -- the online form adds one multiply per
column tile to a sum of positive terms, inside the same allowance).  Every alignment sums T_n + U_n such terms, so with
B_n = 8 (T_n + U_n) 2^-24 max(1, |nll_n|) the loss's own bound (rnnt_loss_ref.bound)

  |nll - ref| <= B_n + (T_n + U_n) delta_n,

and the same for alpha and beta on existing cells (delta_n with the largest |Z| of the utterance's existing cells).
The float32 emulation of this arithmetic sits at 0.0023 of the bound at worst (tests/test_rnnt_score_cpu.py).  The device's
worst ratios are printed by every test here and recorded by tools/rnnt_score_time.py in profiles/rnnt_score_time.json
(0.006 at worst).

The materialised path (``ms_rnnt_joint_forward`` over all cells, then ``ms_rnnt_loss_forward``) forms the same logits with a
float32 dot product of J terms and tanhf: its logits are inside the same eps_v (no split terms, the same J roundings) and its
Z is the loss's, so its nll is inside B_n + (T_n + U_n) delta_n as well; the two paths may differ by the sum of the two.
"""
import numpy as np
import pytest
import torch

import rnnt_loss_ref as R
import rnnt_score_ref as S
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
CASES = S.cases()
worst = {"nll": 0.0, "alpha": 0.0, "beta": 0.0}


def f32(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda().contiguous()


def i32(a):
    return torch.as_tensor(np.ascontiguousarray(a).reshape(-1), dtype=torch.int32).cuda()


def run_abi(enc_p, pred_p, w_out, b_out, in_lens, targets, tgt_lens, blank):
    """One ``ms_rnnt_score`` call; nll and the lattice pre-filled with a sentinel, the workspace with NaN bytes.  Returns
    numpy arrays as the device wrote them: nll [N], lattice [2, N, T, U1] (alpha, beta)."""
    lib = _lib.load()
    T, N, J = enc_p.shape
    U1, V1 = pred_p.shape[0], w_out.shape[0]
    e, p, w = f32(enc_p), f32(pred_p), f32(w_out)
    b = None if b_out is None else f32(b_out)
    xl, yl = i32(in_lens), i32(tgt_lens)
    y = i32(targets) if U1 > 1 else None
    nll = torch.full((N,), SENTINEL, dtype=torch.float32, device="cuda")
    assert lib.ms_rnnt_score_lattice_bytes(N, T, U1) == 8 * N * T * U1
    lattice = torch.full((2, N, T, U1), SENTINEL, dtype=torch.float32, device="cuda")
    nbytes = lib.ms_rnnt_score_workspace_bytes(N, T, U1, J, V1)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    _lib.check(lib.ms_rnnt_score(_lib.ptr(e), _lib.ptr(p), _lib.ptr(w), _lib.ptr(b), _lib.ptr(xl), _lib.ptr(y), _lib.ptr(yl),
                                 _lib.ptr(nll), _lib.ptr(lattice), N, T, U1, J, V1, blank, _lib.ptr(ws), nbytes,
                                 _lib.stream_ptr()), "ms_rnnt_score")
    torch.cuda.synchronize()
    return nll.cpu().numpy(), lattice.cpu().numpy()


def run_case(c, **change):
    c = dict(c, **change)
    return run_abi(c["enc_p"], c["pred_p"], c["w_out"], c["b_out"], c["in_lens"], c["targets"], c["tgt_lens"], c["blank"])


def run_materialised(c):
    """The same nll through the dense logits on the device: ms_rnnt_joint_forward over all N T U1 cells, ms_rnnt_loss_forward."""
    lib = _lib.load()
    T, N, J = c["enc_p"].shape
    U1, V1 = c["pred_p"].shape[0], c["w_out"].shape[0]
    n, t, u = np.meshgrid(np.arange(N), np.arange(T), np.arange(U1), indexing="ij")
    enc_rows = i32(t * N + n)                                                   # row (n, t, u) pairs frame t of n ...
    pred_rows = f32(c["pred_p"].reshape(U1 * N, J)[(u * N + n).reshape(-1)])    # ... with the prediction after y_n[:u]
    e, w, b = f32(c["enc_p"]), f32(c["w_out"]), f32(c["b_out"])
    rows = N * T * U1
    logp = torch.empty((N, T, U1, V1), dtype=torch.float32, device="cuda")
    _lib.check(lib.ms_rnnt_joint_forward(_lib.ptr(e), _lib.ptr(enc_rows), _lib.ptr(pred_rows), _lib.ptr(w), _lib.ptr(b),
                                         _lib.ptr(logp), rows, J, V1, _lib.stream_ptr()), "ms_rnnt_joint_forward")
    xl, yl, y = i32(c["in_lens"]), i32(c["tgt_lens"]), i32(c["targets"])
    nll = torch.full((N,), SENTINEL, dtype=torch.float32, device="cuda")
    lattice = torch.empty((3, N, T, U1), dtype=torch.float32, device="cuda")
    nbytes = lib.ms_rnnt_loss_workspace_bytes(N, T, U1, V1)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")
    _lib.check(lib.ms_rnnt_loss_forward(_lib.ptr(logp), _lib.ptr(xl), _lib.ptr(y), _lib.ptr(yl), _lib.ptr(nll), _lib.ptr(lattice),
                                        N, T, U1, V1, c["blank"], _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "ms_rnnt_loss_forward")
    torch.cuda.synchronize()
    return nll.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def existing_bits(out, exists):
    """nll and the existing cells of alpha / beta, as bytes."""
    nll, lattice = out
    return nll.tobytes() + lattice[0][exists].tobytes() + lattice[1][exists].tobytes()


def check_against(ref, bounds, out, name):
    nll, lattice = out
    w = S.worst_ratios(nll, lattice[0], lattice[1], ref, bounds)
    for k, v in w.items():
        worst[k] = max(worst[k], v)
    print(f"{name}: ratios to the bounds {({k: round(float(v), 4) for k, v in w.items()})}  nll {np.round(nll, 4).tolist()}  "
          f"bounds {[float(f'{b:.3g}') for b in bounds]}")
    print("worst ratios so far", {k: round(float(v), 4) for k, v in worst.items()})
    assert max(w.values()) <= 1.0, (name, w)
    return w


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_within_the_bounds(name):
    """(a) partial cell tile, ragged J slab and column tile, U_n = 0 and T_n = 1; (b) several cell tiles, the lattice's wave
    crossing, tiles that exit early; (c) three column tiles, the last ragged, blank first / in the middle / last; (d) small
    nll; (e) 4096 symbols, 32 column tiles."""
    c = CASES[name]
    ref, _, bounds = S.reference(name)
    out = run_case(c)
    check_against(ref, bounds, out, name)
    assert not (out[0] == SENTINEL).any() and not (out[1][:, ref.exists] == SENTINEL).any()
    if name == "d_peaked":
        assert (out[0] < 20).all()


def test_minus_inf_bias_means_an_impossible_symbol():
    c = CASES["a_ragged"]
    # a column off the targets (and not the blank): finite, inside the bound
    off = next(v for v in range(7) if v != c["blank"] and not (c["targets"] == v).any())
    b = c["b_out"].copy()
    b[off] = -np.inf
    x = S.joint_logits(c["enc_p"], c["pred_p"], c["w_out"], b)
    ref = R.rnnt_loss(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"])
    eps = S.eps_v(c["w_out"], b, c["enc_p"].shape[2])
    out = run_case(c, b_out=b)
    assert np.isfinite(out[0]).all()
    check_against(ref, S.utterance_bounds(ref, c["in_lens"], c["tgt_lens"], eps), out, "-inf off the targets")
    # a column on a label utterance 0 needs (and the others do not): +inf for that utterance only
    needed = next(int(v) for v in c["targets"][0, :c["tgt_lens"][0]]
                  if not any((c["targets"][n, :c["tgt_lens"][n]] == v).any() for n in (1, 2)))
    b = c["b_out"].copy()
    b[needed] = -np.inf
    x = S.joint_logits(c["enc_p"], c["pred_p"], c["w_out"], b)
    ref = R.rnnt_loss(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"])
    assert ref.nll[0] == np.inf and np.isfinite(ref.nll[1:]).all()
    out = run_case(c, b_out=b)
    assert out[0][0] == np.inf
    check_against(ref, S.utterance_bounds(ref, c["in_lens"], c["tgt_lens"], S.eps_v(c["w_out"], b, 24)), out,
                  "-inf on a needed label (the other utterances)")


def test_first_column_tile_all_minus_inf_gives_no_nan():
    """Case c with -inf in b_out[0:128] -- the whole first column tile -- and the blank and the targets outside that range."""
    c = S.make_case(33, 2, 9, 6, 96, 300, [9, 6], [5, 3], 150, labels=range(128, 300))
    assert c["targets"].min() >= 128
    c["b_out"][0:128] = -np.inf
    x = S.joint_logits(c["enc_p"], c["pred_p"], c["w_out"], c["b_out"])
    ref = R.rnnt_loss(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"])
    assert np.isfinite(ref.nll).all()
    out = run_case(c)
    assert np.isfinite(out[0]).all() and np.isfinite(out[1][:, ref.exists]).all()
    eps = S.eps_v(c["w_out"], c["b_out"], 96)
    check_against(ref, S.utterance_bounds(ref, c["in_lens"], c["tgt_lens"], eps), out, "first column tile -inf")
    # every symbol impossible: Z is not finite, NaN
    out = run_case(c, b_out=np.full(300, -np.inf, dtype=np.float32))
    assert np.isnan(out[0]).all()


def test_nan_poisons_its_own_utterance_only():
    name = "b_tiles"
    c = CASES[name]
    ref, _, bounds = S.reference(name)
    clean = run_case(c)
    enc = c["enc_p"].copy()
    enc[11, 0, 40] = np.nan                                       # an existing frame of utterance 0
    out = run_case(c, enc_p=enc)
    assert np.isnan(out[0][0])
    assert same_bits(out[0][1:], clean[0][1:])
    assert same_bits(out[1][:, 1][:, ref.exists[1]], clean[1][:, 1][:, ref.exists[1]])
    check_against(ref._replace(nll=np.array([np.nan, ref.nll[1]])), bounds, out, "NaN in utterance 0")


@pytest.mark.parametrize("name", ["a_ragged", "b_tiles"])
def test_padding_changes_no_bit_and_runs_repeat(name):
    c = CASES[name]
    exists = S.reference(name)[0].exists
    clean = run_case(c)
    assert same_bits(clean[0], run_case(c)[0]) and existing_bits(clean, exists) == existing_bits(run_case(c), exists)
    enc, pred, y = c["enc_p"].copy(), c["pred_p"].copy(), c["targets"].copy()
    junk = np.array([np.nan, np.inf, 3e38, -np.inf, -3e38], dtype=np.float32)
    dirty = 0
    for n, (Tn, Un) in enumerate(zip(c["in_lens"], c["tgt_lens"])):
        enc[Tn:, n] = np.resize(junk, enc[Tn:, n].shape)
        pred[Un + 1:, n] = np.resize(junk[::-1], pred[Un + 1:, n].shape)
        dirty += enc[Tn:, n].size + pred[Un + 1:, n].size
        y[n, Un:] = [(-7, 1 << 30, c["blank"], 10 ** 6)[(n + k) % 4] for k in range(y.shape[1] - Un)]
    assert dirty > 0 and np.isnan(enc).any() and np.isnan(pred).any()
    out = run_case(c, enc_p=enc, pred_p=pred, targets=y)
    assert existing_bits(out, exists) == existing_bits(clean, exists)


@pytest.mark.parametrize("name", ["a_ragged", "b_tiles", "c_columns_blank0", "c_columns_blank150", "c_columns_blank299"])
def test_agrees_with_the_materialised_path_on_the_device(name):
    c = CASES[name]
    _, _, bounds = S.reference(name)
    fused = run_case(c)[0]
    dense = run_materialised(c)
    ratio = np.abs(fused.astype(np.float64) - dense) / (2 * bounds)
    print(f"{name}: fused {fused.tolist()} materialised {dense.tolist()} |difference| / (sum of the two bounds) {ratio.tolist()}")
    assert (ratio <= 1.0).all()


def test_the_callers_errors_and_the_supported_shapes():
    c = CASES["a_ragged"]
    clean = run_case(c)
    y = c["targets"].copy()
    y[0, 1] = 10 ** 6                                             # a label past V1
    out = run_case(c, targets=y, in_lens=[5, 0, 3], tgt_lens=[3, 2, 4])
    assert (out[0] == np.inf).all()
    out = run_case(c, tgt_lens=[3, -1, 0])
    assert out[0][1] == np.inf and same_bits(out[0][[0, 2]], clean[0][[0, 2]])
    # U1 == 1 takes NULL targets; no bias
    rng = np.random.default_rng(9)
    e, p = rng.standard_normal((4, 2, 10)).astype(np.float32), rng.standard_normal((1, 2, 10)).astype(np.float32)
    w = S.draw_weights(rng, 5, 10, 1.0)
    x = S.joint_logits(e, p, w, None)
    ref = R.rnnt_loss(x, [4, 2], np.zeros((2, 0), dtype=np.int32), [0, 0], 2)
    out = run_abi(e, p, w, None, [4, 2], np.zeros((2, 0), dtype=np.int32), [0, 0], 2)
    check_against(ref, S.utterance_bounds(ref, [4, 2], [0, 0], S.eps_v(w, None, 10)), out, "U1 = 1, no bias")
    # past the supported shapes: MS_ERR_UNSUPPORTED, nothing launched
    lib = _lib.load()
    z = torch.zeros((1025, 2), device="cuda")
    nll = torch.full((1,), SENTINEL, device="cuda")
    lat = torch.full((2 * 1025,), SENTINEL, device="cuda")
    nbytes = lib.ms_rnnt_score_workspace_bytes(1, 1, 1025, 2, 2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    one, yy = i32([1]), i32(np.zeros(1024))
    rc = lib.ms_rnnt_score(_lib.ptr(z), _lib.ptr(z), _lib.ptr(z), None, _lib.ptr(one), _lib.ptr(yy), _lib.ptr(one), _lib.ptr(nll),
                           _lib.ptr(lat), 1, 1, 1025, 2, 2, 1, _lib.ptr(ws), nbytes, _lib.stream_ptr())
    assert _lib.ERR_NAMES[rc] == "MS_ERR_UNSUPPORTED"
    rc = lib.ms_rnnt_score(_lib.ptr(z), _lib.ptr(z), _lib.ptr(z), None, _lib.ptr(one), _lib.ptr(yy), _lib.ptr(one), _lib.ptr(nll),
                           _lib.ptr(lat), 1, 1, 4, 2, 2, 1, _lib.ptr(ws), 16, _lib.stream_ptr())
    assert _lib.ERR_NAMES[rc] == "MS_ERR_WORKSPACE"
    torch.cuda.synchronize()
    assert float(nll[0]) == SENTINEL and bool((lat == SENTINEL).all())


def _tiny():
    import test_rnnt_loss_cpu as C
    from myrtlespeech_amd.model.rnnt import RNNT
    pred, joint, enc, lens = C.tiny_transducer()
    return RNNT(torch.nn.Identity(), pred, joint), pred, joint, enc, lens


def _model_bounds(joint, lattice, lens, y, y_lens):
    """Per utterance: the bound of either path for the tiny model, from the float64 restatement on the materialised lattice."""
    ref = R.rnnt_loss(lattice.cpu().numpy(), lens.numpy(), y.numpy(), y_lens.numpy(), 8)
    w, b = joint.out.weight.detach().cpu().numpy(), joint.out.bias.detach().cpu().numpy()
    # (joint_lattice holds log-probabilities: its Z is 0; the logits' own Z is at most max |x| + log 9 <= sum |w| + |b| + 2.2)
    zmax = float(np.max(np.abs(w).sum(-1) + np.abs(b))) + 2.2
    eps_max = float(np.max(S.eps_v(w, b, w.shape[1])))
    return ref, np.array([R.bound(int(lens[n]), int(y_lens[n]), ref.nll[n]) +
                          (int(lens[n]) + int(y_lens[n])) * S.delta(eps_max, zmax) for n in range(len(ref.nll))])


def test_transcript_nll_agrees_with_the_loss_on_the_joint_lattice():
    from myrtlespeech_amd.loss.rnnt_loss import RNNTLoss
    model, pred, joint, enc, lens = _tiny()
    rng = np.random.default_rng(3)
    y = torch.as_tensor(rng.integers(0, 8, size=(3, 6)))
    y_lens = torch.tensor([6, 3, 0])
    y_pad = y.clone()
    y_pad[1, 3:], y_pad[2, :] = -3, 99                            # the padding is never a label
    lattice = model.joint_lattice(enc.cuda(), lens, y_pad, y_lens)
    dense = RNNTLoss(blank=8, reduction="none")((lattice, lens), (y_pad, y_lens)).cpu().numpy()
    fused = model.transcript_nll(enc.cuda(), lens, y_pad, y_lens)
    assert fused.shape == (3,) and fused.dtype == torch.float32 and fused.is_cuda and not fused.requires_grad
    fused = fused.cpu().numpy()
    _, bounds = _model_bounds(joint, lattice, lens, y_pad, y_lens)
    ratio = np.abs(fused.astype(np.float64) - dense) / (2 * bounds)
    print(f"transcript_nll {fused.tolist()} loss(joint_lattice) {dense.tolist()} |difference| / (sum of the bounds) {ratio.tolist()}")
    assert (ratio <= 1.0).all()
    # forward_targets is the predictor's steps in one call: row u = the prediction after y[:u]
    seq = pred.forward_targets(y_pad, y_lens)
    assert seq.shape == (7, 3, 32)
    state, labels = pred.zero_state(3), torch.full((3,), 8, dtype=torch.int32, device="cuda")
    for u in range(4):
        step, state = pred.step(labels, state)
        np.testing.assert_allclose(seq[u, :2].cpu().numpy(), step[:2].cpu().numpy(), rtol=0, atol=1e-5)
        labels = y[:, u].to(device="cuda", dtype=torch.int32)


def test_beam_score_is_below_the_fused_score_of_its_hypothesis():
    """The beam sums a subset of its hypothesis's alignments (premise: tests/test_rnnt_loss_cpu.py)."""
    from myrtlespeech_amd.post_process.rnnt_decoder import RNNTBeamDecoder
    model, pred, joint, enc, lens = _tiny()
    dec = RNNTBeamDecoder(pred, joint)
    hyps = dec(enc.cuda(), lens)
    scores = dec.last_scores
    assert any(len(h) > 0 for h in hyps)
    u_max = max(len(h) for h in hyps)
    y = torch.full((len(hyps), u_max), -3, dtype=torch.int64)
    for n, h in enumerate(hyps):
        y[n, :len(h)] = torch.tensor(h, dtype=torch.int64)
    y_lens = torch.tensor([len(h) for h in hyps])
    nll = model.transcript_nll(enc.cuda(), lens, y, y_lens).cpu().numpy()
    lattice = model.joint_lattice(enc.cuda(), lens, y, y_lens)
    _, bounds = _model_bounds(joint, lattice, lens, y, y_lens)
    for n, h in enumerate(hyps):
        print(f"utterance {n}: hypothesis {h} beam score {scores[n]:.6f} -transcript_nll {-nll[n]:.6f} bound {bounds[n]:.3g}")
        assert scores[n] <= -nll[n] + bounds[n]
