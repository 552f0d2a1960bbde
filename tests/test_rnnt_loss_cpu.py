"""Transducer loss, the part that needs no GPU: the numpy restatement of the specification (tests/rnnt_loss_ref.py) against
brute-force enumeration and finite differences, the size queries of the C ABI, ``RNNTLoss``'s argument validation, and the
premises of tests/test_rnnt_loss_gpu.py (the float32 restatement inside a quarter of the GPU bounds on the GPU cases; the
oracle's beam score below the full log-likelihood of its hypothesis)."""
import numpy as np
import pytest
import torch

import rnnt_loss_ref as R


@pytest.mark.parametrize("T,U", [(1, 0), (1, 2), (3, 2), (4, 3)])
def test_restatement_equals_brute_force_enumeration(T, U):
    rng = np.random.default_rng(10 * T + U)
    V1, blank = 4, 3
    x = (rng.standard_normal((2, T, U + 1, V1)) * 2).astype(np.float64)
    y = R.random_targets(rng, 2, U, V1, blank)
    r = R.rnnt_loss(x, [T, T], y, [U, U], blank)
    for n in range(2):
        want = R.brute_force_ll(x[n], T, y[n].tolist(), blank)
        assert abs(-r.nll[n] - want) < 1e-12 * max(1.0, abs(want))
        assert abs(r.beta[n, 0, 0] - (-r.nll[n])) < 1e-12 * max(1.0, abs(want))         # beta(0, 0) == ll
    # blank in the middle of the symbol range, ragged: the enumeration again
    x = (rng.standard_normal((1, T + 1, U + 2, V1)) * 2).astype(np.float64)
    y = R.random_targets(rng, 1, U + 1, V1, 1)
    r = R.rnnt_loss(x, [T], y, [U], 1)
    assert abs(-r.nll[0] - R.brute_force_ll(x[0], T, y[0, :U].tolist(), 1)) < 1e-12 * max(1.0, abs(r.nll[0]))
    assert not r.exists[0, T:].any() and not r.exists[0, :, U + 1:].any() and (r.grad[0][~r.exists[0]] == 0).all()


def test_float64_gradient_equals_central_differences_and_rows_sum_to_zero():
    rng = np.random.default_rng(3)
    N, T, U, V1, blank = 2, 3, 2, 4, 1
    x = rng.standard_normal((N, T, U + 1, V1)) * 1.5
    y = R.random_targets(rng, N, U, V1, blank)
    in_lens, tgt_lens, w = [3, 2], [2, 1], np.array([0.7, -1.3])
    r = R.rnnt_loss(x, in_lens, y, tgt_lens, blank, grad_nll=w)
    h = 1e-6
    fd = np.zeros_like(x)
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        fd[idx] = float(w @ (R.rnnt_loss(xp, in_lens, y, tgt_lens, blank).nll - R.rnnt_loss(xm, in_lens, y, tgt_lens, blank).nll)) / (2 * h)
    assert np.max(np.abs(fd - r.grad)) < 1e-8
    assert np.max(np.abs(r.grad.sum(-1))) < 1e-14              # log-softmax included: every row sums to 0
    assert (r.grad[~r.exists] == 0).all() and np.abs(r.grad[r.exists]).max() > 0.1


def test_restatement_edge_cases():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((3, 4, 3, 5)).astype(np.float32)
    y = np.array([[0, 1], [2, 3], [1, 1]], dtype=np.int32)
    clean = R.rnnt_loss(x, [4, 3, 4], y, [2, 1, 2], 4)
    # impossible transcript: a needed label is -inf everywhere
    xi = x.copy()
    xi[0, :, :, 1] = -np.inf
    r = R.rnnt_loss(xi, [4, 3, 4], y, [2, 1, 2], 4)
    assert r.nll[0] == np.inf and (r.grad[0] == 0).all() and r.nll[1] == clean.nll[1] and np.isfinite(r.nll[2])
    # poison in an existing cell of utterance 1 only; garbage outside the existing cells changes nothing
    xn = x.copy()
    xn[1, 2, 1, 0] = np.nan
    xn[1, 3, 0, 0] = np.nan                                    # t = 3 >= T_1: not an existing cell
    xn[0, 0, 0, 3] = -np.inf
    r = R.rnnt_loss(xn, [4, 3, 4], y, [2, 1, 2], 4)
    assert np.isnan(r.nll[1]) and np.isnan(r.grad[1][r.exists[1]]).all() and (r.grad[1][~r.exists[1]] == 0).all()
    assert np.isfinite(r.nll[[0, 2]]).all() and r.nll[2] == clean.nll[2] and (r.grad[0, 0, 0, 3] == 0)
    # the caller's errors: nll = +inf, zero gradient
    for in_lens, tgt_lens, yy in (([0, 3, 4], [2, 1, 2], y), ([5, 3, 4], [2, 1, 2], y), ([4, 3, 4], [3, 1, 2], y),
                                  ([4, 3, 4], [2, 1, 2], np.array([[0, 4], [2, 3], [1, 1]])),
                                  ([4, 3, 4], [2, 1, 2], np.array([[0, 5], [2, 3], [1, 1]]))):
        r = R.rnnt_loss(x, in_lens, yy, tgt_lens, 4)
        assert r.nll[0] == np.inf and (r.grad[0] == 0).all() and r.nll[1] == clean.nll[1]


def test_size_queries(lib):
    assert lib.ms_rnnt_loss_lattice_bytes(16, 501, 121) == 3 * 16 * 501 * 121 * 4
    assert lib.ms_rnnt_loss_lattice_bytes(1, 1, 1) == 12
    plane = lambda n, t, u1: -(-(n * (t + u1 - 1) * u1 * 4) // 256) * 256    # noqa: E731  [N][T + U1 - 1][U1] floats, skewed
    assert lib.ms_rnnt_loss_workspace_bytes(16, 501, 121, 29) == 2 * plane(16, 501, 121)
    assert lib.ms_rnnt_loss_workspace_bytes(1, 1, 1, 1) == 512
    assert lib.ms_rnnt_loss_workspace_bytes(3, 7, 5, 9) == lib.ms_rnnt_loss_workspace_bytes(3, 7, 5, 4000)   # no V1-sized row
    for bad in ((0, 5, 3), (2, 0, 3), (2, 5, 0), (-1, 5, 3)):
        assert lib.ms_rnnt_loss_lattice_bytes(*bad) == 0
        assert lib.ms_rnnt_loss_workspace_bytes(*bad, 7) == 0
    assert lib.ms_rnnt_loss_workspace_bytes(2, 5, 3, 0) == 0
    # large shapes do not wrap: N T U1 past 2^31 elements
    assert lib.ms_rnnt_loss_lattice_bytes(64, 4000, 1024) == 3 * 64 * 4000 * 1024 * 4


def test_argument_validation_raises_value_error_before_a_device_is_needed():
    from myrtlespeech_amd.loss.rnnt_loss import RNNTLoss
    for bad in (dict(blank=0, reduction="avg"), dict(blank=-1)):
        with pytest.raises(ValueError):
            RNNTLoss(**bad)
    loss = RNNTLoss(blank=4, reduction="none")
    x = torch.zeros(2, 5, 4, 5)
    xl, y, yl = torch.tensor([5, 3]), torch.tensor([[0, 1, 2], [3, 3, 0]]), torch.tensor([3, 1])
    bad_calls = {
        "logits dimension": ((x[0], xl), (y, yl)),
        "targets dimension": ((x, xl), (y.reshape(-1), yl)),
        "targets batch": ((x, xl), (y[:1], yl)),
        "targets width": ((x, xl), (y[:, :2], yl)),
        "float targets": ((x, xl), (y.float(), yl)),
        "logit lengths batch": ((x, xl[:1]), (y, yl)),
        "target lengths batch": ((x, xl), (y, torch.tensor([3, 1, 1]))),
        "logit length 0": ((x, torch.tensor([5, 0])), (y, yl)),
        "logit length > T": ((x, torch.tensor([6, 3])), (y, yl)),
        "target length < 0": ((x, xl), (y, torch.tensor([3, -1]))),
        "target length > U": ((x, xl), (y, torch.tensor([4, 1]))),
        "float logit lengths": ((x, xl.float()), (y, yl)),
        "float target lengths": ((x, xl), (y, yl.float())),
    }
    for name, (a, b) in bad_calls.items():
        with pytest.raises(ValueError):
            loss(a, b)
            pytest.fail(name)
    with pytest.raises(ValueError, match="blank"):
        RNNTLoss(blank=5)((x, xl), (y, yl))                      # blank outside [0, V1)
    with pytest.raises(ValueError, match="1024"):
        RNNTLoss(blank=0)((torch.zeros(1, 1, 1026, 2), torch.tensor([1])),
                          (torch.ones(1, 1025, dtype=torch.int64), torch.tensor([3])))
    if not torch.cuda.is_available():                            # valid arguments: only now is the device asked for
        with pytest.raises(RuntimeError, match="HIP device"):
            loss((x, xl), (y, yl))


_ref64 = {}


def ref64(name):
    if name not in _ref64:
        c = R.gpu_cases()[name]
        _ref64[name] = (c, R.rnnt_loss(c["logits"], c["in_lens"], c["targets"], c["tgt_lens"], c["blank"]))
    return _ref64[name]


@pytest.mark.parametrize("name", sorted(R.gpu_cases()))
def test_float32_restatement_stays_within_a_quarter_of_the_gpu_bounds(name):
    """The GPU tests hold the device to B_n (nll, alpha, beta) and 4 B_n |grad_nll| (gradient) against the float64 restatement;
    the specification evaluated in float32 must sit well inside them, or the bounds would ask more than the number format
    gives.  The float32 restatement keeps its running sums as compensated pairs, as the device does (rnnt_loss_ref._Sums):
    measured here, its worst ratios over the cases are 0.051 (nll), 0.131 (alpha), 0.137 (beta), 0.012 (gradient).  With PLAIN
    float32 running sums the ratios of cases (a) .. (e) and (g) are at most 0.051 / 0.019 / 0.051 / 0.012, but the peaked case (f)
    -- nll of 3, alpha and beta down to -317 off the boosted alignment, every plain sum there rounding by 2^-17 = B_n / 8 --
    comes to 0.025 / 0.382 / 1.013 / 0.001: outside the quarter, and for beta outside the bound itself.  The plain figures are
    printed beside the asserted ones."""
    c, r64 = ref64(name)
    args = (c["logits"], c["in_lens"], c["targets"], c["tgt_lens"], c["blank"])
    assert np.isfinite(r64.nll).all()
    r32 = R.rnnt_loss(*args, dtype=np.float32)
    w = R.worst_ratios(r32.nll, r32.alpha, r32.beta, r32.grad, r64, c["in_lens"], c["tgt_lens"])
    plain = R.rnnt_loss(*args, dtype=np.float32, compensated=False)
    wp = R.worst_ratios(plain.nll, plain.alpha, plain.beta, plain.grad, r64, c["in_lens"], c["tgt_lens"])
    print(name, "float32:", {k: round(v, 4) for k, v in w.items()}, "plain sums:", {k: round(v, 4) for k, v in wp.items()},
          "nll", np.round(r64.nll, 3).tolist())
    assert max(w.values()) <= 0.25, (name, w)
    if name == "f_peaked":
        assert (r64.nll < 20).all()                              # the small-nll, tight-bound case


def tiny_transducer(seed=0):
    """The tiny seeded model of the end-to-end GPU test: predictor hidden 32, 1 layer, joint 32, V = 8, encoder features 16."""
    from myrtlespeech_amd.model.rnnt import RNNTJoint, RNNTPredictor
    torch.manual_seed(seed)
    pred = RNNTPredictor(8, 8, 32, num_layers=1).eval()
    joint = RNNTJoint(16, 32, 32, 8).eval()
    with torch.no_grad():
        joint.out.bias[:8] += 1.0                                # labels likely enough for non-empty hypotheses
    enc = torch.randn(12, 3, 16)
    return pred, joint, enc, torch.tensor([12, 9, 5])


def oracle_joint_lattice(psd, jsd, enc_n, hyp, hidden, layers, blank):
    """[T_n, U + 1, V + 1] log-probabilities of one utterance's hypothesis, from the oracle's own pieces."""
    from oracle import rnnt_oracle as RO
    preds, state, label = [], RO._zero_state(layers, hidden), blank
    for u in range(len(hyp) + 1):
        p, state = RO.predictor_step(psd, label, state, hidden, layers)
        preds.append(p)
        if u < len(hyp):
            label = hyp[u]
    return np.stack([np.stack([RO.joint_logprobs(jsd, enc_n[t], p) for p in preds]) for t in range(enc_n.shape[0])])


def test_premise_beam_score_is_below_the_log_likelihood_of_its_hypothesis():
    """The beam sums a SUBSET of its hypothesis's alignments (merged blank transitions of one prefix), so its score cannot
    exceed the full sum the loss computes: the end-to-end GPU test asserts exactly this of the device's two sides."""
    from oracle import rnnt_oracle as RO
    pred, joint, enc, lens = tiny_transducer()
    psd = {k: v.detach().cpu().numpy() for k, v in pred.state_dict().items()}
    jsd = {k: v.detach().cpu().numpy() for k, v in joint.state_dict().items()}
    e = enc.numpy()
    hyps, scores = RO.beam_decode(e, lens.numpy(), psd, jsd, 32, 1, 8, 8, 3)
    assert any(len(h) > 0 for h in hyps)
    for n, (hyp, score) in enumerate(zip(hyps, scores)):
        Tn = int(lens[n])
        lat = oracle_joint_lattice(psd, jsd, e[:Tn, n], hyp, 32, 1, 8)
        y = np.array([hyp], dtype=np.int32).reshape(1, len(hyp))
        r = R.rnnt_loss(lat[None], [Tn], y, [len(hyp)], 8)
        print(f"utterance {n}: hypothesis {hyp} beam score {score:.5f} ll {-r.nll[0]:.5f}")
        assert score <= -r.nll[0] + 1e-4
