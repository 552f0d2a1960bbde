"""The fused transducer scorer, the part that needs no GPU: the size queries of the C ABI, the argument validation of
``rnnt_score`` / ``RNNT.transcript_nll``, and the premise of tests/test_rnnt_score_gpu.py -- the float32 emulation of the
device's arithmetic (tests/rnnt_score_ref.py: fp16 hi + lo planes of both operands, three products, float32 sums, online
log-sum-exp over the kernel's column tiles) sits inside the bounds derived there, on every case the GPU tests run.

Worst ratios of the emulation to the bounds over the cases, measured here: logits 0.080 of eps_v, Z 0.080 of its 16 * 2^-24
max(1, |Z|), nll / alpha / beta 0.0015 / 0.0023 / 0.0022 of B_n + (T_n + U_n) delta_n.
"""
import numpy as np
import pytest
import torch

import rnnt_loss_ref as R
import rnnt_score_ref as S


def test_size_queries(lib):
    assert lib.ms_rnnt_score_lattice_bytes(16, 250, 121) == 8 * 16 * 250 * 121
    assert lib.ms_rnnt_score_lattice_bytes(1, 1, 1) == 8
    for n, t, u1, j, v1 in ((16, 250, 121, 512, 30), (1, 1, 1, 1, 1), (3, 7, 5, 24, 4000), (32, 501, 121, 512, 5001)):
        planes = lib.ms_rnnt_loss_workspace_bytes(n, t, u1, v1)                  # the loss's two skewed planes
        got = lib.ms_rnnt_score_workspace_bytes(n, t, u1, j, v1)
        assert got >= planes + 4 * j * v1 and got % 16 == 0                     # ... and w_out as fp16 hi + lo
        assert got <= planes + 4 * (j + 63) * (v1 + 127)
    # no V1-wide row per cell: the 38.8 GB lattice of the issue's word-piece shape is 50 MB here
    assert lib.ms_rnnt_score_workspace_bytes(32, 501, 121, 512, 5001) + lib.ms_rnnt_score_lattice_bytes(32, 501, 121) < 51e6
    for bad in ((0, 5, 3), (2, 0, 3), (2, 5, 0), (-1, 5, 3)):
        assert lib.ms_rnnt_score_lattice_bytes(*bad) == 0
        assert lib.ms_rnnt_score_workspace_bytes(*bad, 8, 7) == 0
    assert lib.ms_rnnt_score_workspace_bytes(2, 5, 3, 0, 7) == 0 and lib.ms_rnnt_score_workspace_bytes(2, 5, 3, 8, -1) == 0
    assert lib.ms_rnnt_score_lattice_bytes(64, 4000, 1024) == 2 * 64 * 4000 * 1024 * 4      # past 2^31: no wrap


def test_rnnt_score_validation_raises_value_error_before_a_device_is_needed():
    from myrtlespeech_amd.loss.rnnt_loss import rnnt_score
    enc_p, pred_p, w, b = torch.zeros(5, 2, 6), torch.zeros(4, 2, 6), torch.zeros(5, 6), torch.zeros(5)
    xl, y, yl = torch.tensor([5, 3]), torch.tensor([[0, 1, 2], [3, 3, 0]]), torch.tensor([3, 1])
    good = dict(enc_p=enc_p, pred_p=pred_p, w_out=w, b_out=b, in_lens=xl, targets=y, target_lens=yl, blank=4)
    bad_calls = {
        "enc_p dimension": dict(enc_p=enc_p[0]),
        "pred_p dimension": dict(pred_p=pred_p[0]),
        "pred_p batch": dict(pred_p=pred_p[:, :1]),
        "joint features": dict(w_out=torch.zeros(5, 7)),
        "bias shape": dict(b_out=torch.zeros(4)),
        "targets dimension": dict(targets=y.reshape(-1)),
        "targets batch": dict(targets=y[:1]),
        "targets width": dict(targets=y[:, :2]),
        "float targets": dict(targets=y.float()),
        "input lengths batch": dict(in_lens=xl[:1]),
        "target lengths batch": dict(target_lens=torch.tensor([3, 1, 1])),
        "input length 0": dict(in_lens=torch.tensor([5, 0])),
        "input length > T": dict(in_lens=torch.tensor([6, 3])),
        "target length < 0": dict(target_lens=torch.tensor([3, -1])),
        "target length > U": dict(target_lens=torch.tensor([4, 1])),
        "float input lengths": dict(in_lens=xl.float()),
        "float target lengths": dict(target_lens=yl.float()),
        "blank past the symbols": dict(blank=5),
        "negative blank": dict(blank=-1),
    }
    for name, change in bad_calls.items():
        with pytest.raises(ValueError):
            rnnt_score(**dict(good, **change))
            pytest.fail(name)
    with pytest.raises(ValueError, match="1024"):
        rnnt_score(torch.zeros(1, 1, 2), torch.zeros(1026, 1, 2), torch.zeros(2, 2), None, torch.tensor([1]),
                   torch.ones(1, 1025, dtype=torch.int64), torch.tensor([3]), 0)
    if not torch.cuda.is_available():                            # valid arguments: only now is the device asked for
        with pytest.raises(RuntimeError, match="HIP device"):
            rnnt_score(**good)


def test_transcript_nll_and_forward_targets_validation():
    import test_rnnt_loss_cpu as C
    from myrtlespeech_amd.model.rnnt import RNNT
    pred, joint, enc, lens = C.tiny_transducer()
    model = RNNT(torch.nn.Identity(), pred, joint)
    y, yl = torch.tensor([[0, 1], [2, 3], [4, 5]]), torch.tensor([2, 1, 0])
    bad_calls = {
        "enc dimension": (enc[0], lens, y, yl),
        "targets dimension": (enc, lens, y.reshape(-1), yl),
        "targets batch": (enc, lens, y[:2], yl),
        "float targets": (enc, lens, y.float(), yl),
        "lengths batch": (enc, lens[:2], y, yl),
        "target lengths batch": (enc, lens, y, yl[:2]),
        "length > T": (enc, torch.tensor([13, 9, 5]), y, yl),
        "target length > U": (enc, lens, y, torch.tensor([3, 1, 0])),
        "float lengths": (enc, lens.float(), y, yl),
        "float target lengths": (enc, lens, y, yl.float()),
    }
    for name, args in bad_calls.items():
        with pytest.raises(ValueError):
            model.transcript_nll(*args)
            pytest.fail(name)
    with pytest.raises(ValueError, match="1024"):
        model.transcript_nll(enc, lens, torch.zeros(3, 1025, dtype=torch.int64), yl)
    for args in ((y.float(), yl), (y.reshape(-1), yl), (y, yl[:2])):
        with pytest.raises(ValueError):
            pred.forward_targets(*args)
    # a predictor whose blank lies past the joint's symbols
    from myrtlespeech_amd.model.rnnt import RNNTPredictor
    torch.manual_seed(0)
    other = RNNT(torch.nn.Identity(), RNNTPredictor(9, 8, 32, num_layers=1), joint)
    with pytest.raises(ValueError, match="blank"):
        other.transcript_nll(enc, lens, y, yl)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            model.transcript_nll(enc, lens, y, yl)
        with pytest.raises(RuntimeError, match="HIP device"):
            pred.forward_targets(y, yl)


def test_online_logsumexp_edges():
    """The first tiles all -inf give no NaN; a row of -inf only, a NaN and a +inf give NaN."""
    x = np.full((4, 300), -np.inf, dtype=np.float32)
    x[0, 200], x[0, 290] = 1.0, 2.0
    x[2, 5], x[2, 250] = np.nan, 3.0
    x[3, 130], x[3, 0] = np.inf, 0.0
    z = S.online_logsumexp(x, 128)
    assert abs(z[0] - np.log(np.exp(1.0) + np.exp(2.0))) < 1e-6 and np.isnan(z[1:]).all()


@pytest.mark.parametrize("name", sorted(S.cases()))
def test_float32_emulation_stays_inside_the_bounds(name):
    c = S.cases()[name]
    ref, eps, bounds = S.reference(name)
    assert np.isfinite(ref.nll).all() and np.isfinite(bounds).all()
    aw = np.abs(c["w_out"])
    assert aw.min() >= S.W_MIN and aw.max() <= S.W_MAX            # the range the bound is stated for
    x64 = S.joint_logits(c["enc_p"], c["pred_p"], c["w_out"], c["b_out"])
    x32 = S.emulate_logits(c["enc_p"], c["pred_p"], c["w_out"], c["b_out"])
    ex = ref.exists
    r_logit = float(np.max(np.abs(x32[ex] - x64[ex]) / eps))
    z = S.online_logsumexp(x32, S.column_tile_width(c["w_out"].shape[0]))
    # Z of the emulated logits against Z of the SAME logits in float64: the log-sum-exp's own share of delta
    z64 = np.array([R.logsumexp_row(row, np.float64) for row in x32[ex].astype(np.float64)])
    r_z = float(np.max(np.abs(z[ex] - z64) / (16 * S.U24 * np.maximum(1.0, np.abs(z64)))))
    r32 = R.rnnt_loss(x32, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"], dtype=np.float32)
    w = S.worst_ratios(r32.nll, r32.alpha, r32.beta, ref, bounds)
    print(name, "logits", round(r_logit, 4), "Z", round(r_z, 4), {k: round(v, 4) for k, v in w.items()},
          "nll", np.round(ref.nll, 3).tolist(), "bounds", bounds.tolist())
    assert r_logit <= 1.0 and r_z <= 1.0 and max(w.values()) <= 1.0, (name, r_logit, r_z, w)
    if name == "d_peaked":
        assert (ref.nll < 20).all()                              # the tight end of the bound
