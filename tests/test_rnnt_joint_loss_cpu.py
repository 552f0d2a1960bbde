"""The fused transducer loss with gradient, the part that needs no GPU: the size queries of the C ABI, the argument validation
of ``rnnt_joint_loss`` / ``RNNTJointLoss``, and the premises of tests/test_rnnt_joint_loss_gpu.py -- the numpy restatement
tests/rnnt_joint_loss_ref.py agrees with central finite differences of its own float64 nll, the float32 emulation of the
device's arithmetic sits inside the derived bounds on every case the GPU tests run, and a one-plane (fp16 hi only)
emulation does not.

Worst ratios of the two-plane emulation to the bounds over the cases, measured here: d_enc_p 0.0003, d_pred_p 0.0004,
d_w_out 0.0005, d_b_out 0.0004 of the full bounds; 0.074 / 0.16 / 0.10 / 0.096 of the backward's own share (b_tiles and
e_vocabulary are the worst).

The full bound carries the forward's allowance 3 (B_n + (T_n + U_n) delta_n) in the exponent of every term of g -- a
worst-case sum over the T_n + U_n steps of a path, 0.14 at b_tiles, three hundred times the 2^-11 of an fp16 plane -- so NO
single-plane product can leave it: the one-plane emulation sits at 0.58 (a_ragged), 0.035 (b_tiles), 0.25
(c_columns_blank150), 0.0001 (d_peaked) and 0.059 (e_vocabulary) of it.  That the bound is not vacuous is therefore shown
on the share that belongs to the products: against the float64 gradients that follow from the emulation's OWN forward
lattice (``gradients_given_lattice``) and ``bounds(..., lattice_share=False)``, the one-plane emulation misses by 28
(a_ragged), 15 (b_tiles), 9.1 (c_columns_blank150) and 5.3 (e_vocabulary) while the two-plane one stays inside.  The GPU
tests hold the device to BOTH bounds.
"""
import numpy as np
import pytest
import torch

import rnnt_joint_loss_ref as G
import rnnt_score_ref as S


def test_size_queries(lib):
    assert lib.ms_rnnt_joint_loss_lattice_bytes(16, 250, 121) == 12 * 16 * 250 * 121
    assert lib.ms_rnnt_joint_loss_lattice_bytes(64, 4000, 1024) == 3 * 64 * 4000 * 1024 * 4      # past 2^31: no wrap
    lo, hi = lib.ms_rnnt_joint_loss_backward_workspace_min_bytes, lib.ms_rnnt_joint_loss_backward_workspace_bytes
    # the word-piece shape of the issue: the dense logits are 38.8 GB
    assert 0 < lo(32, 501, 121, 512, 5001) <= hi(32, 501, 121, 512, 5001) <= 512e6
    for n, t, u1, j, v1 in ((16, 250, 121, 512, 30), (1, 1, 1, 1, 1), (3, 7, 5, 24, 4000), (2, 19, 70, 64, 29),
                            (16, 250, 121, 512, 5001)):
        a, b = lo(n, t, u1, j, v1), hi(n, t, u1, j, v1)
        assert 0 < a <= b and a % 16 == 0 and b % 16 == 0
        assert b <= max(a, 512e6)
        # no V1-wide row per cell for the whole lattice: a unit is 8 frames of one utterance, g twice and h once as fp16
        # hi + lo and da as float32, on top of w_out packed twice
        assert a >= 8 * u1 * 8 * (v1 + j) + 8 * j * v1
    # one unit that is larger than the preferred size: the minimum is the preferred size, and it does not wrap
    big = lo(4, 4000, 1024, 4096, 200000)
    assert big == hi(4, 4000, 1024, 4096, 200000) > 2 ** 33
    for bad in ((0, 5, 3), (2, 0, 3), (2, 5, 0), (-1, 5, 3)):
        assert lib.ms_rnnt_joint_loss_lattice_bytes(*bad) == 0
        assert lo(*bad, 8, 7) == 0 and hi(*bad, 8, 7) == 0
    assert lo(2, 5, 3, 0, 7) == 0 and hi(2, 5, 3, 8, -1) == 0


def test_validation_raises_value_error_before_a_device_is_needed():
    from myrtlespeech_amd.loss import RNNTJointLoss, rnnt_joint_loss
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
        "reduction": dict(reduction="average"),
    }

    def module_call(enc_p, pred_p, w_out, b_out, in_lens, targets, target_lens, blank, reduction="mean"):
        return RNNTJointLoss(blank, reduction)((enc_p, in_lens), pred_p, w_out, b_out, (targets, target_lens))

    for call in (rnnt_joint_loss, module_call):
        for name, change in bad_calls.items():
            with pytest.raises(ValueError):
                call(**dict(good, **change))
                pytest.fail(name)
        with pytest.raises(ValueError, match="1024"):
            call(torch.zeros(1, 1, 2), torch.zeros(1026, 1, 2), torch.zeros(2, 2), None, torch.tensor([1]),
                 torch.ones(1, 1025, dtype=torch.int64), torch.tensor([3]), 0)
        if not torch.cuda.is_available():                        # valid arguments: only now is the device asked for
            with pytest.raises(RuntimeError, match="HIP device"):
                call(**good)
            with pytest.raises(RuntimeError, match="HIP device"):
                call(**dict(good, enc_p=enc_p.clone().requires_grad_()))
    assert "blank=4" in repr(RNNTJointLoss(4, "sum"))


def test_restatement_agrees_with_finite_differences():
    """Case a_ragged, every input tensor, 20 random directions: central differences of the float64 weighted nll with step
    1e-5 (truncation O(h^2)) against the directional derivative of the restated gradient, to 1e-6 relative."""
    c = S.cases()["a_ragged"]
    gn, ref, _ = G.reference("a_ragged")
    base = {k: c[k].astype(np.float64) for k in ("enc_p", "pred_p", "w_out", "b_out")}
    grads = dict(enc_p=ref.grads.d_enc_p, pred_p=ref.grads.d_pred_p, w_out=ref.grads.d_w_out, b_out=ref.grads.d_b_out)
    rng = np.random.default_rng(7)
    h = 1e-5
    worst = 0.0
    for key in base:
        for _ in range(20):
            d = rng.standard_normal(base[key].shape)

            def f(step):
                moved = dict(base, **{key: base[key] + step * d})
                return G.weighted_nll(moved["enc_p"], moved["pred_p"], moved["w_out"], moved["b_out"], c, gn)

            fd = (f(h) - f(-h)) / (2 * h)
            an = float(np.sum(grads[key] * d))
            worst = max(worst, abs(fd - an) / max(abs(an), abs(fd)))
            assert abs(fd - an) <= 1e-6 * max(abs(an), abs(fd)), (key, fd, an)
    print("finite differences: worst relative disagreement", worst)


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_float32_emulation_stays_inside_the_bounds(name):
    c = S.cases()[name]
    gn, ref, bnd = G.reference(name)
    assert (np.abs(gn) >= G.GN_MIN).all() and (np.abs(gn) <= G.GN_MAX).all()     # the range the bounds are stated for
    assert np.isfinite(ref.loss.nll).all() and all(np.isfinite(getattr(bnd, k)).all() for k in G.TENSORS)
    got, r32 = G.emulate(c, gn)
    w = G.worst_ratios(got, ref, bnd)
    own, x = G.gradients_given_lattice(c, gn, r32)
    w_own = G.worst_ratios(got, own, G.bounds(own, x, lattice_share=False))
    print(name, "full bounds", {k: round(v, 5) for k, v in w.items()}, "own share", {k: round(v, 5) for k, v in w_own.items()})
    assert max(w.values()) <= 1.0 and max(w_own.values()) <= 1.0, (name, w, w_own)


def test_one_plane_emulation_misses_the_bound():
    """fp16 hi planes only in the three products (module docstring): outside the backward's own share of the bound on b_tiles,
    in every gradient; the full bound's forward allowance is out of a single product's reach, its ratios are printed."""
    for name in ("b_tiles", "a_ragged", "c_columns_blank150"):
        c = S.cases()[name]
        gn, ref, bnd = G.reference(name)
        got, r32 = G.emulate(c, gn, planes=1)
        own, x = G.gradients_given_lattice(c, gn, r32)
        w_own = G.worst_ratios(got, own, G.bounds(own, x, lattice_share=False))
        print(name, "one plane: own share", {k: round(v, 3) for k, v in w_own.items()},
              "full bounds", {k: round(v, 4) for k, v in G.worst_ratios(got, ref, bnd).items()})
        assert min(w_own.values()) > 1.0, (name, w_own)
