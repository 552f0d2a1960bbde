"""The bidirectional LSTM backward's specification, pinned on the CPU: tests/bilstm_backward_ref.py (the unidirectional
restatement applied to the flipped case, flipped back) against ``torch.nn.LSTM(bidirectional=True)`` in float64 with autograd
(``pack_padded_sequence`` for ragged lengths) -- every output and every gradient, the ``_reverse`` weights included, to 1e-10
of the tensor's largest magnitude -- and a float32 emulation of the device's order of operations against the bounds of
tests/lstm_backward_ref.py evaluated on the flipped case.  Also the ValueErrors of ``rnn_train``,
``RNN.forward(differentiable=True)`` and ``DeepSpeech1.forward(differentiable=True)``, raised before a device is needed, and
the DeepSpeech1 training yardstick of tests/test_ds1_train_gpu.py checked on its own.
"""
import numpy as np
import pytest
import torch

import bilstm_backward_ref as B
import lstm_backward_ref as L

CASES = B.cases()


@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_restatement_is_torch_bidirectional_lstm(name):
    k = CASES[name]
    want = B.torch_layer(k)
    got = B.layer_backward(k)
    assert set(want) <= set(got)
    for key, w in want.items():
        err = L.rel_err(got[key], w)
        assert err <= 1e-10, (name, key, err)


def test_flip_is_within_each_length():
    a = np.arange(4 * 3, dtype=np.float64).reshape(4, 3, 1)
    f = B.flip_time(a, np.array([4, 2, 1]))
    assert f[:, 0, 0].tolist() == [9, 6, 3, 0] and f[:, 1, 0].tolist() == [4, 1, 7, 10] and f[:, 2, 0].tolist() == [2, 5, 8, 11]
    assert np.array_equal(B.flip_time(f, np.array([4, 2, 1])), a)
    assert np.array_equal(B.flip_time(a, None), a[::-1])


def test_emulation_stays_inside_the_bounds():
    """Every operation rounded to float32 in the device's order, both directions: the recompute from the float32 output, then
    the backward from the emulated gates and c."""
    worst = {}
    for name in B.CASE_NAMES:
        live = B.live_mask(name)
        for d in (0, 1):
            g32, c32, dG, d_h0, d_c0, d_b = B.emulate(name, d)
            w = dict(B.recompute_ratios(name, d, g32, c32), **B.backward_ratios(name, d, dG, d_h0, d_c0, d_b))
            assert max(w.values()) <= 1.0, (name, d, w)
            assert not np.any(np.where(live, 0, dG))          # rows past a length: exact zeros
            for key, v in w.items():
                worst[key] = max(worst.get(key, 0.0), v)
    print("emulation, worst ratio to the bounds:", {key: round(v, 4) for key, v in worst.items()})
    # the unidirectional file's check, mirrored: a reverse-direction result that is off in the fourth digit in every sequence's
    # LAST row (step 0 of the flipped run) is not inside them
    name = "t9_n33_h72_ragged"
    r, lens = B.reference(name), CASES[name]["lens"]
    bad = B.flip_time(r["dG"][1], lens).copy()
    bad[0] *= 1.001
    assert L.norm_ratio(B.flip_time(bad, lens), r["dG"][1], r["e_dG"][1]) > 1.0


def test_unsupported_stacks_raise_before_a_device_is_needed():
    from myrtlespeech_amd.model.hard_lstm import HardLSTM
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.rnn_autograd import linear_clamp_train, rnn_train
    x, lens = torch.zeros(3, 2, 4), torch.tensor([3, 2])
    bi = lambda **kw: RNN(RNNType.LSTM, 4, 8, bidirectional=True, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="LSTM"):
        rnn_train(RNN(RNNType.GRU, 4, 8, bidirectional=True), x, lens)
    with pytest.raises(ValueError, match="LSTM"):
        rnn_train(RNN(RNNType.BASIC_RNN, 4, 8), x, lens)
    with pytest.raises(ValueError, match="HardLSTM"):
        rnn_train(HardLSTM(4, 8, bidirectional=True), x, lens)
    for bidirectional in (False, True):
        with pytest.raises(ValueError, match="dropout"):
            rnn_train(RNN(RNNType.LSTM, 4, 8, num_layers=2, dropout=0.1, bidirectional=bidirectional).train(), x, lens)
    with pytest.raises(ValueError, match="sorted"):
        rnn_train(bi(), x, torch.tensor([2, 3]))
    with pytest.raises(ValueError, match="lengths"):
        rnn_train(bi(), x, torch.tensor([4, 3]))
    with pytest.raises(ValueError, match="lengths"):
        rnn_train(bi(), x, torch.tensor([3, 0]))
    with pytest.raises(ValueError, match="lengths"):
        rnn_train(bi(), x, torch.tensor([3]))
    with pytest.raises(ValueError, match="integer"):
        rnn_train(bi(), x, torch.tensor([3.0, 2.0]))
    with pytest.raises(ValueError, match=r"\[T, N, In\]"):
        rnn_train(bi(), torch.zeros(3, 2, 5), lens)
    with pytest.raises(ValueError, match="hx"):      # a unidirectional stack's states: half the rows
        rnn_train(bi(), x, lens, (torch.zeros(1, 2, 8), torch.zeros(1, 2, 8)))
    with pytest.raises(ValueError, match="hx"):
        rnn_train(bi(num_layers=2), x, lens, (torch.zeros(4, 2, 8),))
    # RNN.forward(differentiable=True) is the same node behind the transposes
    with pytest.raises(ValueError, match="LSTM"):
        RNN(RNNType.GRU, 4, 8)((x, lens), differentiable=True)
    with pytest.raises(ValueError, match="sorted"):
        bi()((x, torch.tensor([2, 3])), differentiable=True)
    with pytest.raises(ValueError, match=r"\[T, N, In\]"):      # batch-major [N, T, In] with N = 3: two lengths do not fit
        bi(batch_first=True)((torch.zeros(3, 2, 5), lens), differentiable=True)
    with pytest.raises(ValueError, match="lengths"):
        bi(batch_first=True)((torch.zeros(3, 2, 4), lens), differentiable=True)
    with pytest.raises(ValueError, match="three"):
        bi()((torch.zeros(3, 4), lens), differentiable=True)
    with pytest.raises(ValueError, match="lo < hi"):
        linear_clamp_train(torch.zeros(2, 4), torch.nn.Linear(4, 3), 1.0, 1.0)


def test_deep_speech_1_differentiable_validates_before_a_device_is_needed():
    from myrtlespeech_amd.model.deep_speech_1 import DeepSpeech1
    x, lens = torch.zeros(2, 1, 5, 4), torch.tensor([4, 3])
    with pytest.raises(ValueError, match="hard_lstm"):
        DeepSpeech1(5, 1, 8, 6, 0.0, hard_lstm=True)((x, lens), differentiable=True)
    with pytest.raises(ValueError, match="drop"):
        DeepSpeech1(5, 1, 8, 6, 0.25).train()((x, lens), differentiable=True)
    with pytest.raises(ValueError, match="seq_len"):
        DeepSpeech1(5, 1, 8, 6, 0.0)((torch.zeros(2, 1, 4, 4), lens), differentiable=True)
    if not torch.cuda.is_available():
        # past the checks: dropout is no obstacle in .eval(), nor with drop_prob = 0 in training mode -- what stops these is
        # the missing device, an error of another kind
        for model in (DeepSpeech1(5, 1, 8, 6, 0.25).eval(), DeepSpeech1(5, 1, 8, 6, 0.0).train()):
            with pytest.raises(RuntimeError, match="HIP device"):
                model((x, lens), differentiable=True)


def test_training_yardstick_clamp_regimes_and_learning_rate():
    """The yardstick of tests/test_ds1_train_gpu.py on its own: its two float64 forms agree (the chain with the restatement of
    the project's specification as the LSTM layer, and the whole chain in torch ops); every parameter is reached; in the live
    rows every clipped layer has units at the lower edge and units strictly inside, and at least two layers, fc4 among them,
    have units at the upper edge; under plain SGD at the learning rate that test uses the loss falls at every step."""
    import ds1_train_ref as M
    w, d = M.make()
    loss, grads = M.yardstick(w, d)
    loss2, grads2 = M.torch_full(w, d)
    assert len(grads) == 18
    assert abs(loss - loss2) <= 1e-9 * abs(loss)
    for key, g in grads.items():
        assert L.rel_err(grads2[key], g) <= 1e-9, key
        assert np.any(g), key
    upper = []
    for name, a in zip(("fc1", "fc2", "fc3", "fc4"), M.activations(w, d)):
        lo, hi, inside = float(np.mean(a == 0.0)), float(np.mean(a == M.CLIP)), float(np.mean((a > 0.0) & (a < M.CLIP)))
        print(f"{name}: live units at the lower edge {lo:.3f}, at the upper edge {hi:.3f}, strictly inside {inside:.3f}")
        assert lo > 0 and inside > 0, name
        if hi > 0:
            upper.append(name)
    assert len(upper) >= 2 and "fc4" in upper, upper
    losses = M.sgd_losses(w, d)
    print("float64 SGD losses:", [round(v, 6) for v in losses])
    assert len(losses) == M.STEPS + 1 and all(b < a for a, b in zip(losses, losses[1:]))
