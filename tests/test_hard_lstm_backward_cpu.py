"""The HardLSTM backward's specification, checked without a device (tests/hard_lstm_backward_ref.py, ``R``):

  1. conventions -- the float64 restatement equals torch float64 autograd of the same cell (``torch.clamp`` for the hard sigmoid,
     ``torch.nn.Hardtanh`` for the hard tanh) to 1e-12 on every case, and a kink table pins P (closed) and Q (open) in float32
     against torch float32 autograd, bit for bit; a = -2.5 comes out INSIDE, which a fused 0.2 a + 0.5 gets wrong;
  2. case conditions -- every random case keeps its distance from every kink (>= 16 x its largest derived bound on a recomputed
     value; the device test asks for 8 x on the device's own forward) and, with T >= 3, visits every saturated region and every
     interior;
  3. refusals, all before a device is needed.
"""
import numpy as np
import pytest
import torch

import hard_lstm_backward_ref as R

CASES = R.cases()
KEYS = ("out", "h_n", "c_n", "dx", "d_h0", "d_c0", "d_w_ih", "d_w_hh", "d_b")


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_restatement_equals_torch_float64_autograd(name):
    k = CASES[name]
    got, want = R.layer_backward(k), R.torch_layer(k)
    for key in KEYS:
        if key == "d_b" and key not in want:
            continue
        scale = max(1.0, float(np.max(np.abs(want[key]))))
        assert got[key].shape == want[key].shape, key
        assert float(np.max(np.abs(got[key] - want[key]))) <= 1e-12 * scale, (name, key)
    # the states' gradients are zero or not exactly as torch has them where the case gives none
    assert got["d_b"].shape == (k["ndir"], 4 * k["H"])


def test_kink_table_is_torch_float32_autograd_bit_for_bit():
    kt = R.kink_table()
    H = kt["H"]
    want, got = R.kink_expected(np.float32), R.kink_emulate()
    for key in ("c", "dA", "d_c0"):
        assert want[key].dtype == np.float32 and got[key].tobytes() == want[key].tobytes(), key
    dA = want["dA"].reshape(4, H)
    at = {n: j for j, n in enumerate(kt["names"])}
    lo, mid, hi = (repr(v) for v in R._nbrs(-2.5))
    # P is closed: z == 0 (a = -2.5, TWO roundings) and z == 1 (a = 2.5) pass the gradient; one float32 below -2.5 does not
    for gate, name in enumerate(("a_i", "a_f", None, "a_o")):
        if name is None:
            continue
        assert dA[gate, at[f"{name}={mid}"]] != 0, "a = -2.5 must come out inside the clamp"
        assert dA[gate, at[f"{name}={lo}"]] == 0
        assert dA[gate, at[f"{name}={hi}"]] != 0
        assert dA[gate, at[f"{name}={np.float32(2.5)!r}"]] != 0
    # Q is open: +-1 themselves pass nothing, their inner neighbours do
    for v0 in (-1.0, 1.0):
        out_, on, in_ = sorted(R._nbrs(v0), key=lambda v: -abs(float(v)))
        assert dA[2, at[f"a_g={on!r}"]] == 0 and dA[2, at[f"a_g={out_!r}"]] == 0 and dA[2, at[f"a_g={in_!r}"]] != 0
        # (through c only d_out o Q(c) reaches d_c0 = f dc beside d_cn = 0.75, and f = 1 in these rows)
        assert want["d_c0"][at[f"c={on!r}"]] == 0.75 and want["d_c0"][at[f"c={out_!r}"]] == 0.75
        assert want["d_c0"][at[f"c={in_!r}"]] > 0.75
    # the one row a fused multiply-add gets wrong: -7.45e-9 is outside
    fused = R.kink_emulate(fused=True)["dA"].reshape(4, H)
    for gate, name in ((0, "a_i"), (1, "a_f"), (3, "a_o")):
        assert fused[gate, at[f"{name}={mid}"]] == 0


def test_kink_table_agrees_in_float64_where_float64_sees_the_same_side():
    """The float64 restatement's P and Q on the table's exact points (-2.5 is z = 0 in float64 up to 0.2's own rounding, so only
    the g and c rows, which involve no product, are compared): the same zeros."""
    kt = R.kink_table()
    H = kt["H"]
    a = kt["a"].astype(np.float64).reshape(4, H)
    want = R.kink_expected(np.float32)["dA"].reshape(4, H)
    rows = [j for j, n in enumerate(kt["names"]) if n.startswith("a_g=")]
    assert np.array_equal(R.Q(a[2, rows]) > 0, want[2, rows] != 0)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_case_conditions(name):
    k, r = CASES[name], R.case_reference(name)
    for d in range(k["ndir"]):
        print(name, d, "margin", r["margin"][d], "largest bound", r["e_kink"][d], "ratio", r["margin"][d] / r["e_kink"][d])
        assert r["margin"][d] >= 16.0 * r["e_kink"][d], (name, d)
        if k["T"] >= 3:
            reg = r["regions"][d]
            print(name, d, {key: round(v, 3) for key, v in reg.items()})
            for key, v in reg.items():
                assert v >= (0.20 if key.endswith("_in") else 0.05), (name, d, key, v)


def test_the_case_table_is_the_issue_s():
    shapes = [c[1] for c in R._CASES]
    for want in ((1, 1, 1, 1, 1), (3, 2, 5, 8, 1), (3, 2, 5, 8, 2), (4, 33, 7, 40, 2), (2, 65, 3, 32, 1), (6, 3, 4, 33, 2)):
        assert want in shapes
    # (3, 2, 5, 8, 1) runs both with and without states / state gradients, and with NULL biases
    both = [c for c in R._CASES if c[1] == (3, 2, 5, 8, 1)]
    assert {(c[2], c[3], c[4], c[5]) for c in both} == {(True, True, True, True), (False, False, False, False)}


def test_a_bound_notices_a_flipped_gate():
    """A single gate decided the other way moves dA by far more than the bound: what the margin is kept for."""
    import lstm_backward_ref as L
    name = "t3_n2_h8_states"
    k, r = CASES[name], R.case_reference(name)
    u = R.dir_view(k, 0)
    pre = r["pre"][0].copy()
    H = k["H"]
    j = int(np.argmax(np.abs(r["dA"][0][-1, 0, :H])))          # an i gate that passes a gradient at the last step
    pre[-1, 0, j] = -0.25                                       # ... pushed below the clamp
    dA, _, _, _ = R.backward_steps(u["p"], pre, r["c"][0], u["c0"], u["d_out"], u["d_hn"], u["d_cn"])
    assert L.norm_ratio(dA, r["dA"][0], r["e_dA"][0]) > 1e3


def test_refusals_before_a_device_is_needed():
    from myrtlespeech_amd.model.cnn import Conv1dTo2d      # noqa: F401  (the package imports without a device)
    from myrtlespeech_amd.model.deep_speech_1 import DeepSpeech1
    from myrtlespeech_amd.model.deep_speech_2 import DeepSpeech2
    from myrtlespeech_amd.model.fully_connected import FullyConnected
    from myrtlespeech_amd.model.hard_lstm import HardLSTM
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.rnn_autograd import gru_train, hard_lstm_train, rnn_train
    x, lens = torch.zeros(3, 2, 4), torch.tensor([3, 2])
    with pytest.raises(ValueError, match="HardLSTM"):
        hard_lstm_train(RNN(RNNType.LSTM, 4, 8), x)
    with pytest.raises(ValueError, match="HardLSTM"):
        hard_lstm_train(torch.nn.LSTM(4, 8), x)
    hard = HardLSTM(4, 8, num_layers=2, bidirectional=True)
    assert hard.hard_backward is False
    for bad in (torch.zeros(3, 2, 5), torch.zeros(3, 4), torch.zeros(0, 2, 4)):
        with pytest.raises(ValueError, match=r"\[T, N, In\]"):
            hard_lstm_train(hard, bad)
    for bad in ((torch.zeros(2, 2, 8), torch.zeros(2, 2, 8)),          # a unidirectional / one-layer stack's states
                (torch.zeros(4, 2, 8), torch.zeros(4, 3, 8)),
                (torch.zeros(4, 2, 8),), torch.zeros(4, 2, 8)):
        with pytest.raises(ValueError, match="hx"):
            hard_lstm_train(hard, x, bad)
    with pytest.raises(ValueError, match="hx"):
        hard((x, lens), (torch.zeros(4, 2, 8), torch.zeros(4, 2, 7)), differentiable=True)
    with pytest.raises(ValueError, match=r"\[T, N, In\]"):      # batch-major input of the wrong width
        HardLSTM(4, 8, batch_first=True)((torch.zeros(2, 3, 5), lens), differentiable=True)
    # the other entries keep refusing the module outright
    for train in (rnn_train, gru_train):
        with pytest.raises(ValueError, match="HardLSTM"):
            train(hard, x, lens)
    # the models: refused with the switch off, as before ...
    ds1 = DeepSpeech1(5, 1, 8, 6, 0.0, hard_lstm=True)
    assert isinstance(ds1.bi_lstm, HardLSTM) and ds1.bi_lstm.hard_backward is False
    feats = (torch.zeros(2, 1, 5, 4), torch.tensor([4, 3]))
    with pytest.raises(ValueError, match="hard_lstm"):
        ds1(feats, differentiable=True)
    ds2 = DeepSpeech2(None, HardLSTM(5, 8), None, FullyConnected(8, 6, 0, None, None))
    with pytest.raises(ValueError, match="HardLSTM"):
        ds2(feats, differentiable=True)
    if not torch.cuda.is_available():
        # ... and past every check with it on: what stops these is the missing device, an error of another kind
        ds1.bi_lstm.hard_backward = True
        ds2.rnn.hard_backward = True
        for call in (lambda: ds1(feats, differentiable=True), lambda: ds2(feats, differentiable=True),
                     lambda: hard_lstm_train(hard, x), lambda: hard((x, lens), differentiable=True)):
            with pytest.raises(RuntimeError, match="HIP device"):
                call()
