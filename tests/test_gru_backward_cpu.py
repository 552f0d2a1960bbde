"""The GRU backward's specification, pinned on the CPU: the float64 numpy restatement tests/gru_backward_ref.py against
``torch.nn.GRU`` in float64 with autograd on packed sequences -- every output and every gradient of both directions and of a
two-layer bidirectional stack to 1e-12 of the tensor's largest magnitude -- the tanh-as-GRU slices against ``torch.nn.RNN``, and
a float32 emulation of the device's order of operations against the bounds that file derives.  Also the ValueErrors of
``gru_train``, raised before a device is needed, the opt-in switch ``RNN.gru_backward``, and the yardstick of
tests/test_gru_train_gpu.py checked on its own.
"""
import numpy as np
import pytest
import torch

import gru_backward_ref as G

CASES = G.cases()
PIN = 1e-12


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_restatement_is_torch_gru(name):
    k = CASES[name]
    want = G.torch_layer(k)
    got = G.layer_backward(k)
    assert set(want) <= set(got)
    for key, w in want.items():
        err = G.rel_err(got[key], w)
        assert err <= PIN, (name, key, err)
    # direction 0 alone is the unidirectional layer
    u = G.dir_view(k, 0)
    h0 = None if u["h0"] is None else u["h0"][None]
    d_hn = None if u["d_hn"] is None else u["d_hn"][None]
    want = G.torch_stack([(u["p"],)], u["x"], h0, u["lens"], u["d_out"], d_hn, bidirectional=False)
    got = G.dir_layer_backward(u["p"], u["x"], u["h0"], u["lens"], u["d_out"], u["d_hn"])
    for key, w in dict(out=want["out"], h_n=want["h_n"][0], dx=want["dx"], d_h0=want["d_h0"][0],
                       **{a: b[0] for a, b in want["layers"][0].items()}).items():
        assert G.rel_err(got[key], w) <= PIN, (name, key)


def test_restatement_is_torch_gru_on_a_two_layer_bidirectional_stack():
    s = G.stack_case()
    want = G.torch_stack(s["layers"], s["x"], s["h0"], s["lens"], s["d_out"], s["d_hn"])
    got = G.stack_backward(s["layers"], s["x"], s["h0"], s["lens"], s["d_out"], s["d_hn"])
    for key in ("out", "h_n", "dx", "d_h0"):
        assert G.rel_err(got[key], want[key]) <= PIN, key
    for i, layer in enumerate(want["layers"]):
        for key, w in layer.items():
            assert G.rel_err(got["layers"][i][key], w) <= PIN, (i, key)


def tanh_as_gru_np(p):
    """``tanh_rnn_as_gru`` (the module's own function, on CPU tensors) on one direction's numpy parameters."""
    from myrtlespeech_amd.model.rnn import tanh_rnn_as_gru
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float32))      # noqa: E731
    wi, wh, bi, bh = tanh_rnn_as_gru([(t(p["w_ih"]), t(p["w_hh"]), t(p["b_ih"]), t(p["b_hh"]))])[0]
    return dict(w_ih=wi.numpy(), w_hh=wh.numpy(), b_ih=bi.numpy(), b_hh=bh.numpy())


@pytest.mark.parametrize("name", ("t9_n3_h7_ragged", "t2_n3_h40_equal"))
def test_tanh_as_gru_slices_are_torch_rnn(name):
    """A tanh layer's parameters are the n-block rows of a case's: its gradients are rows [2H:3H] of the GRU's on
    ``tanh_rnn_as_gru``'s parameters, dx and d_h0 as they are; r is exactly 1, z exactly 0, so da_r, da_z are exact zeros."""
    k = CASES[name]
    H = k["H"]
    cut = lambda p: {key: (None if v is None else v[2 * H:]) for key, v in p.items()}      # noqa: E731
    tanh_p = tuple(cut(p) for p in k["p"])
    want = G.torch_stack([tanh_p], k["x"], k["h0"], k["lens"], k["d_out"], k["d_hn"], tanh=True)
    with np.errstate(over="ignore"):
        got = G.layer_backward(dict(k, p=tuple(tanh_as_gru_np(p) for p in tanh_p)))
    for key in ("out", "h_n", "dx", "d_h0"):
        assert G.rel_err(got[key], want[key]) <= PIN, (name, key)
    for key, w in want["layers"][0].items():
        assert G.rel_err(got[key][:, 2 * H:], w) <= PIN, (name, key)
        assert not np.any(got[key][:, :2 * H]), (name, key)


def test_emulation_stays_inside_the_bounds():
    """Every operation rounded to float32 in the device's order, both directions: the recompute from the float32 output, then
    the backward from the emulated gates and q.  A ratio above 1 would mean the derivation is wrong."""
    worst = {}
    for name in G.CASE_NAMES:
        live = G.live_mask(name)
        for d in (0, 1):
            g32, q32, dGi, dGh, d_h0, d_bi, d_bh = G.emulate(name, d)
            w = dict(G.recompute_ratios(name, d, g32, q32), **G.backward_ratios(name, d, dGi, dGh, d_h0, d_bi, d_bh))
            assert max(w.values()) <= 1.0, (name, d, w)
            assert not np.any(np.where(live, 0, dGi)) and not np.any(np.where(live, 0, dGh))      # rows past a length: exact zeros
            for key, v in w.items():
                worst[key] = max(worst.get(key, 0.0), v)
    print("emulation, worst ratio to the bounds:", {key: round(v, 4) for key, v in worst.items()})
    # a bound must bite: dGh off in the fourth digit at the step the errors have travelled furthest to is not inside it, in
    # the forward direction (t = 0) and in the reverse one (every sequence's LAST row: step 0 of the flipped run)
    name = G.LARGEST_RAGGED
    r, lens = G.reference(name), CASES[name]["lens"]
    bad = r["dGh"][0].copy()
    bad[0] *= 1.001
    assert G.norm_ratio(bad, r["dGh"][0], r["e_dGh"][0]) > 1.0
    bad = G.flip_time(r["dGh"][1], lens).copy()
    bad[0] *= 1.001
    assert G.norm_ratio(G.flip_time(bad, lens), r["dGh"][1], r["e_dGh"][1]) > 1.0


def test_bounds_are_small():
    """The bounds are float32 rounding, not slack, where a wrong or missing term is of order 1 (tests/test_lstm_backward_cpu.py's
    figures: gates and q below 1e-3 of the tensor's largest magnitude, the gradients' row norms below 2e-2 of the largest).  The
    bias sums get 1e-1: their bound adds the bounds of up to 170 rows by the triangle inequality while the sum of that many
    rows of mixed sign grows like the square root of their number, so it is an order of magnitude looser than a row's."""
    for name in G.CASE_NAMES:
        r = G.reference(name)
        for d in (0, 1):
            for key, bound in (("gates", "e_gates"), ("q", "e_q")):
                scale = float(np.max(np.abs(r[key][d])))
                assert float(np.max(r[bound][d])) <= 1e-3 * scale, (name, d, key)
            for key, bound in (("dGi", "e_dGi"), ("dGh", "e_dGh"), ("d_h0", "e_h0"), ("d_b_ih", "e_b_ih"), ("d_b_hh", "e_b_hh")):
                scale = float(np.max(np.sqrt((r[key][d] ** 2).sum(-1))))
                if scale > 0:
                    cap = 1e-1 if key.startswith("d_b") else 2e-2
                    assert float(np.max(r[bound][d])) <= cap * scale, (name, d, key, float(np.max(r[bound][d])) / scale)


def test_every_gate_regime_occurs():
    """At the cases' scale saturated and unsaturated gates all occur: r and z below 0.1 and above 0.9, |n| above 0.9 and below
    0.5, each in at least 2 % of the live elements of every case that has at least 500 of them."""
    seen = 0
    for name in G.CASE_NAMES:
        for d in (0, 1):
            shares, count = G.regime_shares(name, d)
            print(name, d, count, {key: round(float(v), 3) for key, v in shares.items()})
            if count >= 500:
                seen += 1
                assert min(shares.values()) >= 0.02, (name, d, shares)
    assert seen >= 8


def test_header_declares_and_library_exports_the_entries():
    from myrtlespeech_amd import _lib
    names = ("ms_gru_recompute_workspace_bytes", "ms_gru_recompute", "ms_gru_backward_steps")
    declared = set(_lib.header_symbols())
    lib = _lib.load()
    for name in names:
        assert name in declared and hasattr(lib, name), name
    assert lib.ms_gru_recompute_workspace_bytes(9, 33, 74) == 2 * ((9 * 33 * 222 * 4 + 255) // 256 * 256)
    assert lib.ms_gru_recompute_workspace_bytes(1, 1, 7) == 2 * 256
    for shape in ((0, 3, 7), (9, 0, 7), (9, 3, 0), (-1, 3, 7)):
        assert lib.ms_gru_recompute_workspace_bytes(*shape) == 0


def test_gru_train_raises_before_a_device_is_needed():
    from myrtlespeech_amd.model.hard_lstm import HardLSTM
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.rnn_autograd import gru_train
    x, lens = torch.zeros(3, 2, 4), torch.tensor([3, 2])
    gru = lambda **kw: RNN(RNNType.GRU, 4, 8, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="rnn_train"):
        gru_train(RNN(RNNType.LSTM, 4, 8), x, lens)
    with pytest.raises(ValueError, match="rnn_train"):
        gru_train(RNN(RNNType.LSTM, 4, 8, bidirectional=True), x, lens)
    with pytest.raises(ValueError, match="HardLSTM"):
        gru_train(HardLSTM(4, 8), x, lens)
    for kind in (RNNType.GRU, RNNType.BASIC_RNN):
        for bidirectional in (False, True):
            with pytest.raises(ValueError, match="dropout"):
                gru_train(RNN(kind, 4, 8, num_layers=2, dropout=0.1, bidirectional=bidirectional).train(), x, lens)
    with pytest.raises(ValueError, match="sorted"):
        gru_train(gru(), x, torch.tensor([2, 3]))
    with pytest.raises(ValueError, match="lengths"):
        gru_train(gru(), x, torch.tensor([4, 3]))
    with pytest.raises(ValueError, match="lengths"):
        gru_train(gru(), x, torch.tensor([3, 0]))
    with pytest.raises(ValueError, match="lengths"):          # short: one length for two sequences
        gru_train(gru(), x, torch.tensor([3]))
    with pytest.raises(ValueError, match="integer"):
        gru_train(gru(), x, torch.tensor([3.0, 2.0]))
    with pytest.raises(ValueError, match=r"\[T, N, In\]"):
        gru_train(gru(), torch.zeros(3, 2, 5), lens)
    with pytest.raises(ValueError, match=r"\[T, N, In\]"):
        gru_train(gru(), torch.zeros(3, 4), lens)
    with pytest.raises(ValueError, match="hx"):               # a unidirectional stack's state for a bidirectional one
        gru_train(gru(bidirectional=True), x, lens, torch.zeros(1, 2, 8))
    with pytest.raises(ValueError, match="hx"):               # an LSTM's (h0, c0)
        gru_train(gru(), x, lens, (torch.zeros(1, 2, 8), torch.zeros(1, 2, 8)))
    with pytest.raises(ValueError, match="hx"):
        gru_train(RNN(RNNType.BASIC_RNN, 4, 8, num_layers=2), x, lens, torch.zeros(2, 3, 8))
    if not torch.cuda.is_available():
        # past the checks: what stops a valid call is the missing device, an error of another kind
        for rnn in (gru(), gru(bidirectional=True, num_layers=2), RNN(RNNType.BASIC_RNN, 4, 8)):
            with pytest.raises(RuntimeError, match="HIP device"):
                gru_train(rnn, x, lens)
        with pytest.raises(RuntimeError, match="HIP device"):
            gru_train(gru(num_layers=2, dropout=0.1).eval(), x, lens, torch.zeros(2, 2, 8))


def test_the_switch_is_off_by_default_and_opts_in():
    from myrtlespeech_amd.model.deep_speech_2 import DeepSpeech2
    from myrtlespeech_amd.model.fully_connected import FullyConnected
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    x, lens = torch.zeros(3, 2, 4), torch.tensor([3, 2])
    for kind in (RNNType.GRU, RNNType.BASIC_RNN):
        rnn = RNN(kind, 4, 8)
        assert rnn.gru_backward is False
        with pytest.raises(ValueError, match="LSTM"):          # a fresh module refuses exactly as before
            rnn((x, lens), differentiable=True)
        model = DeepSpeech2(None, rnn, None, FullyConnected(8, 5, 0, None, None))
        with pytest.raises(ValueError, match="LSTM"):
            model._train_plan()
        rnn.gru_backward = True
        assert model._train_plan() == ([], None)
        with pytest.raises(ValueError, match="sorted"):         # now gru_train's own vetting answers
            rnn((x, torch.tensor([2, 3])), differentiable=True)
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="HIP device"):
                rnn((x, lens), differentiable=True)
    lstm = RNN(RNNType.LSTM, 4, 8)
    lstm.gru_backward = True          # the switch does not touch LSTM stacks: rnn_train's vetting answers
    with pytest.raises(ValueError, match="hx"):
        lstm((x, lens), torch.zeros(1, 2, 8), differentiable=True)


def test_training_yardstick_and_learning_rate():
    """The yardstick of tests/test_gru_train_gpu.py: every parameter is reached, and under plain SGD at the learning rate that
    test uses the float64 loss falls at every step."""
    import gru_train_ref as M
    w, d = M.make()
    loss, grads = M.yardstick(w, d)
    assert np.isfinite(loss) and len(grads) == 11
    for key, g in grads.items():
        assert np.any(g), key
    losses = M.sgd_losses(w, d)
    print("float64 SGD losses:", [round(v, 6) for v in losses])
    assert len(losses) == M.STEPS + 1 and all(b < a for a, b in zip(losses, losses[1:]))
