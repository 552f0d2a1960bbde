"""The dropout specification pinned on the CPU: the Philox known answers, the threshold and the scale, the statistics of the
numpy restatement (tests/dropout_ref.py) at fixed seeds, the generator's bookkeeping, and the opt-in: with no generator attached
every differentiable entry refuses dropout exactly as before; with one, the same calls pass the vetting and stop at the missing
device."""
import numpy as np
import pytest
import torch

import dropout_ref as R

from myrtlespeech_amd import _lib

KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)
SEED, N, P = 0x1234567890abcdef, 65536, 0.25


def test_philox_known_answers():
    for counter, key, want in KAT:
        assert tuple(int(v) for v in R.philox(np.array(counter), np.array(key))) == want
    # vectorised over a leading axis, and the element layout: element e is word e & 3 of counter (e >> 2, 0, offset_lo, offset_hi)
    got = R.philox(np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT]))
    assert [tuple(int(v) for v in row) for row in got] == [k[2] for k in KAT]
    assert [int(v) for v in R.words(4, 0, 0)] == list(KAT[0][2])
    off = (0x03707344 << 32) | 0x13198a2e
    seed = (0x299f31d0 << 32) | 0xa4093822
    w = R.words(4 * 5 + 3, seed, off)
    assert [int(v) for v in w[20:]] == [int(v) for v in R.philox(np.array([5, 0, 0x13198a2e, 0x03707344]), np.array(KAT[2][1]))[:3]]


@pytest.mark.parametrize("p, thr, scale", [
    (0.25, 1 << 30, 4.0 / 3.0), (0.5, 1 << 31, 2.0), (2.0 ** -32, 1, 1.0), (1.0 - 2.0 ** -24, (1 << 32) - 256, 2.0 ** 24),
    (1.0, 1 << 32, 0.0)])
def test_threshold_and_scale(p, thr, scale):
    from myrtlespeech_amd.model import dropout as D
    assert D.threshold(p) == R.threshold(p) == thr
    assert D.scale_of(p) == float(R.scale(p)) == float(np.float32(scale))
    assert isinstance(D.threshold(p), int)


def test_threshold_rounds_up_and_refuses_p_outside_the_range():
    from myrtlespeech_amd.model import dropout as D
    assert D.threshold(0.1) == 429496730          # 0.1 as a double is just above 1/10: ceil(429496729.6...)
    assert D.threshold(2.0 ** -40) == 1           # never 0: p > 0 drops the word 0
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="probability"):
            D.threshold(bad)
        with pytest.raises(ValueError, match="probability"):
            D.scale_of(bad)


def test_drop_rate_and_independence_of_two_offsets():
    sigma = np.sqrt(P * (1 - P) / N)
    assert abs(sigma - 0.00169) < 1e-5
    a, b = R.mask(N, P, SEED, 3), R.mask(N, P, SEED, 4)
    rate = 1.0 - a.mean()
    print("drop rate", rate, "sigma", sigma)
    assert abs(rate - 0.24881) < 5e-6 and abs(rate - P) <= 4 * sigma
    q = P * P + (1 - P) * (1 - P)
    agree = float((a == b).mean())
    print("offsets 3 and 4 agree on", agree, "independent masks would on", q)
    assert abs(agree - q) <= 4 * np.sqrt(q * (1 - q) / N)
    assert not np.array_equal(a, R.mask(N, P, SEED + 1, 3))
    # the multiplier and the one multiply: NaN and Inf survive a drop, a negative value dropped is -0
    m = R.multiplier(8, 0.5, 1, 2)
    assert set(m.tolist()) <= {0.0, 2.0}
    x = np.array([np.nan, np.inf, -np.inf, -1.5, 1.5, 0.0, -0.0, 3.0], dtype=np.float32)
    y = R.forward(x, 1.0, 0, 0)
    assert np.isnan(y[:3]).all() and np.signbit(y[3]) and y[3] == 0 and not np.signbit(y[4])


def test_generator_bookkeeping():
    from myrtlespeech_amd.model import dropout as D
    g = D.DropoutGenerator(7)
    assert g.state_dict() == {"seed": 7, "offset": 0}
    assert [g.next_offset(), g.next_offset()] == [0, 1] and g.offset == 2
    call = D.dropout_call(0.25, g)
    assert call == (1 << 30, float(np.float32(4.0 / 3.0)), 7, 2) and g.offset == 3
    state = g.state_dict()
    h = D.DropoutGenerator()
    assert h.state_dict() == {"seed": 0, "offset": 0}
    h.load_state_dict(state)
    assert h.state_dict() == state == {"seed": 7, "offset": 3} and h.next_offset() == 3
    g.manual_seed(SEED)
    assert g.state_dict() == {"seed": SEED, "offset": 0}
    assert D.DropoutGenerator(-1).seed == 2 ** 64 - 1
    with pytest.raises(ValueError, match="DropoutGenerator"):
        D.dropout_call(0.25, None)
    with pytest.raises(ValueError, match="probability"):
        D.dropout_call(0.0, g)
    assert g.offset == 0                                   # a refused call consumes none


def test_offsets_advance_per_application_and_not_in_eval_or_with_p_zero():
    from myrtlespeech_amd.model import dropout as D
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.rnn_autograd import _dropout_steps, _stack_dropout
    g = D.DropoutGenerator(5)
    rnn = RNN(RNNType.LSTM, 4, 8, num_layers=3, dropout=0.5, bidirectional=True).train()
    calls = _stack_dropout(rnn, g, "test")
    assert [c[3] for c in calls] == [0, 1] and all(c[:3] == (1 << 31, 2.0, 5) for c in calls) and g.offset == 2
    assert _stack_dropout(rnn.eval(), g, "test") is None and g.offset == 2
    assert _stack_dropout(RNN(RNNType.GRU, 4, 8, num_layers=3).train(), g, "test") is None and g.offset == 2
    assert _stack_dropout(RNN(RNNType.GRU, 4, 8, num_layers=1, dropout=0.0).train(), g, "test") is None and g.offset == 2
    rnn.train().dropout_generator = g                      # the attached one serves where none is passed
    assert [c[3] for c in _stack_dropout(rnn, None, "test")] == [2, 3]
    other = D.DropoutGenerator(6)                          # ... and an explicit one wins
    assert [c[2:] for c in _stack_dropout(rnn, other, "test")] == [(6, 0), (6, 1)] and g.offset == 4
    # a chain: Dropout(0) takes no step, a Dropout joins the layer in front of it, one without a layer stands alone
    lin = [torch.nn.Linear(3, 3) for _ in range(3)]
    chain = [torch.nn.Dropout(0.1), lin[0], torch.nn.Hardtanh(0.0, 1.0), torch.nn.Dropout(0.25), lin[1], torch.nn.Dropout(0.0),
             lin[2], torch.nn.Dropout(0.5)]
    assert _dropout_steps(chain) == [[None, None, 0.1], [lin[0], (0.0, 1.0), 0.25], [lin[1], None, None], [lin[2], None, 0.5]]
    with pytest.raises(NotImplementedError):
        _dropout_steps([lin[0], torch.nn.Dropout(0.5), torch.nn.Hardtanh(0.0, 1.0)])


def _ds2(**kw):
    from test_conv_backward_cpu import _ds2 as make
    return make(**kw)


def test_attach_reaches_every_class_and_leaves_state_dicts_alone():
    from myrtlespeech_amd.model import dropout as D
    from myrtlespeech_amd.model.deep_speech_1 import DeepSpeech1
    from myrtlespeech_amd.model.deep_speech_2 import DeepSpeech2
    from myrtlespeech_amd.model.fully_connected import FullyConnected
    from myrtlespeech_amd.model.rnn import RNN
    for cls in (DeepSpeech1, DeepSpeech2, RNN, FullyConnected):
        assert cls.dropout_generator is None
    g = D.DropoutGenerator(3)
    ds1 = DeepSpeech1(5, 1, 8, 6, 0.25)
    keys = sorted(ds1.state_dict())
    assert D.attach(ds1, g) is ds1 and ds1.dropout_generator is g and ds1.bi_lstm.dropout_generator is g
    assert sorted(ds1.state_dict()) == keys and not any(m is g for m in ds1.modules())
    ds2 = torch.nn.Sequential(_ds2())                      # found under a wrapper, as under SeqToSeq.model
    D.attach(ds2, g)
    assert ds2[0].dropout_generator is g and ds2[0].rnn.dropout_generator is g and ds2[0].fully_connected.dropout_generator is g
    D.attach(ds2, None)
    assert ds2[0].dropout_generator is None and ds2[0].rnn.dropout_generator is None
    with pytest.raises(ValueError, match="DropoutGenerator"):
        D.attach(ds1, torch.Generator())


def _refusals():
    """name -> (call taking a generator-or-None, the pinned message fragment): every refusal of dropout that earlier tests pin."""
    from myrtlespeech_amd.model import dropout as D
    from myrtlespeech_amd.model.deep_speech_1 import DeepSpeech1
    from myrtlespeech_amd.model.fully_connected import FullyConnected
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.rnn_autograd import gru_train, linear_stack_train, lstm_train, rnn_train
    x, lens = torch.zeros(3, 2, 4), torch.tensor([3, 2])
    stack = lambda kind, **kw: RNN(kind, 4, 8, num_layers=2, dropout=0.1, **kw).train()      # noqa: E731
    ds2_x = (torch.zeros(2, 1, 9, 14), torch.tensor([14, 9]))

    def attached(module, gen):
        return D.attach(module, gen) if gen is not None else module

    def ds1(gen):
        return attached(DeepSpeech1(5, 1, 8, 6, 0.25).train(), gen)((torch.zeros(2, 1, 5, 4), torch.tensor([4, 3])), differentiable=True)

    def ds2_rnn(gen):
        return attached(_ds2(rnn=RNN(RNNType.LSTM, 20, 8, num_layers=2, dropout=0.5)).train(), gen)(ds2_x, differentiable=True)

    def ds2_fc(gen):
        fc = FullyConnected(8, 6, 1, 8, torch.nn.Hardtanh(0.0, 1.0), dropout=0.5)
        return attached(_ds2(fc=fc).train(), gen)(ds2_x, differentiable=True)

    def chain(gen):
        return linear_stack_train(torch.zeros(3, 8), torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Dropout(0.5)), True, gen)

    inter = " does not serve inter-layer dropout"
    return {
        "rnn_train": (lambda gen: rnn_train(stack(RNNType.LSTM, bidirectional=True), x, lens, generator=gen), "rnn_train" + inter),
        "lstm_train": (lambda gen: lstm_train(stack(RNNType.LSTM), x, lens, generator=gen), "lstm_train" + inter),
        "gru_train": (lambda gen: gru_train(stack(RNNType.GRU), x, lens, generator=gen), "gru_train" + inter),
        "tanh_train": (lambda gen: gru_train(stack(RNNType.BASIC_RNN, bidirectional=True), x, lens, generator=gen), "gru_train" + inter),
        "rnn_forward": (lambda gen: attached(stack(RNNType.LSTM), gen)((x, lens), differentiable=True), "rnn_train" + inter),
        "ds1": (ds1, "does not serve dropout masks: train in .eval\\(\\) or with drop_prob = 0"),
        "ds2_rnn": (ds2_rnn, "does not serve inter-layer dropout in training mode"),
        "ds2_fc": (ds2_fc, "does not serve dropout masks: train in .eval\\(\\) or with dropout = 0"),
        "linear_stack": (chain, "linear_stack_train does not serve dropout masks: train in .eval\\(\\) or with dropout = 0"),
    }


@pytest.mark.parametrize("name", ["rnn_train", "lstm_train", "gru_train", "tanh_train", "rnn_forward", "ds1", "ds2_rnn", "ds2_fc",
                                  "linear_stack"])
def test_no_generator_refuses_as_before_and_one_gets_past_the_vetting(name):
    from myrtlespeech_amd.model import dropout as D
    call, message = _refusals()[name]
    with pytest.raises(ValueError, match=message):
        call(None)
    if not torch.cuda.is_available():
        g = D.DropoutGenerator(1)
        with pytest.raises(RuntimeError, match="HIP device"):
            call(g)
        assert g.offset == 0                               # a call that cannot run consumes no offset


def test_the_other_refusals_do_not_move_when_a_generator_is_attached():
    from myrtlespeech_amd.model import dropout as D
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.rnn_autograd import gru_train, lstm_train, rnn_train
    g = D.DropoutGenerator(1)
    x, lens = torch.zeros(3, 2, 4), torch.tensor([3, 2])
    with pytest.raises(ValueError, match="LSTM"):
        rnn_train(RNN(RNNType.GRU, 4, 8, num_layers=2, dropout=0.1).train(), x, lens, generator=g)
    with pytest.raises(ValueError, match="bidirectional"):
        lstm_train(RNN(RNNType.LSTM, 4, 8, num_layers=2, dropout=0.1, bidirectional=True).train(), x, lens, generator=g)
    with pytest.raises(ValueError, match="rnn_train"):
        gru_train(RNN(RNNType.LSTM, 4, 8, num_layers=2, dropout=0.1).train(), x, lens, generator=g)
    with pytest.raises(ValueError, match="sorted"):
        rnn_train(RNN(RNNType.LSTM, 4, 8, num_layers=2, dropout=0.1).train(), x, torch.tensor([2, 3]), generator=g)
    with pytest.raises(ValueError, match="probability"):
        D.dropout_train(torch.zeros(4), 0.0, g)
    with pytest.raises(ValueError, match="DropoutGenerator"):
        D.dropout_train(torch.zeros(4), 0.5, None)
    assert g.offset == 0


def test_new_symbols_are_declared_bound_and_exported(lib):
    for name in ("ms_dropout_forward", "ms_clamp_dropout_backward"):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    import ctypes
    assert _lib.SIGNATURES["ms_dropout_forward"][1][2:7] == [ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_uint64,
                                                             ctypes.c_uint64]
    # the argument checks need no device: nothing is launched
    z = ctypes.c_void_p(0)
    assert lib.ms_dropout_forward(z, z, 0, 1 << 30, 1.0, 0, 0, z) == 0             # n == 0: MS_OK, pointers not looked at
    assert lib.ms_dropout_forward(z, z, 4, 1 << 30, 1.0, 0, 0, z) == 1             # NULL with n > 0
    assert lib.ms_clamp_dropout_backward(z, z, z, 4, 0.0, 1.0, 1 << 30, 1.0, 0, 0, z) == 1
    assert lib.ms_dropout_forward(z, z, 0, 0, 1.0, 0, 0, z) == 1                   # thr == 0
    assert lib.ms_dropout_forward(z, z, 0, (1 << 32) + 1, 1.0, 0, 0, z) == 1       # thr > 2^32
    assert lib.ms_dropout_forward(z, z, 0, 1 << 32, 0.0, 0, 0, z) == 0             # thr == 2^32 is p == 1
    for bad in (-1.0, float("inf"), float("nan")):
        assert lib.ms_dropout_forward(z, z, 0, 1 << 30, bad, 0, 0, z) == 1
        assert lib.ms_clamp_dropout_backward(z, z, z, 0, 0.0, 1.0, 1 << 30, bad, 0, 0, z) == 1
    assert lib.ms_dropout_forward(z, z, -1, 1 << 30, 1.0, 0, 0, z) == 1
