"""What tests/conv_backward_cases.py promises, proved on the CPU: its float64 restatements agree with torch float64 autograd of
the reference's own op chain (mask, ``F.pad``, ``F.conv2d`` / grouped ``F.conv1d``, ``F.hardtanh``) to 1e-12 on every case, the
exact family stays under its caps, every clamp shows its three regimes, the library exports the new entry points, and
``DeepSpeech2.forward(differentiable=True)`` refuses what it does not serve before a device is needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_backward_cases as B
from myrtlespeech_amd import _lib

TOL = 1e-12
CASES = B.cases()
LCASES = B.lookahead_cases()


def close(got, ref, what):
    scale = max(1.0, float(np.abs(ref).max()))
    assert np.abs(got - ref).max() <= TOL * scale, (what, float(np.abs(got - ref).max()), scale)


def torch_conv(c, family):
    """(y, dx, dw, db) float64 from autograd of mask -> F.pad -> F.conv2d (F.conv1d for the one-row form) -> F.hardtanh."""
    x, w, b, _, dy = B.make(c, family)
    act = B.clamp_of(c, family)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True) if c.bias else None
    live = torch.arange(c.Tin)[None, :] < torch.tensor(B.eff_lens(c))[:, None]
    xm = xt * live[:, None, None, :].to(torch.float64)
    right_f = max(0, (c.Fout - 1) * c.SF + (c.KF - 1) * c.DF + 1 - c.pad_f - c.Fin)
    right_t = max(0, (c.Tout - 1) * c.ST + (c.KT - 1) * c.DT + 1 - c.pad_t - c.Tin)
    xp = F.pad(xm, (c.pad_t, right_t, c.pad_f, right_f))
    if c.Fin == 1 and c.KF == 1 and c.pad_f == 0:
        y = F.conv1d(xp[:, :, 0], wt[:, :, 0], bt, stride=c.ST, dilation=c.DT).unsqueeze(2)
    else:
        y = F.conv2d(xp, wt, bt, stride=(c.SF, c.ST), dilation=(c.DF, c.DT))
    y = y[:, :, :c.Fout, :c.Tout]
    assert y.shape[2:] == (c.Fout, c.Tout)
    if act is not None:
        y = F.hardtanh(y, act[0], act[1])
    (y * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    n = lambda t: None if t is None else t.grad.numpy()      # noqa: E731
    return y.detach().numpy(), n(xt), n(wt), n(bt)


@pytest.mark.parametrize("family", B.FAMILIES)
@pytest.mark.parametrize("c", CASES, ids=[c.tag for c in CASES])
def test_restatement_is_torch_float64_autograd(c, family):
    y, dx, dw, db = torch_conv(c, family)
    _, _, _, y32, _ = B.make(c, family)
    assert np.array_equal(y.astype(np.float32), y32)
    rdx, rdw, rdb = B.want(c, family)
    close(rdx, dx, (c.tag, "dx"))
    close(rdw, dw, (c.tag, "dw"))
    if c.bias:
        close(rdb, db, (c.tag, "db"))
    # masked frames carry no gradient, and it is +0
    for n, ln in enumerate(B.eff_lens(c)):
        assert not np.any(rdx[n, :, :, ln:]) and not np.signbit(rdx[n, :, :, ln:]).any()


@pytest.mark.parametrize("c", CASES, ids=[c.tag for c in CASES])
def test_caps_and_regimes(c):
    sdx, sdw, sdb = B.scales(c, "dense")
    assert sdx.max() < B.CAP and sdw.max() < B.CAP and sdb.max() < B.CAP
    assert c.lens is None or (c.N == 1 or (1 in c.lens and c.Tin in c.lens))
    if c.act:
        for family in B.FAMILIES:
            y = B.make(c, family)[3]
            lo, hi = B.CLAMP[family]
            assert (y == lo).any() and (y == hi).any() and ((y > lo) & (y < hi)).any(), (c.tag, family)


def test_the_case_list_covers_what_it_names():
    by = {c.tag: c for c in CASES}
    d = by["d_s3_d2_nopad"]
    unread = B.unread_positions(d)
    assert unread.any() and not unread.all()
    dx = B.want(d, "gauss")[0]
    assert not np.any(dx[:, :, unread]) and np.any(dx[0][:, ~unread])
    assert by["a_lens_null"].lens is None and not by["f_bias_null"].bias
    ks = sorted(c.N * c.Fout * c.Tout for c in CASES if c.tag.startswith("g_k"))
    assert ks == [B.SLICE - 1, B.SLICE, B.SLICE + 1, 2 * B.SLICE - 1, 2 * B.SLICE, 2 * B.SLICE + 1]
    assert [B.slices(c) for c in CASES if c.tag.startswith("g_k")] == [1, 1, 2, 2, 2, 3]
    with open(_lib.HEADER_PATH.replace("include/ms_hotpath.h", "myrtlespeech_amd/csrc/conv_backward.hip")) as f:
        assert f"constexpr int CBW_SLICE = {B.SLICE};" in f.read()
    # readers / window: the two predicates are each other's transpose
    c = by["a_cin3_cout5"]
    mx, mw = B.dy_window(c, 0, 1, 2)
    for (n, ci, fi, ti) in np.argwhere(mx)[:6]:
        fo_to = [(fo, to) for fo in range(c.Fout) for to in range(c.Tout)]
        assert B.x_readers(c, n, ci, fi, ti)[0, ci].any()
        assert any(B.dy_window(c, n, fo, to)[0][n, ci, fi, ti] for fo, to in fo_to)
    assert mw.shape == (c.Cin, c.KF, c.KT) and mw.any()


@pytest.mark.parametrize("family", B.FAMILIES)
@pytest.mark.parametrize("c", LCASES, ids=[c.tag for c in LCASES])
def test_lookahead_restatement_is_torch_float64_autograd(c, family):
    x, w, y32, dy = B.lookahead_make(c, family)
    act = B.LCLAMP[family] if c.act else None
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(F.pad(xt, (0, c.ctx - 1)), wt[:, None, :], groups=c.F)
    if act is not None:
        y = F.hardtanh(y, act[0], act[1])
    (y * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    assert np.array_equal(y.detach().numpy().astype(np.float32), y32)
    (rdx, rdw), (sdx, sdw) = B.lookahead_want(c, family)
    close(rdx, xt.grad.numpy(), (c.tag, "dx"))
    close(rdw, wt.grad.numpy(), (c.tag, "dw"))
    if family == "dense":
        assert sdx.max() < B.CAP and sdw.max() < B.CAP
    if c.act and c.T > 1:
        lo, hi = act
        assert (y32 == lo).any() and (y32 == hi).any() and ((y32 > lo) & (y32 < hi)).any()


def test_library_exports_the_backward_entry_points():
    lib = _lib.load()
    for name in ("ms_maskconv_backward_workspace_bytes", "ms_maskconv_backward_data", "ms_maskconv_backward_weight",
                 "ms_lookahead_backward"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in _lib.header_symbols()
    # pure host arithmetic: slices x Cout x (Cin KF KT + 1) floats
    up = lambda v: -(-v // 256) * 256      # noqa: E731
    assert lib.ms_maskconv_backward_workspace_bytes(1, 2, 3, 1, B.SLICE + 1, 1, 3) == up(2 * 3 * 7 * 4)
    assert lib.ms_maskconv_backward_workspace_bytes(32, 32, 32, 41, 501, 21, 11) == up(81 * 32 * (32 * 231 + 1) * 4)
    assert lib.ms_maskconv_backward_workspace_bytes(0, 1, 1, 1, 1, 1, 1) == 0


def _ds2(cnn=None, rnn=None, lookahead=None, fc=None):
    from myrtlespeech_amd.model.cnn import MaskConv2d, PaddingMode
    from myrtlespeech_amd.model.deep_speech_2 import DeepSpeech2
    from myrtlespeech_amd.model.fully_connected import FullyConnected
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.seq_len_wrapper import SeqLenWrapper
    act = lambda: SeqLenWrapper(torch.nn.Hardtanh(0.0, 1.0), torch.nn.Identity())      # noqa: E731
    cnn = cnn or torch.nn.Sequential(MaskConv2d(1, 4, [5, 3], [2, 2], PaddingMode.SAME), act())
    rnn = rnn or RNN(RNNType.LSTM, 4 * 5, 8)
    fc = fc or FullyConnected(8, 6, 0, None, None)
    return DeepSpeech2(cnn, rnn, lookahead, fc)


def test_deep_speech_2_differentiable_refuses_before_a_device_is_needed():
    from myrtlespeech_amd.model.cnn import MaskConv2d, PaddingMode
    from myrtlespeech_amd.model.fully_connected import FullyConnected
    from myrtlespeech_amd.model.hard_lstm import HardLSTM
    from myrtlespeech_amd.model.lookahead import Lookahead
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.seq_len_wrapper import SeqLenWrapper
    x = (torch.zeros(2, 1, 9, 14), torch.tensor([14, 9]))
    wrap = lambda m: SeqLenWrapper(m, torch.nn.Identity())      # noqa: E731
    bad = {
        "gru": _ds2(rnn=RNN(RNNType.GRU, 20, 8)),
        "tanh": _ds2(rnn=RNN(RNNType.BASIC_RNN, 20, 8)),
        "hard_lstm": _ds2(rnn=HardLSTM(20, 8)),
        "rnn_dropout": _ds2(rnn=RNN(RNNType.LSTM, 20, 8, num_layers=2, dropout=0.5)).train(),
        "fc_dropout": _ds2(fc=FullyConnected(8, 6, 1, 8, torch.nn.Hardtanh(0.0, 1.0), dropout=0.5)).train(),
        "groups": _ds2(cnn=torch.nn.Sequential(MaskConv2d(2, 4, [5, 3], [2, 2], PaddingMode.SAME, groups=2))),
        "foreign_cnn": _ds2(cnn=torch.nn.Sequential(MaskConv2d(1, 4, [5, 3], [2, 2], PaddingMode.SAME), wrap(torch.nn.Tanh()))),
        "foreign_lookahead": _ds2(lookahead=torch.nn.Sequential(Lookahead(8, 3), wrap(torch.nn.Tanh()))),
        "bare_lookahead_module": _ds2(lookahead=torch.nn.Conv1d(8, 8, 3)),
    }
    for name, model in bad.items():
        with pytest.raises(ValueError):
            model(x, differentiable=True)
        assert all(p.grad is None for p in model.parameters()), name
    from myrtlespeech_amd.model.conv_autograd import maskconv_train
    from myrtlespeech_amd.model.rnn_autograd import linear_stack_train
    with pytest.raises(ValueError):
        maskconv_train(MaskConv2d(2, 4, 3, groups=2), x)
    with pytest.raises(ValueError):
        linear_stack_train(torch.zeros(3, 8), torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Dropout(0.5)), training=True)
    # what IS served passes the vetting: on a machine without a device the chain then stops at the device check
    ok = _ds2(lookahead=torch.nn.Sequential(Lookahead(8, 3), wrap(torch.nn.Hardtanh(0.0, 1.0))))
    front, la = ok._train_plan()
    assert len(front) == 1 and front[0][1] == (0.0, 1.0) and la[1] == (0.0, 1.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            ok(x, differentiable=True)
