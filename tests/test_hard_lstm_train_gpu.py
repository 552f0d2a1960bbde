"""Training ``HardLSTM`` on the device through the public interface: ``hard_lstm_train`` / ``HardLSTM.forward(differentiable=
True)`` on three stacks, ``DeepSpeech1(hard_lstm=True)`` and a DeepSpeech2 miniature holding a ``HardLSTM`` under the project's
``CTCLoss`` with ``hard_backward = True``, two ``fit()`` steps, and the refusals with the switch off.

Yardstick: torch float64 autograd on the CPU of the restated stack (``R.torch_cell_stack``: tests/rnn_ref64.py's hard cell with
``torch.clamp`` and ``torch.nn.Hardtanh``; tests/test_hard_lstm_backward_cpu.py pins it).  Criterion: that of the soft stacks
(tests/test_dropout_train_gpu.py, tests/test_ds1_train_gpu.py) -- every gradient within 1e-3 of its tensor's largest magnitude.
The hard cell's derivative jumps at its kinks, so the weights are scaled as the C-ABI cases' are and the seeds were chosen on
the CPU such that every layer keeps the kink margin of tests/test_hard_lstm_backward_cpu.py (>= 16 x the largest derived bound
on a recomputed value, ``R.stack_margin_ratio``); each test asserts that before it looks at the device.
"""
import numpy as np
import pytest
import torch

import ds1_train_ref as M
import hard_lstm_backward_ref as R
import lstm_backward_ref as L

pytestmark = pytest.mark.gpu

REL = 1e-3
MARGIN = 16.0

# name: (In, H, num_layers, bidirectional, batch_first, T, N, weight scale, seed)
STACKS = {
    "two_layers_bidirectional": (6, 8, 2, True, False, 6, 3, 3.0, 18),
    "one_layer_h40": (5, 40, 1, False, False, 5, 3, 5.0, 538),
    "batch_first_h4": (5, 4, 1, False, True, 6, 2, 5.0, 32),
}


def stack_case(name, with_hx):
    In, H, nl, bi, bf, T, N, scale, seed = STACKS[name]
    ndir = 2 if bi else 1
    w = R.scaled_stack(In, H, nl, bi, scale, seed)
    rng = np.random.default_rng(seed + 1000)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    d = dict(x=f(T, N, In), d_out=f(T, N, ndir * H), d_hn=f(nl * ndir, N, H), d_cn=f(nl * ndir, N, H),
             h0=rng.uniform(-1, 1, (nl * ndir, N, H)).astype(np.float32), c0=rng.uniform(-2, 2, (nl * ndir, N, H)).astype(np.float32))
    if not with_hx:
        d["h0"] = d["c0"] = None
    return w, d


def rel_report(name, got, want):
    errs = {key: L.rel_err(got[key], v) for key, v in want.items()}
    print(name, {k: f"{e:.2e}" for k, e in errs.items()})
    for key, e in errs.items():
        assert e <= REL, (name, key, e)


def twin_stack(w, d, nl, bi, dtype=torch.float64):
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in w.items()}
    t = lambda a: None if a is None else torch.tensor(a, dtype=dtype, requires_grad=True)      # noqa: E731
    x, h0, c0 = t(d["x"]), t(d["h0"]), t(d["c0"])
    out, hn, cn = R.torch_cell_stack(R.stack_layers(p, nl, bi), x, h0, c0, dtype)
    ((out * torch.tensor(d["d_out"], dtype=dtype)).sum() + (hn * torch.tensor(d["d_hn"], dtype=dtype)).sum()
     + (cn * torch.tensor(d["d_cn"], dtype=dtype)).sum()).backward()
    res = dict(out=out, h_n=hn, c_n=cn, dx=x.grad, **{k: q.grad for k, q in p.items()})
    if h0 is not None:
        res.update(d_h0=h0.grad, d_c0=c0.grad)
    return {k: v.detach().numpy().astype(np.float64) for k, v in res.items()}


def load(module, w, prefix=""):
    params = dict(module.named_parameters())
    with torch.no_grad():
        for key, v in w.items():
            params[prefix + key].copy_(torch.as_tensor(v))
    return params


@pytest.mark.parametrize("with_hx", (False, True), ids=("zeros", "hx"))
@pytest.mark.parametrize("name", tuple(STACKS))
def test_stack_gradients(name, with_hx):
    from myrtlespeech_amd.model.hard_lstm import HardLSTM
    In, H, nl, bi, bf, T, N, _, _ = STACKS[name]
    w, d = stack_case(name, with_hx)
    ratio = R.stack_margin_ratio(R.stack_layers(w, nl, bi), d["x"], d["h0"], d["c0"])
    print(name, "kink margin over the largest bound, worst layer:", ratio)
    assert ratio >= MARGIN
    want = twin_stack(w, d, nl, bi)
    rnn = HardLSTM(In, H, num_layers=nl, bidirectional=bi, batch_first=bf)
    params = load(rnn, w, "rnn.")
    assert len(params) == len(w)
    dev = lambda a: None if a is None else torch.tensor(a, device="cuda", requires_grad=True)      # noqa: E731
    xs, h, c = dev(d["x"]), dev(d["h0"]), dev(d["c0"])
    hx = None if h is None else (h, c)
    lens = torch.full((N,), T)
    inp = xs.transpose(0, 1) if bf else xs          # the module's own layout: batch-major where batch_first
    (out, out_lens), (hn, cn) = rnn((inp, lens), hx, differentiable=True)
    assert out_lens is lens and hn.shape == cn.shape == (nl * (2 if bi else 1), N, H)
    out_tm = out.transpose(0, 1) if bf else out
    assert out_tm.shape == (T, N, (2 if bi else 1) * H)
    ((out_tm * torch.tensor(d["d_out"], device="cuda")).sum() + (hn * torch.tensor(d["d_hn"], device="cuda")).sum()
     + (cn * torch.tensor(d["d_cn"], device="cuda")).sum()).backward()
    got = dict(out=out_tm, h_n=hn, c_n=cn, dx=xs.grad, **{k[len("rnn."):]: q.grad for k, q in params.items()})
    if hx is not None:
        got.update(d_h0=h.grad, d_c0=c.grad)
    assert all(v is not None for v in got.values()), [k for k, v in got.items() if v is None]
    assert sorted(got) == sorted(want)
    rel_report(f"{name} {'hx' if with_hx else 'zeros'}", {k: v.detach().cpu().numpy() for k, v in got.items()}, want)
    # the values are the default forward's, bit for bit
    with torch.no_grad():
        (o2, _), (hn2, cn2) = rnn((inp.detach(), lens), None if hx is None else (h.detach(), c.detach()))
    assert torch.equal(out.detach(), o2) and torch.equal(hn.detach(), hn2) and torch.equal(cn.detach(), cn2)


# ---- DeepSpeech1(hard_lstm=True) ----------------------------------------------------------------------------------------------
DS1_SCALE, DS1_SEED = 5.0, 65
HARD_PREFIX = "bi_lstm.rnn."


def ds1_weights():
    """tests/ds1_train_ref.py's Linear weights and batch, the soft LSTM's parameters replaced by a scaled hard cell's."""
    w, d = M.make()
    w = {k: v for k, v in w.items() if not k.startswith("bi_lstm.")}
    w.update({HARD_PREFIX + k: v for k, v in R.scaled_stack(2 * M.HID, M.HID, 1, True, DS1_SCALE, DS1_SEED).items()})
    return w, d


def ds1_twin(w, d, dtype=torch.float64):
    """(loss, gradients, the LSTM's input [T, N, 2 HID]) of the whole chain under torch autograd on the CPU.  HardLSTM ignores
    the lengths: every sequence runs its T steps, padding included, and only the loss knows the lengths."""
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in w.items()}
    x = torch.tensor(d["x"], dtype=dtype)
    n, c, f, t = x.shape
    h = x.reshape(n, c * f, t).permute(2, 0, 1)
    for name in ("fc1.0", "fc2.0", "fc3.0"):
        h = torch.nn.functional.hardtanh(torch.nn.functional.linear(h, p[f"{name}.weight"], p[f"{name}.bias"]), 0.0, M.CLIP)
    lstm_in = h
    hard = {k[len(HARD_PREFIX):]: q for k, q in p.items() if k.startswith(HARD_PREFIX)}
    h, _, _ = R.torch_cell_stack(R.stack_layers(hard, 1, True), h, None, None, dtype)
    h = torch.nn.functional.hardtanh(torch.nn.functional.linear(h, p["fc4.0.weight"], p["fc4.0.bias"]), 0.0, M.CLIP)
    logits = torch.nn.functional.linear(h, p["out.weight"], p["out.bias"])
    loss = torch.nn.functional.ctc_loss(torch.log_softmax(logits, -1), torch.as_tensor(d["targets"]), torch.as_tensor(d["lens"]),
                                        torch.as_tensor(d["target_lens"]), blank=0, reduction="mean")
    loss.backward()
    return float(loss.detach()), {k: q.grad.detach().numpy().astype(np.float64) for k, q in p.items()}, lstm_in.detach().numpy()


def build_ds1(w, switch=True):
    from myrtlespeech_amd.model.deep_speech_1 import DeepSpeech1
    model = DeepSpeech1(M.F_IN, 1, M.HID, M.V, 0.0, relu_clip=M.CLIP, hard_lstm=True)
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(w) and len(params) == 18
    load(model, w)
    model.bi_lstm.hard_backward = switch
    return model, params


def batch(d):
    return ((torch.tensor(d["x"], device="cuda"), torch.as_tensor(d["lens"])),
            (torch.as_tensor(d["targets"]), torch.as_tensor(d["target_lens"])))


def test_ds1_hard_ctc_loss_gradients_reach_all_18_parameters():
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    w, d = ds1_weights()
    want_loss, want, lstm_in = ds1_twin(w, d)
    hard = {k[len(HARD_PREFIX):]: v for k, v in w.items() if k.startswith(HARD_PREFIX)}
    ratio = R.stack_margin_ratio(R.stack_layers(hard, 1, True), lstm_in)
    print("DeepSpeech1 hard cell: kink margin over the largest bound", ratio)
    assert ratio >= MARGIN
    model, params = build_ds1(w)
    inputs, targets = batch(d)
    (before, _), _ = model(inputs)
    before = before.clone()
    (out, out_lens), hid = model(inputs, differentiable=True)
    assert out.shape == (M.T, M.N, M.V) and out_lens.tolist() == list(M.LENS)
    assert hid[0].shape == hid[1].shape == (2, M.N, M.HID)
    loss = CTCLoss()((out, out_lens), targets)
    loss.backward()
    print("loss", float(loss.detach()), "float64", want_loss)
    assert abs(float(loss.detach()) - want_loss) <= REL * abs(want_loss)
    assert all(q.grad is not None for q in params.values())
    rel_report("DeepSpeech1(hard_lstm=True) + CTCLoss", {k: q.grad.detach().cpu().numpy() for k, q in params.items()}, want)
    (after, _), _ = model(inputs)
    assert torch.equal(after, before)
    np.testing.assert_allclose(out.detach().cpu().numpy(), before.cpu().numpy(), rtol=1e-4, atol=1e-4)


def _fit_run(steps=2):
    from myrtlespeech_amd import optim
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    from myrtlespeech_amd.model.seq_to_seq import SeqToSeq
    from myrtlespeech_amd.run.train import fit
    w, d = ds1_weights()
    model, params = build_ds1(w, switch=False)
    model.bi_lstm.hard_backward = True              # the one line
    s = SeqToSeq(model, CTCLoss(), [])
    s.optim = optim.SGD(list(params.values()), lr=M.LR)
    start = {k: q.detach().clone() for k, q in params.items()}
    fit(s, 1, [batch(d)] * steps)
    return start, {k: q.detach().clone() for k, q in params.items()}


def test_fit_trains_the_hard_model_and_is_deterministic():
    start, a = _fit_run()
    _, b = _fit_run()
    for key in a:
        assert bool(torch.isfinite(a[key]).all()), key
        assert not torch.equal(a[key], start[key]), f"{key} did not change"
        assert torch.equal(a[key], b[key]), key


# ---- DeepSpeech2 holding a HardLSTM -------------------------------------------------------------------------------------------
DS2 = dict(n=3, c=1, f=5, t=7, hid=8, v=6, scale=5.0, seed=207)


def build_ds2(switch):
    from myrtlespeech_amd.model.deep_speech_2 import DeepSpeech2
    from myrtlespeech_amd.model.fully_connected import FullyConnected
    from myrtlespeech_amd.model.hard_lstm import HardLSTM
    k = DS2
    torch.manual_seed(9)
    fc = FullyConnected(k["hid"], k["v"], 1, 8, torch.nn.Hardtanh(0.0, 1.0))
    model = DeepSpeech2(None, HardLSTM(k["c"] * k["f"], k["hid"]), None, fc)
    with torch.no_grad():
        fc.fully_connected[0].weight.mul_(4.0)
    hard = R.scaled_stack(k["c"] * k["f"], k["hid"], 1, False, k["scale"], k["seed"])
    load(model, hard, "rnn.rnn.")
    model.rnn.hard_backward = switch
    return model, hard


def test_ds2_miniature_holding_a_hard_lstm():
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    k = DS2
    n, c, f, t = k["n"], k["c"], k["f"], k["t"]
    model, hard = build_ds2(True)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n, c, f, t)).astype(np.float32)
    lens = torch.as_tensor([7, 5, 2])
    targets, target_lens = torch.as_tensor(M.TARGETS), torch.as_tensor(M.TARGET_LENS)
    sd = {key: q.detach().cpu().numpy() for key, q in model.named_parameters()}
    x_tm = np.ascontiguousarray(x.reshape(n, c * f, t).transpose(2, 0, 1))
    ratio = R.stack_margin_ratio(R.stack_layers(hard, 1, False), x_tm)
    print("DeepSpeech2 miniature hard cell: kink margin over the largest bound", ratio)
    assert ratio >= MARGIN

    p = {key: torch.tensor(a, dtype=torch.float64, requires_grad=True) for key, a in sd.items()}
    h, _, _ = R.torch_cell_stack(R.stack_layers({key[len("rnn.rnn."):]: q for key, q in p.items() if key.startswith("rnn.rnn.")}, 1, False),
                                 torch.tensor(x_tm, dtype=torch.float64), None, None, torch.float64)
    fcs = sorted(key for key in p if key.startswith("fully_connected.") and key.endswith(".weight"))
    assert len(fcs) == 2
    h = torch.nn.functional.hardtanh(torch.nn.functional.linear(h, p[fcs[0]], p[fcs[0].replace("weight", "bias")]), 0.0, 1.0)
    y = torch.nn.functional.linear(h, p[fcs[1]], p[fcs[1].replace("weight", "bias")])
    want_loss = torch.nn.functional.ctc_loss(torch.log_softmax(y, -1), targets, lens, target_lens, blank=0, reduction="mean")
    want_loss.backward()
    want = {key: q.grad.detach().numpy().astype(np.float64) for key, q in p.items()}

    (out, out_lens), _ = model((torch.tensor(x, device="cuda"), lens), differentiable=True)
    loss = CTCLoss()((out, out_lens), (targets, target_lens))
    loss.backward()
    assert abs(float(loss.detach()) - float(want_loss.detach())) <= REL * abs(float(want_loss.detach()))
    got = {key: q.grad for key, q in model.named_parameters()}
    assert all(v is not None for v in got.values()) and sorted(got) == sorted(want)
    rel_report("DeepSpeech2 miniature with a HardLSTM", {key: v.detach().cpu().numpy() for key, v in got.items()}, want)


def test_both_models_refuse_with_the_switch_off():
    w, d = ds1_weights()
    model, _ = build_ds1(w, switch=False)
    with pytest.raises(ValueError, match="hard_lstm"):
        model(batch(d)[0], differentiable=True)
    ds2, _ = build_ds2(False)
    x = torch.zeros(DS2["n"], DS2["c"], DS2["f"], DS2["t"], device="cuda")
    with pytest.raises(ValueError, match="HardLSTM"):
        ds2((x, torch.as_tensor([7, 5, 2])), differentiable=True)
