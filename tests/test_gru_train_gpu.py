"""Training GRU and tanh stacks on the device through the public interface: ``rnn_autograd.gru_train``,
``RNN.forward(differentiable=True)`` with ``gru_backward = True``, and the shipped DeepSpeech2 architecture in miniature
(tests/gru_train_ref.py: the cnn of tests/ds2_train_ref.py, GRU 12 -> 8 unidirectional, ``Lookahead``, the output layer) under
the project's ``CTCLoss``, five SGD steps.  The yardstick is torch float64 autograd on the CPU (``torch.nn.GRU`` /
``torch.nn.RNN`` with ``pack_padded_sequence``; tests/test_gru_backward_cpu.py checks what is taken from it).

Criterion: that of tests/test_ds1_train_gpu.py, for the reason given there.  The kernels' own bounds are checked through the C
ABI (tests/test_gru_backward_gpu.py); here the backward consumes the FORWARD's outputs, which the project holds to 1e-4, and a
gradient term is a product of fewer than ten such values, so the loss and every gradient are held to 1e-3 of the tensor's
largest magnitude.  Each test prints the device's error as a multiple of the error of torch's float32 CPU autograd on the same
case (both against float64, an error of torch's below 2^-24 counts as 2^-24); the cap is four times the worst measured multiple,
recorded below as MEASURED_*.
"""
import numpy as np
import pytest
import torch

import gru_backward_ref as G
import gru_train_ref as M

pytestmark = pytest.mark.gpu

REL = 1e-3
FWD = 1e-4
# worst multiple of torch's float32 CPU error, measured on one MI355X (recorded in profiles/gru_backward_time.json)
MEASURED_STACK = 5.92       # over the four GRU stacks (3.45: gru_l1_h40's bias_hh_l0) and the tanh stack (bias_ih_l0, error 2.3e-6)
MEASURED_MODEL = 3.96       # the miniature DeepSpeech2 under CTCLoss: cnn.0.bias (error 3.7e-7)
T, N, IN = 6, 3, 5
LENS = (6, 4, 1)
# name: cell, layers, bidirectional, H (40: two workgroups of hidden units and a 120-wide K; 7: below a tile, unaligned rows)
STACKS = {"gru_l1_h40": ("gru", 1, False, 40), "gru_l2_h7": ("gru", 2, False, 7), "bigru_l1_h7": ("gru", 1, True, 7),
          "bigru_l2_h7": ("gru", 2, True, 7), "bitanh_l2_h7": ("tanh", 2, True, 7)}


def report(name, got, want, f32, measured):
    """name -> worst multiple of torch's float32 error; asserts the criterion."""
    out = {}
    for key, w in want.items():
        err = G.rel_err(got[key], w)
        base = max(G.rel_err(f32[key], w), 2.0 ** -24)
        out[key] = (err, err / base)
    print(name, {k: (f"{e:.2e}", round(m, 2)) for k, (e, m) in out.items()})
    worst = max(m for _, m in out.values())
    print(name, "worst multiple of torch's float32 error:", round(worst, 3))
    for key, (err, _) in out.items():
        assert err <= REL, (name, key, err)
    if measured is not None:
        assert worst <= 4.0 * measured, (name, worst)
    return worst


def make_stack(name):
    """(layers as torch_stack takes them, x, h0, d_out, d_hn) for STACKS[name], the cases' input scale."""
    cell, nl, bidir, H = STACKS[name]
    ndir = 2 if bidir else 1
    rng = np.random.default_rng(sum(map(ord, name)))
    f32 = lambda a: a.astype(np.float32)       # noqa: E731
    layers = []
    for i in range(nl):
        ps = tuple(G._params(rng, IN if i == 0 else ndir * H, H, True) for _ in range(ndir))
        if cell == "tanh":      # one gate block
            ps = tuple({key: v[:H] for key, v in p.items()} for p in ps)
        layers.append(ps)
    return (layers, f32(rng.standard_normal((T, N, IN))), f32(rng.standard_normal((nl * ndir, N, H)) * 0.5),
            f32(rng.standard_normal((T, N, ndir * H))), f32(rng.standard_normal((nl * ndir, N, H))))


def flat(res):
    """``torch_stack``'s result as one dict keyed like the module's parameters, plus x and hx."""
    out = dict(x=res["dx"], hx=res["d_h0"])
    for i, layer in enumerate(res["layers"]):
        for key, tname in (("d_w_ih", "weight_ih"), ("d_w_hh", "weight_hh"), ("d_b_ih", "bias_ih"), ("d_b_hh", "bias_hh")):
            for d, sfx in enumerate(("", "_reverse")[:layer[key].shape[0]]):
                out[f"{tname}_l{i}{sfx}"] = layer[key][d]
    return out


def build_rnn(name, layers, **kw):
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    cell, nl, bidir, H = STACKS[name]
    rnn = RNN(RNNType.GRU if cell == "gru" else RNNType.BASIC_RNN, IN, H, num_layers=nl, bidirectional=bidir, **kw).eval()
    with torch.no_grad():
        for i, ps in enumerate(layers):
            for d, sfx in enumerate(("", "_reverse")[:len(ps)]):
                for key, tname in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh")):
                    getattr(rnn.rnn, f"{tname}_l{i}{sfx}").copy_(torch.as_tensor(ps[d][key]))
    return rnn


def device_grads(rnn, x, hx, d_out, d_hn, lens=LENS, poison=False):
    """out, h_n and every gradient of ``gru_train`` under sum(out d_out) + sum(h_n d_hn).  ``poison``: NaN in the rows of x past
    the lengths."""
    from myrtlespeech_amd.model.rnn_autograd import gru_train
    x = x.copy()
    if poison:
        for n, ln in enumerate(lens):
            x[ln:, n] = np.nan
    xd = torch.tensor(x, device="cuda", requires_grad=True)
    hd = torch.tensor(hx, device="cuda", requires_grad=True)
    for p in rnn.parameters():
        p.grad = None
    out, h_n = gru_train(rnn, xd, torch.tensor(lens), hd)
    assert isinstance(h_n, torch.Tensor)
    ((out * torch.tensor(d_out, device="cuda")).sum() + (h_n * torch.tensor(d_hn, device="cuda")).sum()).backward()
    grads = dict(x=xd.grad, hx=hd.grad, **{k: p.grad for k, p in rnn.rnn.named_parameters()})
    assert all(g is not None for g in grads.values())
    return out.detach().cpu().numpy(), h_n.detach().cpu().numpy(), {k: g.cpu().numpy() for k, g in grads.items()}


@pytest.mark.parametrize("name", tuple(STACKS))
def test_stack_gradients(name):
    layers, x, hx, d_out, d_hn = make_stack(name)
    cell, nl, bidir, H = STACKS[name]
    lens = np.array(LENS)
    want = G.torch_stack(layers, x, hx, lens, d_out, d_hn, bidirectional=bidir, tanh=cell == "tanh")
    t32 = G.torch_stack(layers, x, hx, lens, d_out, d_hn, bidirectional=bidir, tanh=cell == "tanh", dtype=np.float32)
    rnn = build_rnn(name, layers)
    assert rnn.gru_backward is False          # gru_train is the explicit entry: it needs no switch
    call = lambda: rnn((torch.tensor(x, device="cuda"), torch.tensor(LENS)), torch.tensor(hx, device="cuda"))      # noqa: E731
    (before, _), hid_before = call()
    before, hid_before = before.clone(), hid_before.clone()
    out, h_n, grads = device_grads(rnn, x, hx, d_out, d_hn)
    # the node's values are RNN.forward's and the yardstick's within the forward's tolerance; rows past a length are 0
    np.testing.assert_allclose(out, before.cpu().numpy(), rtol=FWD, atol=FWD)
    np.testing.assert_allclose(h_n, hid_before.cpu().numpy(), rtol=FWD, atol=FWD)
    np.testing.assert_allclose(out, want["out"], rtol=FWD, atol=FWD)
    np.testing.assert_allclose(h_n, want["h_n"], rtol=FWD, atol=FWD)
    live = (np.arange(T)[:, None] < lens[None, :])[..., None]
    assert not np.any(np.where(live, 0, out))
    # the default path gives the same bits after the call as before it
    (after, _), hid_after = call()
    assert torch.equal(after, before) and torch.equal(hid_after, hid_before)
    wf, tf = flat(want), flat(t32)
    assert sorted(wf) == sorted(grads)
    report(name, grads, wf, tf, MEASURED_STACK)
    # NaN in layer 0's input rows past the lengths changes no bit of any gradient
    _, _, poisoned = device_grads(rnn, x, hx, d_out, d_hn, poison=True)
    for key, g in grads.items():
        assert g.tobytes() == poisoned[key].tobytes(), (name, key)


def test_batch_first_with_the_switch_on():
    """``RNN(GRU, batch_first=True)`` under ``differentiable=True``: refused as before until ``gru_backward`` is set, then the
    time-major node between two transposes autograd sees."""
    name = "gru_l1_h40"
    layers, x, hx, d_out, d_hn = make_stack(name)
    want = flat(G.torch_stack(layers, x, hx, np.array(LENS), d_out, d_hn, bidirectional=False))
    rnn = build_rnn(name, layers, batch_first=True)
    xd = torch.tensor(x.transpose(1, 0, 2).copy(), device="cuda", requires_grad=True)
    hd = torch.tensor(hx, device="cuda", requires_grad=True)
    with pytest.raises(ValueError, match="LSTM"):
        rnn((xd, torch.tensor(LENS)), hd, differentiable=True)
    rnn.gru_backward = True
    (out, lens), hid = rnn((xd, torch.tensor(LENS)), hd, differentiable=True)
    assert out.shape == (N, T, 40) and isinstance(hid, torch.Tensor) and hid.shape == (1, N, 40) and lens.tolist() == list(LENS)
    with torch.no_grad():
        (ref, _), hid_ref = rnn((xd.detach(), torch.tensor(LENS)), hd.detach())
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.cpu().numpy(), rtol=FWD, atol=FWD)
    np.testing.assert_allclose(hid.detach().cpu().numpy(), hid_ref.cpu().numpy(), rtol=FWD, atol=FWD)
    ((out * torch.tensor(d_out.transpose(1, 0, 2).copy(), device="cuda")).sum() + (hid * torch.tensor(d_hn, device="cuda")).sum()).backward()
    got = dict(x=xd.grad.cpu().numpy().transpose(1, 0, 2), hx=hd.grad.cpu().numpy(),
               **{k: p.grad.cpu().numpy() for k, p in rnn.rnn.named_parameters()})
    for key, w in want.items():
        assert G.rel_err(got[key], w) <= REL, key


def build_model(w, switch=True):
    from myrtlespeech_amd.model.cnn import MaskConv2d, PaddingMode
    from myrtlespeech_amd.model.deep_speech_2 import DeepSpeech2
    from myrtlespeech_amd.model.fully_connected import FullyConnected
    from myrtlespeech_amd.model.lookahead import Lookahead
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.seq_len_wrapper import SeqLenWrapper
    D = M.M
    act = lambda: SeqLenWrapper(torch.nn.Hardtanh(0.0, D.CLIP), torch.nn.Identity())      # noqa: E731
    cnn = torch.nn.Sequential(MaskConv2d(1, 4, [5, 3], [2, 2], PaddingMode.SAME), act(),
                              MaskConv2d(4, 4, [3, 3], [2, 1], PaddingMode.SAME), act())
    net = DeepSpeech2(cnn, RNN(RNNType.GRU, D.RNN_IN, D.HID), torch.nn.Sequential(Lookahead(D.HID, D.CTX), act()),
                      FullyConnected(D.HID, D.V, 0, None, None)).eval()
    params = dict(net.named_parameters())
    assert sorted(params) == sorted(w), (sorted(params), sorted(w))
    with torch.no_grad():
        for key, p in params.items():
            p.copy_(torch.as_tensor(w[key]))
    net.rnn.gru_backward = switch
    return net, params


def batch(d):
    return ((torch.tensor(d["x"], device="cuda"), torch.as_tensor(d["lens"])),
            (torch.as_tensor(d["targets"]), torch.as_tensor(d["target_lens"])))


def test_shipped_architecture_in_miniature_trains_under_ctc_loss():
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    D = M.M
    w, d = M.make()
    want_loss, want = M.yardstick(w, d)
    f32_loss, f32 = M.torch_full(w, d, torch.float32)
    net, params = build_model(w)
    inputs, targets = batch(d)
    (before, _), _ = net((inputs[0].clone(), inputs[1]))
    before = before.clone()
    (out, out_lens), hid = net(inputs, differentiable=True)
    assert out.shape == (max(D.OUT_LENS), D.N, D.V) and out_lens.tolist() == list(D.OUT_LENS)
    assert isinstance(hid, torch.Tensor) and hid.shape == (1, D.N, D.HID)
    loss = CTCLoss()((out, out_lens), targets)
    loss.backward()
    print("loss", float(loss.detach()), "float64", want_loss, "torch float32", f32_loss)
    assert abs(float(loss.detach()) - want_loss) <= REL * abs(want_loss), (float(loss.detach()), want_loss)
    assert all(p.grad is not None for p in params.values())
    got = {k: p.grad.detach().cpu().numpy() for k, p in params.items()}
    report("miniature shipped DeepSpeech2 + CTCLoss", got, want, f32, MEASURED_MODEL)
    (after, _), _ = net((inputs[0].clone(), inputs[1]))
    assert torch.equal(after, before)
    np.testing.assert_allclose(out.detach().cpu().numpy(), before.cpu().numpy(), rtol=FWD, atol=FWD)
    np.testing.assert_allclose(out.detach().cpu().numpy(), M.logits(w, d), rtol=FWD, atol=FWD)


def test_five_sgd_steps_lower_the_loss():
    """Plain SGD at the learning rate at which the float64 yardstick's own loss falls at every step
    (tests/test_gru_backward_cpu.py checks that on the CPU)."""
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    w, d = M.make()
    net, params = build_model(w)
    inputs, targets = batch(d)
    ctc = CTCLoss()
    params = list(params.values())

    def step_loss():
        (out, out_lens), _ = net(inputs, differentiable=True)
        return ctc((out, out_lens), targets)

    losses = []
    for _ in range(M.STEPS):
        for p in params:
            p.grad = None
        loss = step_loss()
        loss.backward()
        losses.append(float(loss.detach()))
        with torch.no_grad():
            for p in params:
                p -= M.LR * p.grad
    with torch.no_grad():
        losses.append(float(step_loss()))
    want = M.sgd_losses(w, d)
    print("device SGD losses", [round(v, 5) for v in losses], "float64", [round(v, 5) for v in want])
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert all(abs(a - b) <= REL * abs(b) for a, b in zip(losses, want)), (losses, want)


def test_the_same_model_with_the_switch_off_still_refuses():
    w, d = M.make()
    net, params = build_model(w, switch=False)
    inputs, _ = batch(d)
    with pytest.raises(ValueError, match="LSTM"):
        net(inputs, differentiable=True)
    assert all(p.grad is None for p in params.values())
