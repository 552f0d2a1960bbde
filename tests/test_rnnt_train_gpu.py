"""Training through the prediction network on the device: ``lstm_train`` on a two-layer stack, ``RNNT.loss`` on a tiny
model, five SGD steps.  Yardsticks on the CPU in float64: ``torch.nn.LSTM`` with autograd for the stack, and
tests/rnnt_train_ref.py for the model (torch autograd through the embedding, the LSTM and the projections, composed with the
float64 gradients of tests/rnnt_joint_loss_ref.py).

Criterion.  The kernels' own bounds are checked through the C ABI (tests/test_lstm_backward_gpu.py,
tests/test_rnnt_joint_loss_gpu.py).  Here the backward consumes the FORWARD's outputs, which the project holds to 1e-4
(tests/test_gpu_parity.py, TOL): every layer output, gate and cell state a gradient term is made of is good to that, a term
is a product of fewer than ten of them (two layers, each output times gate factors times a weight; the joint's tanh and
softmax), so every gradient is held to 1e-3 of its tensor's largest magnitude.  Each test also prints the device's error as a
multiple of the error of torch's float32 CPU autograd on the same case (both against float64, both relative to the tensor's
largest magnitude).  Measured on one MI355X: the device's errors are 6e-8 .. 9e-7, torch's float32 errors 7e-8 .. 4e-7, and
the worst multiples are MEASURED_STACK / MEASURED_MODEL below; the asserted cap is four times the worst
measured multiple of each test (room for another reduction order; a wrong term shows as orders of magnitude).
"""
import numpy as np
import pytest
import torch

import lstm_backward_ref as L
import rnnt_train_ref as M

pytestmark = pytest.mark.gpu

REL = 1e-3
# worst multiple of torch's float32 CPU error, measured on one MI355X (recorded in profiles/lstm_backward_time.json)
MEASURED_STACK = 3.31      # h_n; every gradient of the stack is at or below 2.03
MEASURED_MODEL = 2.46      # enc.grad; the parameters are at or below 2.35


def report(name, got, want, f32):
    """name -> (relative error, multiple of torch's float32 error); asserts the criterion."""
    out = {}
    for key, w in want.items():
        err = L.rel_err(got[key], w)
        base = max(L.rel_err(f32[key], w), 2.0 ** -24)
        out[key] = (err, err / base)
    print(name, {k: (f"{e:.2e}", round(m, 2)) for k, (e, m) in out.items()})
    worst = max(m for _, m in out.values())
    print(name, "worst multiple of torch's float32 error:", round(worst, 3))
    for key, (err, _) in out.items():
        assert err <= REL, (name, key, err)
    return worst


def cpu_stack(params, x, lens, h0, c0, d_out, d_hn, d_cn, dtype):
    nl = len(params)
    m = torch.nn.LSTM(x.shape[2], h0.shape[2], num_layers=nl).to(dtype)
    with torch.no_grad():
        for layer, ws in enumerate(params):
            for key, w in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), ws):
                getattr(m, f"{key}_l{layer}").copy_(torch.as_tensor(w, dtype=dtype))
    t = lambda a: torch.tensor(a, dtype=dtype, requires_grad=True)      # noqa: E731
    xs, h, c = t(x), t(h0), t(c0)
    packed = torch.nn.utils.rnn.pack_padded_sequence(xs, torch.as_tensor(lens, dtype=torch.int64))
    out, (hn, cn) = m(packed, (h, c))
    out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=x.shape[0])
    ((out * torch.as_tensor(d_out, dtype=dtype)).sum() + (hn * torch.as_tensor(d_hn, dtype=dtype)).sum()
     + (cn * torch.as_tensor(d_cn, dtype=dtype)).sum()).backward()
    res = dict(out=out, h_n=hn, c_n=cn, dx=xs.grad, d_h0=h.grad, d_c0=c.grad)
    for layer in range(nl):
        for key in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            res[f"{key}_l{layer}"] = getattr(m, f"{key}_l{layer}").grad
    return {k: v.detach().numpy().astype(np.float64) for k, v in res.items()}


def test_lstm_train_two_layers_ragged():
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.rnn_autograd import lstm_train
    In, H, T, N, nl = 5, 40, 7, 3, 2
    rng = np.random.default_rng(11)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    x, h0, c0 = f(T, N, In), 0.5 * f(nl, N, H), 0.5 * f(nl, N, H)
    d_out, d_hn, d_cn = f(T, N, H), f(nl, N, H), f(nl, N, H)
    lens = np.array([7, 4, 1])
    torch.manual_seed(3)
    rnn = RNN(RNNType.LSTM, In, H, num_layers=nl)
    params = [[p.detach().cpu().numpy() for p in layer[0]] for layer in rnn._layer_params()]
    want = cpu_stack(params, x, lens, h0, c0, d_out, d_hn, d_cn, torch.float64)
    f32 = cpu_stack(params, x, lens, h0, c0, d_out, d_hn, d_cn, torch.float32)

    dev = lambda a: torch.tensor(a, device="cuda", requires_grad=True)      # noqa: E731
    xs, h, c = dev(x), dev(h0), dev(c0)
    out, (hn, cn) = lstm_train(rnn, xs, torch.as_tensor(lens), (h, c))
    ((out * torch.tensor(d_out, device="cuda")).sum() + (hn * torch.tensor(d_hn, device="cuda")).sum()
     + (cn * torch.tensor(d_cn, device="cuda")).sum()).backward()
    got = dict(out=out, h_n=hn, c_n=cn, dx=xs.grad, d_h0=h.grad, d_c0=c.grad)
    for layer in range(nl):
        for key in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            got[f"{key}_l{layer}"] = getattr(rnn.rnn, f"{key}_l{layer}").grad
    got = {k: v.detach().cpu().numpy() for k, v in got.items()}
    assert not np.any(got["dx"][4:, 1]) and not np.any(got["dx"][1:, 2])       # rows past a length carry no gradient
    worst = report("lstm_train", got, want, f32)
    if MEASURED_STACK is not None:
        assert worst <= 4.0 * MEASURED_STACK
    # the forward is RNN.forward's, within the forward's existing tolerance (tests/test_gpu_parity.py: TOL)
    with torch.no_grad():
        (o2, _), (hn2, cn2) = rnn((torch.tensor(x, device="cuda"), torch.as_tensor(lens)),
                                  (torch.tensor(h0, device="cuda"), torch.tensor(c0, device="cuda")))
    for a, b in ((out, o2), (hn, hn2), (cn, cn2)):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=1e-4)


def build_model(w):
    from myrtlespeech_amd.model.rnnt import RNNT, RNNTJoint, RNNTPredictor
    pred = RNNTPredictor(M.V, M.D, M.H, num_layers=M.LAYERS)
    joint = RNNTJoint(M.E, M.H, M.J, M.V)
    cp = lambda p, a: p.data.copy_(torch.as_tensor(a))      # noqa: E731
    cp(pred.embedding.weight, w["emb"])
    for layer in range(M.LAYERS):
        for key, name in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh")):
            cp(getattr(pred.rnn.rnn, f"{name}_l{layer}"), w[f"{key}_l{layer}"])
    cp(joint.enc_proj.weight, w["enc_w"])
    cp(joint.enc_proj.bias, w["enc_b"])
    cp(joint.pred_proj.weight, w["pred_w"])
    cp(joint.out.weight, w["out_w"])
    cp(joint.out.bias, w["out_b"])
    return RNNT(torch.nn.Identity(), pred, joint)


def model_params(model):
    pred, joint = model.predictor, model.joint
    out = dict(emb=pred.embedding.weight, enc_w=joint.enc_proj.weight, enc_b=joint.enc_proj.bias, pred_w=joint.pred_proj.weight,
               out_w=joint.out.weight, out_b=joint.out.bias)
    for layer in range(M.LAYERS):
        for key, name in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh")):
            out[f"{key}_l{layer}"] = getattr(pred.rnn.rnn, f"{name}_l{layer}")
    return out


def data_tensors(d):
    return (torch.as_tensor(d["lens"]), torch.as_tensor(d["targets"]), torch.as_tensor(d["target_lens"]))


def test_rnnt_loss_gradients_reach_everything():
    w, d = M.make()
    want_loss, want = M.yardstick(w, d)
    f32_loss, f32 = M.torch_full(w, d, torch.float32)
    model = build_model(w)
    lens, y, yl = data_tensors(d)
    enc_detached = torch.tensor(d["enc"], device="cuda")
    # what the detached paths give before the training call ...
    before_pred = model.predictor.forward_targets(y, yl).clone()
    before_nll = model.transcript_nll(enc_detached, lens, y, yl).clone()
    enc = torch.tensor(d["enc"], device="cuda", requires_grad=True)
    loss = model.loss(enc, lens, y, yl)
    loss.backward()
    loss = loss.detach()
    assert abs(float(loss) - want_loss) <= REL * abs(want_loss), (float(loss), want_loss)
    print("loss", float(loss), "float64", want_loss, "torch float32", f32_loss)
    params = model_params(model)
    assert all(p.grad is not None for p in params.values())
    got = {k: p.grad.detach().cpu().numpy() for k, p in params.items()}
    got["enc"] = enc.grad.cpu().numpy()
    worst = report("RNNT.loss", got, want, f32)
    if MEASURED_MODEL is not None:
        assert worst <= 4.0 * MEASURED_MODEL
    # ... they give bit for bit afterwards
    assert torch.equal(model.predictor.forward_targets(y, yl), before_pred)
    assert torch.equal(model.transcript_nll(enc_detached, lens, y, yl), before_nll)
    # the other reductions are the same node under torch's own reductions
    none = model.loss(enc_detached, lens, y, yl, reduction="none").detach()
    assert none.shape == (M.N,) and abs(float(none.sum()) / M.N - float(loss)) <= 1e-5 * abs(float(loss))


def test_five_sgd_steps_lower_the_loss():
    """Plain SGD at the learning rate and seed at which the float64 yardstick's own loss falls at every step
    (tests/test_lstm_backward_cpu.py checks that on the CPU)."""
    w, d = M.make()
    model = build_model(w)
    lens, y, yl = data_tensors(d)
    enc = torch.tensor(d["enc"], device="cuda")
    params = list(model_params(model).values())
    losses = []
    for _ in range(M.STEPS):
        for p in params:
            p.grad = None
        loss = model.loss(enc, lens, y, yl)
        loss.backward()
        losses.append(float(loss.detach()))
        with torch.no_grad():
            for p in params:
                p -= M.LR * p.grad
    with torch.no_grad():
        losses.append(float(model.loss(enc, lens, y, yl)))
    want = M.sgd_losses(w, d)
    print("device SGD losses", [round(v, 5) for v in losses], "float64", [round(v, 5) for v in want])
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert all(abs(a - b) <= REL * abs(b) for a, b in zip(losses, want)), (losses, want)
