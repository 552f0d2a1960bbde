"""The float64 yardstick of DeepSpeech2 training (TEST INFRASTRUCTURE ONLY): two tiny models under CTC loss (blank 0, reduction
"mean") on the CPU, in torch ops with autograd -- mask, ``F.pad``, ``F.conv2d``, ``F.hardtanh``, ``torch.nn.LSTM`` with
``pack_padded_sequence``, the lookahead as a grouped ``F.conv1d``, ``F.linear``, ``F.ctc_loss`` (tests/test_conv_backward_cpu.py
pins the project's own restatement of the convolution and lookahead backward to the same ops).

Both models share the front end: 9 features -> conv 1 -> 4, taps [5, 3], stride [2, 2] -> conv 4 -> 4, taps [3, 3], stride
[2, 1], both SAME and ``Hardtanh(0, 1)``: 3 features x 4 channels = 12 inputs of the recurrent stack.  N 3, 14 input frames,
lens [14, 9, 3] -> 7 / 5 / 2 output frames; target lengths [3, 2, 1] with a repeated label.
``MODEL = 1``  two bidirectional LSTM layers of 8, one hidden fully connected layer of 8 with ``Hardtanh(0, 1)``, 6 symbols.
``MODEL = 2``  one unidirectional LSTM of 8, ``Lookahead(context 3)`` + ``Hardtanh(0, 1)``, 6 symbols.

``make(model)``                  weights under the model's state_dict keys (float32 values) and the batch.
``torch_full(model, w, d, dt)``  loss, gradients; ``yardstick`` is the same in float64.
``activations(model, w, d)``     every clamp's output in its live frames.
``sgd_losses(model, w, d)``      losses of ``STEPS`` plain SGD steps at ``LR`` in float64, and the one after the last.

The weights in front of a clamp are scaled (``SCALE``) so that each clamp's three regimes occur in live frames
(tests/test_ds2_train_cpu.py checks that)."""
import numpy as np
import torch
import torch.nn.functional as F

F_IN, N, T_IN, HID, V, CTX = 9, 3, 14, 8, 6, 3
LENS = (14, 9, 3)
OUT_LENS = (7, 5, 2)
TARGET_LENS = (3, 2, 1)
TARGETS = ((2, 2, 4), (5, 1, 0), (3, 0, 0))      # a repeated label in the first; padding is 0
CLIP = 1.0
CONVS = (("cnn.0", 1, 4, (5, 3), (2, 2)), ("cnn.2", 4, 4, (3, 3), (2, 1)))
RNN_IN = 12
SCALE = {"cnn.0": 2.0, "cnn.2": 3.0, "fc_hidden": 6.0, "lookahead": 12.0}      # the last two read |h| < 1 of an LSTM
LR = 0.05
STEPS = 5
MODELS = (1, 2)


def lstm_keys(model):
    if model == 1:
        return tuple(f"rnn.rnn.{n}_l{layer}{sfx}" for layer in (0, 1) for sfx in ("", "_reverse")
                     for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    return tuple(f"rnn.rnn.{n}_l0" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


def make(model):
    rng = np.random.default_rng(1512 + model)
    f32 = lambda a: a.astype(np.float32)      # noqa: E731
    w = {}
    for name, cin, cout, (kf, kt), _ in CONVS:
        k = SCALE[name] / np.sqrt(cin * kf * kt)
        w[f"{name}.weight"] = f32(rng.uniform(-k, k, (cout, cin, kf, kt)))
        w[f"{name}.bias"] = f32(rng.uniform(-k, k, cout))
    k = 1.0 / np.sqrt(HID)
    for key in lstm_keys(model):
        if "weight_ih" in key:
            shape = (4 * HID, RNN_IN if "_l0" in key else 2 * HID)
        elif "weight_hh" in key:
            shape = (4 * HID, HID)
        else:
            shape = (4 * HID,)
        w[key] = f32(rng.uniform(-k, k, shape))
    fc = "fully_connected.fully_connected"
    if model == 1:
        k = SCALE["fc_hidden"] / np.sqrt(2 * HID)
        w[f"{fc}.0.weight"], w[f"{fc}.0.bias"] = f32(rng.uniform(-k, k, (HID, 2 * HID))), f32(rng.uniform(-k, k, HID))
        k = 1.0 / np.sqrt(HID)
        w[f"{fc}.2.weight"], w[f"{fc}.2.bias"] = f32(rng.uniform(-k, k, (V, HID))), f32(rng.uniform(-k, k, V))
    else:
        k = SCALE["lookahead"] / np.sqrt(CTX)
        w["lookahead.0.weight"] = f32(rng.uniform(-k, k, (HID, 1, CTX)))
        k = 1.0 / np.sqrt(HID)
        w[f"{fc}.weight"], w[f"{fc}.bias"] = f32(rng.uniform(-k, k, (V, HID))), f32(rng.uniform(-k, k, V))
    d = dict(x=f32(rng.standard_normal((N, 1, F_IN, T_IN))), lens=np.array(LENS, dtype=np.int64),
             targets=np.array(TARGETS, dtype=np.int64), target_lens=np.array(TARGET_LENS, dtype=np.int64))
    return w, d


def _same_pads(length, k, stride):
    """(left, right) as model/cnn.py computes them."""
    out = -(-length // stride)
    total = stride * out - 1 + k - length
    return total // 2, total - total // 2


def _chain(model, w, d, dtype):
    """(loss, parameters as leaf tensors, [(clamped activation, boolean live mask broadcastable to it)], logits [T, N, V])."""
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in w.items()}
    h = torch.tensor(d["x"], dtype=dtype)
    lens = torch.as_tensor(d["lens"])
    acts = []
    for name, _, _, (kf, kt), (sf, st) in CONVS:
        t = h.shape[3]
        h = h * (torch.arange(t)[None, :] < lens[:, None])[:, None, None, :].to(dtype)
        pf, pt = _same_pads(h.shape[2], kf, sf), _same_pads(t, kt, st)
        h = F.hardtanh(F.conv2d(F.pad(h, (pt[0], pt[1], pf[0], pf[1])), p[f"{name}.weight"], p[f"{name}.bias"], stride=(sf, st)),
                       0.0, CLIP)
        lens = torch.floor((lens.to(torch.float32) + float(sum(pt)) - float(kt)) / float(st) + 1.0).to(lens.dtype)
        acts.append((h, (torch.arange(h.shape[3])[None, :] < lens[:, None])[:, None, None, :]))
    assert tuple(lens.tolist()) == OUT_LENS
    n, c, f, t = h.shape
    h = h.reshape(n, c * f, t).permute(2, 0, 1)          # [T, N, C F]
    live = (torch.arange(t)[:, None] < lens[None, :])[:, :, None]      # [T, N, 1]
    m = torch.nn.LSTM(RNN_IN, HID, num_layers=2 if model == 1 else 1, bidirectional=model == 1).to(dtype)
    keys = lstm_keys(model)
    out, _ = torch.func.functional_call(m, {k.split(".")[-1]: p[k] for k in keys}, (torch.nn.utils.rnn.pack_padded_sequence(h, lens),))
    h, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=t)
    fc = "fully_connected.fully_connected"
    if model == 1:
        h = F.hardtanh(F.linear(h, p[f"{fc}.0.weight"], p[f"{fc}.0.bias"]), 0.0, CLIP)
        acts.append((h, live))
        logits = F.linear(h, p[f"{fc}.2.weight"], p[f"{fc}.2.bias"])
    else:
        z = F.conv1d(F.pad(h.permute(1, 2, 0), (0, CTX - 1)), p["lookahead.0.weight"], groups=HID)      # [N, F, T]
        h = F.hardtanh(z, 0.0, CLIP).permute(2, 0, 1)
        acts.append((h, live))
        logits = F.linear(h, p[f"{fc}.weight"], p[f"{fc}.bias"])
    loss = F.ctc_loss(torch.log_softmax(logits, -1), torch.as_tensor(d["targets"]), lens, torch.as_tensor(d["target_lens"]),
                      blank=0, reduction="mean")
    return loss, p, acts, logits


def torch_full(model, w, d, dtype=torch.float64):
    loss, p, _, _ = _chain(model, w, d, dtype)
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach().numpy().astype(np.float64) for k, v in p.items()}


def yardstick(model, w, d):
    return torch_full(model, w, d, torch.float64)


def logits(model, w, d):
    return _chain(model, w, d, torch.float64)[3].detach().numpy()


def activations(model, w, d):
    """Every clamp's output in its live frames (conv1, conv2, then the hidden layer or the lookahead), each a flat float64 array."""
    _, _, acts, _ = _chain(model, w, d, torch.float64)
    return [a.detach()[m.expand_as(a)].numpy() for a, m in acts]


def sgd_losses(model, w, d, lr=LR, steps=STEPS):
    w = {k: v.astype(np.float64) for k, v in w.items()}
    losses = []
    for _ in range(steps):
        loss, grads = torch_full(model, w, d)
        losses.append(loss)
        w = {k: v - lr * grads[k] for k, v in w.items()}
    losses.append(torch_full(model, w, d)[0])
    return losses
