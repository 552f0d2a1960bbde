"""The float64 yardstick of DeepSpeech1 training (TEST INFRASTRUCTURE ONLY): a tiny ``DeepSpeech1(5, 1, 8, 6, 0.0,
relu_clip=1.0)`` -- three clipped Linear layers, one bidirectional LSTM, a fourth clipped layer, the output Linear -- under
CTC loss (blank 0, reduction "mean"), on the CPU.

``make()``                    weights under the model's state_dict keys (float32 values) and the batch: N 3, T 9, lens
                              [9, 6, 2], target lengths [3, 2, 1] with a repeated label.
``torch_full(w, d, dtype)``   the whole chain in torch ops with autograd (``torch.nn.LSTM(bidirectional=True)`` with
                              ``pack_padded_sequence``, ``F.hardtanh``, ``F.ctc_loss``): loss, gradients, clipped activations.
``yardstick(w, d)``           the same chain with the LSTM layer replaced by tests/bilstm_backward_ref.py (the restatement of
                              the project's own specification) as an autograd node; float64.
``sgd_losses(w, d)``          losses of ``STEPS`` plain SGD steps at ``LR`` in float64, and the one after the last.

The weights of the clipped layers are scaled (``SCALE``) so that the clamp's three regimes all occur in the live rows: units at
the lower edge, strictly inside, and -- in more than one layer, fc4 among them -- at the upper edge
(tests/test_bilstm_backward_cpu.py checks that; with default initialisation only fc1 reaches the upper edge).
"""
import numpy as np
import torch

import bilstm_backward_ref as B

F_IN, HID, V, N, T = 5, 8, 6, 3, 9
CLIP = 1.0
LENS = (9, 6, 2)
TARGET_LENS = (3, 2, 1)
TARGETS = ((2, 2, 4), (5, 1, 0), (3, 0, 0))      # a repeated label in the first; padding is 0
SCALE = {"fc1.0": 3.0, "fc2.0": 3.0, "fc3.0": 3.0, "fc4.0": 8.0, "out": 1.0}      # fc4 reads |h| < 1 of the LSTM: it needs more
LR = 0.05
STEPS = 5
LAYERS = (("fc1.0", F_IN, HID), ("fc2.0", HID, HID), ("fc3.0", HID, 2 * HID), ("fc4.0", 2 * HID, HID), ("out", HID, V))


def make():
    rng = np.random.default_rng(1412)
    f32 = lambda a: a.astype(np.float32)      # noqa: E731
    w = {}
    for name, fin, fout in LAYERS:
        k = SCALE[name] / np.sqrt(fin)
        w[f"{name}.weight"] = f32(rng.uniform(-k, k, (fout, fin)))
        w[f"{name}.bias"] = f32(rng.uniform(-k, k, fout))
    k = 1.0 / np.sqrt(HID)
    for sfx in ("", "_reverse"):
        w[f"bi_lstm.rnn.weight_ih_l0{sfx}"] = f32(rng.uniform(-k, k, (4 * HID, 2 * HID)))
        w[f"bi_lstm.rnn.weight_hh_l0{sfx}"] = f32(rng.uniform(-k, k, (4 * HID, HID)))
        w[f"bi_lstm.rnn.bias_ih_l0{sfx}"] = f32(rng.uniform(-k, k, 4 * HID))
        w[f"bi_lstm.rnn.bias_hh_l0{sfx}"] = f32(rng.uniform(-k, k, 4 * HID))
    d = dict(x=f32(rng.standard_normal((N, 1, F_IN, T))), lens=np.array(LENS, dtype=np.int64),
             targets=np.array(TARGETS, dtype=np.int64), target_lens=np.array(TARGET_LENS, dtype=np.int64))
    return w, d


class _RefBiLSTM(torch.autograd.Function):
    """The bidirectional layer of tests/bilstm_backward_ref.py as an autograd node: (x, then direction 0's w_ih, w_hh, b_ih,
    b_hh, then direction 1's) -> out [T, N, 2H]."""

    @staticmethod
    def _case(lens, x, ws, d_out=None):
        p = tuple(dict(w_ih=ws[4 * d].numpy(), w_hh=ws[4 * d + 1].numpy(), b_ih=ws[4 * d + 2].numpy(), b_hh=ws[4 * d + 3].numpy())
                  for d in (0, 1))
        return dict(p=p, T=x.shape[0], N=x.shape[1], H=ws[1].shape[1], In=x.shape[2], lens=lens, x=x.numpy(), h0=None, c0=None,
                    d_out=None if d_out is None else d_out.numpy(), d_hn=None, d_cn=None)

    @staticmethod
    def forward(ctx, lens, x, *ws):
        ctx.lens = lens
        ctx.save_for_backward(x, *ws)
        out, _, _ = B.layer_forward(_RefBiLSTM._case(lens, x.detach(), [w.detach() for w in ws]))
        return torch.from_numpy(out)

    @staticmethod
    def backward(ctx, d_out):
        x, *ws = ctx.saved_tensors
        r = B.layer_backward(_RefBiLSTM._case(ctx.lens, x, ws, d_out))
        t = torch.from_numpy
        grads = []
        for d in (0, 1):
            grads += [t(r["d_w_ih"][d]), t(r["d_w_hh"][d]), t(r["d_b"][d]), t(r["d_b"][d])]
        return (None, t(r["dx"]), *grads)


_LSTM_KEYS = tuple(f"bi_lstm.rnn.{n}_l0{sfx}" for sfx in ("", "_reverse") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


def _chain(w, d, dtype, composed):
    """(loss, parameters as leaf tensors, clipped activations [T, N, *] of fc1 .. fc4)."""
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in w.items()}
    lens = torch.as_tensor(d["lens"])
    x = torch.tensor(d["x"], dtype=dtype)
    n, c, f, t = x.shape
    h = x.reshape(n, c * f, t).permute(2, 0, 1)          # [T, N, C F]
    acts = []
    for name in ("fc1.0", "fc2.0", "fc3.0"):
        h = torch.nn.functional.hardtanh(torch.nn.functional.linear(h, p[f"{name}.weight"], p[f"{name}.bias"]), 0.0, CLIP)
        acts.append(h)
    if composed:
        assert dtype == torch.float64
        h = _RefBiLSTM.apply(d["lens"], h, *[p[k] for k in _LSTM_KEYS])
    else:
        m = torch.nn.LSTM(2 * HID, HID, bidirectional=True).to(dtype)
        names = [k.split(".")[-1] for k in _LSTM_KEYS]
        packed = torch.nn.utils.rnn.pack_padded_sequence(h, lens)
        out, _ = torch.func.functional_call(m, {nm: p[k] for nm, k in zip(names, _LSTM_KEYS)}, (packed,))
        h, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=t)
    h = torch.nn.functional.hardtanh(torch.nn.functional.linear(h, p["fc4.0.weight"], p["fc4.0.bias"]), 0.0, CLIP)
    acts.append(h)
    logits = torch.nn.functional.linear(h, p["out.weight"], p["out.bias"])
    loss = torch.nn.functional.ctc_loss(torch.log_softmax(logits, -1), torch.as_tensor(d["targets"]), lens,
                                        torch.as_tensor(d["target_lens"]), blank=0, reduction="mean")
    return loss, p, acts, logits


def _run(w, d, dtype, composed):
    loss, p, acts, logits = _chain(w, d, dtype, composed)
    loss.backward()
    grads = {k: v.grad.detach().numpy().astype(np.float64) for k, v in p.items()}
    return float(loss.detach()), grads, [a.detach().numpy() for a in acts], logits.detach().numpy()


def torch_full(w, d, dtype=torch.float64):
    loss, grads, _, _ = _run(w, d, dtype, composed=False)
    return loss, grads


def yardstick(w, d):
    loss, grads, _, _ = _run(w, d, torch.float64, composed=True)
    return loss, grads


def activations(w, d):
    """The clipped activations of fc1 .. fc4 in the rows that exist (t < lens[n]), each [rows, units], float64."""
    _, _, acts, _ = _run(w, d, torch.float64, composed=False)
    live = np.arange(T)[:, None] < np.asarray(d["lens"])[None, :]
    return [a[live] for a in acts]


def sgd_losses(w, d, lr=LR, steps=STEPS):
    w = {k: v.astype(np.float64) for k, v in w.items()}
    losses = []
    for _ in range(steps):
        loss, grads = torch_full(w, d)
        losses.append(loss)
        w = {k: v - lr * grads[k] for k, v in w.items()}
    losses.append(torch_full(w, d)[0])
    return losses
