"""The float64 yardstick of training the shipped DeepSpeech2 architecture in miniature (TEST INFRASTRUCTURE ONLY): the front end,
batch and targets of tests/ds2_train_ref.py's model 2 (its docstring describes them), then ONE unidirectional GRU 12 -> 8,
``Lookahead(context 3)`` + ``Hardtanh(0, 1)`` and the output layer of 6 symbols, under CTC loss (blank 0, reduction "mean") on
the CPU in torch ops with autograd -- ``torch.nn.GRU`` with ``pack_padded_sequence`` where that file has ``torch.nn.LSTM``.

``make()``                  weights under the model's state_dict keys (float32 values) and the batch.
``torch_full(w, d, dt)``    loss, gradients; ``yardstick`` is the same in float64.
``logits(w, d)``            the float64 logits [T, N, V].
``sgd_losses(w, d)``        losses of ``STEPS`` plain SGD steps at ``LR`` in float64, and the one after the last.
"""
import numpy as np
import torch
import torch.nn.functional as F

import ds2_train_ref as M

LR = M.LR
STEPS = M.STEPS
GRU_KEYS = tuple(f"rnn.rnn.{n}_l0" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


def make():
    w2, d = M.make(2)
    w = {k: v for k, v in w2.items() if not k.startswith("rnn.")}
    rng = np.random.default_rng(2560)
    k = 1.0 / np.sqrt(M.HID)
    for key in GRU_KEYS:
        shape = (3 * M.HID, M.RNN_IN) if "weight_ih" in key else ((3 * M.HID, M.HID) if "weight_hh" in key else (3 * M.HID,))
        w[key] = rng.uniform(-k, k, shape).astype(np.float32)
    return w, d


def _chain(w, d, dtype):
    """(loss, parameters as leaf tensors, logits [T, N, V])."""
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in w.items()}
    h = torch.tensor(d["x"], dtype=dtype)
    lens = torch.as_tensor(d["lens"])
    for name, _, _, (kf, kt), (sf, st) in M.CONVS:
        t = h.shape[3]
        h = h * (torch.arange(t)[None, :] < lens[:, None])[:, None, None, :].to(dtype)
        pf, pt = M._same_pads(h.shape[2], kf, sf), M._same_pads(t, kt, st)
        h = F.hardtanh(F.conv2d(F.pad(h, (pt[0], pt[1], pf[0], pf[1])), p[f"{name}.weight"], p[f"{name}.bias"], stride=(sf, st)),
                       0.0, M.CLIP)
        lens = torch.floor((lens.to(torch.float32) + float(sum(pt)) - float(kt)) / float(st) + 1.0).to(lens.dtype)
    assert tuple(lens.tolist()) == M.OUT_LENS
    n, c, f, t = h.shape
    h = h.reshape(n, c * f, t).permute(2, 0, 1)          # [T, N, C F]
    m = torch.nn.GRU(M.RNN_IN, M.HID).to(dtype)
    out, _ = torch.func.functional_call(m, {k.split(".")[-1]: p[k] for k in GRU_KEYS}, (torch.nn.utils.rnn.pack_padded_sequence(h, lens),))
    h, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=t)
    z = F.conv1d(F.pad(h.permute(1, 2, 0), (0, M.CTX - 1)), p["lookahead.0.weight"], groups=M.HID)      # [N, F, T]
    h = F.hardtanh(z, 0.0, M.CLIP).permute(2, 0, 1)
    fc = "fully_connected.fully_connected"
    logits_ = F.linear(h, p[f"{fc}.weight"], p[f"{fc}.bias"])
    loss = F.ctc_loss(torch.log_softmax(logits_, -1), torch.as_tensor(d["targets"]), lens, torch.as_tensor(d["target_lens"]),
                      blank=0, reduction="mean")
    return loss, p, logits_


def torch_full(w, d, dtype=torch.float64):
    loss, p, _ = _chain(w, d, dtype)
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach().numpy().astype(np.float64) for k, v in p.items()}


def yardstick(w, d):
    return torch_full(w, d, torch.float64)


def logits(w, d):
    return _chain(w, d, torch.float64)[2].detach().numpy()


def sgd_losses(w, d, lr=LR, steps=STEPS):
    w = {k: v.astype(np.float64) for k, v in w.items()}
    losses = []
    for _ in range(steps):
        loss, grads = torch_full(w, d)
        losses.append(loss)
        w = {k: v - lr * grads[k] for k, v in w.items()}
    losses.append(torch_full(w, d)[0])
    return losses
