"""CPU side of the trainable transducer (``RNNT.loss``; TEST INFRASTRUCTURE ONLY): a tiny model's weights and data, and two
CPU evaluations of loss and gradients.

``yardstick(w, d)``          float64: torch autograd through the embedding, the LSTM stack and the two projections, composed
                             with the float64 gradients of tests/rnnt_joint_loss_ref.py for the joint and the loss.
``torch_full(w, d, dtype)``  the whole chain in torch on the CPU, the transducer recursion written out in torch ops: in
                             float64 it must agree with ``yardstick`` (tests/test_lstm_backward_cpu.py), in float32 it is the
                             error a float32 implementation is expected to make.
``sgd_losses(w, d, lr, k)``  the float64 loss before each of k plain SGD steps and after the last.
"""
import numpy as np
import torch

import rnnt_joint_loss_ref as G

V, D, H, LAYERS, J, E = 7, 6, 40, 2, 32, 12
T, N, U = 6, 3, 4
SEED, LR, STEPS = 5, 0.05, 5
PARAMS = (["emb"] + [f"{k}_l{layer}" for layer in range(LAYERS) for k in ("w_ih", "w_hh", "b_ih", "b_hh")]
          + ["enc_w", "enc_b", "pred_w", "out_w", "out_b"])


def make(seed=SEED):
    """(weights, data): float32 numpy; lengths ragged in both directions, sorted as the encoder's batch is."""
    rng = np.random.default_rng(seed)
    u = lambda k, *shape: rng.uniform(-k, k, shape).astype(np.float32)      # noqa: E731
    w = dict(emb=rng.standard_normal((V + 1, D)).astype(np.float32))
    for layer in range(LAYERS):
        k = 1.0 / np.sqrt(H)
        w[f"w_ih_l{layer}"], w[f"w_hh_l{layer}"] = u(k, 4 * H, D if layer == 0 else H), u(k, 4 * H, H)
        w[f"b_ih_l{layer}"], w[f"b_hh_l{layer}"] = u(k, 4 * H), u(k, 4 * H)
    w["enc_w"], w["enc_b"] = u(1 / np.sqrt(E), J, E), u(1 / np.sqrt(E), J)
    w["pred_w"] = u(1 / np.sqrt(H), J, H)
    w["out_w"], w["out_b"] = u(1 / np.sqrt(J), V + 1, J), u(1 / np.sqrt(J), V + 1)
    d = dict(enc=rng.standard_normal((T, N, E)).astype(np.float32), lens=np.array([6, 5, 3]),
             targets=rng.integers(0, V, size=(N, U)), target_lens=np.array([2, 4, 1]))
    return w, d


def _modules(w, dtype):
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)      # noqa: E731
    p = {k: t(w[k]) for k in PARAMS}
    lstm = torch.nn.LSTM(D, H, num_layers=LAYERS).to(dtype)
    return p, lstm


def _pred_and_proj(p, lstm, d, dtype):
    """enc (leaf), enc_p [T, N, J], pred_p [U + 1, N, J] in torch on the CPU."""
    from torch.func import functional_call
    enc = torch.tensor(d["enc"], dtype=dtype, requires_grad=True)
    idx = torch.cat([torch.full((1, N), V, dtype=torch.int64), torch.as_tensor(d["targets"], dtype=torch.int64).t()], 0)
    emb = p["emb"][idx]                                                           # [U + 1, N, D]
    names = {f"{a}_l{layer}": p[f"{b}_l{layer}"] for layer in range(LAYERS)
             for a, b in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh"))}
    pred, _ = functional_call(lstm, names, (emb,))
    enc_p = enc @ p["enc_w"].t() + p["enc_b"]
    pred_p = pred @ p["pred_w"].t()
    return enc, enc_p, pred_p


def _collect(p, enc):
    out = {k: (None if v.grad is None else v.grad.numpy().astype(np.float64)) for k, v in p.items()}
    out["enc"] = enc.grad.numpy().astype(np.float64)
    return out


def yardstick(w, d, reduction="mean"):
    """(loss, grads) in float64; grads: name -> array for every entry of PARAMS and ``enc``."""
    p, lstm = _modules(w, torch.float64)
    enc, enc_p, pred_p = _pred_and_proj(p, lstm, d, torch.float64)
    c = dict(enc_p=enc_p.detach().numpy(), pred_p=pred_p.detach().numpy(), w_out=np.asarray(w["out_w"], dtype=np.float64),
             b_out=np.asarray(w["out_b"], dtype=np.float64), in_lens=d["lens"], targets=d["targets"], tgt_lens=d["target_lens"],
             blank=V)
    scale = {"mean": 1.0 / N, "sum": 1.0}[reduction]
    ref, _ = G.gradients(c, np.full(N, scale))
    torch.autograd.backward([enc_p, pred_p], [torch.from_numpy(ref.grads.d_enc_p), torch.from_numpy(ref.grads.d_pred_p)])
    grads = _collect(p, enc)
    grads["out_w"], grads["out_b"] = ref.grads.d_w_out, ref.grads.d_b_out
    return float(ref.loss.nll.sum() * scale), grads


def torch_full(w, d, dtype=torch.float64):
    p, lstm = _modules(w, dtype)
    enc, enc_p, pred_p = _pred_and_proj(p, lstm, d, dtype)
    x = torch.tanh(enc_p.transpose(0, 1)[:, :, None, :] + pred_p.transpose(0, 1)[:, None, :, :]) @ p["out_w"].t() + p["out_b"]
    lp = torch.log_softmax(x, -1)                                                 # [N, T, U + 1, V + 1]
    total = 0.0
    for n in range(N):
        tn, un = int(d["lens"][n]), int(d["target_lens"][n])
        alpha = {}
        for t in range(tn):
            for u in range(un + 1):
                terms = []
                if t > 0:
                    terms.append(alpha[t - 1, u] + lp[n, t - 1, u, V])
                if u > 0:
                    terms.append(alpha[t, u - 1] + lp[n, t, u - 1, int(d["targets"][n, u - 1])])
                alpha[t, u] = torch.logsumexp(torch.stack(terms), 0) if terms else torch.zeros((), dtype=dtype)
        total = total - (alpha[tn - 1, un] + lp[n, tn - 1, un, V])
    loss = total / N
    loss.backward()
    return float(loss.detach()), _collect(p, enc)


def sgd_losses(w, d, lr=LR, steps=STEPS):
    w = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    losses = []
    for _ in range(steps):
        loss, g = yardstick(w, d)
        losses.append(loss)
        w = {k: v - lr * g[k] for k, v in w.items()}
    losses.append(yardstick(w, d)[0])
    return losses
