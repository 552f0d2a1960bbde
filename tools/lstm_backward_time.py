"""Times training through the prediction network: the predictor of BASELINE configs[3] as tools/rnnt_score_time.py builds it
(128-wide embedding, two LSTM layers of 512), on [U + 1, N] = [121, 16] transcripts.

  detached_forward_targets        ``RNNTPredictor.forward_targets`` as the scorer calls it
  differentiable_forward_targets  the same with ``differentiable=True`` (layer by layer, the node's tensors saved)
  predictor_forward_backward      that forward, then its backward
  torch_lstm_forward_backward     the yardstick: ``torch.nn.LSTM`` on the device, same shapes, forward + backward
  per layer, through the C ABI:   ``ms_lstm_recompute``, ``ms_lstm_backward_steps`` (and its time per launch), the three
                                  batch products through ``ms_linear_forward``
  rnnt_loss_forward_backward      ``RNNT.loss`` + backward at 29 and 5000 symbols, T = 250 frames, beside
  joint_loss_forward_backward     ``rnnt_joint_loss`` + backward alone on the same projected inputs

The arms alternate in one process after one untimed call each; the median of ``--repeats`` (7) is the figure.  It also runs
tests/test_lstm_backward_gpu.py's cases and tests/test_rnnt_train_gpu.py and records the device's worst ratios to the derived
bounds and its worst multiples of torch's float32 CPU error.  There is no CPU path: without a HIP device the tool fails.

    python tools/lstm_backward_time.py [--repeats 7] [--out profiles/lstm_backward_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import torch  # noqa: E402

N, T, U, J = 16, 250, 120, 512
ENC, HID, EMB, LAYERS = 512, 512, 128, 2
SHAPES = {"small": 29, "large": 5000}


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def timed(arms, repeats, inner=1):
    for fn in arms.values():                                              # untimed
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / inner)
    return ms


def make_model(vocab, seed=11):
    from myrtlespeech_amd.model.rnnt import RNNT, RNNTJoint, RNNTPredictor
    torch.manual_seed(seed)
    pred = RNNTPredictor(vocab, EMB, HID, num_layers=LAYERS).eval()
    joint = RNNTJoint(ENC, HID, J, vocab).eval()
    model = RNNT(torch.nn.Identity(), pred, joint)
    g = torch.Generator().manual_seed(seed + 1)
    enc = torch.randn((T, N, ENC), generator=g).cuda()
    lens = torch.full((N,), T, dtype=torch.int64)
    y = torch.randint(0, vocab, (N, U), generator=g, dtype=torch.int64)
    y_lens = torch.full((N,), U, dtype=torch.int64)
    return model, enc, lens, y, y_lens


class LayerAbi:
    """One layer's backward through the C ABI on fixed device buffers: In -> HID over [U + 1, N]."""

    def __init__(self, in_size, seed=3):
        from myrtlespeech_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.In, self.t, self.rows = in_size, U + 1, (U + 1) * N
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(s, generator=g).cuda()      # noqa: E731
        k = 1.0 / HID ** 0.5
        self.x, self.h = r(self.t, N, in_size), torch.tanh(r(self.t, N, HID))
        self.w_ih, self.w_hh, self.b_ih, self.b_hh = k * r(4 * HID, in_size), k * r(4 * HID, HID), k * r(4 * HID), k * r(4 * HID)
        self.d_out = r(self.t, N, HID)
        e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")      # noqa: E731
        self.gates, self.c, self.dG = e(self.t, N, 4 * HID), e(self.t, N, HID), e(self.t, N, 4 * HID)
        self.d_h0, self.d_c0, self.d_b = e(N, HID), e(N, HID), e(4 * HID)
        self.ws = torch.empty(self.lib.ms_lstm_recompute_workspace_bytes(self.t, N, HID), dtype=torch.uint8, device="cuda")

    def check(self, rc, what):
        if rc != 0:
            sys.exit(f"lstm_backward_time: {what} returned {rc}")

    def recompute(self):
        p = self._lib.ptr
        self.check(self.lib.ms_lstm_recompute(p(self.x), p(self.h), p(None), p(None), p(None), p(self.w_ih), p(self.w_hh),
                                              p(self.b_ih), p(self.b_hh), p(self.gates), p(self.c), self.t, N, self.In, HID,
                                              p(self.ws), self.ws.numel(), self._lib.stream_ptr()), "ms_lstm_recompute")

    def steps(self):
        p = self._lib.ptr
        self.check(self.lib.ms_lstm_backward_steps(p(self.gates), p(self.c), p(None), p(self.w_hh), p(self.d_out), p(None), p(None),
                                                   p(None), self.t, p(self.dG), p(self.d_h0), p(self.d_c0), p(self.d_b), self.t, N,
                                                   HID, self._lib.stream_ptr()), "ms_lstm_backward_steps")

    def products(self):
        from myrtlespeech_amd.model.rnn_autograd import gemm_nt
        g2 = self.dG.reshape(self.rows, 4 * HID)
        g2_t = g2.t().contiguous()
        h_prev = torch.cat([torch.zeros((1, N, HID), device="cuda"), self.h[:-1]], 0)
        gemm_nt(g2_t, self.x.reshape(self.rows, self.In).t())
        gemm_nt(g2_t, h_prev.reshape(self.rows, HID).t())
        gemm_nt(g2, self.w_ih.t())


def predictor_arms(model, y, y_lens):
    pred = model.predictor
    params = [p for p in pred.parameters()]
    ref = torch.nn.LSTM(EMB, HID, num_layers=LAYERS).cuda()
    x_ref = torch.randn((U + 1, N, EMB), device="cuda")

    def detached():
        with torch.no_grad():
            pred.forward_targets(y, y_lens)

    def differentiable():
        pred.forward_targets(y, y_lens, differentiable=True)

    def forward_backward():
        for p in params:
            p.grad = None
        pred.forward_targets(y, y_lens, differentiable=True).sum().backward()

    def torch_lstm():
        for p in ref.parameters():
            p.grad = None
        ref(x_ref)[0].sum().backward()

    return {"detached_forward_targets": detached, "differentiable_forward_targets": differentiable,
            "predictor_forward_backward": forward_backward, "torch_lstm_forward_backward": torch_lstm}


def loss_arms(model, enc, lens, y, y_lens):
    from myrtlespeech_amd.loss.rnnt_loss import rnnt_joint_loss
    params = [p for p in model.parameters()]
    with torch.no_grad():
        enc_p = model.joint.project_encoder(enc).reshape(T, N, J)
        pred_p = model.joint.project_predictor(model.predictor.forward_targets(y, y_lens)).reshape(U + 1, N, J)
    leaves = [x.clone().requires_grad_() for x in (enc_p, pred_p, model.joint.out.weight.detach(), model.joint.out.bias.detach())]
    blank = model.predictor.blank

    def whole():
        for p in params:
            p.grad = None
        model.loss(enc, lens, y, y_lens).backward()

    def joint_alone():
        for x in leaves:
            x.grad = None
        rnnt_joint_loss(*leaves, lens, y, y_lens, blank, "mean").backward()

    return {"rnnt_loss_forward_backward": whole, "joint_loss_forward_backward": joint_alone}


def error_records():
    """The cases of the two GPU test files: worst ratios to the derived bounds, worst multiples of torch's float32 error."""
    import test_lstm_backward_gpu as A
    import test_rnnt_train_gpu as B
    for name in A.L.CASE_NAMES:
        A.test_case_within_the_bounds(name)
    stack = B.report
    worst = {}

    def recording(name, got, want, f32):
        worst[name] = round(stack(name, got, want, f32), 3)
        return worst[name]

    B.report = recording
    try:
        B.test_lstm_train_two_layers_ragged()
        B.test_rnnt_loss_gradients_reach_everything()
    finally:
        B.report = stack
    return {"worst_ratios_to_the_bounds": {k: round(float(v), 5) for k, v in A.worst.items()},
            "worst_multiples_of_torch_float32_error": {"c_abi": {k: round(float(v), 3) for k, v in A.worst_mult.items()}, **worst},
            "bounds": "tests/lstm_backward_ref.py", "multiples": "device error over torch float32 CPU autograd error, both against "
            "float64 and relative to the tensor's largest magnitude"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_backward_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstm_backward_time: a HIP device is required; there is no CPU path")
    out = {"tool": "tools/lstm_backward_time.py", "commit": a.commit,
           "shape": {"N": N, "U_plus_1": U + 1, "T": T, "embedding": EMB, "hidden": HID, "layers": LAYERS, "J": J},
           "statistic": "host clock around calls ending in a device synchronise, per call, ms; the arms alternate in one process "
                        "after one untimed call each; median of the repeats"}
    model, enc, lens, y, y_lens = make_model(SHAPES["small"])
    out["predictor"] = {f"{k}_ms": spread(v) for k, v in timed(predictor_arms(model, y, y_lens), a.repeats).items()}
    layers = {}
    for name, in_size in (("layer0", EMB), ("layer1", HID)):
        c = LayerAbi(in_size)
        ms = timed({"recompute": c.recompute, "steps": c.steps, "batch_products": c.products}, a.repeats, 2)
        rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
        launches = U + 2
        per = statistics.median(ms["steps"]) / launches
        rec["step_launches"] = launches
        rec["step_us_per_launch"] = round(per * 1e3, 2)
        rec["w_hh_bytes_per_step"] = 16 * HID * HID
        rec["w_hh_GBps_at_that_time"] = round(16 * HID * HID / (per * 1e-3) / 1e9, 1)
        layers[name] = rec
    out["backward_per_layer"] = layers
    for name, vocab in SHAPES.items():
        if name != "small":
            del model
            torch.cuda.empty_cache()
            model, enc, lens, y, y_lens = make_model(vocab)
        ms = timed(loss_arms(model, enc, lens, y, y_lens), a.repeats)
        rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
        rec["symbols"] = vocab + 1
        rec["predictor_and_projections_ms"] = round(statistics.median(ms["rnnt_loss_forward_backward"])
                                                    - statistics.median(ms["joint_loss_forward_backward"]), 4)
        out[f"rnnt_loss_{name}"] = rec
    out["errors"] = error_records()
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
