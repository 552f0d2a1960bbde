"""Times the convolution backward at DeepSpeech2's front-end shapes and one whole DS2 training step, on one MI355X.

Shapes: batch 32 of 10 s clips (1001 frames), conv1 1 -> 32, taps [41, 11], stride [2, 2]; conv2 32 -> 32, taps [21, 11],
stride [2, 1] on conv1's output; both SAME with ``Hardtanh(0, 20)``.  Two feature counts: 80 (what bench.py's model reads) and
161 (a linear spectrogram at 16 kHz).

  conv1_weight                ``ms_maskconv_backward_weight`` (conv1's input is data: its data gradient is never asked for)
  conv2_data, conv2_weight    ``ms_maskconv_backward_data`` / ``ms_maskconv_backward_weight``
  torch_*                     ``torch.nn.functional.conv2d``'s own backward on the device for the same gradient, on the padded
                              input (``torch.autograd.grad`` through a retained graph: the backward alone); null if it cannot run
  floor_ms                    FLOP / 157.3e12 with FLOP = 2 N Cout Fout Tout Cin KF KT: the float32-MFMA rate of the device
  ds2_forward_ctc_backward    bench.py's model: ``DeepSpeech2.forward(differentiable=True)`` + ``CTCLoss`` + backward, one step
  ds2_default_forward         the same model's default (inference) forward on the same batch, for scale

The arms alternate in one process after one untimed call each; the median of ``--repeats`` (7) is the figure.  It also runs
tests/test_ds2_train_gpu.py's two models and records the worst multiples of torch's float32 CPU error.  There is no CPU path.

    python tools/conv_backward_time.py [--repeats 7] [--out profiles/conv_backward_time.json]
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

N, T = 32, 1001
CLAMP = (0.0, 20.0)
MFMA_F32_FLOPS = 157.3e12
CONV1 = dict(cin=1, cout=32, taps=(41, 11), stride=(2, 2))
CONV2 = dict(cin=32, cout=32, taps=(21, 11), stride=(2, 1))


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def timed(arms, repeats):
    for fn in arms.values():                                              # untimed
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def die(rc, what):
    if rc != 0:
        sys.exit(f"conv_backward_time: {what} returned {rc}")


class Conv:
    """One convolution's operands on the device and its gradient calls."""

    def __init__(self, spec, x, gen):
        from myrtlespeech_amd import _lib
        from myrtlespeech_amd.model.cnn import pad_same
        self.lib, self.p, self.st = _lib.load(), _lib.ptr, _lib.stream_ptr
        n, cin, fin, tin = x.shape
        (kf, kt), (sf, st) = spec["taps"], spec["stride"]
        cout = spec["cout"]
        self.pf, self.pt = pad_same(fin, kf, sf), pad_same(tin, kt, st)
        fout, tout = -(-fin // sf), -(-tin // st)
        k = 1.0 / (cin * kf * kt) ** 0.5
        self.x = x
        self.w = (k * torch.randn((cout, cin, kf, kt), generator=gen)).cuda()
        self.stride = (sf, st)
        # the saved output with all three regimes of the clamp, and a gradient of the size a mean-reduced loss hands down
        self.y = torch.clamp(8.0 * torch.randn((n, cout, fout, tout), generator=gen) + 6.0, *CLAMP).cuda()
        self.dy = (1e-3 * torch.randn((n, cout, fout, tout), generator=gen)).cuda()
        self.lens = torch.full((n,), tin, dtype=torch.int32, device="cuda")
        self.geom = (n, cin, fin, tin, cout, fout, tout, kf, kt, sf, st, 1, 1, self.pf[0], self.pt[0], _lib.ACT_CLAMP, *CLAMP)
        self.dx, self.dw = torch.empty_like(x), torch.empty_like(self.w)
        self.db = torch.empty(cout, dtype=torch.float32, device="cuda")
        self.nbytes = self.lib.ms_maskconv_backward_workspace_bytes(n, cin, cout, fout, tout, kf, kt)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
        self.flop = 2.0 * n * cout * fout * tout * cin * kf * kt
        self.shape = {"x": list(x.shape), "w": list(self.w.shape), "y": list(self.y.shape), "stride": [sf, st],
                      "workspace_bytes": int(self.nbytes)}

    def data(self):
        p = self.p
        die(self.lib.ms_maskconv_backward_data(p(self.w), p(self.y), p(self.dy), p(self.lens), p(self.dx), *self.geom, self.st()),
            "ms_maskconv_backward_data")

    def weight(self):
        p = self.p
        die(self.lib.ms_maskconv_backward_weight(p(self.x), p(self.y), p(self.dy), p(self.lens), p(self.dw), p(self.db), *self.geom,
                                                 p(self.ws), self.nbytes, self.st()), "ms_maskconv_backward_weight")

    def torch_arms(self, want):
        """{name: fn} of torch's own conv2d backward for the gradients in ``want``; {} (recorded as null) if it cannot run."""
        try:
            xp = torch.nn.functional.pad(self.x, (self.pt[0], self.pt[1], self.pf[0], self.pf[1])).requires_grad_(True)
            w = self.w.clone().requires_grad_(True)
            y = torch.nn.functional.conv2d(xp, w, stride=self.stride)
            g = torch.where((self.y > CLAMP[0]) & (self.y < CLAMP[1]), self.dy, torch.zeros((), device="cuda"))
            arms = {}
            if "data" in want:
                arms["data"] = lambda: torch.autograd.grad(y, xp, g, retain_graph=True)
            if "weight" in want:
                arms["weight"] = lambda: torch.autograd.grad(y, w, g, retain_graph=True)
            for fn in arms.values():
                fn()
            torch.cuda.synchronize()
            return arms
        except Exception as e:      # noqa: BLE001 (a device library that is absent or refuses the shape)
            print("conv_backward_time: torch's conv2d backward cannot run here:", repr(e)[:200], file=sys.stderr)
            return {}


def conv_records(features, repeats):
    gen = torch.Generator().manual_seed(7)
    x1 = torch.randn((N, 1, features, T), generator=gen).cuda()
    c1 = Conv(CONV1, x1, gen)
    c2 = Conv(CONV2, c1.y, gen)
    arms = {"conv1_weight": c1.weight, "conv2_data": c2.data, "conv2_weight": c2.weight}
    t1, t2 = c1.torch_arms(("weight",)), c2.torch_arms(("data", "weight"))
    arms.update({f"torch_conv1_{k}": fn for k, fn in t1.items()})
    arms.update({f"torch_conv2_{k}": fn for k, fn in t2.items()})
    ms = timed(arms, repeats)
    rec = {"conv1": c1.shape, "conv2": c2.shape}
    for name, conv in (("conv1_weight", c1), ("conv2_data", c2), ("conv2_weight", c2)):
        med = statistics.median(ms[name])
        floor = conv.flop / MFMA_F32_FLOPS * 1e3
        tname = "torch_" + name
        rec[name] = {"ms": spread(ms[name]), "flop": conv.flop, "floor_ms": round(floor, 4), "floor_over_measured": round(floor / med, 4),
                     "torch_ms": spread(ms[tname]) if tname in ms else None,
                     "over_torch": round(med / statistics.median(ms[tname]), 3) if tname in ms else None}
    return rec


def ds2_arm():
    import bench
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    model = bench.build_model()
    ctc = CTCLoss()
    g = torch.Generator().manual_seed(3)
    x = torch.randn((bench.BATCH_PER_GPU, 1, bench.FEATURES, bench.FRAMES), generator=g).cuda()
    lens = torch.full((bench.BATCH_PER_GPU,), bench.FRAMES, dtype=torch.int64)
    y, y_lens = torch.randint(1, bench.VOCAB - 1, (bench.BATCH_PER_GPU, 100), generator=g), torch.full((bench.BATCH_PER_GPU,), 100)
    params = list(model.parameters())

    def step():
        for q in params:
            q.grad = None
        (out, out_lens), _ = model((x, lens), differentiable=True)
        ctc((out, out_lens), (y, y_lens)).backward()

    def forward_only():
        with torch.no_grad():
            model((x, lens))

    return {"ds2_forward_ctc_backward": step, "ds2_default_forward": forward_only}


def error_records():
    """tests/test_ds2_train_gpu.py's models: the worst multiples of torch's float32 CPU error."""
    import test_ds2_train_gpu as D
    inner = D.report
    worst = {}

    def recording(name, got, want, f32):
        worst[name] = round(inner(name, got, want, f32), 3)
        return worst[name]

    D.report = recording
    try:
        for model in D.M.MODELS:
            D.test_ds2_ctc_loss_gradients_reach_every_parameter(model)
    finally:
        D.report = inner
    return {"worst_multiples_of_torch_float32_error": worst,
            "multiples": "device error over torch float32 CPU autograd error, both against float64 and relative to the tensor's "
                         "largest magnitude"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--features", type=int, nargs="*", default=[80, 161])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_backward_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conv_backward_time: a HIP device is required; there is no CPU path")
    out = {"tool": "tools/conv_backward_time.py", "commit": a.commit,
           "statistic": "host clock around calls ending in a device synchronise, per call, ms; the arms alternate in one process "
                        "after one untimed call each; median of the repeats",
           "floor": "FLOP / 157.3e12 (float32 MFMA), FLOP = 2 N Cout Fout Tout Cin KF KT (taps that fall on padding included)"}
    for f in a.features:
        out[f"features_{f}"] = conv_records(f, a.repeats)
        torch.cuda.empty_cache()
    out["deep_speech_2"] = {f"{k}_ms": spread(v) for k, v in timed(ds2_arm(), a.repeats).items()}
    torch.cuda.empty_cache()
    out["errors"] = error_records()
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
