"""Times the dropout kernels of csrc/dropout.hip at the two activation shapes of the reference models' widest layers --
[201 * 32, 2048] (DeepSpeech1's fc3 at a batch of 32 four-second clips) and [501 * 32, 1024] -- against torch on the device.

  project_forward            ``ms_dropout_forward``: out = x * m, Philox4x32-10 per four elements
  project_clamp_backward     ``ms_clamp_dropout_backward``: the clamp's gate and the mask in one pass
  torch_dropout_forward      ``torch.nn.functional.dropout(x, p, training=True)``
  torch_dropout_backward     its backward (one multiply with the saved mask)
  torch_where_gate           ``torch.where((y > lo) & (y < hi), dy, 0)``: the gate pass the fused backward replaces

An array here is 53 .. 66 MB and the chip's last-level cache holds 256 MiB, so an arm that ran on the same buffers call after call
would be timed out of that cache.  Every arm therefore owns ``SETS`` sets of buffers (their footprint is well past the cache) and
a timed sample is ``SETS * ROUNDS`` calls, one set after another, between two device synchronises; the figure is the sample over
the number of calls.  The arms of a shape alternate in one process after one untimed sample each; the median of ``--repeats``
(7) is the figure, min and max beside it.  Per arm: the bytes the task needs at the least (8 per element for a forward or a
plain backward, 12 for a gated backward) and the share of the HBM rate (bench.py's HBM_PEAK_GBS) that the time implies.  The
question it answers: does Philox -- about 20 32-bit multiplies per four elements -- leave the forward memory-bound on gfx950?

Then one DeepSpeech1 training step (forward with ``differentiable=True``, CTC loss, backward) at BASELINE configs[0]
([T, N] = [201, 1], n_hidden 1024), in training mode with a generator attached and in ``.eval()`` (no dropout), and the worst
multiples of torch's float32 CPU error of tests/test_dropout_train_gpu.py.  No thresholds: the numbers are the output.  There is
no CPU path.

    python tools/dropout_time.py [--repeats 7] [--out profiles/dropout_time.json]
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

import bench  # noqa: E402

SHAPES = ((201 * 32, 2048), (501 * 32, 1024))
P, LO, HI = 0.25, 0.0, 20.0
SETS, ROUNDS = 6, 4
N, C, F, T, HID, V = 1, 19, 26, 201, 1024, 29


def spread(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5), "repeats": len(v)}


def timed(arms, repeats, calls=1):
    """ms per call: each arm's function makes ``calls`` calls."""
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
            ms[k].append((time.perf_counter() - t0) * 1e3 / calls)
    return ms


def kernel_arms(shape):
    """(arms, least bytes per element of each arm's task)."""
    from myrtlespeech_amd import _lib
    from myrtlespeech_amd.model import dropout
    lib, ptr = _lib.load(), _lib.ptr
    thr, scale = dropout.threshold(P), dropout.scale_of(P)
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda: torch.randn(shape, generator=g, device="cuda")      # noqa: E731
    n = shape[0] * shape[1]
    xs, ys, dys = [rand() for _ in range(SETS)], [rand().clamp_(LO, HI) for _ in range(SETS)], [rand() for _ in range(SETS)]
    outs = [torch.empty(shape, device="cuda") for _ in range(SETS)]
    leaves = [x.clone().requires_grad_(True) for x in xs]
    dropped = [torch.nn.functional.dropout(x, P, True) for x in leaves]      # (their graphs hold the masks)
    zero = torch.zeros((), device="cuda")
    st = _lib.stream_ptr

    def loop(one):
        def run():
            for _ in range(ROUNDS):
                for i in range(SETS):
                    one(i)
        return run

    def fwd(i):
        _lib.check(lib.ms_dropout_forward(ptr(xs[i]), ptr(outs[i]), n, thr, scale, 7, i, st()), "ms_dropout_forward")

    def bwd(i):
        _lib.check(lib.ms_clamp_dropout_backward(ptr(dys[i]), ptr(ys[i]), ptr(outs[i]), n, LO, HI, thr, scale, 7, i, st()),
                   "ms_clamp_dropout_backward")

    arms = {"project_forward": loop(fwd), "project_clamp_backward": loop(bwd),
            "torch_dropout_forward": loop(lambda i: torch.nn.functional.dropout(xs[i], P, True)),
            "torch_dropout_backward": loop(lambda i: torch.autograd.grad(dropped[i], leaves[i], dys[i], retain_graph=True)),
            "torch_where_gate": loop(lambda i: torch.where((ys[i] > LO) & (ys[i] < HI), dys[i], zero))}
    per_element = {"project_forward": 8, "project_clamp_backward": 12, "torch_dropout_forward": 8, "torch_dropout_backward": 8,
                   "torch_where_gate": 12}
    return arms, per_element


def ds1_arms():
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    from myrtlespeech_amd.model import dropout
    from myrtlespeech_amd.model.deep_speech_1 import DeepSpeech1
    torch.manual_seed(0)
    model = DeepSpeech1(F, C, HID, V, P)
    dropout.attach(model, dropout.DropoutGenerator(1))
    ctc = CTCLoss()
    x = torch.randn(N, C, F, T).cuda()
    lens = torch.tensor([T])
    y, y_lens = torch.randint(1, V, (N, 40)), torch.tensor([40])
    params = list(model.parameters())

    def step(training):
        def run():
            model.train(training)
            for q in params:
                q.grad = None
            (out, out_lens), _ = model((x, lens), differentiable=True)
            ctc((out, out_lens), (y, y_lens)).backward()
        return run

    return {"ds1_step_with_dropout": step(True), "ds1_step_in_eval_mode": step(False)}


def error_records():
    """tests/test_dropout_train_gpu.py's cases: the worst multiples of torch's float32 CPU error."""
    import test_dropout_train_gpu as D
    import test_ds1_train_gpu as D1
    inner = D1.report
    worst = {}

    def recording(name, got, want, f32):
        worst[name] = round(inner(name, got, want, f32), 3)
        return worst[name]

    D1.report = recording
    try:
        D.test_ds1_gradients_under_dropout_match_the_masked_float64_chain()
        D.test_two_layer_stacks_with_inter_layer_dropout("bilstm")
        D.test_two_layer_stacks_with_inter_layer_dropout("gru")
        D.test_ds2_miniature_with_fully_connected_dropout()
    finally:
        D1.report = inner
    return {"worst_multiples_of_torch_float32_error": worst,
            "multiples": "device error over torch float32 CPU autograd error on the same masked chain, both against float64 and "
                         "relative to the tensor's largest magnitude"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dropout_time: a HIP device is required; there is no CPU path")
    calls = SETS * ROUNDS
    out = {"tool": "tools/dropout_time.py", "commit": a.commit, "torch": torch.__version__, "p": P, "clamp": [LO, HI],
           "hbm_peak_gbs": bench.HBM_PEAK_GBS, "buffer_sets_per_arm": SETS, "calls_per_sample": calls,
           "statistic": f"host clock around {calls} calls over {SETS} buffer sets ending in a device synchronise, per call, ms; the "
                        "arms of a shape alternate in one process after one untimed sample each; median of the repeats",
           "shapes": {}}
    for shape in SHAPES:
        print(f"dropout_time: {shape}", file=sys.stderr, flush=True)
        arms, per_element = kernel_arms(shape)
        ms = timed(arms, a.repeats, calls)
        n = shape[0] * shape[1]
        rec = {"elements": n, "arms": {}}
        for k, v in ms.items():
            med = statistics.median(v)
            rec["arms"][k] = {"ms": spread(v), "bytes_per_element": per_element[k], "bytes": per_element[k] * n,
                              "fraction_of_hbm_rate": round(per_element[k] * n / (med * 1e-3) / (bench.HBM_PEAK_GBS * 1e9), 4)}
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec["project_forward_over_torch_dropout_forward"] = round(med["project_forward"] / med["torch_dropout_forward"], 3)
        rec["project_clamp_backward_over_torch_where_gate_plus_dropout_backward"] = round(
            med["project_clamp_backward"] / (med["torch_where_gate"] + med["torch_dropout_backward"]), 3)
        out["shapes"]["x".join(map(str, shape))] = rec
        del arms
        torch.cuda.empty_cache()
    print("dropout_time: one DeepSpeech1 training step", file=sys.stderr, flush=True)
    ms = timed(ds1_arms(), a.repeats)
    out["deep_speech_1"] = {f"{k}_ms": spread(v) for k, v in ms.items()}
    out["deep_speech_1"]["input"] = [N, C, F, T]
    out["deep_speech_1"]["dropout_share_ms"] = round(statistics.median(ms["ds1_step_with_dropout"])
                                                     - statistics.median(ms["ds1_step_in_eval_mode"]), 4)
    out["errors"] = error_records()
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
