"""Times the GRU backward at the shape of the one DeepSpeech2 configuration the reference ships (2 x conv2d, 3 x GRU-2560
unidirectional, lookahead 80, FC 1024; 32 clips of 10 s: the stack sees GRU 640 -> 3 x 2560 on [T, N] = [501, 32]).

  gru_train_forward_backward      ``rnn_autograd.gru_train`` on the stack, forward + backward (sum of the output as the loss)
  torch_gru_forward_backward      ``torch.nn.GRU`` on the device, same shape and weights, forward + backward
  backward_steps_layer            ``ms_gru_backward_steps`` alone on one layer (T + 1 launches): the time per launch
  ds2_forward_ctc_backward        the shipped architecture, ``DeepSpeech2.forward(differentiable=True)`` with
                                  ``rnn.gru_backward = True`` + ``CTCLoss`` + backward, one whole training step

The arms of a group alternate in one process after one untimed call each (every shape warmed up); a call is timed with the host
clock around work that ends in a device synchronise; the median of ``--repeats`` (7) is the figure, min and max beside it.  It
also records the transient memory of one layer's backward (the allocator's peak over the stack's backward minus what was
allocated before it; about 16 H floats per (t, n) row), runs the cases of tests/test_gru_backward_gpu.py and
tests/test_gru_train_gpu.py and records the worst ratios to the derived bounds and the worst multiples of torch's float32 CPU
error.  No thresholds: the numbers are the output.  To read them: at H = 2560 the step grid is 80 workgroups on 256 CUs, and
each step streams w_hh's 79 MB.  There is no CPU path.

    python tools/gru_backward_time.py [--repeats 7] [--out profiles/gru_backward_time.json]
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

N, T, IN, HID, LAYERS, V = 32, 501, 640, 2560, 3, 29
F_IN, T_IN = 80, 1001


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


def progress(what):
    print(f"gru_backward_time: {what}", file=sys.stderr, flush=True)


def die(rc, what):
    if rc != 0:
        sys.exit(f"gru_backward_time: {what} returned {rc}")


def stack_arms():
    """(arms, a function measuring the transient memory of the stack's backward)."""
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.rnn_autograd import gru_train
    torch.manual_seed(0)
    rnn = RNN(RNNType.GRU, IN, HID, num_layers=LAYERS).eval()
    rnn.check_status = False
    ref = torch.nn.GRU(IN, HID, num_layers=LAYERS).cuda()
    ref.load_state_dict(rnn.rnn.state_dict())
    x = torch.randn(T, N, IN).cuda()
    lens = torch.full((N,), T, dtype=torch.int64)
    ours, theirs = list(rnn.parameters()), list(ref.parameters())

    def own():
        for q in ours:
            q.grad = None
        gru_train(rnn, x, lens)[0].sum().backward()

    def torch_gru():
        for q in theirs:
            q.grad = None
        ref(x)[0].sum().backward()

    def transient():
        for q in ours:
            q.grad = None
        loss = gru_train(rnn, x, lens)[0].sum()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        loss.backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    return {"gru_train_forward_backward": own, "torch_gru_forward_backward": torch_gru}, transient


def step_arm():
    from myrtlespeech_amd import _lib
    lib, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(s, generator=g).cuda()      # noqa: E731
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")      # noqa: E731
    k = 1.0 / HID ** 0.5
    x, h = r(T, N, HID), torch.tanh(r(1, T, N, HID))
    w_ih, w_hh, b_ih, b_hh = k * r(3 * HID, HID), k * r(3 * HID, HID), k * r(3 * HID), k * r(3 * HID)
    gates, q = e(1, T, N, 3 * HID), e(1, T, N, HID)
    ws = torch.empty(lib.ms_gru_recompute_workspace_bytes(T, N, HID), dtype=torch.uint8, device="cuda")
    die(lib.ms_gru_recompute(p(x), p(h[0]), p(None), p(None), p(w_ih), p(w_hh), p(b_ih), p(b_hh), p(gates[0]), p(q[0]), T, N, HID, HID, 0,
                             p(ws), ws.numel(), st()), "ms_gru_recompute")
    d_out = r(T, N, HID)
    dGi, dGh, d_h0, d_bi, d_bh = e(1, T, N, 3 * HID), e(1, T, N, 3 * HID), e(1, N, HID), e(1, 3 * HID), e(1, 3 * HID)

    def steps():
        die(lib.ms_gru_backward_steps(p(gates), p(q), p(h), p(None), p(w_hh), p(None), p(d_out), p(None), p(None), T, p(dGi), p(dGh),
                                      p(d_h0), p(d_bi), p(d_bh), T, N, HID, 1, st()), "ms_gru_backward_steps")

    return {"backward_steps_layer": steps}


def ds2_arm():
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    from myrtlespeech_amd.model.cnn import MaskConv2d, PaddingMode
    from myrtlespeech_amd.model.deep_speech_2 import DeepSpeech2
    from myrtlespeech_amd.model.fully_connected import FullyConnected
    from myrtlespeech_amd.model.lookahead import Lookahead
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.seq_len_wrapper import SeqLenWrapper

    def act():
        return SeqLenWrapper(torch.nn.Hardtanh(0.0, 20.0), torch.nn.Identity())
    torch.manual_seed(7)
    cnn = torch.nn.Sequential(MaskConv2d(1, 32, [41, 11], [2, 2], PaddingMode.SAME), act(),
                              MaskConv2d(32, 32, [21, 11], [2, 1], PaddingMode.SAME), act())
    rnn = RNN(RNNType.GRU, IN, HID, num_layers=LAYERS)
    la = torch.nn.Sequential(Lookahead(HID, 80), SeqLenWrapper(torch.nn.Identity(), torch.nn.Identity()))
    model = DeepSpeech2(cnn, rnn, la, FullyConnected(HID, V, 1, 1024, torch.nn.Hardtanh(0.0, 20.0))).eval()
    model.rnn.check_status = False
    model.rnn.gru_backward = True
    ctc = CTCLoss()
    x = torch.randn(N, 1, F_IN, T_IN).cuda()
    lens = torch.full((N,), T_IN, dtype=torch.int64)
    y, y_lens = torch.randint(1, V, (N, 120)), torch.full((N,), 120, dtype=torch.int64)
    params = list(model.parameters())

    def step():
        for q in params:
            q.grad = None
        (out, out_lens), _ = model((x, lens), differentiable=True)
        ctc((out, out_lens), (y, y_lens)).backward()

    return {"ds2_forward_ctc_backward": step}


def error_records():
    """The cases of the two GPU test files: worst ratios to the derived bounds, worst multiples of torch's float32 error."""
    import test_gru_backward_gpu as A
    import test_gru_train_gpu as D
    for name in A.G.CASE_NAMES:
        A.test_case_bounds_and_bits(name)
    A.test_backward_from_the_reference_gates()
    inner = D.report
    worst = {}

    def recording(name, got, want, f32, measured):
        worst[name] = round(inner(name, got, want, f32, measured), 3)
        return worst[name]

    D.report = recording
    try:
        for name in D.STACKS:
            D.test_stack_gradients(name)
        D.test_shipped_architecture_in_miniature_trains_under_ctc_loss()
    finally:
        D.report = inner
    return {"worst_ratios_to_the_bounds": {k: round(float(v), 5) for k, v in A.worst.items()},
            "c_abi_worst_multiples_of_torch_float32_error": {k: round(float(v), 3) for k, v in A.worst_multiple.items()},
            "worst_multiples_of_torch_float32_error": worst, "bounds": "tests/gru_backward_ref.py",
            "multiples": "device error over torch float32 CPU autograd error, both against float64 and relative to the tensor's "
                         "largest magnitude"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_backward_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gru_backward_time: a HIP device is required; there is no CPU path")
    out = {"tool": "tools/gru_backward_time.py", "commit": a.commit,
           "shape": {"N": N, "T": T, "gru_input": IN, "hidden": HID, "layers": LAYERS, "ds2_input": [N, 1, F_IN, T_IN], "symbols": V},
           "statistic": "host clock around calls ending in a device synchronise, per call, ms; the arms of a group alternate in one "
                        "process after one untimed call each; median of the repeats"}
    progress("stack forward + backward against torch.nn.GRU")
    arms, transient = stack_arms()
    ms = timed(arms, a.repeats)
    rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
    rec["gru_train_over_torch"] = round(statistics.median(ms["gru_train_forward_backward"]) / statistics.median(ms["torch_gru_forward_backward"]), 3)
    nbytes = transient()
    rec["backward_transient_bytes"] = int(nbytes)
    rec["backward_transient_floats_per_row_over_H"] = round(nbytes / 4 / (T * N) / HID, 2)
    out["stack"] = rec
    del arms, transient
    torch.cuda.empty_cache()
    progress("one layer's backward recurrence")
    steps = timed(step_arm(), a.repeats)["backward_steps_layer"]
    out["backward_recurrence"] = {"backward_steps_layer_ms": spread(steps), "launches": T + 1, "grid": [HID // 32, 1],
                                  "us_per_launch": round(statistics.median(steps) / (T + 1) * 1e3, 2),
                                  "w_hh_bytes_per_launch": 3 * HID * HID * 4}
    torch.cuda.empty_cache()
    progress("one training step of the shipped architecture")
    out["deep_speech_2"] = {f"{k}_ms": spread(v) for k, v in timed(ds2_arm(), a.repeats).items()}
    torch.cuda.empty_cache()
    progress("the GPU test files' cases")
    out["errors"] = error_records()
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
