"""Times the bidirectional LSTM backward at the DeepSpeech1 shape tools/bench_configs.py times (BASELINE configs[0]:
n_hidden 1024, one 4 s clip [1, 19, 26, 201] -> a BiLSTM of In 2048, H 1024 over T 201, N 1).

  steps_bidir                 ``ms_lstm_backward_steps_bidir``: both directions in max_len + 1 launches of grid (H / 32, 2)
  steps_once_per_direction    the unchanged ``ms_lstm_backward_steps`` called once per direction on the same gates / c planes
                              (2 (max_len + 1) launches of grid H / 32): the work as it had to be issued before.  Its second
                              call walks the reverse plane in the forward order -- the same launches, loads and arithmetic,
                              not the reverse direction's values
  torch_bilstm_forward_backward   ``torch.nn.LSTM(bidirectional=True)`` on the device, same shape, forward + backward
  ds1_forward_ctc_backward    ``DeepSpeech1.forward(differentiable=True)`` + ``CTCLoss`` + backward, one step

The arms alternate in one process after one untimed call each; the median of ``--repeats`` (7) is the figure.  Expectation to
confirm or refute: steps_bidir is below steps_once_per_direction, because the loop is bound by launch latency and it halves
the launches.  It also runs tests/test_bilstm_backward_gpu.py's cases and tests/test_ds1_train_gpu.py and records the worst
ratios to the derived bounds and the worst multiples of torch's float32 CPU error.  There is no CPU path.

    python tools/bilstm_backward_time.py [--repeats 7] [--out profiles/bilstm_backward_time.json]
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

N, C, F, T, HID, V = 1, 19, 26, 201, 1024, 29
IN = 2 * HID


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
        sys.exit(f"bilstm_backward_time: {what} returned {rc}")


def step_arms():
    from myrtlespeech_amd import _lib
    lib, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(s, generator=g).cuda()      # noqa: E731
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")      # noqa: E731
    k = 1.0 / HID ** 0.5
    x = r(T, N, IN)
    h = [torch.tanh(r(T, N, HID)) for _ in (0, 1)]
    w = [dict(w_ih=k * r(4 * HID, IN), w_hh=k * r(4 * HID, HID), b_ih=k * r(4 * HID), b_hh=k * r(4 * HID)) for _ in (0, 1)]
    gates, c = e(2, T, N, 4 * HID), e(2, T, N, HID)
    ws = torch.empty(lib.ms_lstm_recompute_workspace_bytes(T, N, HID), dtype=torch.uint8, device="cuda")
    for d in (0, 1):
        die(lib.ms_lstm_recompute_dir(p(x), p(h[d]), p(None), p(None), p(None), p(w[d]["w_ih"]), p(w[d]["w_hh"]), p(w[d]["b_ih"]),
                                      p(w[d]["b_hh"]), p(gates[d]), p(c[d]), T, N, IN, HID, d, p(ws), ws.numel(), st()),
            "ms_lstm_recompute_dir")
    d_out = r(T, N, 2 * HID)
    halves = [d_out[..., :HID].contiguous(), d_out[..., HID:].contiguous()]
    dG, d_h0, d_c0, d_b = e(2, T, N, 4 * HID), e(2, N, HID), e(2, N, HID), e(2, 4 * HID)

    def bidir():
        die(lib.ms_lstm_backward_steps_bidir(p(gates), p(c), p(None), p(w[0]["w_hh"]), p(w[1]["w_hh"]), p(d_out), p(None), p(None),
                                             p(None), T, p(dG), p(d_h0), p(d_c0), p(d_b), T, N, HID, st()),
            "ms_lstm_backward_steps_bidir")

    def per_direction():
        for d in (0, 1):
            die(lib.ms_lstm_backward_steps(p(gates[d]), p(c[d]), p(None), p(w[d]["w_hh"]), p(halves[d]), p(None), p(None), p(None), T,
                                           p(dG[d]), p(d_h0[d]), p(d_c0[d]), p(d_b[d]), T, N, HID, st()), "ms_lstm_backward_steps")

    ref = torch.nn.LSTM(IN, HID, bidirectional=True).cuda()
    params = list(ref.parameters())

    def torch_bilstm():
        for q in params:
            q.grad = None
        ref(x)[0].sum().backward()

    return {"steps_bidir": bidir, "steps_once_per_direction": per_direction, "torch_bilstm_forward_backward": torch_bilstm}


def ds1_arm():
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    from myrtlespeech_amd.model.deep_speech_1 import DeepSpeech1
    torch.manual_seed(0)
    model = DeepSpeech1(F, C, HID, V, 0.25).eval()
    ctc = CTCLoss()
    x = torch.randn(N, C, F, T).cuda()
    lens = torch.tensor([T])
    y, y_lens = torch.randint(1, V, (N, 40)), torch.tensor([40])
    params = list(model.parameters())

    def step():
        for q in params:
            q.grad = None
        (out, out_lens), _ = model((x, lens), differentiable=True)
        ctc((out, out_lens), (y, y_lens)).backward()

    return {"ds1_forward_ctc_backward": step}


def error_records():
    """The cases of the two GPU test files: worst ratios to the derived bounds, worst multiples of torch's float32 error."""
    import test_bilstm_backward_gpu as A
    import test_ds1_train_gpu as D
    for name in A.B.CASE_NAMES:
        A.test_case_bounds_and_bits(name)
    inner = D.report
    worst = {}

    def recording(name, got, want, f32):
        worst[name] = round(inner(name, got, want, f32), 3)
        return worst[name]

    D.report = recording
    try:
        D.test_rnn_train_two_bidirectional_layers_ragged()
        D.test_ds1_ctc_loss_gradients_reach_every_parameter()
    finally:
        D.report = inner
    return {"worst_ratios_to_the_bounds": {k: round(float(v), 5) for k, v in A.worst.items()},
            "worst_multiples_of_torch_float32_error": worst, "bounds": "tests/bilstm_backward_ref.py",
            "multiples": "device error over torch float32 CPU autograd error, both against float64 and relative to the tensor's "
                         "largest magnitude"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilstm_backward_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bilstm_backward_time: a HIP device is required; there is no CPU path")
    out = {"tool": "tools/bilstm_backward_time.py", "commit": a.commit,
           "shape": {"N": N, "T": T, "input": [N, C, F, T], "lstm_input": IN, "hidden": HID, "symbols": V},
           "statistic": "host clock around calls ending in a device synchronise, per call, ms; the arms alternate in one process "
                        "after one untimed call each; median of the repeats"}
    ms = timed(step_arms(), a.repeats)
    rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
    bi, two = statistics.median(ms["steps_bidir"]), statistics.median(ms["steps_once_per_direction"])
    rec["launches"] = {"steps_bidir": T + 1, "steps_once_per_direction": 2 * (T + 1)}
    rec["us_per_launch"] = {"steps_bidir": round(bi / (T + 1) * 1e3, 2), "steps_once_per_direction": round(two / (2 * (T + 1)) * 1e3, 2)}
    rec["bidir_over_once_per_direction"] = round(bi / two, 3)
    out["backward_recurrence"] = rec
    out["deep_speech_1"] = {f"{k}_ms": spread(v) for k, v in timed(ds1_arm(), a.repeats).items()}
    out["errors"] = error_records()
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
