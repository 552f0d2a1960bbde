"""Times the HardLSTM backward beside the soft LSTM's on the same inputs: the recurrent layer of the DeepSpeech1 of
configs[0] -- H = 1024, bidirectional, input 2048 -- on one 2 s clip, [T, N] = [201, 1].

  recompute          ``ms_hard_lstm_recompute`` x 2 directions  beside  ``ms_lstm_recompute_dir`` x 2
  steps              ``ms_hard_lstm_backward_steps`` (ndir = 2) beside  ``ms_lstm_backward_steps_bidir``  (T + 1 launches each)
  training step      one whole DeepSpeech1 step (forward(differentiable=True) + CTCLoss + backward), ``hard_lstm=True`` with
                     ``bi_lstm.hard_backward = True`` beside the soft model; features [1, 1, 26 * 19, 201]

The arms of a pair alternate in one process after one untimed call each; a call is timed with the host clock around work that
ends in a device synchronise; the median of ``--repeats`` (7) is the figure, min and max beside it, and ``hard_over_soft`` the
ratio of the medians.  No thresholds: parity is the expectation (the products and the launches dominate, and the hard cell has
no expf / tanhf), and the numbers are the output.  It also runs the cases of tests/test_hard_lstm_backward_gpu.py and records
the worst ratios to the derived bounds.  There is no CPU path.

    python tools/hard_lstm_backward_time.py [--repeats 7] [--out profiles/hard_lstm_backward_time.json]
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

T, N, IN, HID = 201, 1, 2048, 1024
F_IN, V = 26 * 19, 29


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


def pair(ms):
    rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
    rec["hard_over_soft"] = round(statistics.median(ms["hard"]) / statistics.median(ms["soft"]), 3)
    return rec


def progress(what):
    print(f"hard_lstm_backward_time: {what}", file=sys.stderr, flush=True)


def die(rc, what):
    if rc != 0:
        sys.exit(f"hard_lstm_backward_time: {what} returned {rc}")


def abi_arms():
    """(recompute arms, steps arms) on the same x, h, weights and output gradient."""
    from myrtlespeech_amd import _lib
    lib, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(s, generator=g).cuda()      # noqa: E731
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")      # noqa: E731
    k = 1.0 / HID ** 0.5
    x, h = r(T, N, IN), torch.tanh(r(2, T, N, HID))
    w = [(k * r(4 * HID, IN), k * r(4 * HID, HID), k * r(4 * HID), k * r(4 * HID)) for _ in (0, 1)]
    gates, c = {n: e(2, T, N, 4 * HID) for n in ("hard", "soft")}, {n: e(2, T, N, HID) for n in ("hard", "soft")}
    ws = torch.empty(lib.ms_lstm_recompute_workspace_bytes(T, N, HID), dtype=torch.uint8, device="cuda")
    d_out = r(T, N, 2 * HID)
    dA, d_h0, d_c0, d_b = e(2, T, N, 4 * HID), e(2, N, HID), e(2, N, HID), e(2, 4 * HID)

    def hard_recompute():
        for d in (0, 1):
            die(lib.ms_hard_lstm_recompute(p(x), p(h[d]), p(None), p(None), p(w[d][0]), p(w[d][1]), p(w[d][2]), p(w[d][3]),
                                           p(gates["hard"][d]), p(c["hard"][d]), T, N, IN, HID, d, p(ws), ws.numel(), st()),
                "ms_hard_lstm_recompute")

    def soft_recompute():
        for d in (0, 1):
            die(lib.ms_lstm_recompute_dir(p(x), p(h[d]), p(None), p(None), p(None), p(w[d][0]), p(w[d][1]), p(w[d][2]), p(w[d][3]),
                                          p(gates["soft"][d]), p(c["soft"][d]), T, N, IN, HID, d, p(ws), ws.numel(), st()),
                "ms_lstm_recompute_dir")

    def hard_steps():
        die(lib.ms_hard_lstm_backward_steps(p(gates["hard"]), p(c["hard"]), p(None), p(w[0][1]), p(w[1][1]), p(d_out), p(None), p(None),
                                            p(dA), p(d_h0), p(d_c0), p(d_b), T, N, HID, 2, st()), "ms_hard_lstm_backward_steps")

    def soft_steps():
        die(lib.ms_lstm_backward_steps_bidir(p(gates["soft"]), p(c["soft"]), p(None), p(w[0][1]), p(w[1][1]), p(d_out), p(None), p(None),
                                             p(None), T, p(dA), p(d_h0), p(d_c0), p(d_b), T, N, HID, st()),
            "ms_lstm_backward_steps_bidir")

    return {"hard": hard_recompute, "soft": soft_recompute}, {"hard": hard_steps, "soft": soft_steps}


def model_arms():
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    from myrtlespeech_amd.model.deep_speech_1 import DeepSpeech1
    ctc = CTCLoss()
    x = torch.randn(N, 1, F_IN, T).cuda()
    lens = torch.full((N,), T, dtype=torch.int64)
    y, y_lens = torch.randint(1, V, (N, 30)), torch.full((N,), 30, dtype=torch.int64)
    arms = {}
    for name, hard in (("hard", True), ("soft", False)):
        torch.manual_seed(7)
        model = DeepSpeech1(F_IN, 1, HID, V, 0.0, hard_lstm=hard).eval()
        model.bi_lstm.check_status = False
        if hard:
            model.bi_lstm.hard_backward = True
        params = list(model.parameters())

        def step(model=model, params=params):
            for q in params:
                q.grad = None
            (out, out_lens), _ = model((x, lens), differentiable=True)
            ctc((out, out_lens), (y, y_lens)).backward()

        arms[name] = step
    return arms


def error_records():
    """The cases of tests/test_hard_lstm_backward_gpu.py: the worst ratios to the derived bounds."""
    import test_hard_lstm_backward_gpu as A
    A.test_kink_table_on_the_device_is_torch_float32_autograd_bit_for_bit()
    for name in A.R.CASE_NAMES:
        A.test_case_bounds_and_bits(name)
    return {"worst_ratios_to_the_bounds": {k: round(float(v), 5) for k, v in A.worst.items()},
            "bounds": "tests/hard_lstm_backward_ref.py", "kink_table": "bit-equal to torch float32 autograd"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hard_lstm_backward_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hard_lstm_backward_time: a HIP device is required; there is no CPU path")
    out = {"tool": "tools/hard_lstm_backward_time.py", "commit": a.commit,
           "shape": {"T": T, "N": N, "lstm_input": IN, "hidden": HID, "ndir": 2, "ds1_input": [N, 1, F_IN, T], "symbols": V},
           "statistic": "host clock around calls ending in a device synchronise, per call, ms; the two arms of a pair alternate in "
                        "one process after one untimed call each; median of the repeats; hard_over_soft = ratio of the medians"}
    progress("recompute and steps through the C ABI")
    rec, steps = abi_arms()
    out["recompute_both_directions"] = pair(timed(rec, a.repeats))
    out["backward_steps_bidirectional"] = dict(pair(timed(steps, a.repeats)), launches=T + 1, grid=[HID // 32, 2])
    del rec, steps
    torch.cuda.empty_cache()
    progress("one DeepSpeech1 training step, hard beside soft")
    out["deep_speech_1_training_step"] = pair(timed(model_arms(), a.repeats))
    torch.cuda.empty_cache()
    progress("the C-ABI test file's cases")
    out["errors"] = error_records()
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
