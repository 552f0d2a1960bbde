#!/usr/bin/env python3
"""What a CTC forced alignment costs beside the CTC loss forward, arms alternating in one process.

  align_logits     ``ms_ctc_align`` on logits (its own log-softmax normalisers, the Viterbi scan, back-trace, spans)
  align_log_probs  ``ms_ctc_align`` on log-probabilities (MS_CTC_LOG_PROBS_IN)
  loss_forward     ``ms_ctc_loss_forward`` (reduction none) on the same logits and targets: the sibling scan, the yardstick
  host_numpy       the numpy restatement of the specification (tests/ctc_align_ref.py, float32): what a user has without it
  aligner_call     ``CTCForcedAligner.forward`` end to end: staged upload, the two launches, one read-back, the Python objects

at ``randn(501, 32, V) * 3`` with 120 labels per utterance, V = 29 and V = 5000.  A device arm is the host clock around
``--inner`` back-to-back calls that end in a device synchronise, divided by the calls.  The tool also aligns the small random
cases of tests/test_ctc_align_gpu.py's logits-mode test and records the worst ratios to the derived bound
B = 8 T 2^-24 max(1, |S*|).

    python tools/ctc_align_time.py [--repeats 9] [--inner 10] [--out profiles/ctc_align_time.json] [--kernel-stats CSV]
    python tools/ctc_align_time.py --probe 29     # the launches alone at [501, 32, 29], for the profiler

Kernel times come from a separate run, ``tools/rocprof_script.sh align tools/ctc_align_time.py --probe 29`` (rocprofv3
--kernel-trace --stats); ``--kernel-stats`` copies that run's line per kernel into the JSON.
There is no CPU path: without a HIP device the tool fails.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import numpy as np  # noqa: E402
import torch  # noqa: E402

T, N, LABELS, BLANK = 501, 32, 120, 0
LOG_PROBS_IN = 2


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


class Case:
    """One shape's device buffers and the three ABI calls on them."""

    def __init__(self, V, seed=7):
        from myrtlespeech_amd import _lib
        self.lib, self._lib, self.V = _lib.load(), _lib, V
        g = torch.Generator().manual_seed(seed)
        self.x = (torch.randn(T, N, V, generator=g) * 3).cuda()
        self.lp = torch.log_softmax(self.x, -1)
        self.targets = torch.randint(1, V, (N, LABELS), generator=g, dtype=torch.int32)
        i32 = lambda v: torch.as_tensor(v, dtype=torch.int32).cuda()   # noqa: E731
        self.y, self.off = self.targets.reshape(-1).cuda(), i32(np.arange(N) * LABELS)
        self.xl, self.yl = i32([T] * N), i32([LABELS] * N)
        self.score = torch.empty(N, dtype=torch.float32, device="cuda")
        self.state = torch.empty((N, T), dtype=torch.int32, device="cuda")
        self.start = torch.empty((N, LABELS), dtype=torch.int32, device="cuda")
        self.end, self.logp = torch.empty_like(self.start), torch.empty((N, LABELS), dtype=torch.float32, device="cuda")
        self.nll = torch.empty(N, dtype=torch.float32, device="cuda")
        s_max = 2 * LABELS + 1
        self.ws_a = torch.empty(max(self.lib.ms_ctc_align_workspace_bytes(T, N, V, s_max), 256), dtype=torch.uint8, device="cuda")
        self.ws_l = torch.zeros(self.lib.ms_ctc_loss_workspace_bytes(T, N, V, s_max), dtype=torch.uint8, device="cuda")

    def align(self, log_probs):
        L, p = self._lib, self._lib.ptr
        L.check(self.lib.ms_ctc_align(p(self.lp if log_probs else self.x), p(self.xl), p(self.y), p(self.off), p(self.yl),
                                      p(self.score), p(self.state), p(self.start), p(self.end), p(self.logp), T, N, self.V,
                                      LABELS, BLANK, LOG_PROBS_IN if log_probs else 0, p(self.ws_a), self.ws_a.numel(),
                                      L.stream_ptr()), "ms_ctc_align")

    def loss(self):
        L, p = self._lib, self._lib.ptr
        L.check(self.lib.ms_ctc_loss_forward(p(self.x), p(self.xl), p(self.y), p(self.off), p(self.yl), p(self.nll), None, T, N,
                                             self.V, 2 * LABELS + 1, BLANK, 0, 0, p(self.ws_l), self.ws_l.numel(),
                                             L.stream_ptr()), "ms_ctc_loss_forward")


def host_numpy(lp_host, targets):
    import ctc_align_ref as R
    return [R.align(lp_host[:, n], targets[n], BLANK, log_probs=True, dtype=np.float32) for n in range(len(targets))]


def logits_mode_ratios():
    """The cases of tests/test_ctc_align_gpu.py::test_logits_mode_within_the_derived_bound; worst ratios to the bound."""
    import ctc_align_ref as R
    import test_ctc_align_gpu as G
    worst = {"optimum_gap_over_B": 0.0, "score_minus_rescoring_over_B": 0.0, "token_logp_over_B": 0.0, "utterances": 0,
             "paths_that_differ_from_the_float64_optimum": 0}
    for scale in (1.0, 4.0, 12.0):
        rng = np.random.default_rng(100 + int(scale))
        t, v, blank, n_utt = 120, 30, 29, 16
        x = (rng.standard_normal((t, n_utt, v)) * scale).astype(np.float32)
        in_lens = [int(q) for q in rng.integers(40, t + 1, size=n_utt)]
        in_lens[0] = t
        targets = [G.random_target(rng, int(rng.integers(1, tn // 2)), v, blank) for tn in in_lens]
        score, state, _, _, logp = G.run_abi(x, in_lens, targets, blank, False)
        for n, tgt in enumerate(targets):
            tn, ext = in_lens[n], R.extended(tgt, blank)
            lp64, _ = R.log_softmax(x[:tn, n].astype(np.float64), np.float64)
            best = R.align(lp64, tgt, blank, log_probs=True, dtype=np.float64)
            bound = 8 * tn * 2.0 ** -24 * max(1.0, abs(float(best.score)))
            rescored = R.rescore(state[n, :tn], lp64, ext)
            _, _, logp64 = R.spans(state[n, :tn], lp64, ext, np.float64)
            worst["optimum_gap_over_B"] = max(worst["optimum_gap_over_B"], (float(best.score) - rescored) / bound)
            worst["score_minus_rescoring_over_B"] = max(worst["score_minus_rescoring_over_B"], abs(float(score[n]) - rescored) / bound)
            worst["token_logp_over_B"] = max(worst["token_logp_over_B"],
                                             float(np.max(np.abs(logp[n, :len(tgt)].astype(np.float64) - logp64))) / bound)
            worst["utterances"] += 1
            worst["paths_that_differ_from_the_float64_optimum"] += int(state[n, :tn].tolist() != best.states.tolist())
    return {k: (round(v, 5) if isinstance(v, float) else v) for k, v in worst.items()}


def kernel_stat_lines(path):
    """The rows of a rocprofv3 kernel_stats.csv that belong to the aligner and to the loss forward."""
    keep = ("ctc_align", "ctc_alpha", "ctc_normalise")
    with open(path, newline="") as f:
        return [row for row in csv.DictReader(f) if any(k in row.get("Name", "") for k in keep)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--probe", type=int, default=0, metavar="V",
                    help="20 calls of every device arm at [501, 32, V] and nothing else (for the profiler)")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a profiler run of --probe")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_align_time: a HIP device is required; there is no CPU path")
    from myrtlespeech_amd.post_process import CTCForcedAligner
    from myrtlespeech_amd.post_process import ctc_aligner as A
    if a.probe:
        c = Case(a.probe)
        for _ in range(20):
            c.align(False)
            c.align(True)
            c.loss()
        torch.cuda.synchronize()
        return
    out = {"tool": "tools/ctc_align_time.py", "commit": a.commit, "frames": T, "batch": N, "labels": LABELS,
           "statistic": f"host clock around {a.inner} back-to-back calls ending in a device synchronise, per call, ms; the "
                        "arms alternate in one process after one untimed call each; host_numpy and aligner_call are single calls",
           "logits_mode_worst_ratios_to_the_bound": logits_mode_ratios()}
    for V in (29, 5000):
        c = Case(V)
        arms = {"align_logits": lambda: c.align(False), "align_log_probs": lambda: c.align(True), "loss_forward": c.loss}
        targets = c.targets.tolist()
        lp_host = c.lp.cpu().numpy()
        aligner = CTCForcedAligner(BLANK, log_probs=True)
        lens, yl = torch.full((N,), T), torch.full((N,), LABELS)
        for fn in arms.values():                                              # untimed
            fn()
        torch.cuda.synchronize()
        c.align(True)
        torch.cuda.synchronize()
        dev_score, dev_state = c.score.cpu().numpy(), c.state.cpu().numpy()
        ref = host_numpy(lp_host, targets)
        if not all(r.states is not None and float(r.score) == float(dev_score[n]) and r.states.tolist() == dev_state[n].tolist()
                   for n, r in enumerate(ref)):
            sys.exit(f"ctc_align_time: V = {V}: the device and the numpy restatement disagree")
        got = aligner(c.lp, lens, c.targets, yl)
        if [g.score for g in got] != [float(s) for s in dev_score]:
            sys.exit(f"ctc_align_time: V = {V}: CTCForcedAligner and the ABI call disagree")
        c.loss()
        c.align(False)
        torch.cuda.synchronize()
        if not bool((c.score.cpu() <= -c.nll.cpu() * (1 - 2e-5) + 1e-2).all()):
            sys.exit(f"ctc_align_time: V = {V}: a best path beats the sum over paths")
        ms = {k: [] for k in list(arms) + ["host_numpy", "aligner_call"]}
        for rep in range(a.repeats):
            for k, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    fn()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / a.inner)
            t0 = time.perf_counter()
            aligner(c.lp, lens, c.targets, yl)
            ms["aligner_call"].append((time.perf_counter() - t0) * 1e3)
            if rep < 3:
                t0 = time.perf_counter()
                host_numpy(lp_host, targets)
                ms["host_numpy"].append((time.perf_counter() - t0) * 1e3)
        rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
        for k in arms:
            rec[f"{k}_us_per_frame"] = round(statistics.median(ms[k]) * 1e3 / T, 4)
        rec["align_logits_over_loss_forward"] = round(statistics.median(ms["align_logits"]) / statistics.median(ms["loss_forward"]), 2)
        rec["host_numpy_over_align_log_probs"] = round(statistics.median(ms["host_numpy"]) / statistics.median(ms["align_log_probs"]), 1)
        rec["back_pointers"] = "LDS" if A.backpointers_in_lds(T, LABELS) else "global workspace"
        rec["back_pointer_bytes_per_utterance"] = T * A.backpointer_row_bytes(LABELS)
        out[f"[{T}, {N}, {V}] x {LABELS} labels"] = rec
    if a.kernel_stats:
        out["kernel_stats_source"] = "rocprofv3 --kernel-trace --stats over `tools/ctc_align_time.py --probe 29` (a run of its own)"
        out["kernel_stats"] = kernel_stat_lines(a.kernel_stats)
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
