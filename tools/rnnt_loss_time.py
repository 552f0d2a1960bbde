#!/usr/bin/env python3
"""What the transducer loss costs: forward and forward + backward, arms alternating in one process.

  forward           ``ms_rnnt_loss_forward``  (normaliser pass over the logits, then the alpha / beta lattice pass)
  forward_backward  the same followed by ``ms_rnnt_loss_backward`` (the gradient pass: logits in, grad out)

at ``3 randn`` logits of ``[16, 501, 121, 29]`` (a character model) and ``[8, 250, 61, 1024]`` (a word-piece model), every
utterance full length.  An arm is the host clock around ``--inner`` back-to-back calls that end in a device synchronise,
divided by the calls.  Beside each time stand the bytes the pass has to move -- the forward reads the logits once, the
backward reads them once and writes the gradient once -- and the time those bytes take at the HBM peak read from the device
(memory clock x bus width x 2; the nominal 8 TB/s when the device does not say).  The tool also runs the cases of
tests/test_rnnt_loss_gpu.py and records the device's worst ratios to the derived bounds.

    python tools/rnnt_loss_time.py [--repeats 9] [--inner 10] [--out profiles/rnnt_loss_time.json] [--kernel-stats CSV]
    python tools/rnnt_loss_time.py --probe 0        # 20 forward + backward calls at shape 0 and nothing else, for the profiler

Per-pass times come from a separate run, ``tools/rocprof_script.sh rnnt_loss tools/rnnt_loss_time.py --probe 0`` (rocprofv3
--kernel-trace --stats; ``--probe 1`` for the second shape); ``--kernel-stats`` (repeatable, ``SHAPE=CSV``) copies that run's
line per kernel into the JSON and derives the lattice pass's microseconds per anti-diagonal.
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

SHAPES = [(16, 501, 121, 29), (8, 250, 61, 1024)]
NOMINAL_HBM_GBS = 8000.0


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def hbm_peak_gbs():
    """(GB/s, where the figure comes from)."""
    p = torch.cuda.get_device_properties(0)
    clock_khz, width = getattr(p, "memory_clock_rate", 0), getattr(p, "memory_bus_width", 0)
    if clock_khz and width:
        return 2.0 * clock_khz * 1e3 * width / 8 / 1e9, f"2 x memory_clock_rate ({clock_khz} kHz) x memory_bus_width ({width} bit)"
    return NOMINAL_HBM_GBS, "nominal (the device properties carry no memory clock / bus width)"


class Case:
    """One shape's device buffers and the two ABI calls on them."""

    def __init__(self, shape, seed=7):
        from myrtlespeech_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.N, self.T, self.U1, self.V1 = shape
        N, T, U1, V1 = shape
        self.blank = V1 - 1
        g = torch.Generator().manual_seed(seed)
        self.x = torch.empty(shape, dtype=torch.float32, device="cuda")
        for n in range(N):                                               # (filled by utterance: the host copy stays small)
            self.x[n] = (torch.randn((T, U1, V1), generator=g) * 3).cuda()
        i32 = lambda v: torch.as_tensor(v, dtype=torch.int32).cuda()     # noqa: E731
        self.y = torch.randint(0, V1 - 1, (N, U1 - 1), generator=g, dtype=torch.int32).reshape(-1).cuda()
        self.xl, self.yl = i32([T] * N), i32([U1 - 1] * N)
        self.nll = torch.empty(N, dtype=torch.float32, device="cuda")
        self.lattice = torch.empty(self.lib.ms_rnnt_loss_lattice_bytes(N, T, U1) // 4, dtype=torch.float32, device="cuda")
        self.ws = torch.empty(self.lib.ms_rnnt_loss_workspace_bytes(N, T, U1, V1), dtype=torch.uint8, device="cuda")
        self.grad_nll = torch.full((N,), 1.0 / N, dtype=torch.float32, device="cuda")
        self.grad = torch.empty_like(self.x)

    def forward(self):
        L, p = self._lib, self._lib.ptr
        L.check(self.lib.ms_rnnt_loss_forward(p(self.x), p(self.xl), p(self.y), p(self.yl), p(self.nll), p(self.lattice), self.N,
                                              self.T, self.U1, self.V1, self.blank, p(self.ws), self.ws.numel(), L.stream_ptr()),
                "ms_rnnt_loss_forward")

    def backward(self):
        L, p = self._lib, self._lib.ptr
        L.check(self.lib.ms_rnnt_loss_backward(p(self.x), p(self.xl), p(self.y), p(self.yl), p(self.nll), p(self.lattice),
                                               p(self.grad_nll), p(self.grad), self.N, self.T, self.U1, self.V1, self.blank,
                                               L.stream_ptr()), "ms_rnnt_loss_backward")

    def forward_backward(self):
        self.forward()
        self.backward()


def case_ratios():
    """The cases of tests/test_rnnt_loss_gpu.py::test_case_within_the_bounds; the device's worst ratios to the bounds."""
    import test_rnnt_loss_gpu as G
    worst = {}
    for name in sorted(G.CASES):
        c = G.CASES[name]
        n_utt = len(c["in_lens"])
        grad_nll = np.random.default_rng(17).uniform(0.5, 2.0, size=n_utt).astype(np.float32) * np.where(np.arange(n_utt) % 2, -1, 1)
        w = G.check_against(G.ref64(name), G.run_case(c, grad_nll=grad_nll), c["in_lens"], c["tgt_lens"], grad_nll, name)
        worst[name] = {k: round(v, 5) for k, v in w.items()}
    worst["all"] = {k: max(w[k] for w in worst.values()) for k in ("nll", "alpha", "beta", "grad", "Z")}
    worst["bounds"] = ("B_n = 8 (T_n + U_n) 2^-24 max(1, |nll_n|) for nll, alpha, beta; 4 B_n |grad_nll| for the gradient; "
                       "16 2^-24 max(1, |Z|) for Z; against the float64 restatement tests/rnnt_loss_ref.py")
    return worst


def kernel_stat_lines(path):
    """The rows of a rocprofv3 kernel_stats.csv that belong to the loss."""
    with open(path, newline="") as f:
        return [row for row in csv.DictReader(f) if "rnnt_loss" in row.get("Name", "")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--probe", type=int, default=None, metavar="SHAPE",
                    help="20 forward + backward calls at SHAPES[SHAPE] and nothing else (for the profiler)")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="SHAPE=CSV",
                    help="kernel_stats.csv of a profiler run of --probe SHAPE")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rnnt_loss_time: a HIP device is required; there is no CPU path")
    if a.probe is not None:
        c = Case(SHAPES[a.probe])
        for _ in range(20):
            c.forward_backward()
        torch.cuda.synchronize()
        return
    peak, peak_source = hbm_peak_gbs()
    out = {"tool": "tools/rnnt_loss_time.py", "commit": a.commit,
           "statistic": f"host clock around {a.inner} back-to-back calls ending in a device synchronise, per call, ms; the arms "
                        "alternate in one process after one untimed call each",
           "hbm_peak_GBs": round(peak, 1), "hbm_peak_source": peak_source,
           "worst_ratios_to_the_bounds": case_ratios()}
    stats = dict(s.split("=", 1) for s in a.kernel_stats)
    for i, shape in enumerate(SHAPES):
        c = Case(shape)
        N, T, U1, V1 = shape
        arms = {"forward": c.forward, "forward_backward": c.forward_backward}
        for fn in arms.values():                                              # untimed
            fn()
        torch.cuda.synchronize()
        nll = c.nll.cpu().numpy()
        row_sums = float(c.grad.sum(-1).abs().max())
        if not np.isfinite(nll).all() or not (nll > 0).all() or row_sums > 1e-4:
            sys.exit(f"rnnt_loss_time: {shape}: nll {nll.tolist()} / gradient row sums {row_sums} are not what a loss gives")
        ms = {k: [] for k in arms}
        for _ in range(a.repeats):
            for k, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    fn()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / a.inner)
        logits_bytes = 4 * N * T * U1 * V1
        lattice_bytes, plane_bytes = 12 * N * T * U1, c.ws.numel()
        rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
        rec["backward_ms_by_difference"] = round(statistics.median(ms["forward_backward"]) - statistics.median(ms["forward"]), 4)
        rec["bytes"] = {"normalise_pass": logits_bytes + lattice_bytes // 3 + plane_bytes,
                        "lattice_pass": plane_bytes + 2 * lattice_bytes // 3,
                        "gradient_pass": 2 * logits_bytes + lattice_bytes,
                        "note": "normalise: logits in, Z and the b / e planes out; lattice: b / e in, alpha and beta out; "
                                "gradient: logits and the lattice in, grad out"}
        rec["ms_at_hbm_peak"] = {k: round(v / (peak * 1e6), 4) for k, v in rec["bytes"].items() if k != "note"}
        rec["anti_diagonals"] = T + U1 - 1
        rec["mean_nll"] = round(float(nll.mean()), 3)
        if str(i) in stats:
            rows = kernel_stat_lines(stats[str(i)])
            rec["kernel_stats_source"] = (f"rocprofv3 --kernel-trace --stats over `tools/rnnt_loss_time.py --probe {i}` (a run of "
                                          "its own; 20 calls of each pass)")
            rec["kernel_stats"] = rows
            for row in rows:
                if "lattice" in row.get("Name", ""):
                    avg_ns = float(row.get("AverageNs") or row.get("Average") or 0)
                    rec["lattice_pass_us_per_anti_diagonal"] = round(avg_ns / 1e3 / (T + U1 - 1), 4)
        out[str(list(shape))] = rec
        del c
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
