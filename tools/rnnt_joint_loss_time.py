"""Times the fused transducer loss with gradient at [N, T, U + 1] = [16, 250, 121], J = 512, with 30 and with 5001 symbols:

  forward           ``ms_rnnt_joint_loss_forward`` (pack, cells, lattice: ms_rnnt_score's launches plus the Z plane)
  forward_backward  the same followed by ``ms_rnnt_joint_loss_backward`` with its preferred workspace
  at 30 symbols, through Python: ``rnnt_joint_loss`` + autograd beside the materialised route (torch float32 joint,
  ``RNNTLoss``, autograd), forward and forward + backward

The arms alternate in one process after one untimed call each.  It also runs the cases of tests/test_rnnt_joint_loss_gpu.py and
records the device's worst ratios to the derived bounds, the workspace sizes, and the backward's time against three times
the cells kernel of the commit before (the backward does three times the forward's MFMA work).

    python tools/rnnt_joint_loss_time.py [--repeats 5] [--out profiles/rnnt_joint_loss_time.json] [--kernel-stats SHAPE=CSV]
    python tools/rnnt_joint_loss_time.py --probe large     # 3 forward + backward calls at that shape only, for the profiler
    python tools/rnnt_joint_loss_time.py --merge JSON --kernel-stats large=CSV [--out JSON]    # add a trace's lines, no device

Per-kernel times come from a run of its own, ``tools/rocprof_script.sh rnnt_joint_loss_large tools/rnnt_joint_loss_time.py
--probe large`` (``--probe small`` for 30 symbols); ``--kernel-stats large=CSV`` copies that run's lines.
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

N, T, U, J = 16, 250, 120, 512
SHAPES = {"small": 29, "large": 5000}
PARENT_CELLS_MS = {"large": 16.0}          # rnnt_score_cells_kernel<4> at 5001 symbols, profiles/rnnt_score_time.json


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


class AbiCase:
    """The two entry points on fixed device buffers."""

    def __init__(self, vocab, seed=5):
        from myrtlespeech_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.V1 = vocab + 1
        g = torch.Generator().manual_seed(seed)
        self.enc_p = torch.randn((T, N, J), generator=g).cuda()
        self.pred_p = torch.randn((U + 1, N, J), generator=g).cuda()
        self.w = (torch.randn((self.V1, J), generator=g) * (4.0 / J ** 0.5)).cuda()
        self.b = torch.randn((self.V1,), generator=g).cuda()
        self.y_host = torch.randint(0, vocab, (N, U), generator=g, dtype=torch.int32)
        self.y = self.y_host.reshape(-1).cuda()
        i32 = lambda v: torch.as_tensor(v, dtype=torch.int32).cuda()     # noqa: E731
        self.xl, self.yl = i32([T] * N), i32([U] * N)
        self.grad_nll = torch.full((N,), 1.0 / N, device="cuda")
        self.nll = torch.empty(N, dtype=torch.float32, device="cuda")
        dims = (N, T, U + 1, J, self.V1)
        self.lattice = torch.empty(self.lib.ms_rnnt_joint_loss_lattice_bytes(N, T, U + 1) // 4, dtype=torch.float32, device="cuda")
        self.ws = torch.empty(self.lib.ms_rnnt_score_workspace_bytes(*dims), dtype=torch.uint8, device="cuda")
        self.bytes = {"forward_workspace": self.ws.numel(), "lattice": 4 * self.lattice.numel(),
                      "backward_workspace_min": self.lib.ms_rnnt_joint_loss_backward_workspace_min_bytes(*dims),
                      "backward_workspace_preferred": self.lib.ms_rnnt_joint_loss_backward_workspace_bytes(*dims),
                      "dense_logits": 4 * N * T * (U + 1) * self.V1}
        self.bws = torch.empty(self.bytes["backward_workspace_preferred"], dtype=torch.uint8, device="cuda")
        self.grads = [torch.empty_like(x) for x in (self.enc_p, self.pred_p, self.w, self.b)]

    def forward(self):
        L, p = self._lib, self._lib.ptr
        rc = self.lib.ms_rnnt_joint_loss_forward(p(self.enc_p), p(self.pred_p), p(self.w), p(self.b), p(self.xl), p(self.y),
                                                 p(self.yl), p(self.nll), p(self.lattice), N, T, U + 1, J, self.V1, self.V1 - 1,
                                                 p(self.ws), self.ws.numel(), L.stream_ptr())
        if rc != 0:
            sys.exit(f"rnnt_joint_loss_time: ms_rnnt_joint_loss_forward returned {rc}")

    def forward_backward(self):
        self.forward()
        L, p = self._lib, self._lib.ptr
        rc = self.lib.ms_rnnt_joint_loss_backward(p(self.enc_p), p(self.pred_p), p(self.w), p(self.b), p(self.xl), p(self.y),
                                                  p(self.yl), p(self.nll), p(self.lattice), p(self.grad_nll), p(self.grads[0]),
                                                  p(self.grads[1]), p(self.grads[2]), p(self.grads[3]), N, T, U + 1, J, self.V1,
                                                  self.V1 - 1, p(self.bws), self.bws.numel(), L.stream_ptr())
        if rc != 0:
            sys.exit(f"rnnt_joint_loss_time: ms_rnnt_joint_loss_backward returned {rc}")


def timed(arms, repeats, inner):
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


def case_ratios():
    """The runs of tests/test_rnnt_joint_loss_gpu.py::test_case_within_the_bounds; the device's worst ratios to the bounds."""
    import test_rnnt_joint_loss_gpu as G
    for name, workspace in G.RUNS:
        G.test_case_within_the_bounds(name, workspace)
    out = {k: round(float(v), 5) for k, v in G.worst.items()}
    out["bounds"] = "tests/rnnt_joint_loss_ref.py (the gradients, full and own share) and tests/test_rnnt_score_gpu.py (the forward)"
    return out


def kernel_stat_lines(path):
    with open(path, newline="") as f:
        return [row for row in csv.DictReader(f) if any(s in row.get("Name", "") for s in ("rnnt_score", "rnnt_loss_lattice", "rjl_"))]


def add_kernel_stats(rec, name, path):
    rec["kernel_stats_source"] = (f"rocprofv3 --kernel-trace --stats over `tools/rnnt_joint_loss_time.py --probe {name}` (a run of "
                                  "its own; 3 forward + backward calls)")
    rec["kernel_stats"] = kernel_stat_lines(path)


def python_arms(c):
    """``rnnt_joint_loss`` and the materialised route on the same inputs, forward and forward + backward."""
    from myrtlespeech_amd.loss import rnnt_joint_loss
    from myrtlespeech_amd.loss.rnnt_loss import RNNTLoss
    leaves = [x.clone().requires_grad_() for x in (c.enc_p, c.pred_p, c.w, c.b)]
    lens, y_lens = torch.full((N,), T), torch.full((N,), U)
    dense = RNNTLoss(c.V1 - 1, "mean")

    def fused():
        return rnnt_joint_loss(*leaves, lens, c.y_host, y_lens, c.V1 - 1, "mean")

    def materialised():
        e, p, w, b = leaves
        logits = torch.tanh(e.transpose(0, 1)[:, :, None, :] + p.transpose(0, 1)[:, None, :, :]) @ w.t() + b
        return dense((logits, lens), (c.y_host, y_lens))

    def with_backward(fn):
        def run():
            for x in leaves:
                x.grad = None
            fn().backward()
        return run

    def no_grad(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    return {"fused_forward": no_grad(fused), "fused_forward_backward": with_backward(fused),
            "materialised_forward": no_grad(materialised), "materialised_forward_backward": with_backward(materialised)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--probe", choices=sorted(SHAPES), default=None,
                    help="3 forward + backward calls at that shape and nothing else (for the profiler)")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="SHAPE=CSV")
    ap.add_argument("--merge", default=None, metavar="JSON",
                    help="add the --kernel-stats lines to a record this tool wrote earlier (needs no device) and write it to --out")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    stats = dict(s.split("=", 1) for s in a.kernel_stats)
    if a.merge is not None:
        with open(a.merge) as f:
            out = json.load(f)
        for name, path in stats.items():
            add_kernel_stats(out[name], name, path)
        with open(a.out or a.merge, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        return
    if not torch.cuda.is_available():
        sys.exit("rnnt_joint_loss_time: a HIP device is required; there is no CPU path")
    if a.probe is not None:
        c = AbiCase(SHAPES[a.probe])
        for _ in range(3):
            c.forward_backward()
        torch.cuda.synchronize()
        return
    out = {"tool": "tools/rnnt_joint_loss_time.py", "commit": a.commit, "shape": {"N": N, "T": T, "U": U, "J": J},
           "statistic": "host clock around back-to-back calls ending in a device synchronise, per call, ms; the arms alternate in "
                        "one process after one untimed call each",
           "worst_ratios_to_the_bounds": case_ratios()}
    cells = N * T * (U + 1)
    for name, vocab in SHAPES.items():
        c = AbiCase(vocab)
        ms = timed({"forward": c.forward, "forward_backward": c.forward_backward}, a.repeats, 2)
        rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
        rec["symbols"] = c.V1
        rec["bytes"] = c.bytes
        nll = c.nll.cpu().numpy()
        if not np.isfinite(nll).all() or not all(bool(torch.isfinite(g).all()) for g in c.grads):
            sys.exit(f"rnnt_joint_loss_time: {name}: nll {nll.tolist()} or a gradient is not finite")
        rec["mean_nll"] = round(float(nll.mean()), 3)
        rec["sum_of_d_b_out"] = float(c.grads[3].sum())            # a softmax gradient: the column sums cancel
        back = statistics.median(ms["forward_backward"]) - statistics.median(ms["forward"])
        rec["backward_ms"] = round(back, 4)
        rec["mfma_flop_backward"] = 3 * 3 * 2 * cells * J * c.V1
        rec["achieved_TFLOPs_backward_counting_the_nine_products"] = round(3 * 3 * 2 * cells * J * c.V1 / (back * 1e-3) / 1e12, 2)
        if name in PARENT_CELLS_MS:
            rec["backward_over_three_times_the_parents_cells_kernel"] = round(back / (3 * PARENT_CELLS_MS[name]), 3)
            rec["parents_cells_kernel_ms"] = PARENT_CELLS_MS[name]
        if name == "small":
            pms = timed(python_arms(c), a.repeats, 1)
            rec["python"] = {f"{k}_ms": spread(v) for k, v in pms.items()}
            rec["python"]["materialised_over_fused_forward_backward"] = round(
                statistics.median(pms["materialised_forward_backward"]) / statistics.median(pms["fused_forward_backward"]), 3)
        else:
            rec["materialised"] = f"not run: its logits alone are {c.bytes['dense_logits'] / 1e9:.1f} GB, and so is their gradient"
        if name in stats:
            add_kernel_stats(rec, name, stats[name])
        out[name] = rec
        del c
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
