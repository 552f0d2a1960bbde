#!/usr/bin/env python3
"""What scoring transcripts under a transducer costs, with and without the logit lattice; arms alternating in one process.

  (a) materialised  ``RNNT.joint_lattice`` (U + 1 rounds of predictor step + joint launch, [N, T, U + 1, V + 1] floats written)
                    followed by ``RNNTLoss(reduction="none")`` (which reads them back)
  (b) fused         ``RNNT.transcript_nll`` (one predictor pass, ``ms_rnnt_score``: pack, cells, lattice)

on a seeded model (encoder features 512, predictor 2 x 512, joint 512) at ``[N = 16, T = 250, U = 120]`` with V = 29, and arm
(b) alone with V = 5000, where (a)'s lattice cannot be allocated.  An arm is the host clock around ``--inner`` back-to-back
calls that end in a device synchronise, divided by the calls.  Beside the times stand the bytes either path writes and reads
for the lattice, the two arms' largest difference, and the device's worst ratios to the bounds of
tests/test_rnnt_score_gpu.py (its cases are run here).

    python tools/rnnt_score_time.py [--repeats 7] [--out profiles/rnnt_score_time.json] [--kernel-stats SHAPE=CSV]
                                    [--probe-lib LIB]
    python tools/rnnt_score_time.py --probe large      # 10 ms_rnnt_score calls at the V = 5000 shape only, for the profiler

Per-pass times (pack, cells, lattice) come from a run of its own, ``tools/rocprof_script.sh rnnt_score_large
tools/rnnt_score_time.py --probe large`` (``--probe small`` for V = 29); ``--kernel-stats large=CSV`` copies that run's lines.
``--probe-lib`` names a second build of the library whose cells kernel forms its A operand WITHOUT the tanh (rnnt_score.hip
compiled with -DRS_PROBE_NO_TANH; results are meaningless, the MFMA work and the memory traffic are the same): the two
builds' ``ms_rnnt_score`` alternate on the same buffers and the difference is what forming (and, above one column tile,
re-forming) the tanh rows costs.
There is no CPU path: without a HIP device the tool fails.
"""
import argparse
import csv
import ctypes
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
ENC, HID, EMB, LAYERS = 512, 512, 128, 2
SHAPES = {"small": 29, "large": 5000}


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


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


class AbiCase:
    """``ms_rnnt_score`` on fixed device buffers, callable on any build of the library."""

    def __init__(self, vocab, seed=5):
        from myrtlespeech_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.V1 = vocab + 1
        g = torch.Generator().manual_seed(seed)
        self.enc_p = torch.randn((T * N, J), generator=g).cuda()
        self.pred_p = torch.randn(((U + 1) * N, J), generator=g).cuda()
        self.w = (torch.randn((self.V1, J), generator=g) * (4.0 / J ** 0.5)).cuda()
        self.b = torch.randn((self.V1,), generator=g).cuda()
        i32 = lambda v: torch.as_tensor(v, dtype=torch.int32).cuda()     # noqa: E731
        self.y = torch.randint(0, vocab, (N, U), generator=g, dtype=torch.int32).reshape(-1).cuda()
        self.xl, self.yl = i32([T] * N), i32([U] * N)
        self.nll = torch.empty(N, dtype=torch.float32, device="cuda")
        self.lattice = torch.empty(self.lib.ms_rnnt_score_lattice_bytes(N, T, U + 1) // 4, dtype=torch.float32, device="cuda")
        self.ws = torch.empty(self.lib.ms_rnnt_score_workspace_bytes(N, T, U + 1, J, self.V1), dtype=torch.uint8, device="cuda")

    def call(self, fn):
        L, p = self._lib, self._lib.ptr
        rc = fn(p(self.enc_p), p(self.pred_p), p(self.w), p(self.b), p(self.xl), p(self.y), p(self.yl), p(self.nll),
                p(self.lattice), N, T, U + 1, J, self.V1, self.V1 - 1, p(self.ws), self.ws.numel(), L.stream_ptr())
        if rc != 0:
            sys.exit(f"rnnt_score_time: ms_rnnt_score returned {rc}")

    def run(self):
        self.call(self.lib.ms_rnnt_score)


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
    """The cases of tests/test_rnnt_score_gpu.py::test_case_within_the_bounds; the device's worst ratios to the bounds."""
    import rnnt_score_ref as S
    import test_rnnt_score_gpu as G
    out = {}
    for name in sorted(G.CASES):
        ref, _, bounds = S.reference(name)
        w = G.check_against(ref, bounds, G.run_case(G.CASES[name]), name)
        out[name] = {k: round(float(v), 5) for k, v in w.items()}
    out["all"] = {k: max(w[k] for w in out.values()) for k in ("nll", "alpha", "beta")}
    out["bounds"] = ("B_n + (T_n + U_n) delta_n for nll, alpha, beta, delta = 2 max_v eps_v + 16 2^-24 max(1, |Z|), eps_v = 2^-24 "
                     "((J + 16) sum_j |w_out[v, j]| + |b_out[v]|); against the float64 reference tests/rnnt_score_ref.py")
    return out


def kernel_stat_lines(path):
    with open(path, newline="") as f:
        return [row for row in csv.DictReader(f) if "rnnt_score" in row.get("Name", "") or "rnnt_loss_lattice" in row.get("Name", "")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--probe", choices=sorted(SHAPES), default=None,
                    help="10 ms_rnnt_score calls at that shape and nothing else (for the profiler)")
    ap.add_argument("--probe-lib", default=None, help="a build of the library with -DRS_PROBE_NO_TANH")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="SHAPE=CSV")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rnnt_score_time: a HIP device is required; there is no CPU path")
    if a.probe is not None:
        c = AbiCase(SHAPES[a.probe])
        for _ in range(10):
            c.run()
        torch.cuda.synchronize()
        return
    from myrtlespeech_amd.loss.rnnt_loss import RNNTLoss
    out = {"tool": "tools/rnnt_score_time.py", "commit": a.commit,
           "shape": {"N": N, "T": T, "U": U, "J": J, "encoder_features": ENC, "predictor": [LAYERS, HID], "embedding": EMB},
           "statistic": f"host clock around {a.inner} back-to-back calls ending in a device synchronise, per call, ms; the arms "
                        "alternate in one process after one untimed call each",
           "worst_ratios_to_the_bounds": case_ratios()}
    stats = dict(s.split("=", 1) for s in a.kernel_stats)
    cells = N * T * (U + 1)
    for name, vocab in SHAPES.items():
        model, enc, lens, y, y_lens = make_model(vocab)
        v1 = vocab + 1
        loss = RNNTLoss(blank=vocab, reduction="none")
        arms = {"fused": lambda: model.transcript_nll(enc, lens, y, y_lens)}
        dense_bytes = 4 * cells * v1
        if name == "small":
            arms = {"materialised": lambda: loss((model.joint_lattice(enc, lens, y, y_lens), lens), (y, y_lens)), **arms}
        ms = timed(arms, a.repeats, a.inner)
        rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
        rec["symbols"] = v1
        from myrtlespeech_amd import _lib
        L = _lib.load()
        rec["bytes"] = {
            "materialised_logit_lattice": dense_bytes,
            "materialised_written_then_read": 2 * dense_bytes + 12 * cells + L.ms_rnnt_loss_workspace_bytes(N, T, U + 1, v1),
            "fused_workspace_and_lattice": L.ms_rnnt_score_workspace_bytes(N, T, U + 1, J, v1) + 8 * cells,
            "fused_inputs": 4 * J * (T * N + (U + 1) * N + v1),
            "note": "materialised: the logits written by the joint and read by the loss, the loss's lattice and planes; fused: "
                    "the two skewed planes, the packed weights, alpha and beta"}
        fused = model.transcript_nll(enc, lens, y, y_lens).cpu().numpy()
        if not np.isfinite(fused).all() or not (fused > 0).all():
            sys.exit(f"rnnt_score_time: {name}: nll {fused.tolist()} is not what a loss gives")
        rec["mean_nll"] = round(float(fused.mean()), 3)
        if name == "small":
            dense = loss((model.joint_lattice(enc, lens, y, y_lens), lens), (y, y_lens)).cpu().numpy()
            rec["largest_difference_of_the_arms"] = float(np.abs(fused.astype(np.float64) - dense).max())
            rec["materialised_over_fused"] = round(statistics.median(ms["materialised"]) / statistics.median(ms["fused"]), 3)
        else:
            rec["materialised"] = f"not run: its logit lattice alone is {dense_bytes / 1e9:.1f} GB"
        arms = model = enc = None
        torch.cuda.empty_cache()
        # the library call alone, and against the build without the tanh
        c = AbiCase(vocab)
        abi_arms = {"ms_rnnt_score": c.run}
        if a.probe_lib:
            other = ctypes.CDLL(os.path.abspath(a.probe_lib))
            fn = other.ms_rnnt_score
            fn.restype, fn.argtypes = _lib.SIGNATURES["ms_rnnt_score"]
            abi_arms["ms_rnnt_score_without_tanh"] = lambda: c.call(fn)
        ms = timed(abi_arms, a.repeats, 10)
        rec["abi"] = {f"{k}_ms": spread(v) for k, v in ms.items()}
        tiles = -(-v1 // (32 if v1 <= 32 else 64 if v1 <= 64 else 128))
        rec["abi"]["column_tiles"] = tiles
        rec["abi"]["mfma_flop"] = 3 * 2 * cells * J * v1
        rec["abi"]["achieved_TFLOPs_counting_the_three_products"] = round(
            3 * 2 * cells * J * v1 / (statistics.median(ms["ms_rnnt_score"]) * 1e-3) / 1e12, 2)
        if a.probe_lib:
            full, bare = statistics.median(ms["ms_rnnt_score"]), statistics.median(ms["ms_rnnt_score_without_tanh"])
            rec["abi"]["tanh_share_of_the_call"] = round(1.0 - bare / full, 4)
            rec["abi"]["tanh_share_note"] = (f"the tanh rows are formed {tiles} time(s) per cell tile (once per column tile): "
                                             "what holding them would save is at most this share times (tiles - 1) / tiles")
        if name in stats:
            rec["kernel_stats_source"] = (f"rocprofv3 --kernel-trace --stats over `tools/rnnt_score_time.py --probe {name}` (a run "
                                          "of its own; 10 calls)")
            rec["kernel_stats"] = kernel_stat_lines(stats[name])
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
