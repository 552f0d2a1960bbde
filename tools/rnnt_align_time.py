#!/usr/bin/env python3
"""What forced alignment under a transducer costs beside scoring the same transcripts; arms alternating in one process.

  fused    ``ms_rnnt_align_joint`` (pack, cells, walk + back-trace + read-out: N workgroups) against ``ms_rnnt_score`` (pack,
           cells, lattice pass: 2 N workgroups) on the same inputs, at ``[N = 16, T = 250, U = 120]``, J = 512, with V1 = 29
           and V1 = 5000.  The cells work is identical, so the scorer is the yardstick.
  logits   ``ms_rnnt_align`` (normaliser pass, walk) against ``ms_rnnt_loss_forward`` (normaliser pass, lattice pass) on the
           same ``[N, T, U + 1, 29]`` logits.
  walk     the Viterbi launch alone is not an entry point of its own; it is reported as ``ms_rnnt_align`` in log-probability
           mode on a ``[N, T, U + 1, 2]`` table (the gather launch moves 16 bytes per cell) minus the same call on utterances
           whose lengths are out of range, where both launches exit at once (the floor of two launches).

An arm is the host clock around ``--inner`` back-to-back calls that end in a device synchronise, divided by the calls.

    python tools/rnnt_align_time.py [--repeats 7] [--inner 10] [--out profiles/rnnt_align_time.json] [--probe-lib LIB]

``--probe-lib`` names a second build of the library whose walk kernel skips the serial back-trace (rnnt_align.hip compiled
with -DRA_PROBE_NO_BACKTRACE; its paths are meaningless, the walk and the read-out are the same): the two builds' calls
alternate on the same buffers in the ``walk`` arm, and the difference is what the back-trace by one lane costs.

There is no CPU path: without a HIP device the tool fails.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

N, T, U, J = 16, 250, 120, 512
U1 = U + 1
SHAPES = {"small": 29, "large": 5000}          # V1: the symbols, blank (the last) included
LOG_PROBS_IN = 2


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


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


class Buffers:
    """Device buffers of one shape: the lengths, the targets, the five outputs of the aligner."""

    def __init__(self, vocab, gen, lens_ok=True):
        i32 = lambda v: torch.as_tensor(v, dtype=torch.int32).cuda()      # noqa: E731
        self.y = torch.randint(0, vocab, (N, U), generator=gen, dtype=torch.int32).reshape(-1).cuda()
        self.xl, self.yl = i32([T] * N), i32([U if lens_ok else -1] * N)
        self.score = torch.empty(N, dtype=torch.float32, device="cuda")
        self.t_frame = torch.empty((N, U), dtype=torch.int32, device="cuda")
        self.t_logp = torch.empty((N, U), dtype=torch.float32, device="cuda")
        self.f_u = torch.empty((N, T), dtype=torch.int32, device="cuda")
        self.f_logp = torch.empty((N, T), dtype=torch.float32, device="cuda")

    def outputs(self, p):
        return p(self.score), p(self.t_frame), p(self.t_logp), p(self.f_u), p(self.f_logp)


def check(rc, what):
    if rc != 0:
        sys.exit(f"rnnt_align_time: {what} returned {rc}")


def fused_arms(L, lib, vocab):
    v1, p = vocab + 1, L.ptr
    g = torch.Generator().manual_seed(5)
    enc_p = torch.randn((T * N, J), generator=g).cuda()
    pred_p = torch.randn((U1 * N, J), generator=g).cuda()
    w = (torch.randn((v1, J), generator=g) * (4.0 / J ** 0.5)).cuda()
    b = torch.randn((v1,), generator=g).cuda()
    buf = Buffers(vocab, g)
    nll = torch.empty(N, dtype=torch.float32, device="cuda")
    lattice = torch.empty(lib.ms_rnnt_score_lattice_bytes(N, T, U1) // 4, dtype=torch.float32, device="cuda")
    ws_s = torch.empty(lib.ms_rnnt_score_workspace_bytes(N, T, U1, J, v1), dtype=torch.uint8, device="cuda")
    ws_a = torch.empty(lib.ms_rnnt_align_joint_workspace_bytes(N, T, U1, J, v1), dtype=torch.uint8, device="cuda")

    def score():
        check(lib.ms_rnnt_score(p(enc_p), p(pred_p), p(w), p(b), p(buf.xl), p(buf.y), p(buf.yl), p(nll), p(lattice), N, T, U1, J,
                                v1, vocab, p(ws_s), ws_s.numel(), L.stream_ptr()), "ms_rnnt_score")

    def align():
        check(lib.ms_rnnt_align_joint(p(enc_p), p(pred_p), p(w), p(b), p(buf.xl), p(buf.y), p(buf.yl), *buf.outputs(p), N, T, U1,
                                      J, v1, vocab, p(ws_a), ws_a.numel(), L.stream_ptr()), "ms_rnnt_align_joint")

    return {"ms_rnnt_score": score, "ms_rnnt_align_joint": align}, buf, nll, (ws_s.numel(), ws_a.numel())


def dense_arms(L, lib, vocab):
    v1, p = vocab + 1, L.ptr
    g = torch.Generator().manual_seed(6)
    x = (torch.randn((N, T, U1, v1), generator=g) * 3.0).cuda()
    buf = Buffers(vocab, g)
    nll = torch.empty(N, dtype=torch.float32, device="cuda")
    lattice = torch.empty(lib.ms_rnnt_loss_lattice_bytes(N, T, U1) // 4, dtype=torch.float32, device="cuda")
    ws_l = torch.empty(lib.ms_rnnt_loss_workspace_bytes(N, T, U1, v1), dtype=torch.uint8, device="cuda")
    ws_a = torch.empty(lib.ms_rnnt_align_workspace_bytes(N, T, U1, v1), dtype=torch.uint8, device="cuda")

    def loss():
        check(lib.ms_rnnt_loss_forward(p(x), p(buf.xl), p(buf.y), p(buf.yl), p(nll), p(lattice), N, T, U1, v1, vocab, p(ws_l),
                                       ws_l.numel(), L.stream_ptr()), "ms_rnnt_loss_forward")

    def align():
        check(lib.ms_rnnt_align(p(x), p(buf.xl), p(buf.y), p(buf.yl), *buf.outputs(p), N, T, U1, v1, vocab, 0, p(ws_a),
                                ws_a.numel(), L.stream_ptr()), "ms_rnnt_align")

    return {"ms_rnnt_loss_forward": loss, "ms_rnnt_align": align}, buf, nll


def walk_arms(L, lib, probe_lib=None):
    p = L.ptr
    g = torch.Generator().manual_seed(7)
    x = -(torch.rand((N, T, U1, 2), generator=g) * 4.0).cuda()
    live, dead = Buffers(1, g), Buffers(1, g, lens_ok=False)
    ws = torch.empty(lib.ms_rnnt_align_workspace_bytes(N, T, U1, 2), dtype=torch.uint8, device="cuda")

    def arm(buf, lib=lib):
        def run():
            check(lib.ms_rnnt_align(p(x), p(buf.xl), p(buf.y), p(buf.yl), *buf.outputs(p), N, T, U1, 2, 1, LOG_PROBS_IN, p(ws),
                                    ws.numel(), L.stream_ptr()), "ms_rnnt_align")
        return run

    arms = {"gather_and_walk": arm(live), "two_launches_that_exit_at_once": arm(dead)}
    if probe_lib:
        other = ctypes.CDLL(os.path.abspath(probe_lib))
        other.ms_rnnt_align.restype, other.ms_rnnt_align.argtypes = L.SIGNATURES["ms_rnnt_align"]
        arms["gather_and_walk_without_backtrace"] = arm(Buffers(1, g), other)
    return arms, live


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--probe-lib", default=None, help="a build of the library with -DRA_PROBE_NO_BACKTRACE")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rnnt_align_time: a HIP device is required; there is no CPU path")
    from myrtlespeech_amd import _lib as L
    from myrtlespeech_amd.post_process import rnnt_aligner as P
    lib = L.load()
    out = {"tool": "tools/rnnt_align_time.py", "commit": a.commit, "shape": {"N": N, "T": T, "U": U, "J": J},
           "statistic": f"host clock around {a.inner} back-to-back calls ending in a device synchronise, per call, ms; the arms "
                        "alternate in one process after one untimed call each",
           "backpointers": {"bytes_per_utterance": P.backpointer_bytes(T, U1), "in_lds": P.backpointers_in_lds(T, U1)}}
    for name, v1 in SHAPES.items():
        arms, buf, nll, ws_bytes = fused_arms(L, lib, v1 - 1)
        ms = timed(arms, a.repeats, a.inner)
        score, neg = buf.score.cpu().numpy(), -nll.cpu().numpy()
        if not np.isfinite(score).all() or not (score <= neg + 1e-2).all():
            sys.exit(f"rnnt_align_time: {name}: score {score.tolist()} against -nll {neg.tolist()}")
        rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
        rec["symbols"] = v1
        rec["align_over_score"] = round(statistics.median(ms["ms_rnnt_align_joint"]) / statistics.median(ms["ms_rnnt_score"]), 4)
        rec["workspace_bytes"] = {"ms_rnnt_score": ws_bytes[0] + 8 * N * T * U1, "ms_rnnt_align_joint": ws_bytes[1],
                                  "note": "the scorer's figure includes its alpha / beta lattice; the aligner has none"}
        rec["mean_score"], rec["mean_minus_nll"] = round(float(score.mean()), 3), round(float(neg.mean()), 3)
        out[f"fused_{name}"] = rec
        del arms, buf, nll
        torch.cuda.empty_cache()
    arms, buf, nll = dense_arms(L, lib, SHAPES["small"] - 1)
    ms = timed(arms, a.repeats, a.inner)
    score, neg = buf.score.cpu().numpy(), -nll.cpu().numpy()
    if not np.isfinite(score).all() or not (score <= neg + 1e-2).all():
        sys.exit(f"rnnt_align_time: logits: score {score.tolist()} against -nll {neg.tolist()}")
    rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
    rec["symbols"] = SHAPES["small"]
    rec["align_over_loss_forward"] = round(statistics.median(ms["ms_rnnt_align"]) / statistics.median(ms["ms_rnnt_loss_forward"]), 4)
    out["logits_small"] = rec
    del arms, buf, nll
    torch.cuda.empty_cache()
    arms, buf = walk_arms(L, lib, a.probe_lib)
    ms = timed(arms, a.repeats, a.inner)
    if not np.isfinite(buf.score.cpu().numpy()).all():
        sys.exit("rnnt_align_time: walk: no path")
    rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
    rec["viterbi_launch_ms"] = round(statistics.median(ms["gather_and_walk"]) -
                                     statistics.median(ms["two_launches_that_exit_at_once"]), 4)
    rec["note"] = ("log-probability mode on a [N, T, U + 1, 2] table: the walk over T + U diagonals, the back-trace of T + U - 1 "
                   "steps by one lane and the read-out, plus a gather of 16 bytes per cell; minus the floor of two launches")
    if a.probe_lib:
        rec["backtrace_ms"] = round(statistics.median(ms["gather_and_walk"]) -
                                    statistics.median(ms["gather_and_walk_without_backtrace"]), 4)
        rec["backtrace_note"] = f"{T + U - 1} dependent steps by one lane, back-pointers in LDS; against a build that skips them"
    out["walk"] = rec
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
