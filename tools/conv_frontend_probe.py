#!/usr/bin/env python3
"""Diagnostic: the DS2 convolution front end alone at the bench shapes (80 features x 1001 frames, N = 32 and 64), the shipped
dispatch (ms_conv_set_variant(0)) against the kernels and passes it replaces (variant 1), interleaved in ONE process and timed
with HIP events: conv1 alone, and conv1 -> clamp -> conv2 as the model's CNN loop runs it (variant 0 hands the planes over).
PROBE_LAUNCHES=60 launches per variant and shape after 5 warm-up launches; prints a JSON line per measurement."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from myrtlespeech_amd import _lib  # noqa: E402

lib = _lib.load()
launches = int(os.environ.get("PROBE_LAUNCHES", "60"))
model = bench.build_model()
conv1 = model.cnn[0]


def timed(fn, variant):
    lib.ms_conv_set_variant(variant)
    try:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(3_000_000)      # the device spins ~1 ms while the host queues fn's launches: device time is measured
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3, out
    finally:
        lib.ms_conv_set_variant(0)


with torch.no_grad():
    for n in (32, 64):
        x = torch.randn(n, 1, bench.FEATURES, bench.FRAMES, device="cuda")
        lens = _lib.attach_host(torch.full((n,), bench.FRAMES, device="cuda"), torch.full((n,), bench.FRAMES))
        for name, fn in (("conv1", lambda: conv1((x, lens), fused_activation=(0.0, 20.0))),
                         ("conv1+conv2", lambda: model._run_cnn((x, lens)))):
            us = {0: [], 1: []}
            outs = {}
            for i in range(5 + launches):
                for v in (0, 1):
                    t, outs[v] = timed(fn, v)
                    if i >= 5:
                        us[v].append(t)
            rec = {"what": name, "N": n, "launches": launches, "equal": bool(torch.equal(outs[0][0], outs[1][0]))}
            for v in (0, 1):
                s = sorted(us[v])
                rec[f"variant{v}_us"] = {"median": round(s[len(s) // 2], 1), "min": round(s[0], 1), "max": round(s[-1], 1)}
            print(json.dumps(rec), flush=True)
