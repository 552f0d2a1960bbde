#!/usr/bin/env python3
"""What streaming costs the RNN-T greedy decode: the whole-clip RNNTGreedyDecoder against StreamingRNNTGreedyDecoder pushed
with chunks of 32 encoder frames, on the model and inputs of tests/golden/gen_rnnt_cfg4.py (BASELINE configs[3]: 16 streams,
501 frames, 2 x LSTM-1024 predictor, joint 512).  -> profiles/rnnt_stream_time.json

Two densities: the fixture as it is (greedy emits ~1.7 labels per frame, far denser than speech) and with joint.out.bias[V]
raised until greedy emits about 0.15 labels per frame.  The arms alternate in one process; every timing is a host clock
around a call that ends in a device synchronisation (both decoders block).  Per arm: median, minimum and maximum over the
repeats.  Iterations: what the event-driven loop needs (from the transcripts' emission frames: labels + blocks of 32 blank
frames, per push the busiest stream's) for both arms, and what the streaming arm actually launched (it polls a few
iterations behind its queue, so every push launches a few more).  A record, not a test: there is no pass mark.

    python tools/rnnt_stream_time.py [--repeats 7] [--warmup 2] [--chunk 32] [--out profiles/rnnt_stream_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def needed_iterations(exist, emitted_at, max_symbols, block=32):
    """Rounds of (score `block` pending frames, step the predictor after the first label) for one stream's `exist` rows,
    given the rows that emitted (one entry per label, in order)."""
    pos, nsym, k, rounds = 0, 0, 0, 0
    while pos < exist:
        rounds += 1
        if k < len(emitted_at) and emitted_at[k] < pos + block:
            nsym = (nsym if emitted_at[k] == pos else 0) + 1
            pos, k = emitted_at[k], k + 1
            if nsym >= max_symbols:
                pos, nsym = pos + 1, 0
        else:
            pos, nsym = min(pos + block, exist), 0
    return rounds


def iterations_by_chunk(frames, lens, total, chunk, max_symbols):
    """Sum over pushes of the busiest stream's rounds."""
    out = 0
    for t0 in range(0, total, chunk):
        worst = 0
        for f, n in zip(frames, lens):
            exist = min(max(n - t0, 0), chunk)
            worst = max(worst, needed_iterations(exist, [v - t0 for v in f if t0 <= v < t0 + chunk], max_symbols))
        out += worst
    return out


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def measure(pred, joint, enc, lens, max_symbols, chunk, repeats, warmup):
    from myrtlespeech_amd.post_process.rnnt_decoder import RNNTGreedyDecoder
    from myrtlespeech_amd.post_process.rnnt_streaming import StreamingRNNTGreedyDecoder
    total, n, _ = enc.shape
    whole = RNNTGreedyDecoder(pred, joint, max_symbols=max_symbols)
    stream = StreamingRNNTGreedyDecoder(pred, joint, max_symbols=max_symbols)
    host_lens = [int(v) for v in lens]
    t_whole, t_sum, t_push, t_begin = [], [], [], []
    want = frames = launched = None
    for rep in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got_whole = whole(enc, lens)                         # ends in its read-back
        t1 = time.perf_counter()
        stream.begin(n, total * max_symbols, total_lens=lens)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        pushes = []
        for r0 in range(0, total, chunk):
            a = time.perf_counter()
            stream.push(enc[r0:r0 + chunk]).result()         # ends in the news' read-back
            pushes.append((time.perf_counter() - a) * 1e3)
        if rep == 0:
            want, frames, launched = stream.transcripts(), stream.timestamps(), stream.iterations()
            if want != got_whole:
                raise SystemExit("the streamed transcripts differ from the whole-clip decoder's")
        if rep >= warmup:
            t_whole.append((t1 - t0) * 1e3)
            t_begin.append((t2 - t1) * 1e3)
            t_sum.append(sum(pushes))
            t_push.append(pushes)
    labels = sum(len(w) for w in want)
    per_push = [statistics.median(p[k] for p in t_push) for k in range(len(t_push[0]))]
    res = dict(labels=labels, labels_per_frame=round(labels / sum(host_lens), 4), pushes=len(per_push),
               whole_clip=spread(t_whole), stream_begin=spread(t_begin), stream_sum_of_pushes=spread(t_sum),
               stream_push_mean_ms=round(statistics.mean(per_push), 3), stream_push_worst_ms=round(max(per_push), 3),
               iterations_needed_whole_clip=iterations_by_chunk(frames, host_lens, total, total, max_symbols),
               iterations_needed_stream=iterations_by_chunk(frames, host_lens, total, chunk, max_symbols),
               iterations_launched_stream=launched)
    res["sum_of_pushes_over_whole_clip"] = round(res["stream_sum_of_pushes"]["median_ms"] / res["whole_clip"]["median_ms"], 3)
    return res


def labels_per_frame(pred, joint, enc, lens, max_symbols):
    from myrtlespeech_amd.post_process.rnnt_decoder import RNNTGreedyDecoder
    got = RNNTGreedyDecoder(pred, joint, max_symbols=max_symbols)(enc, lens)
    return sum(len(g) for g in got) / float(sum(int(v) for v in lens))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--target", type=float, default=0.15, help="labels per frame of the sparse arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_stream_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnnt_stream_time.py measures on the GPU: no HIP device")
    import gen_rnnt_cfg4 as G
    pred, joint = G.parts()
    enc, lens = G.inputs()
    enc = enc.cuda()
    out = dict(device=torch.cuda.get_device_name(0), model="tests/golden/gen_rnnt_cfg4.py parts(), inputs()",
               shape=dict(N=G.N, T=G.T, V=G.V, D=G.D, P=G.P, J=G.J, L=G.L, max_symbols=G.MS), chunk=args.chunk,
               repeats=args.repeats, warmup=args.warmup,
               parent_whole_clip_greedy_decode_ms=40.3)       # profiles/r06_bench_detail_20steps.json
    with torch.no_grad():
        out["fixture"] = measure(pred, joint, enc, lens, G.MS, args.chunk, args.repeats, args.warmup)
        # raise the blank bias until greedy emits about `target` labels per frame (bisection on the whole-clip decoder)
        base = float(joint.out.bias[G.V])
        lo, hi = 0.0, 64.0
        for _ in range(12):
            mid = 0.5 * (lo + hi)
            joint.out.bias[G.V] = base + mid
            if labels_per_frame(pred, joint, enc, lens, G.MS) > args.target:
                lo = mid
            else:
                hi = mid
        joint.out.bias[G.V] = base + hi
        out["sparse"] = dict(blank_bias_raised_by=round(hi, 4),
                             **measure(pred, joint, enc, lens, G.MS, args.chunk, args.repeats, args.warmup))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
