#!/usr/bin/env python3
"""What the range-safe mode costs the CTC prefix beam search (width 8, [501, 32, 29]), arms alternating in one process.

  plain  ``CTCBeamDecoder(...)``: the reference's linear float32 search (ms_ctc_beam_decode)
  safe   ``CTCBeamDecoder(..., range_safe=True)``: the same search with an unbounded exponent (ms_ctc_beam_decode_ex)

on (i) ``softmax(12 * randn(501, 32, 29))``, where both survive and must agree, and (ii) ``softmax(4 * randn(501, 32, 29))``,
where the plain search underflows (its beams run empty and END the search early, so its time is recorded but is not a
comparison: it times less work).  Every decode ends in a device synchronise (the transcripts are read back); the figure is
host-clock ms, min / median / max.  The number of rescales is read from the n-best read-out (scale_log2) and counted exactly
by a frame-by-frame run that watches scale_log2 change.

    python tools/beam_range_time.py [--repeats 7] [--out profiles/beam_range_time.json] [--commit ID]

There is no CPU path: without a HIP device the tool fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch  # noqa: E402

WIDTH, THR, BLANK, FRAMES, BATCH, SYMBOLS = 8, 1e-3, 28, 501, 32, 29


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def count_rescales(x, lens):
    """Rescales per utterance: the search advanced a frame per call, scale_log2 read after each (it changes exactly when the
    rule fires: e <= -33)."""
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    frames, n, v = x.shape
    ld = lens.to(torch.int32).cuda()
    bufs = dict(out_idx=torch.empty((n, frames), dtype=torch.int32, device="cuda"),
                out_len=torch.empty(n, dtype=torch.int32, device="cuda"),
                beam_len=torch.empty(n, dtype=torch.int32, device="cuda"),
                beam_idx=torch.empty((n, WIDTH, frames), dtype=torch.int32, device="cuda"),
                beam_plen=torch.empty((n, WIDTH), dtype=torch.int32, device="cuda"),
                score=torch.empty((n, WIDTH), dtype=torch.float32, device="cuda"))
    ws = torch.zeros(lib.ms_ctc_beam_workspace_bytes(frames, n, v, WIDTH), dtype=torch.uint8, device="cuda")
    scales = torch.zeros((frames, n), dtype=torch.int32, device="cuda")
    for t in range(frames):
        _lib.check(lib.ms_ctc_beam_decode_ex(
            _lib.ptr(x), _lib.ptr(ld), _lib.ptr(bufs["out_idx"]), _lib.ptr(bufs["out_len"]), frames, n, v, BLANK, WIDTH,
            float(THR), -1, None, t, t + 1, 0, frames, None, 0, _lib.ptr(bufs["beam_len"]), _lib.ptr(bufs["beam_idx"]),
            _lib.ptr(bufs["beam_plen"]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(), None, None, 0, 1,
            _lib.ptr(bufs["score"]), _lib.ptr(scales[t])), "ms_ctc_beam_decode_ex")
    s = torch.cat([torch.zeros((1, n), dtype=torch.int32), scales.cpu()])
    return (s[1:] != s[:-1]).sum(dim=0).tolist(), s[-1].tolist()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("beam_range_time: a HIP device is required; there is no CPU path")
    from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
    out = {"tool": "tools/beam_range_time.py", "commit": a.commit, "beam_width": WIDTH, "prune_threshold": THR,
           "shape": [FRAMES, BATCH, SYMBOLS],
           "statistic": "host clock of one decode that ends with its transcripts on the host, ms; the arms alternate in one "
                        "process after one untimed decode each",
           "arms": {"plain": "CTCBeamDecoder (ms_ctc_beam_decode)", "safe": "CTCBeamDecoder(range_safe=True) (ms_ctc_beam_decode_ex)"}}
    lens = torch.full((BATCH,), FRAMES, dtype=torch.int64)
    for scale in (12, 4):
        torch.manual_seed(0)
        x = torch.softmax(scale * torch.randn(FRAMES, BATCH, SYMBOLS), dim=2).cuda()
        decs = {"plain": CTCBeamDecoder(BLANK, WIDTH, THR), "safe": CTCBeamDecoder(BLANK, WIDTH, THR, range_safe=True)}
        got = {k: d(x, lens) for k, d in decs.items()}                  # untimed
        empty = sum(len(v) == 0 for v in got["plain"])
        if empty == 0 and got["plain"] != got["safe"]:
            sys.exit(f"beam_range_time: scale {scale}: both searches survive and disagree")
        ms = {k: [] for k in decs}
        for _ in range(a.repeats):
            for k, d in decs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d(x, lens)
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        rescales, scales = count_rescales(x, lens)
        hyps = decs["safe"].decode_nbest(x, lens, n=1)
        rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
        rec["plain_utterances_whose_beam_ran_empty"] = empty
        rec["plain_is_a_comparison"] = empty == 0
        rec["transcripts_equal"] = got["plain"] == got["safe"]
        rec["safe_minus_plain_ms"] = round(statistics.median(ms["safe"]) - statistics.median(ms["plain"]), 4) if empty == 0 else None
        rec["rescales_per_utterance"] = {"min": min(rescales), "max": max(rescales), "all_utterances": sum(rescales)}
        rec["scale_log2"] = {"min": min(scales), "max": max(scales)}
        rec["ln_p_of_the_best_hypothesis"] = {"min": round(min(h[0].log_prob for h in hyps), 3),
                                              "max": round(max(h[0].log_prob for h in hyps), 3)}
        rec["labels_per_transcript"] = {"min": min(len(v) for v in got["safe"]), "max": max(len(v) for v in got["safe"])}
        out[f"softmax_{scale}_randn"] = rec
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
