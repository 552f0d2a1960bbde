#!/usr/bin/env python3
"""What a language model costs the CTC prefix beam search (width 8, 501 frames, 29 symbols), arms alternating in one process.

  a  model-free decode (separator + word weight only)
  b  the n-gram model resident on the device: ``CTCBeamDecoder(language_model=NGramLanguageModel)``, one launch
  c  the host-model path given ``lm.weighted_callable(lm_weight)`` and lm_weight 1.0: identical factors, the kernel stopped
     at every frame whose separator survives pruning

on (i) ``softmax(randn(501, N, 29) * 12)``, N = 4 and 32 -- random posteriors spell mostly out-of-vocabulary words: the
<unk> / back-off walk -- and (ii) the sentence-shaped posteriors of tests/ngram_lm_cases.py tiled to 120 frames (words of the
vocabulary; the search is the reference's linear float32 arithmetic, and with a factor below 1 per word on top of the
acoustics these sentences underflow to an EMPTY beam from ~150 frames on, which would time nothing).  Every decode ends in a device synchronise (the transcripts are read back); the figure is host-clock ms.

    python tools/beam_lm_time.py [--repeats 7] [--out profiles/beam_lm_time.json] [--arms abc] [--commit ID]

Kernel times come from a separate run: ``rocprofv3 --kernel-trace --stats -- python tools/beam_lm_time.py --arms ab``.
There is no CPU path: without a HIP device the tool fails.
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

WIDTH, THR, LM_WEIGHT, WORD_WEIGHT, BLANK, SEP, ORDER = 8, 1e-3, 1.3, 1.2, 28, 0, 3


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def workloads():
    import ngram_lm_cases as C
    out = []
    for n in (4, 32):
        torch.manual_seed(5)
        x = torch.softmax(torch.randn(501, n, 29) * 12, dim=2)
        out.append((f"random_n{n}", x.cuda(), torch.full((n,), 501, dtype=torch.int64)))
    x, lens = C.sentence_posteriors(tile_to=120)
    out.append(("sentences_n4_120_frames", torch.from_numpy(x).cuda(), torch.from_numpy(lens)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--arms", default="abc")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("beam_lm_time: a HIP device is required; there is no CPU path")
    import ngram_lm_cases as C
    from myrtlespeech_amd import _lib
    from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
    # (<unk> at 10 ** -0.05: with the tests' 10 ** -2.4 the fifty out-of-vocabulary words of a random clip underflow the linear
    # float32 search to an empty beam, and a search that has ended times nothing; the look-ups do not depend on the values)
    lm = C.decoder_model(ORDER, unk_log10_p=-0.05)
    lib = _lib.load()
    out = {"tool": "tools/beam_lm_time.py", "commit": a.commit, "beam_width": WIDTH, "prune_threshold": THR,
           "lm_weight": LM_WEIGHT, "word_weight": WORD_WEIGHT, "model": repr(lm), "table_bytes": int(lm.packed(LM_WEIGHT).size),
           "statistic": "host clock of one decode that ends with its transcripts on the host, ms; the arms alternate in one "
                        "process after one untimed decode each",
           "arms": {"a": "model-free", "b": "n-gram model on the device (one launch)",
                    "c": "host-model path with lm.weighted_callable (identical factors)"}}
    for name, x, lens in workloads():
        decs = {"a": CTCBeamDecoder(BLANK, WIDTH, THR, separator_index=SEP, word_weight=WORD_WEIGHT),
                "b": CTCBeamDecoder(BLANK, WIDTH, THR, language_model=lm, lm_weight=LM_WEIGHT, separator_index=SEP,
                                    word_weight=WORD_WEIGHT),
                "c": CTCBeamDecoder(BLANK, WIDTH, THR, language_model=lm.weighted_callable(LM_WEIGHT), lm_weight=1.0,
                                    separator_index=SEP, word_weight=WORD_WEIGHT)}
        arms = [k for k in "abc" if k in a.arms]
        got = {k: decs[k](x, lens) for k in arms}                      # untimed; and the arms agree
        if "b" in got and "c" in got and got["b"] != got["c"]:
            sys.exit(f"beam_lm_time: {name}: the device model and the host path disagree")
        ms = {k: [] for k in arms}
        for _ in range(a.repeats):
            for k in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                decs[k](x, lens)
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        rec = {f"{k}_ms": spread(v) for k, v in ms.items()}
        # (a beam that runs empty -- float32 underflow -- ends its utterance's search early: such a decode times less work)
        rec["utterances_whose_beam_ran_empty"] = {k: sum(len(v) == 0 for v in got[k]) for k in arms}
        n = x.shape[1]
        need = ~(x[:, :, SEP].cpu() <= torch.tensor(THR, dtype=torch.float32)) & (torch.arange(x.shape[0])[:, None] < lens[None, :])
        rec["frames_that_consult_the_model"] = {"all_utterances": int(need.sum()), "busiest_utterance": int(need.sum(0).max())}
        if "b" in arms:
            per_utt = lib.ms_ctc_beam_lm_workspace_bytes(x.shape[0], 1, 29, WIDTH, lm.order)
            hdr = decs["b"]._workspace.buf[:per_utt * n].view(torch.int32).view(n, per_utt // 4)[:, :16].cpu()
            rec["nodes_made"] = {"all_utterances": int(hdr[:, 0].sum()), "busiest_utterance": int(hdr[:, 0].max())}
            rec["factors_computed"] = {"all_utterances": int(hdr[:, 13].sum()), "busiest_utterance": int(hdr[:, 13].max())}
            rec["transcripts_changed_by_the_model"] = sum(p != q for p, q in zip(got.get("a", got["b"]), got["b"]))
        if "a" in arms and "b" in arms:
            # (the model changes the search -- other prefixes survive, other candidate counts per frame -- so this difference is
            # not the price of the look-ups; the stamped S0 phase below is)
            rec["b_minus_a_ms"] = round(statistics.median(ms["b"]) - statistics.median(ms["a"]), 4)
        # where the frame goes: one stamped decode of arms a and b (utterance 0's thread 0 sums the 100 MHz wall clock per
        # barrier-separated phase, csrc/beam.hip MS_BEAM_STAMPS); S0 is the language-model phase
        names = ["top", "S1", "S2", "S3", "S4a", "S4b", "S5", "S6", "S0_language_model"]
        frames0 = int(lens[0])
        os.environ["MS_BEAM_STAMPS"] = "1"
        for k in [k for k in "ab" if k in arms]:
            decs[k](x, lens)
            torch.cuda.synchronize()
            h0 = decs[k]._workspace.buf[:64].view(torch.int32).cpu().tolist()
            rec[f"{k}_ns_per_frame_by_phase_utterance_0"] = {nm: round(h0[4 + i] * 10.0 / frames0, 1) for i, nm in enumerate(names)
                                                            if k == "b" or i < 8}
            if k == "b":
                consult0, factors0 = int(need[:, 0].sum()), h0[13]
                rec["S0_utterance_0"] = {"us": round(h0[12] * 0.01, 2), "frames_that_consult_the_model": consult0,
                                         "factors_computed": factors0,
                                         "us_per_consulting_frame": round(h0[12] * 0.01 / max(consult0, 1), 3),
                                         "us_per_factor": round(h0[12] * 0.01 / max(factors0, 1), 3)}
        os.environ["MS_BEAM_STAMPS"] = "0"
        if "b" in arms and "c" in arms:
            rec["c_over_b"] = round(statistics.median(ms["c"]) / statistics.median(ms["b"]), 2)
            rec["host_model_calls"], rec["host_model_stops"] = decs["c"].lm_calls, decs["c"].lm_frames
        out[name] = rec
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
