"""Times the word error rate of an EVAL pass on the host and on the device, and the edit-distance kernels alone.

On peaky [501, 32, 29] posteriors (DeepSpeech2's output for a batch of 32 ten-second clips: a blank-dominated best path that
spells a transcript of about 100 characters close to the reference's), 8 batches a sample:

  host_per_batch     ``CTCGreedyDecoder`` (launch, copy, wait) + ``WordErrorRate.update`` per batch: the reference's arithmetic
  device_per_batch   ``CTCGreedyDecoder.launch_device`` + ``DeviceWordErrorRate.update`` per batch, ONE synchronise after the 8
                     (``value()``: the read-back of the six sums)

and, on the same labels, ``ms_edit_distance`` alone in word and in token mode, and one utterance of 4096 x 4096 tokens.  The
arms of a group alternate in one process after one untimed sample each; the figure is the median of ``--repeats`` (7), min and
max beside it.  The yardstick is ``host_per_batch`` in the same run: the ratio is reported, and the kernel's time per
anti-diagonal (units of the hypothesis + units of the reference + 1 of the longest utterance).  Both arms must report the same
rate, bit for bit, or the tool fails.  No thresholds: the numbers are the output.  There is no CPU path.

    python tools/wer_time.py [--repeats 7] [--out profiles/wer_time.json]
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

T, N, V, BATCHES = 501, 32, 29, 8
SYMBOLS = list(" abcdefghijklmnopqrstuvwxyz'")       # 28 symbols, the separator is label 0, the blank label 28
BLANK = len(SYMBOLS)
LIMIT = 4096


def spread(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5), "repeats": len(v)}


def timed(arms, repeats, calls=1):
    """ms per call: each arm's function makes ``calls`` calls and ends synchronised or is synchronised here."""
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
            ms[k].append((time.perf_counter() - t0) * 1e3 / calls)
    return ms


def make_batches(seed=0):
    """BATCHES x (logits [T, N, V] on the device, frame counts, targets [N, 110] int32, target lengths)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(BATCHES):
        target_lens = rng.integers(90, 111, size=N)
        targets = np.zeros((N, 110), dtype=np.int32)
        logits = np.full((T, N, V), -4.0, dtype=np.float32)
        logits[:, :, BLANK] = 4.0
        for n in range(N):
            row = []
            while len(row) < target_lens[n]:
                row += rng.integers(1, V - 1, size=int(rng.integers(2, 8))).tolist() + [0]
            row = np.asarray(row[:target_lens[n]])
            targets[n, :len(row)] = row
            # the posterior spells the reference with about one label in twelve wrong, every label on frames of its own
            said = np.where(rng.integers(0, 12, size=len(row)) == 0, rng.integers(0, V - 1, size=len(row)), row)
            logits[4 * np.arange(len(row)) + 1, n, said] = 9.0
        logits += 0.1 * rng.standard_normal(logits.shape).astype(np.float32)
        out.append((torch.from_numpy(logits).cuda(), torch.full((N,), T), torch.from_numpy(targets),
                    torch.from_numpy(target_lens.astype(np.int32))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wer_time.json"))
    args = ap.parse_args()
    from myrtlespeech_amd import _lib
    from myrtlespeech_amd.data.alphabet import Alphabet
    from myrtlespeech_amd.post_process import edit_distance
    from myrtlespeech_amd.post_process.ctc_greedy_decoder import CTCGreedyDecoder
    from myrtlespeech_amd.wer import DeviceWordErrorRate, WordErrorRate, WordSegmentor
    _lib.require_gpu()
    alphabet, segmentor, dec = Alphabet(SYMBOLS), WordSegmentor(" "), CTCGreedyDecoder(BLANK)
    data = make_batches()
    rates = {}

    def host():
        wer = WordErrorRate(alphabet, segmentor)
        for x, lens, y, y_lens in data:
            wer.update(dec(x, lens), y, y_lens)
        rates["host"] = wer.value()

    device_wer = DeviceWordErrorRate(alphabet, segmentor)

    def device():
        device_wer.reset()
        for x, lens, y, y_lens in data:
            device_wer.update(dec.launch_device(x, lens), y, y_lens)
        rates["device"] = device_wer.value()

    result = {"shape": {"T": T, "N": N, "V": V, "batches": BATCHES}, "device": torch.cuda.get_device_name(0)}
    ms = timed({"host_per_batch": host, "device_per_batch": device}, args.repeats, calls=BATCHES)
    if rates["host"] != rates["device"]:
        raise SystemExit(f"the two arms disagree: host {rates['host']!r}, device {rates['device']!r}")
    result["wer_percent"] = rates["host"]
    result["eval_ms_per_batch"] = {k: spread(v) for k, v in ms.items()}
    result["host_over_device"] = round(statistics.median(ms["host_per_batch"]) / statistics.median(ms["device_per_batch"]), 3)

    # the kernels alone, on one batch's labels as they lie on the device
    x, lens, y, y_lens = data[0]
    labels, label_lens = dec.launch_device(x, lens)
    y_dev, y_lens_dev = y.cuda(), y_lens.cuda()
    word_counts = edit_distance(labels, label_lens, y_dev, y_lens_dev, separator_index=0, n_symbols=len(SYMBOLS)).cpu()
    token_counts = edit_distance(labels, label_lens, y_dev, y_lens_dev).cpu()
    arms = {"kernel_words": lambda: edit_distance(labels, label_lens, y_dev, y_lens_dev, separator_index=0, n_symbols=len(SYMBOLS)),
            "kernel_tokens": lambda: edit_distance(labels, label_lens, y_dev, y_lens_dev)}
    ms = timed(arms, args.repeats)
    result["kernel_ms"] = {k: spread(v) for k, v in ms.items()}
    for key, counts in (("kernel_words", word_counts), ("kernel_tokens", token_counts)):
        diagonals = int((counts[:, 4] + counts[:, 5]).max()) + 1
        result["kernel_ms"][key]["anti_diagonals_of_the_longest"] = diagonals
        result["kernel_ms"][key]["us_per_anti_diagonal"] = round(statistics.median(ms[key]) * 1e3 / diagonals, 4)

    base = torch.arange(LIMIT + 1, dtype=torch.int32) % 251
    hyp, ref = base[:-1].reshape(1, -1).cuda(), base[1:].reshape(1, -1).cuda()
    one = torch.tensor([LIMIT], dtype=torch.int32, device="cuda")
    if edit_distance(hyp, one, ref, one).cpu().tolist() != [[2, 0, 1, 1, LIMIT, LIMIT]]:
        raise SystemExit("the 4096 x 4096 utterance is wrong")
    ms = timed({"one_utterance_4096x4096_tokens": lambda: edit_distance(hyp, one, ref, one)}, args.repeats)
    result["limit_ms"] = spread(ms["one_utterance_4096x4096_tokens"])
    result["limit_ms"]["us_per_anti_diagonal"] = round(statistics.median(ms["one_utterance_4096x4096_tokens"]) * 1e3 / (2 * LIMIT + 1), 4)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
