#!/usr/bin/env python3
"""What the streaming decoders add to a chunk of the carried-context leg, measured in one process.

The workload is ``tools/bench_configs.py::leg_stream_context``'s: the shipped architecture (2 x conv2d, 3 x GRU-2560,
lookahead 80, FC 1024), 32 streams, 32-frame chunks, ``ChunkedDeepSpeech2(carry_context=True)`` with its HIP-graph replays.
A REGION is one pass over the clip: 8 untimed pushes (the held-back context fills, the graph attaches), then ``--chunks``
timed pushes, the last of which flushes; its figure is host-clock milliseconds per chunk over work that ends in a device
synchronise.  Regions alternate between the arms on the same resident inputs, after one untimed region per arm:

  A0  push alone, one synchronise at the end of the region (``leg_stream_context``'s own loop)
  A   push + a synchronise per chunk (a consumer that looks at every chunk's rows: the base line of B and C)
  B   push + the streaming decoder on the rows + its read-back per chunk
      greedy: ``StreamingCTCGreedyDecoder.push(rows).result()``; beam: softmax + ``StreamingCTCBeamDecoder.push`` + ``best()``
  C   push + the whole-clip decoder on the chunk's rows alone + its read-back per chunk (what a caller could do with a chunk
      before: stateless, wrong across chunk boundaries)
      greedy: ``CTCGreedyDecoder.launch(rows, lens).result()``; beam: softmax + ``CTCBeamDecoder(rows, lens)``

    python tools/stream_decode_time.py [--decoder greedy|beam|both] [--arm A0|A|B|C|all] [--regions 7] [--chunks 24]
                                       [--commit ID] [--no-calibration] [--out FILE]

Kernel times come from a separate run: ``rocprofv3 --kernel-trace --stats -- python tools/stream_decode_time.py --arm B``
(the step kernel is ``ctc_greedy_stream_kernel``).  There is no CPU path: without a HIP device the tool fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tools")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import torch  # noqa: E402

N, CHUNK, WARM_PUSHES, BEAM_WIDTH, BLANK = 32, 32, 8, 8, 28


def shipped_model():
    """``leg_stream_context``'s model, seed included."""
    from myrtlespeech_amd.model.cnn import MaskConv2d, PaddingMode
    from myrtlespeech_amd.model.deep_speech_2 import DeepSpeech2
    from myrtlespeech_amd.model.fully_connected import FullyConnected
    from myrtlespeech_amd.model.lookahead import Lookahead
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    from myrtlespeech_amd.model.seq_len_wrapper import SeqLenWrapper

    def act():
        return SeqLenWrapper(torch.nn.Hardtanh(0.0, 20.0), torch.nn.Identity())
    torch.manual_seed(7)
    cnn = torch.nn.Sequential(MaskConv2d(1, 32, [41, 11], [2, 2], PaddingMode.SAME), act(),
                              MaskConv2d(32, 32, [21, 11], [2, 1], PaddingMode.SAME), act())
    rnn = RNN(RNNType.GRU, 640, 2560, num_layers=3, bidirectional=False)
    la = torch.nn.Sequential(Lookahead(2560, 80), SeqLenWrapper(torch.nn.Identity(), torch.nn.Identity()))
    fc = FullyConnected(2560, 29, 1, 1024, torch.nn.Hardtanh(0.0, 20.0))
    m = DeepSpeech2(cnn, rnn, la, fc).eval()
    m.rnn.check_status = False
    return m


class Bench:
    def __init__(self, chunks):
        from myrtlespeech_amd import _lib
        from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
        from myrtlespeech_amd.post_process.ctc_greedy_decoder import CTCGreedyDecoder
        from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder, StreamingCTCGreedyDecoder
        from myrtlespeech_amd.streaming import ChunkedDeepSpeech2
        self._lib = _lib
        self.chunks = chunks
        self.total = CHUNK * (chunks + WARM_PUSHES)
        g = torch.Generator().manual_seed(8)
        self.x = torch.randn(N, 1, 80, self.total, generator=g).cuda()
        self.lens = torch.full((N,), self.total, dtype=torch.int64)
        self.st = ChunkedDeepSpeech2(shipped_model(), CHUNK, carry_context=True)
        self.stream_greedy, self.stream_beam = StreamingCTCGreedyDecoder(BLANK), StreamingCTCBeamDecoder(BLANK, BEAM_WIDTH)
        self.clip_greedy, self.clip_beam = CTCGreedyDecoder(BLANK), CTCBeamDecoder(BLANK, BEAM_WIDTH)
        self._chunk_lens = {}
        self.labels = 0

    def chunk_lens(self, rows):
        """Device lengths of a chunk whose every stream has all `rows` rows, with their host values attached."""
        if rows not in self._chunk_lens:
            self._chunk_lens[rows] = self._lib.lens_to_device(torch.full((N,), rows, dtype=torch.int64))
        return self._chunk_lens[rows]

    def region(self, arm, decoder):
        """One pass over the clip; returns host-clock ms per timed chunk."""
        st = self.st
        st.begin(self.lens, self.total)
        greedy = decoder == "greedy"
        if arm == "B":
            if greedy:
                self.stream_greedy.begin(N, max(st.total_out, 1), total_lens=st.out_lens)
            else:
                self.stream_beam.begin(st.out_lens, max(st.total_out, 1))
        dec = self.stream_greedy if greedy else self.stream_beam

        def consume(rows):
            if arm == "A0":
                return
            if arm == "A" or rows is None:
                if arm == "A":
                    torch.cuda.current_stream().synchronize()
                elif arm == "B" and greedy:
                    dec.push(None)
                return
            if arm == "B":
                if greedy:
                    self.labels += sum(len(v) for v in dec.push(rows).result())
                else:
                    dec.push(torch.softmax(rows, -1))
                    self.labels += sum(len(v) for v in dec.best())
            else:
                lens = self.chunk_lens(rows.shape[0])
                if greedy:
                    self.labels += sum(len(v) for v in self.clip_greedy.launch(rows, lens).result())
                else:
                    self.labels += sum(len(v) for v in self.clip_beam(torch.softmax(rows, -1), lens))

        t0 = 0
        with torch.no_grad():
            for _ in range(WARM_PUSHES):
                consume(st.push(self.x[..., t0:t0 + CHUNK]))
                t0 += CHUNK
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            for k in range(self.chunks):
                consume(st.push(self.x[..., t0:t0 + CHUNK], final=(k == self.chunks - 1)))
                t0 += CHUNK
            torch.cuda.synchronize()
            return (time.perf_counter() - w0) / self.chunks * 1e3


def spread(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4), "regions": len(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--decoder", choices=["greedy", "beam", "both"], default="both")
    ap.add_argument("--arm", choices=["A0", "A", "B", "C", "all"], default="all")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--chunks", type=int, default=24)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--no-calibration", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stream_decode_time: a HIP device is required; there is no CPU path")
    import bench
    arms = ["A0", "A", "B", "C"] if a.arm == "all" else [a.arm]
    decoders = ["greedy", "beam"] if a.decoder == "both" else [a.decoder]
    b = Bench(a.chunks)
    out = {"tool": "tools/stream_decode_time.py", "commit": a.commit, "precision": bench.precision_label(),
           "workload": f"shipped DS2 (3xGRU-2560 + lookahead 80) with carried context, {N} streams, {CHUNK}-frame chunks, "
                       f"{a.chunks} timed chunks per region after {WARM_PUSHES} untimed pushes",
           "statistic": "host clock over a region that ends in a device synchronise, ms per chunk; regions alternate between "
                        "the arms in one process",
           "beam_width": BEAM_WIDTH}
    if not a.no_calibration:
        import bench_configs as bc
        cal = {"barrier_step_us": round(bc.barrier_step_us(), 4)}
        try:
            cal["shader_clock_under_gemm_ghz"] = round(bc.shader_clock_under_projection_ghz(), 4)
        except Exception as e:  # noqa: BLE001 -- a calibration figure, never a reason to lose the measurement
            cal["shader_clock_error"] = f"{type(e).__name__}: {e}"[:200]
        out["calibration"] = cal
    for decoder in decoders:
        for arm in arms:                                   # every shape of every arm once, untimed
            if not (arm in ("A0", "A") and decoder != decoders[0]):
                b.region(arm, decoder)
        ms = {arm: [] for arm in arms}
        for _ in range(a.regions):
            for arm in arms:
                ms[arm].append(b.region(arm, decoder))
        rec = {f"{arm}_ms_per_chunk": spread(v) for arm, v in ms.items()}
        if "A" in ms:
            for arm in ("B", "C"):
                if arm in ms:
                    rec[f"{arm}_minus_A_ms"] = round(statistics.median(ms[arm]) - statistics.median(ms["A"]), 4)
                    rec[f"{arm}_minus_A_ms_per_region"] = [round(x - y, 4) for x, y in zip(ms[arm], ms["A"])]
        out[decoder] = rec
    out["hip_graph_replays"], out["hip_graph_error"] = b.st.graph_replays, b.st.graph_error
    out["labels_read_back"] = b.labels
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
