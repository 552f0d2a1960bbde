"""numpy restatement of ms_ctc_greedy_stream_step's specification (include/ms_hotpath.h) and the seeded inputs the
streaming-decode tests share.  A test helper: the expectations themselves come from the whole-clip decoders."""
import numpy as np


class GreedyStreamRef:
    """State: per stream the symbol of its previous existing row (None at the start), its labels, the frames at which
    their runs began, and its rows seen."""

    def __init__(self, batch, blank, cap, total_lens=None):
        self.N, self.blank, self.cap = batch, blank, cap
        self.total = None if total_lens is None else [int(v) for v in total_lens]
        self.prev = [None] * batch
        self.labels = [[] for _ in range(batch)]
        self.frames = [[] for _ in range(batch)]
        self.count = [0] * batch
        self.seen = [0] * batch
        self.overflow = False

    def step(self, x, chunk_lens=None):
        """x [rows, n, V]: the next rows of the first n streams; returns the labels appended per stream of the batch."""
        rows, n, _ = x.shape
        assert n <= self.N and (chunk_lens is None) != (self.total is None)
        news = [[] for _ in range(self.N)]
        for i in range(n):
            exist = int(chunk_lens[i]) if chunk_lens is not None else self.total[i] - self.seen[i]
            exist = min(max(exist, 0), rows)
            for r in range(exist):
                row = x[r, i]
                nan = np.isnan(row)
                sym = int(np.argmax(nan)) if nan.any() else int(np.argmax(row))     # first NaN, else first maximum
                if sym != self.blank and sym != self.prev[i]:
                    if self.count[i] < self.cap:
                        self.labels[i].append(sym)
                        self.frames[i].append(self.seen[i] + r)
                        news[i].append(sym)
                    else:
                        self.overflow = True
                    self.count[i] += 1
                self.prev[i] = sym
            self.seen[i] += exist
        return news


def run_chunked(x, lens, blank, chunk, cap=None):
    """Feed x [T, N, V] to the restatement `chunk` rows at a time (total_lens addressing); returns the object."""
    T, N, _ = x.shape
    ref = GreedyStreamRef(N, blank, cap or max(T, 1), total_lens=lens)
    for t0 in range(0, T, chunk):
        ref.step(x[t0:t0 + chunk])
    return ref


def boundary_inputs(seed=20261016, T=203, N=6, V=9, lens=(203, 203, 150, 97, 16, 0)):
    """Inputs whose runs span chunk boundaries: per stream, runs of 1 .. 4 rows of one symbol, each row normal noise with
    +6 on the run's symbol.  Returns (x [T, N, V] float32, lens int64, blank = V - 1)."""
    rng = np.random.default_rng(seed)
    x = np.empty((T, N, V), dtype=np.float32)
    for n in range(N):
        t = 0
        while t < T:
            run = int(rng.integers(1, 5))
            sym = int(rng.integers(0, V))
            for _ in range(min(run, T - t)):
                row = rng.normal(size=V).astype(np.float32)
                row[sym] += np.float32(6.0)
                x[t, n] = row
                t += 1
    return x, np.asarray(lens, dtype=np.int64), V - 1


def spanning_runs(x, lens, blank, chunk):
    """Non-blank runs of the per-row arg max that continue across a multiple of `chunk` inside the stream's length."""
    am = x.argmax(-1)
    count = 0
    for n, ln in enumerate(lens):
        for t in range(chunk, int(ln), chunk):
            if am[t, n] == am[t - 1, n] and am[t, n] != blank:
                count += 1
    return count


def stitched_stateless(x, lens, blank, chunk, whole_clip_decode):
    """What a caller of the whole-clip decoder gets who decodes every chunk on its own and joins the lists."""
    T, N, _ = x.shape
    out = [[] for _ in range(N)]
    for t0 in range(0, T, chunk):
        cl = np.clip(np.asarray(lens) - t0, 0, min(chunk, T - t0))
        for n, lab in enumerate(whole_clip_decode(x[t0:t0 + chunk], cl, blank)):
            out[n] += lab
    return out


def ragged_sorted_lens(rng, T, N):
    """Sorted lengths in [0, T]: the longest is T, the shortest 0."""
    lens = np.sort(rng.integers(1, T + 1, size=N))[::-1].astype(np.int64)
    lens[0] = T
    if N > 1:
        lens[-1] = 0
    return lens
