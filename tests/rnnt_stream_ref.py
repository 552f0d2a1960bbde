"""float64 numpy restatement of ms_rnnt_greedy_stream_begin / _step (include/ms_hotpath.h): the greedy loop of
oracle/rnnt_oracle.py::greedy_decode with an explicit carried state, cut between frames, and the seeded cases the streaming
transducer tests share.  A test helper.  Besides labels and emission frames it records the MARGIN: the smallest gap between
the best and the second-best logit over every decision taken -- a float32 / f16x3 device can only be held to a float64 arg
max away from ties."""
import numpy as np

# id -> (V, E, D, P, J, model seed, data seed, blank bias, max_symbols, steps, lens); two LSTM layers everywhere.
# The label counts and margins of these cases are in the issue that introduced them and are asserted by the tests.
CASES = {
    "A0": (9, 24, 8, 64, 32, 10, 0, 0.0, 1, 150, (150, 97, 64, 33, 0)),
    "A2": (9, 24, 8, 64, 32, 12, 2, 0.5, 3, 150, (150, 97, 64, 33, 0)),
    "A4": (9, 24, 8, 64, 32, 14, 4, 1.0, 2, 150, (150, 97, 64, 33, 0)),
    "A5": (9, 24, 8, 64, 32, 15, 5, 1.5, 3, 150, (150, 97, 64, 33, 0)),
    "A6": (9, 24, 8, 64, 32, 16, 6, 30.0, 3, 150, (150, 97, 64, 33, 0)),
    "B24": (300, 24, 16, 96, 96, 24, 24, 1.0, 3, 70, (70, 41, 32, 1)),
    "B25": (300, 24, 16, 96, 96, 25, 25, 1.0, 3, 70, (70, 41, 32, 1)),
    "C32": (29, 40, 32, 128, 64, 32, 32, 1.0, 2, 100, (100, 99, 67, 35, 31, 2)),
    # beside the issue's cases: D, P and J that are no multiples of 4 or 16 (the kernels' scalar loads, a ragged last K step);
    # seed chosen on the CPU with this restatement, margin 3.27e-3
    "S42": (9, 24, 10, 66, 34, 42, 42, 1.0, 2, 70, (70, 41, 32, 1)),
    # ... and a joint wider than the 1024 units whose tanh rows the score kernel holds in LDS at once, with more than four
    # column blocks of symbols, so that the rows are formed slab by slab and again for the second group of blocks (margin 1.40e-2)
    "W53": (140, 24, 8, 64, 1040, 53, 53, 1.0, 2, 40, (40, 17)),
}
LABEL_COUNTS = {
    "A0": [136, 87, 58, 30, 0], "A2": [318, 222, 144, 66, 0], "A4": [52, 42, 20, 12, 0], "A5": [0, 4, 0, 3, 0],
    "A6": [0, 0, 0, 0, 0], "B24": [132, 78, 60, 3], "B25": [96, 54, 45, 0], "C32": [70, 84, 50, 20, 26, 2],
    "S42": [36, 16, 26, 2], "W53": [44, 24],
}
CHUNKS = (1, 7, 32, 33, None)      # None: the whole clip in one push
MARGIN_FLOOR = 1e-4                # the project's tolerance on the joint's log-probabilities (test_rnnt_kernels_vs_numpy)
LAYERS = 2


def build_case(name):
    """(predictor, joint, enc [steps, N, E] float32, lens int64, case tuple): modules as tests/test_gpu_parity.py::_rnnt_parts
    makes them (on the GPU when there is one)."""
    import torch
    from myrtlespeech_amd.model.rnnt import RNNTJoint, RNNTPredictor
    V, E, D, P, J, mseed, dseed, bias, ms, steps, lens = CASES[name]
    torch.manual_seed(mseed)
    pred = RNNTPredictor(V, D, P, num_layers=LAYERS).eval()
    joint = RNNTJoint(E, P, J, V).eval()
    with torch.no_grad():
        joint.out.bias[V] += bias
    enc = (np.random.default_rng(dseed).normal(size=(steps, len(lens), E)) * 2.0).astype(np.float32)
    return pred, joint, enc, np.array(lens, dtype=np.int64), CASES[name]


def state_dicts(pred, joint):
    cpu = lambda v: v.detach().cpu().numpy()
    return {k: cpu(v) for k, v in pred.state_dict().items()}, {k: cpu(v) for k, v in joint.state_dict().items()}


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


class RNNTGreedyStreamRef:
    def __init__(self, pred_sd, joint_sd, hidden, layers, blank, max_symbols):
        f = lambda a: np.asarray(a, dtype=np.float64)
        self.emb = f(pred_sd["embedding.weight"])
        self.w_ih = [f(pred_sd[f"rnn.rnn.weight_ih_l{l}"]) for l in range(layers)]
        self.w_hh = [f(pred_sd[f"rnn.rnn.weight_hh_l{l}"]) for l in range(layers)]
        self.b = [f(pred_sd[f"rnn.rnn.bias_ih_l{l}"]) + f(pred_sd[f"rnn.rnn.bias_hh_l{l}"]) for l in range(layers)]
        self.w_enc, self.b_enc = f(joint_sd["enc_proj.weight"]), f(joint_sd["enc_proj.bias"])
        self.w_pred = f(joint_sd["pred_proj.weight"])
        self.w_out, self.b_out = f(joint_sd["out.weight"]), f(joint_sd["out.bias"])
        self.H, self.L, self.blank, self.max_symbols = hidden, layers, blank, max_symbols
        self.N = None

    def _predictor(self, label, state):
        """One step on `label` from state (h [L, H], c [L, H]) -> (pred_p [J], new state)."""
        h, c = state
        x = self.emb[label]
        hn, cn = np.empty_like(h), np.empty_like(c)
        for l in range(self.L):
            g = self.w_ih[l] @ x + self.w_hh[l] @ h[l] + self.b[l]
            i, fg, gg, o = np.split(g, 4)
            cn[l] = _sigmoid(fg) * c[l] + _sigmoid(i) * np.tanh(gg)
            hn[l] = _sigmoid(o) * np.tanh(cn[l])
            x = hn[l]
        return self.w_pred @ x, (hn, cn)

    def begin(self, batch, cap=None, total_lens=None):
        zero = (np.zeros((self.L, self.H)), np.zeros((self.L, self.H)))
        pp, st = self._predictor(self.blank, zero)            # the same for every stream
        self.N, self.cap = batch, cap
        self.total = None if total_lens is None else [int(v) for v in total_lens]
        self.pp = [pp.copy() for _ in range(batch)]
        self.state = [(st[0].copy(), st[1].copy()) for _ in range(batch)]
        self.labels = [[] for _ in range(batch)]
        self.frames = [[] for _ in range(batch)]
        self.count = [0] * batch
        self.seen = [0] * batch
        self.overflow = False
        self.margin = np.inf
        self.iterations = 0        # score + predictor-step rounds a device that scores 32 pending frames at once needs

    def push(self, rows, lens=None):
        """rows [r, n, E]: the next encoder rows of the first n streams; returns the labels appended per stream."""
        r_max, n, _ = rows.shape
        assert n <= self.N and (lens is None) != (self.total is None)
        news = [[] for _ in range(self.N)]
        iters = 0
        for i in range(n):
            exist = int(lens[i]) if lens is not None else self.total[i] - self.seen[i]
            exist = min(max(exist, 0), r_max)
            e = np.asarray(rows[:exist, i], dtype=np.float64) @ self.w_enc.T + self.b_enc
            emitted_at = []                                    # rows of this push that emitted, one entry per label
            for r in range(exist):
                for _ in range(self.max_symbols):
                    x = self.w_out @ np.tanh(e[r] + self.pp[i]) + self.b_out
                    k = int(np.argmax(x))
                    top = np.partition(x, -2)[-2:]
                    self.margin = min(self.margin, float(top[1] - top[0]))
                    if k == self.blank:
                        break
                    if self.cap is None or self.count[i] < self.cap:
                        self.labels[i].append(k)
                        self.frames[i].append(self.seen[i] + r)
                        news[i].append(k)
                    else:
                        self.overflow = True
                    self.count[i] += 1
                    self.pp[i], self.state[i] = self._predictor(k, self.state[i])
                    emitted_at.append(r)
            iters = max(iters, device_iterations(exist, emitted_at, self.max_symbols))
            self.seen[i] += exist
        self.iterations += iters
        return news


def device_iterations(exist, emitted_at, max_symbols, block=32):
    """Rounds (score `block` pending frames against the current prediction, step the predictor after the first label) that
    the event-driven loop needs for one stream's `exist` rows, given the rows that emitted (one entry per label, in order)."""
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


def run_chunked(ref, enc, lens, chunk, cap=None):
    """Feed enc [T, N, E] to the restatement `chunk` rows at a time (total-lengths addressing); returns the joined news."""
    T, N, _ = enc.shape
    ref.begin(N, cap, total_lens=lens)
    joined = [[] for _ in range(N)]
    for t0 in range(0, T, chunk or T):
        for i, lab in enumerate(ref.push(enc[t0:t0 + (chunk or T)])):
            joined[i] += lab
    return joined
