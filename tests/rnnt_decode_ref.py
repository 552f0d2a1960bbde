"""float64 restatement of the RNN-T greedy and beam decode (``oracle/rnnt_oracle.py``, ``include/ms_hotpath.h``) that also
reports HOW CLOSE every discrete decision was (TEST INFRASTRUCTURE ONLY).

The decode's outputs are label lists: a float32 reference says nothing about whether a device transcript that differs is
wrong or merely on the other side of a near-tie.  This one takes the modules' float32 weights upcast to float64, follows the
header's list rules (list order, first arrival keeps its state, ties to the lowest flat index, blank transitions of equal
prefixes merged by logaddexp) with plain loops and returns, per utterance, the smallest gap over every MEMBERSHIP decision:

* greedy: top-1 minus top-2 logit at every scored (frame, prefix);
* beam: the ``w``-th against the ``(w+1)``-th finite candidate of every extension round, the ``w``-th against the
  ``(w+1)``-th entry of B at every frame end, best against second best at the finish.

The ORDER inside a selected set is not a decision: it moves entries inside the lists, and equal prefixes carry equal predictor
states, so neither a later membership nor a merged score depends on it.  A case whose margins all exceed twice the device's
score error therefore has exactly one right transcript.
"""
from typing import Dict, List, Sequence

import numpy as np

F64 = np.float64
GREEDY_CHUNK = 32      # frames a greedy iteration scores per utterance (csrc/rnnt_decode.hip)


class Net:
    """The prediction and joint networks' weights in float64, any number of layers ``L``."""

    def __init__(self, pred_sd: Dict[str, np.ndarray], joint_sd: Dict[str, np.ndarray], layers: int, zero_bias: bool = False):
        up = lambda a: np.asarray(a, dtype=F64)
        self.L = layers
        self.emb = up(pred_sd["embedding.weight"])
        self.V = self.emb.shape[0] - 1
        self.wih = [up(pred_sd[f"rnn.rnn.weight_ih_l{l}"]) for l in range(layers)]
        self.whh = [up(pred_sd[f"rnn.rnn.weight_hh_l{l}"]) for l in range(layers)]
        self.b = [up(pred_sd[f"rnn.rnn.bias_ih_l{l}"]) + up(pred_sd[f"rnn.rnn.bias_hh_l{l}"]) for l in range(layers)]
        if zero_bias:
            self.b = [np.zeros_like(b) for b in self.b]
        self.H = self.whh[0].shape[1]
        self.we, self.be = up(joint_sd["enc_proj.weight"]), up(joint_sd["enc_proj.bias"])
        self.wp = up(joint_sd["pred_proj.weight"])
        self.wo, self.bo = up(joint_sd["out.weight"]), up(joint_sd["out.bias"])

    def zero_state(self):
        return [np.zeros(self.H)] * self.L, [np.zeros(self.H)] * self.L

    def step(self, label: int, state):
        """One prediction-network step: embedding -> L LSTM cells (gates i, f, g, o) -> pred_proj."""
        H = self.H
        x, (h, c) = self.emb[label], state
        nh, nc = [], []
        for l in range(self.L):
            g = self.wih[l] @ x + self.whh[l] @ h[l] + self.b[l]
            i, f, o = (1.0 / (1.0 + np.exp(-g[k * H:(k + 1) * H])) for k in (0, 1, 3))
            cc = f * c[l] + i * np.tanh(g[2 * H:3 * H])
            x = o * np.tanh(cc)
            nh.append(x)
            nc.append(cc)
        return self.wp @ x, (nh, nc)

    def project(self, enc: np.ndarray) -> np.ndarray:
        return np.asarray(enc, dtype=F64) @ self.we.T + self.be

    def logits(self, enc_p_vec: np.ndarray, pred_p: np.ndarray) -> np.ndarray:
        return self.wo @ np.tanh(enc_p_vec + pred_p) + self.bo


def log_softmax(x: np.ndarray) -> np.ndarray:
    m = x.max()
    return x - m - np.log(np.exp(x - m).sum())


def chunked_walk(labels_per_frame: Sequence[int], max_symbols: int):
    """The greedy decode's iterations for one utterance whose frame t emits ``labels_per_frame[t]`` labels: an iteration walks
    up to GREEDY_CHUNK frames from the current one and stops at the first label; ``max_symbols`` labels on one frame advance
    the frame.  Returns (iterations until the frame reaches the length -- zero for an empty utterance --, the chunk rows at
    which a frame used its whole quota)."""
    n, t, nsym, iters, quota_rows = len(labels_per_frame), 0, 0, 0, []
    while t < n:
        iters += 1
        for c in range(GREEDY_CHUNK):
            if t >= n:
                break
            if nsym < labels_per_frame[t]:
                nsym += 1
                if nsym >= max_symbols:
                    quota_rows.append(c)
                    t, nsym = t + 1, 0
                break
            t, nsym = t + 1, 0
    return iters, quota_rows


def greedy_decode(net: Net, enc: np.ndarray, lens: Sequence[int], max_symbols: int) -> List[dict]:
    """Per utterance: ``hyp``, ``margin`` (top-1 minus top-2 logit over every scored pair), ``labels_per_frame``,
    ``quota_frames_mod32`` (frame index mod 32 of every frame that used its whole quota), ``quota_rows`` (the row of the
    iteration's chunk at which that happened) and ``iterations`` (of the chunked walk)."""
    enc_p = net.project(enc)
    blank, out = net.V, []
    for n in range(enc.shape[1]):
        hyp, margin, per_frame = [], np.inf, []
        pred, state = net.step(blank, net.zero_state())
        for t in range(int(lens[n])):
            k_t = 0
            for _ in range(max_symbols):
                lg = net.logits(enc_p[t, n], pred)
                order = np.argsort(-lg, kind="stable")
                margin = min(margin, lg[order[0]] - lg[order[1]])
                k = int(order[0])
                if k == blank:
                    break
                hyp.append(k)
                k_t += 1
                pred, state = net.step(k, state)
            per_frame.append(k_t)
        iters, rows = chunked_walk(per_frame, max_symbols)
        out.append(dict(hyp=hyp, margin=float(margin), labels_per_frame=per_frame, iterations=iters, quota_rows=rows,
                        quota_frames_mod32=sorted({t % GREEDY_CHUNK for t, k in enumerate(per_frame) if k == max_symbols})))
    return out


def beam_decode(net: Net, enc: np.ndarray, lens: Sequence[int], beam_width: int, max_symbols: int) -> List[dict]:
    """Per utterance: ``hyp``, ``score``, ``margin`` and the path statistics ``max_b`` (largest B), ``merges`` (logaddexp
    merges), ``max_live`` (largest live set), ``last_selected`` (the highest position in B, in arrival order, of a survivor of a
    frame end; ``best_last_selected``: the same over the returned hypothesis' own ancestors, so that it is what the output shows),
    ``moved`` (survivors of a frame end that were not the frame-start hypothesis of
    the same position), ``labels_per_frame`` (of the returned hypothesis) and ``blank_sum`` (the root hypothesis' blank
    log-probabilities added over the frames: the score when ``max_symbols == 1``)."""
    enc_p = net.project(enc)
    blank, w, out = net.V, beam_width, []
    for n in range(enc.shape[1]):
        pred0, st0 = net.step(blank, net.zero_state())
        # a hypothesis: (prefix, score, state, projected predictor output, emission frames, where its state lives, the highest
        # position in B from which it or an ancestor was selected)
        beam = [((), 0.0, st0, pred0, (), ("start", 0), 0)]
        margin, max_b, merges, max_live, moved, blank_sum, last_sel = np.inf, 0, 0, 1, 0, 0.0, 0
        for t in range(int(lens[n])):
            A = list(beam)
            B: Dict[tuple, list] = {}
            order: List[tuple] = []
            blank_sum += log_softmax(net.logits(enc_p[t, n], pred0))[blank]
            for v in range(max_symbols):
                if not A:
                    break
                max_live = max(max_live, len(A))
                lps = [log_softmax(net.logits(enc_p[t, n], h[3])) for h in A]
                for h, lp in zip(A, lps):
                    s = h[1] + lp[blank]
                    if h[0] in B:
                        B[h[0]][0] = np.logaddexp(B[h[0]][0], s)
                        merges += 1
                    else:
                        B[h[0]] = [s, h]
                        order.append(h[0])
                if v == max_symbols - 1:
                    break
                cand = np.stack([h[1] + lp for h, lp in zip(A, lps)])
                cand[:, blank] = -np.inf
                flat = cand.reshape(-1)
                idx = np.argsort(-flat, kind="stable")
                if len(idx) > w and np.isfinite(flat[idx[w]]):
                    margin = min(margin, flat[idx[w - 1]] - flat[idx[w]])
                A_new = []
                for q, i in enumerate(idx[:w]):
                    if not np.isfinite(flat[i]):
                        continue
                    hi, k = divmod(int(i), cand.shape[1])
                    h = A[hi]
                    pred, st = net.step(k, h[2])
                    A_new.append((h[0] + (k,), float(flat[i]), st, pred, h[4] + (t,), ("round", v, q), h[6]))
                A = A_new
            max_b = max(max_b, len(order))
            items = [(p, B[p], at) for at, p in enumerate(order)]
            items.sort(key=lambda it: -it[1][0])          # stable: ties keep first-arrival order
            last_sel = max([last_sel] + [at for _, _, at in items[:w]])
            if len(items) > w:
                margin = min(margin, items[w - 1][1][0] - items[w][1][0])
            beam = []
            for q, (p, (s, h), at) in enumerate(items[:w]):
                moved += h[5] != ("start", q)
                beam.append((p, float(s), h[2], h[3], h[4], ("start", q), max(h[6], at)))
        scores = sorted((b[1] for b in beam), reverse=True)
        if len(scores) > 1:
            margin = min(margin, scores[0] - scores[1])
        best = max(range(len(beam)), key=lambda i: (beam[i][1], -i))
        frames = beam[best][4]
        out.append(dict(hyp=list(beam[best][0]), score=float(beam[best][1]), margin=float(margin), max_b=max_b, merges=merges,
                        max_live=max_live, moved=int(moved), blank_sum=float(blank_sum), last_selected=last_sel,
                        best_last_selected=beam[best][6],
                        labels_per_frame=[sum(1 for f in frames if f == t) for t in range(int(lens[n]))]))
    return out
