"""The range-safe CTC prefix beam search restated in numpy: the reference's loop (ctc_beam_decoder.py:175-258, as
``oracle.ds_oracle.ctc_beam_decode`` restates it in explicit float32) plus the rescaling rule of ``ms_ctc_beam_decode_ex``:

1. frame t has been processed, the new beam ``A_prev`` chosen and found non-empty;
2. ``s0 = dtype(Pb[t][A_prev[0]] + Pnb[t][A_prev[0]])`` -- the raw value, without the word-count factor;
3. if ``s0 < 2^-32``: ``e = floor(log2 s0)`` (the float's unbiased exponent; a subnormal's is the format's smallest, -126 in
   float32), every entry of ``Pb[t]`` and ``Pnb[t]`` is multiplied by ``2^-e`` and ``e`` is added to ``scale_log2``;
4. true value = stored value * 2^scale_log2; nothing else changes.

``dtype=np.float64`` is the twin that needs no rescaling on the test inputs: the same loop in double on the same float32
posteriors, thresholds and factors.  Shared by tests/test_beam_range_cpu.py and tests/test_beam_range_gpu.py."""
import math
from collections import OrderedDict
from typing import Callable, List, NamedTuple, Optional, Tuple

import numpy as np

F32 = np.float32
MIN_EXP = {np.float32: -126, np.float64: -1022}


class Search(NamedTuple):
    beam: List[Tuple[int, ...]]      # the final beam, best first
    scores: np.ndarray               # [len(beam)] dtype: the stored Pb + Pnb of each entry
    scale_log2: int
    rescaled_at: List[int]           # the frames behind which the rule fired


def _n_words(prefix, sep):
    n, prev = 0, None      # (ctc_beam_decoder.py:106-114: a leading separator counts)
    for s in prefix:
        if s == sep and prev != sep:
            n += 1
        prev = s
    return n


def search(x, length, blank_index: int, beam_width: int, prune_threshold: float = 0.001,
           language_model: Optional[Callable[[Tuple[int, ...]], float]] = None, lm_weight: Optional[float] = None,
           separator_index: Optional[int] = None, word_weight: float = 1.0, range_safe: bool = False,
           dtype=np.float32, hook: Optional[Callable] = None) -> Search:
    """One utterance: ``x [T, V]`` float32 posteriors, the first ``length`` rows.

    ``hook(t, scores, keys, pnb_only, order)`` is called once per frame, behind the sort: the sort scores and prefixes of
    ``A_next`` in insertion order, how many of them exist in ``Pnb[t]`` only, and the stable descending order.  It may return
    another order (the tie-break experiments of tests/test_beam_ties_cpu.py); None leaves the search as it is."""
    D = dtype
    ctc = np.asarray(x, dtype=F32)
    V = ctc.shape[1]
    thr = F32(prune_threshold)
    limit = D(2.0 ** -32)
    pb_prev = {(): D(1.0)}
    pnb_prev = {(): D(0.0)}
    a_prev: List[tuple] = [()]
    scale, rescaled_at = 0, []
    zero = D(0)
    for t in range(int(length)):
        pb: "OrderedDict[tuple, np.floating]" = OrderedDict()
        pnb: "OrderedDict[tuple, np.floating]" = OrderedDict()
        in_beam = set(a_prev)
        row = ctc[t]
        p_blank = D(row[blank_index])
        for l in a_prev:
            pb_l = pb_prev.get(l, zero)
            pnb_l = pnb_prev.get(l, zero)
            for c in range(V):
                if row[c] <= thr:
                    continue
                p = D(row[c])
                if c == blank_index:
                    pb[l] = D(pb.get(l, zero) + D(p * D(pb_l + pnb_l)))
                else:
                    lp = l + (c,)
                    if len(l) > 0 and c == l[-1]:
                        pnb[lp] = D(pnb.get(lp, zero) + D(p * pb_l))
                        pnb[l] = D(pnb.get(l, zero) + D(p * pnb_l))
                    else:
                        plp = D(p * D(pb_l + pnb_l))
                        if separator_index is not None and language_model is not None and c == separator_index:
                            plp = D(plp * D(F32(language_model(lp) ** lm_weight)))
                        pnb[lp] = D(pnb.get(lp, zero) + plp)
                    if lp not in in_beam:
                        pb[lp] = D(pb.get(lp, zero) + D(p_blank * D(pb_prev.get(lp, zero) + pnb_prev.get(lp, zero))))
                        pnb[lp] = D(pnb.get(lp, zero) + D(p * pnb_prev.get(lp, zero)))
        a_next: "OrderedDict[tuple, np.floating]" = OrderedDict()      # Pb[t] + Pnb[t]  (Counter.__add__)
        for k, v in pb.items():
            s = D(v + pnb.get(k, zero))
            if s > 0:
                a_next[k] = s
        for k, v in pnb.items():
            if k not in pb and v > 0:
                a_next[k] = v
        if separator_index is None:
            keyed = [(a_next[k], k) for k in a_next]
        else:
            keyed = [(D(a_next[k] * D(F32((1 + _n_words(k, separator_index)) ** word_weight))), k) for k in a_next]
        order = sorted(range(len(keyed)), key=lambda j: -float(keyed[j][0]))      # stable, descending
        if hook is not None:
            pnb_only = sum(1 for k in a_next if k not in pb)
            order = hook(t, [s for s, _ in keyed], [k for _, k in keyed], pnb_only, order) or order
        a_prev = [keyed[j][1] for j in order][:beam_width]
        if range_safe and a_prev:
            s0 = D(pb.get(a_prev[0], zero) + pnb.get(a_prev[0], zero))
            if s0 < limit:
                e = max(int(np.frexp(s0)[1]) - 1, MIN_EXP[D])
                mul = np.ldexp(D(1.0), -e)
                assert mul.dtype == np.dtype(D)
                for k in pb:
                    pb[k] = D(pb[k] * mul)
                for k in pnb:
                    pnb[k] = D(pnb[k] * mul)
                scale += e
                rescaled_at.append(t)
        pb_prev, pnb_prev = pb, pnb
    scores = np.asarray([D(pb_prev.get(k, zero) + pnb_prev.get(k, zero)) for k in a_prev], dtype=D)
    return Search(a_prev, scores, scale, rescaled_at)


def decode(x, lengths, blank_index, beam_width, **kw) -> List[Search]:
    """Every utterance of ``x [T, N, V]``."""
    x = np.asarray(x, dtype=F32)
    return [search(x[:, n], int(np.asarray(lengths)[n]), blank_index, beam_width, **kw) for n in range(x.shape[1])]


def transcripts(results: List[Search]) -> List[List[int]]:
    return [list(r.beam[0]) if r.beam else [] for r in results]


def log_probs(r: Search) -> List[float]:
    """ln P of every beam entry, in double (``BeamHypothesis.log_prob``)."""
    return [math.log(float(s)) + r.scale_log2 * math.log(2.0) for s in r.scores]
