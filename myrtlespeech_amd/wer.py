"""Decode -> transcripts -> word error rate: the arithmetic of the reference's
``ReportCTCDecoder`` callback (run/run.py:29-109) without the callback plumbing (``run.callbacks.ReportCTCDecoder`` has it),
on the host (``WordErrorRate``) and on the device (``DeviceWordErrorRate``)."""
from typing import Iterable, List, Sequence, Tuple

import torch

from myrtlespeech_amd import _lib
from myrtlespeech_amd.post_process.edit_distance import EditCounts, edit_distance
from myrtlespeech_amd.post_process.utils import levenshtein


class WordSegmentor:
    """Groups a sequence of symbols into words at ``separator`` (run/run.py:29-48);
    empty words are dropped."""

    def __init__(self, separator: str):
        self.separator = separator

    def __call__(self, sentence: List[str]) -> List[str]:
        words, word = [], []
        for symbol in sentence:
            if symbol == self.separator:
                if word:
                    words.append("".join(word))
                    word = []
            else:
                word.append(symbol)
        if word:
            words.append("".join(word))
        return words


class WordErrorRate:
    """Accumulates (hypothesis, reference) index sequences over batches and reports
    ``100 * sum(edit distances) / sum(reference lengths)`` in words (run/run.py:84-109)."""

    def __init__(self, alphabet, word_segmentor: WordSegmentor):
        self.alphabet = alphabet
        self.word_segmentor = word_segmentor
        self.transcripts: List[Tuple[List[str], List[str]]] = []
        self.distances: List[int] = []
        self.lengths: List[int] = []

    def _words(self, indices: Iterable[int]) -> List[str]:
        return self.word_segmentor(self.alphabet.get_symbols(list(indices)))

    def update(self, hypotheses: Sequence[Sequence[int]], targets, target_lens) -> None:
        for hyp, target, n in zip(hypotheses, targets, target_lens):
            act = self._words(hyp)
            exp = self._words(int(e) for e in target[:int(n)])
            self.transcripts.append((act, exp))
            self.distances.append(levenshtein(act, exp))
            self.lengths.append(len(exp))

    def value(self) -> float:
        return float(sum(self.distances)) / sum(self.lengths) * 100


class DeviceWordErrorRate:
    """``WordErrorRate`` with the sums kept on the device: ``update`` launches ``ms_edit_distance`` on the batch and returns
    without waiting, ``value()`` reads 48 bytes back once.  ``unit="word"`` counts the words ``WordSegmentor`` makes of
    ``alphabet.get_symbols``; ``unit="token"`` counts labels.

    The device compares words as label sequences, the host as joined strings.  The two agree iff joining is injective and
    cutting happens at a label, so the constructor raises ``ValueError`` for a symbol that is not a single character, a segmentor
    other than ``WordSegmentor`` and a separator that is not one character.  A one-character separator outside the alphabet
    never occurs in ``get_symbols``' output: no separator (-1).  No transcripts are kept here; ``ReportCTCDecoder`` keeps them."""

    def __init__(self, alphabet, word_segmentor, unit: str = "word"):
        if unit not in ("word", "token"):
            raise ValueError(f"unit={unit!r} must be 'word' or 'token'")
        self.alphabet, self.word_segmentor, self.unit = alphabet, word_segmentor, unit
        self.separator_index = None
        if unit == "word":
            multi = [s for s in alphabet.symbols if not isinstance(s, str) or len(s) != 1]
            if multi:
                raise ValueError(f"symbols {multi[:3]} are not single characters: equal words need not have equal labels")
            if type(word_segmentor) is not WordSegmentor:
                raise ValueError(f"{type(word_segmentor).__name__} is not wer.WordSegmentor: the device cuts words as it does")
            separator = word_segmentor.separator
            if not isinstance(separator, str) or len(separator) != 1:
                raise ValueError(f"separator {separator!r} is not one character")
            index = alphabet.get_index(separator)
            self.separator_index = -1 if index is None else index
        self._totals = None

    def reset(self) -> None:
        if self._totals is not None:
            self._totals.zero_()

    def update(self, hypotheses, targets, target_lens):
        """``hypotheses``: ``CTCGreedyDecoder.launch_device``'s ``(labels, label_lens)`` pair, or a list of label lists.
        Returns the batch's ``[N, 6]`` device tensor (``post_process.EditCounts`` rows)."""
        if isinstance(hypotheses, tuple) and len(hypotheses) == 2 and isinstance(hypotheses[0], torch.Tensor) \
                and hypotheses[0].dim() == 2:
            hyp, hyp_lens = hypotheses
        else:
            hyp, hyp_lens = list(hypotheses), None
        if self._totals is None:
            _lib.require_gpu()
            self._totals = torch.zeros(6, dtype=torch.int64, device="cuda")
        return edit_distance(hyp, hyp_lens, targets, target_lens, separator_index=self.separator_index,
                             n_symbols=len(self.alphabet) if self.unit == "word" else None, totals=self._totals)

    def counts(self):
        """The six sums so far (one read-back)."""
        return EditCounts(*(self._totals.cpu().tolist() if self._totals is not None else [0] * 6))

    def value(self) -> float:
        c = self.counts()
        return float(c.distance) / c.ref_units * 100
