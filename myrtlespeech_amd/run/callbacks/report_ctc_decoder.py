"""``ReportCTCDecoder``: the reference's word-error-rate callback (run/run.py:50-109), on the host as it is there or with the
edit distances and their sums on the device."""
from typing import List, Optional

import torch

from myrtlespeech_amd.post_process.ctc_greedy_decoder import CTCGreedyDecoder
from myrtlespeech_amd.post_process.utils import levenshtein
from myrtlespeech_amd.run.callbacks.callback import Callback
from myrtlespeech_amd.wer import DeviceWordErrorRate


def _to_pinned(t: torch.Tensor) -> torch.Tensor:
    """A device tensor on its way to pinned host memory; a host tensor's own copy (the loader may reuse its buffer)."""
    if not t.is_cuda:
        return t.detach().clone()
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t.detach(), non_blocking=True)
    return host


class ReportCTCDecoder(Callback):
    """``reports[type(ctc_decoder).__name__] = {"wer": ..., "transcripts": [(act, exp), ...]}`` for every pass that is not a
    training pass: reset to ``{"wer": -1.0, "transcripts": []}`` in ``on_train_begin`` and ``on_epoch_begin``, ``wer`` written in
    ``on_epoch_end`` as ``float(sum(distances)) / sum(lengths) * 100`` over the words of the pass (``ZeroDivisionError`` when
    the references hold no word, as in the reference).

    ``on_device=False``: the reference's host arithmetic, literally -- decode, read back, symbols, words, ``levenshtein``, once
    per batch.  ``on_device=True``: ``wer.DeviceWordErrorRate`` (its ``ValueError`` for an alphabet or segmentor whose words the
    device cannot reproduce); a ``CTCGreedyDecoder`` is driven through ``launch_device`` so that nothing leaves the device, any
    other decoder is called as usual and its lists are uploaded.  ``on_device=None`` takes the device path when
    ``DeviceWordErrorRate`` accepts the arguments and the host path otherwise.

    On the device path a batch costs launches only.  With ``keep_transcripts=True`` the labels are also copied to pinned memory
    without waiting and become the ``(act, exp)`` word lists in ``on_epoch_end``, before ``wer`` is set; with ``False`` the list
    stays empty and a pass's only read-back is the six sums.  ``last_target`` may be on the host or on the device."""

    def __init__(self, ctc_decoder, alphabet, word_segmentor, on_device: Optional[bool] = None, keep_transcripts: bool = True):
        super().__init__()
        self.ctc_decoder = ctc_decoder
        self.alphabet = alphabet
        self.word_segmentor = word_segmentor
        self.keep_transcripts = keep_transcripts
        self.device_wer = None
        if on_device is None:
            try:
                self.device_wer = DeviceWordErrorRate(alphabet, word_segmentor)
            except ValueError:
                pass
        elif on_device:
            self.device_wer = DeviceWordErrorRate(alphabet, word_segmentor)
        self.on_device = self.device_wer is not None

    @property
    def _name(self) -> str:
        return self.ctc_decoder.__class__.__name__

    def _reset(self, **kwargs):
        kwargs["reports"][self._name] = {"wer": -1.0, "transcripts": []}
        self.distances: List[int] = []
        self.lengths: List[int] = []
        self._pending = []               # device path: (hypotheses, targets, target lengths, copies-done event) per batch
        if self.device_wer is not None:
            self.device_wer.reset()

    def on_train_begin(self, **kwargs):
        self._reset(**kwargs)

    def on_epoch_begin(self, **kwargs):
        self._reset(**kwargs)

    def _process(self, sentence: List[int]) -> List[str]:
        symbols = self.alphabet.get_symbols(sentence)
        return self.word_segmentor(symbols)

    def on_batch_end(self, **kwargs):
        if self.training:
            return
        targets = kwargs["last_target"][0]
        target_lens = kwargs["last_target"][1]
        if self.on_device:
            self._device_batch(kwargs["last_output"], targets, target_lens)
            return
        transcripts = kwargs["reports"][self._name]["transcripts"]
        acts = self.ctc_decoder(*kwargs["last_output"])
        for act, target, target_len in zip(acts, targets, target_lens):
            act = self._process(act)
            exp = self._process([int(e) for e in target[:int(target_len)]])

            transcripts.append((act, exp))

            distance = levenshtein(act, exp)
            self.distances.append(distance)
            self.lengths.append(len(exp))

    def _device_batch(self, last_output, targets, target_lens) -> None:
        if isinstance(self.ctc_decoder, CTCGreedyDecoder):
            hyp = self.ctc_decoder.launch_device(*last_output)
        else:
            hyp = self.ctc_decoder(*last_output)
        self.device_wer.update(hyp, targets, target_lens)
        if not self.keep_transcripts:
            return
        if isinstance(hyp, tuple):
            hyp = (_to_pinned(hyp[0]), _to_pinned(hyp[1]))
        done = torch.cuda.Event()
        self._pending.append((hyp, _to_pinned(targets), _to_pinned(target_lens), done))
        done.record()

    def _collect(self, transcripts) -> None:
        for hyp, targets, target_lens, done in self._pending:
            done.synchronize()
            if isinstance(hyp, tuple):
                labels, lens = hyp[0].numpy(), hyp[1].tolist()
                hyp = [labels[n, :lens[n]].tolist() for n in range(len(lens))]
            rows = targets.numpy()
            for act, n, target_len in zip(hyp, range(len(rows)), target_lens.tolist()):
                transcripts.append((self._process(act), self._process(rows[n, :target_len].tolist())))
        self._pending = []

    def on_epoch_end(self, **kwargs):
        if self.training:
            return
        if self.on_device:
            self._collect(kwargs["reports"][self._name]["transcripts"])
            wer = self.device_wer.value()
        else:
            wer = float(sum(self.distances)) / sum(self.lengths) * 100
        kwargs["reports"][self._name]["wer"] = wer
