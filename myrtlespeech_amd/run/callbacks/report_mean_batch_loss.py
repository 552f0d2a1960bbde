from typing import Optional

from myrtlespeech_amd.run.callbacks.callback import Callback


class ReportMeanBatchLoss(Callback):
    """``reports["ReportMeanBatchLoss"]``: the mean of ``last_loss.item()`` over the batches of the pass that just ended (None
    from the start of a pass until its end; 0.0 for a pass without batches).  Reading the loss synchronises once per batch."""

    def _reset(self, reports) -> None:
        reports[type(self).__name__] = None
        self.loss: Optional[float] = None

    def on_train_begin(self, **kwargs) -> None:
        self._reset(kwargs["reports"])

    def on_epoch_begin(self, **kwargs) -> None:
        self._reset(kwargs["reports"])

    def on_backward_begin(self, **kwargs) -> None:
        self.loss = (self.loss or 0.0) + kwargs["last_loss"].item()

    def on_epoch_end(self, **kwargs) -> None:
        kwargs["reports"][type(self).__name__] = (self.loss or 0.0) / float(max(1, kwargs["epoch_batches"]))
