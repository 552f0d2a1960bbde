from typing import Dict, Optional

from myrtlespeech_amd.run.callbacks.callback import Callback


class StopEpochAfter(Callback):
    """Ends a pass once ``epoch_batches`` batches of it are done (the handler counts a batch after its ``on_batch_end`` hooks,
    hence the ``+ 1``)."""

    def __init__(self, epoch_batches: int = 1):
        super().__init__()
        self.epoch_batches = epoch_batches

    def on_batch_end(self, **kwargs) -> Optional[Dict]:
        if kwargs["epoch_batches"] + 1 >= self.epoch_batches:
            return {"stop_epoch": True}
        return None
