"""The callback protocol of the reference (run/callbacks/callback.py), restated.

A ``Callback`` has one method per point of ``train.fit``'s loop; each is called with the handler's ``state_dict`` as keyword
arguments and may return a dict, whose keys must already be in the state and whose values replace the state's.  The state:

``epoch``                 training epochs finished            ``epochs``          the ``fit`` argument
``total_train_batches``   training batches finished           ``epoch_batches``   batches finished in this stage's pass
``reports``               dict that reporting callbacks fill  ``last_input`` / ``last_target`` / ``last_output``
``loss``                  ``{"last_output", "last_target"}``: what the loss is called with (``on_loss_begin`` may replace it)
``last_loss``             the loss value                      ``skip_bwd`` / ``skip_step`` / ``skip_zero`` / ``stop_epoch`` /
``stop_training``         switches a callback returns to suppress the backward, the step, ``zero_grad``, the rest of the
                          epoch, the rest of training; each is reset to False right before its hook runs.
"""
from typing import Any, Collection, Dict, Optional, Tuple

import torch


class Callback:
    """Every hook does nothing.  ``training`` mirrors the handler's mode."""

    def __init__(self, training: bool = True):
        self.training = training

    def on_train_begin(self, **kwargs) -> Optional[Dict]:
        return None

    def on_epoch_begin(self, **kwargs) -> Optional[Dict]:
        return None

    def on_batch_begin(self, **kwargs) -> Optional[Dict]:
        return None

    def on_loss_begin(self, **kwargs) -> Optional[Dict]:
        return None

    def on_backward_begin(self, **kwargs) -> Optional[Dict]:
        return None

    def on_backward_end(self, **kwargs) -> Optional[Dict]:
        return None

    def on_step_end(self, **kwargs) -> Optional[Dict]:
        return None

    def on_batch_end(self, **kwargs) -> Optional[Dict]:
        return None

    def on_epoch_end(self, **kwargs) -> Optional[Dict]:
        return None

    def on_train_end(self, **kwargs) -> Optional[Dict]:
        return None

    def train(self, mode: bool = True) -> "Callback":
        self.training = mode
        return self


class ModelCallback(Callback):
    """A callback that holds the model it acts on."""

    def __init__(self, model: torch.nn.Module, training: bool = True):
        super().__init__(training=training)
        self.model = model


class CallbackHandler:
    """Owns the state and runs every registered callback's hook of a given name, in registration order."""

    def __init__(self, callbacks: Optional[Collection[Callback]] = None, training: bool = True):
        self.callbacks = callbacks if callbacks is not None else []
        self.state_dict: Dict = {}
        self.training = training

    def __call__(self, hook: str) -> None:
        for callback in self.callbacks:
            new = getattr(callback, hook)(**self.state_dict)
            if new is None:
                continue
            for key, value in new.items():
                if key not in self.state_dict:
                    raise ValueError(f"{type(callback).__name__}.{hook} returned {key!r}, which is not a key of the "
                                     "CallbackHandler's state")
                self.state_dict[key] = value

    def _reset_and_run(self, hook: str, **values) -> None:
        self.state_dict.update(values)
        self(hook)

    def on_train_begin(self, epochs: int) -> None:
        self._reset_and_run("on_train_begin", epoch=0, epochs=epochs, total_train_batches=0, epoch_batches=0, reports={})

    def on_epoch_begin(self) -> None:
        self._reset_and_run("on_epoch_begin", epoch_batches=0)

    def on_batch_begin(self, x: Any, y: Any) -> Tuple[Any, Any]:
        self._reset_and_run("on_batch_begin", last_input=x, last_target=y)
        return self.state_dict["last_input"], self.state_dict["last_target"]

    def on_loss_begin(self, out: Any, y: Any) -> Tuple[Any, Any]:
        self._reset_and_run("on_loss_begin", last_output=out, last_target=y, loss={"last_output": out, "last_target": y})
        loss_args = self.state_dict["loss"]
        return loss_args["last_output"], loss_args["last_target"]

    def on_backward_begin(self, loss: torch.Tensor) -> Tuple[torch.Tensor, bool]:
        self._reset_and_run("on_backward_begin", skip_bwd=False, last_loss=loss)
        return self.state_dict["last_loss"], self.state_dict["skip_bwd"]

    def on_backward_end(self) -> bool:
        self._reset_and_run("on_backward_end", skip_step=False)
        return self.state_dict["skip_step"]

    def on_step_end(self) -> bool:
        self._reset_and_run("on_step_end", skip_zero=False)
        return self.state_dict["skip_zero"]

    def on_batch_end(self) -> bool:
        """``epoch_batches`` counts every finished batch of the pass, ``total_train_batches`` the training ones; both move
        AFTER the callbacks ran."""
        self._reset_and_run("on_batch_end", stop_epoch=False)
        self.state_dict["epoch_batches"] += 1
        if self.training:
            self.state_dict["total_train_batches"] += 1
        return self.state_dict["stop_epoch"]

    def on_epoch_end(self) -> bool:
        """``epoch`` moves after the callbacks ran, and only at the end of a training pass."""
        self._reset_and_run("on_epoch_end", stop_training=False)
        if self.training:
            self.state_dict["epoch"] += 1
        return self.state_dict["stop_training"]

    def on_train_end(self) -> None:
        self("on_train_end")

    def train(self, mode: bool = True) -> "CallbackHandler":
        self.training = mode
        for callback in self.callbacks:
            callback.train(mode=mode)
        return self
