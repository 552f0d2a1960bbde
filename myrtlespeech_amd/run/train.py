"""``fit``: the reference's loop (run/train.py:13-91), restated.  Stage order: an EVAL pass before the first epoch and after
every epoch when there is an eval loader, a TRAIN pass always.  Per stage: ``seq_to_seq.train(mode)`` and the handler's,
``on_epoch_begin``, then per batch ``on_batch_begin`` -> model -> ``on_loss_begin`` -> loss -> ``on_backward_begin`` ->
``backward`` (unless ``skip_bwd``) -> ``on_backward_end`` -> ``optim.step()`` (unless ``skip_step``) -> ``on_step_end`` ->
``optim.zero_grad()`` (unless ``skip_zero``) -> ``on_batch_end`` (the epoch stops on ``stop_epoch``); the scheduler steps once
per training epoch; ``on_epoch_end`` (training stops on ``stop_training``: the reference's ``break`` leaves only the
stage loop, against its own documentation -- here it ends ``fit``); ``on_train_end`` at the very end.  As in the
reference, the backward and the optimizer hooks belong to the TRAIN stage, and the hooks around the step are only run when the
model has an optimizer.

The one deliberate difference: the TRAIN stage calls ``seq_to_seq.model(x, differentiable=True)`` -- this project's default
forward is the detached inference path; the EVAL stage calls ``seq_to_seq.model(x)`` under ``torch.no_grad()``.

Limits: the differentiable forwards serve dropout in training mode only with a source of randomness attached, so ``fit`` on the
shipped DeepSpeech1 configuration (``drop_prob: 0.25``) needs one line in front of it --
``dropout.attach(seq_to_seq.model, dropout.DropoutGenerator(seed))`` (``myrtlespeech_amd.model.dropout``) -- and raises the
forward's ``ValueError`` at the first training batch without it; the masks are a pure function of ``(seed, offset)``, so two runs
from the same seed end in the same parameters, and the EVAL stages consume no offset.  The shipped DeepSpeech2 configuration has
no dropout and trains once ``model.rnn.gru_backward = True``.  ``fit`` itself knows nothing of either switch."""
from typing import Collection, Iterable, Optional

import torch

from myrtlespeech_amd.run.callbacks.callback import Callback, CallbackHandler
from myrtlespeech_amd.stage import Stage


def fit(seq_to_seq, epochs: int, train_loader: Iterable, eval_loader: Optional[Iterable] = None,
        callbacks: Optional[Collection[Callback]] = None) -> None:
    """Fits ``seq_to_seq`` for at most ``epochs`` passes over ``train_loader`` (fewer if a callback sets ``stop_training``).
    A loader is anything that yields ``(x, y)`` batches the model and the loss accept."""
    cb_handler = CallbackHandler(callbacks)
    cb_handler.on_train_begin(epochs)
    lr_scheduler = getattr(seq_to_seq, "lr_scheduler", None)

    for epoch in range(epochs):
        stages = [Stage.TRAIN]
        if eval_loader is not None:
            stages = ([Stage.EVAL] if epoch == 0 else []) + stages + [Stage.EVAL]

        stop_training = False
        for stage in stages:
            is_training = stage is Stage.TRAIN
            seq_to_seq.train(mode=is_training)
            cb_handler.train(mode=is_training)
            cb_handler.on_epoch_begin()

            with torch.enable_grad() if is_training else torch.no_grad():
                for x, y in (train_loader if is_training else eval_loader):
                    x, y = cb_handler.on_batch_begin(x, y)
                    out, _ = seq_to_seq.model(x, differentiable=True) if is_training else seq_to_seq.model(x)

                    loss_out, loss_y = cb_handler.on_loss_begin(out, y)
                    loss = seq_to_seq.loss(loss_out, loss_y)
                    loss, skip_bwd = cb_handler.on_backward_begin(loss)

                    if is_training:
                        if not skip_bwd:
                            loss.backward()
                        if seq_to_seq.optim is not None:
                            if not cb_handler.on_backward_end():
                                seq_to_seq.optim.step()
                            if not cb_handler.on_step_end():
                                seq_to_seq.optim.zero_grad()

                    if cb_handler.on_batch_end():
                        break

                if is_training and lr_scheduler is not None:
                    lr_scheduler.step()

            if cb_handler.on_epoch_end():
                stop_training = True
                break
        if stop_training:
            break

    cb_handler.on_train_end()
