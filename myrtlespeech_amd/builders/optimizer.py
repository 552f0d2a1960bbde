"""``train_config`` -> ``(optim, lr_scheduler)``: this project's device ``SGD`` / ``Adam`` (myrtlespeech_amd/optim.py) and
torch's schedulers, under the reference's field-presence rules (builders/task_config.py:53-100, 159-215): an optional
``FloatValue`` is passed on only when it is set, the booleans always, ``constant_lr`` gives no scheduler, and an unset oneof
is a ``ValueError``.  Datasets and loaders are not built here."""
from typing import Iterable, Optional, Tuple

import torch

from myrtlespeech_amd import optim as device_optim


def build(train_config, parameters: Iterable[torch.Tensor], max_grad_norm: Optional[float] = None
          ) -> Tuple[torch.optim.Optimizer, Optional[torch.optim.lr_scheduler.LRScheduler]]:
    """``max_grad_norm``: clip inside the optimizer's step (the config has no field for it; the reference clips from a
    callback)."""
    which = train_config.WhichOneof("supported_optimizers")
    kwargs = {}
    if which == "sgd":
        sgd = train_config.sgd
        if sgd.HasField("momentum"):
            kwargs["momentum"] = sgd.momentum.value
        if sgd.HasField("l2_weight_decay"):
            kwargs["weight_decay"] = sgd.l2_weight_decay.value
        kwargs["nesterov"] = sgd.nesterov_momentum
        optim = device_optim.SGD(parameters, lr=sgd.learning_rate, max_grad_norm=max_grad_norm, **kwargs)
    elif which == "adam":
        adam = train_config.adam
        betas = [0.9, 0.999]
        if adam.HasField("beta_1"):
            betas[0] = adam.beta_1.value
        if adam.HasField("beta_2"):
            betas[1] = adam.beta_2.value
        if adam.HasField("eps"):
            kwargs["eps"] = adam.eps.value
        if adam.HasField("l2_weight_decay"):
            kwargs["weight_decay"] = adam.l2_weight_decay.value
        kwargs["amsgrad"] = adam.amsgrad
        optim = device_optim.Adam(parameters, lr=adam.learning_rate, betas=tuple(betas), max_grad_norm=max_grad_norm, **kwargs)
    else:
        raise ValueError(f"unsupported optimizer {which}")
    return optim, _lr_scheduler(train_config, optim)


def _lr_scheduler(train_config, optim):
    which = train_config.WhichOneof("supported_lr_scheduler")
    sched = torch.optim.lr_scheduler
    if which == "constant_lr":
        return None
    if which == "step_lr":
        kwargs = {"step_size": train_config.step_lr.step_size}
        if train_config.step_lr.HasField("gamma"):
            kwargs["gamma"] = train_config.step_lr.gamma.value
        return sched.StepLR(optim, **kwargs)
    if which == "exponential_lr":
        return sched.ExponentialLR(optim, gamma=train_config.exponential_lr.gamma)
    if which == "cosine_annealing_lr":
        kwargs = {"T_max": train_config.cosine_annealing_lr.t_max}
        if train_config.cosine_annealing_lr.HasField("eta_min"):
            kwargs["eta_min"] = train_config.cosine_annealing_lr.eta_min.value
        return sched.CosineAnnealingLR(optim, **kwargs)
    raise ValueError(f"unsupported learning rate scheduler {which}")
