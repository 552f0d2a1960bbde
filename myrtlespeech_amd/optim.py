"""Optimizers whose step runs on the device in two passes (csrc/optim.hip; arithmetic in include/ms_hotpath.h, "training:
gradient norm, clip and the fused optimizer steps"): one pass reads every gradient once for the global norm, one pass per
parameter group reads ``p, g`` and the state once and writes ``p`` and the state once, with the clip coefficient applied in
registers.

``SGD`` and ``Adam`` subclass ``torch.optim.Optimizer``: parameter groups and their ``lr`` work, so every
``torch.optim.lr_scheduler`` drives them, and the state keys are torch's (``momentum_buffer``; ``step`` -- a CPU float32 scalar
tensor --, ``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq``), so ``state_dict()`` loads into the torch optimizer of the same
name and back.  Not served: dampening, ``maximize``, decoupled weight decay, ``foreach`` / ``fused`` / ``capturable`` /
``differentiable`` switches, sparse gradients, any dtype but float32, capture of ``step()`` into a HIP graph.

Clipping inside the optimizer (``max_grad_norm``): the norm is taken over ALL groups' gradients first
(``optimizer.last_grad_norm``, the device tensor ``[norm, non-finite flag]``) and the steps scale the gradient in registers.
``.grad`` KEEPS ITS UNCLIPPED VALUES -- unlike ``clip_grad_norm_`` below and the ``ClipGradNorm`` callback
(run/callbacks/clip_grad_norm.py), which rewrite the gradients in place as ``torch.nn.utils.clip_grad_norm_`` does.

``skip_nonfinite=True`` (needs ``max_grad_norm``): a step whose gradient norm is NaN or infinite writes nothing.  The 4-byte
flag is read back after the launches were enqueued -- the one synchronisation, and only in this mode -- so that a skipped step
does not advance ``state["step"]`` (Adam's bias correction must not see a step that did not happen); skips are counted in
``optimizer.skipped_steps``.

The version protocol: the kernels write through raw pointers, so autograd's version counters do not move on their own, and
every packed-weight cache of this project (model/fully_connected.py, model/rnn.py, model/cnn.py, the graph signatures of
streaming.py) is keyed on ``(data_ptr, _version)``.  After its launches ``step()`` bumps the version of every parameter and
state tensor that was in a list exactly once (``_bump``); the next forward then repacks.
"""
import ctypes
import math
from typing import Iterable, List, Optional

import torch

from myrtlespeech_amd import _lib


def _bump(tensors: List[torch.Tensor]) -> None:
    """``_version += 1`` of each tensor, once.  (A list: given a bare tensor the function iterates it and bumps once per row.)"""
    if tensors:
        torch._C._increment_version(list(tensors))


class _Lists:
    """Host arrays of one tensor list set: ``ptrs[k]`` a ``void*[n]`` per role (None: that role is absent), ``numels`` an
    ``int64[n]``; rebuilt by the owner when any ``data_ptr`` changed (``key``)."""

    def __init__(self, roles: List[Optional[List[torch.Tensor]]]):
        first = next(r for r in roles if r is not None)
        self.n = len(first)
        self.key = tuple(tuple(t.data_ptr() for t in r) if r is not None else None for r in roles)
        self.numels = (ctypes.c_int64 * max(self.n, 1))(*[t.numel() for t in first])
        self.ptrs = []
        for r in roles:
            if r is None:
                self.ptrs.append(None)
                continue
            for t, f in zip(r, first):
                if t.numel() != f.numel():
                    raise ValueError("a gradient or state tensor does not have its parameter's element count")
            self.ptrs.append((ctypes.c_void_p * max(self.n, 1))(*[_lib.ptr(t).value or 0 for t in r]))

    @staticmethod
    def key_of(roles):
        return tuple(tuple(t.data_ptr() for t in r) if r is not None else None for r in roles)


def _check_tensor(t: torch.Tensor, what: str) -> None:
    """The refusals that need no device: raised before anything is launched."""
    if t.is_sparse or t.layout != torch.strided:
        raise ValueError(f"{what}: sparse tensors are not served")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {t.dtype} is not served, only float32")
    if not t.is_contiguous():
        raise ValueError(f"{what}: shape {tuple(t.shape)} with strides {tuple(t.stride())} is not contiguous")


def _with_grad(params: Iterable[torch.Tensor]) -> List[torch.Tensor]:
    """Parameters that have a gradient, checked (parameter and gradient): the others are left out of the lists, as in torch."""
    out = []
    for p in params:
        if p.grad is None:
            continue
        _check_tensor(p.grad, "gradient")      # (first: a sparse gradient is refused as sparse whatever else it is)
        _check_tensor(p, "parameter")
        out.append(p)
    return out


class _NormWorkspace:
    """The norm's launches for one owner: cached host lists, a grow-only workspace and the ``[2]`` output."""

    def __init__(self):
        self.lists = None
        self.ws = _lib.Workspace()

    def norm(self, grads: List[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
        _lib.require_gpu()
        lib = _lib.load()
        if self.lists is None or self.lists.key != _Lists.key_of([grads]):
            self.lists = _Lists([grads])
        li = self.lists
        if out is None:
            out = torch.empty(2, dtype=torch.float32, device="cuda")
        nbytes = lib.ms_grad_norm_workspace_bytes(li.numels, li.n)
        ws = self.ws.get(nbytes, zero=False)
        _lib.check(lib.ms_grad_norm(li.ptrs[0], li.numels, li.n, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "ms_grad_norm")
        return out

    def clip(self, norm: torch.Tensor, max_norm: float) -> None:
        li = self.lists
        _lib.check(_lib.load().ms_grad_clip(li.ptrs[0], li.numels, li.n, _lib.ptr(norm), float(max_norm), _lib.stream_ptr()),
                   "ms_grad_clip")


def _params_of(parameters) -> List[torch.Tensor]:
    if isinstance(parameters, torch.Tensor):
        return [parameters]
    return list(parameters)


def grad_norm(parameters) -> torch.Tensor:
    """Device tensor ``[2]``: the 2-norm of all gradients taken as one vector, and 1.0 where that is NaN or infinite (else 0.0).
    Parameters without a gradient are left out.  Nothing is read back."""
    params = _with_grad(_params_of(parameters))
    return _NormWorkspace().norm([p.grad for p in params])


def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` in two launch sets (``ms_grad_norm`` + ``ms_grad_clip``): scales every gradient in
    place by ``max_norm / (norm + 1e-6)`` where that is below 1 (or NaN) and returns the device ``[norm, non-finite flag]``.
    Only the 2-norm is served."""
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_ serves norm_type 2 only, not {norm_type}")
    params = _with_grad(_params_of(parameters))
    work = _NormWorkspace()
    grads = [p.grad for p in params]
    norm = work.norm(grads)
    work.clip(norm, max_norm)
    _bump(grads)
    return norm


class _DeviceOptimizer(torch.optim.Optimizer):
    """What ``SGD`` and ``Adam`` share: the checks, the global norm, the skip read-back and the version bumps."""

    def __init__(self, params, defaults, max_grad_norm, skip_nonfinite):
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        if skip_nonfinite and max_grad_norm is None:
            raise ValueError("skip_nonfinite needs max_grad_norm: the flag is a by-product of the gradient norm")
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self.skipped_steps = 0
        self.last_grad_norm = None
        self._norm_work = _NormWorkspace()
        self._lists = {}

    def _cached_lists(self, slot, roles) -> _Lists:
        li = self._lists.get(slot)
        if li is None or li.key != _Lists.key_of(roles):
            li = self._lists[slot] = _Lists(roles)
        return li

    def _enqueue(self, gi, group, params, norm):
        """Launches of one group; returns the state tensors written."""
        raise NotImplementedError

    def _advance(self, group, params):
        """Host-side bookkeeping of a step that happened."""

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        per_group = [_with_grad(g["params"]) for g in self.param_groups]      # every refusal before the first launch
        if not any(per_group):
            return loss
        _lib.require_gpu()
        norm = None
        if self.max_grad_norm is not None:
            if self.last_grad_norm is None:
                self.last_grad_norm = torch.empty(2, dtype=torch.float32, device="cuda")
            norm = self._norm_work.norm([p.grad for ps in per_group for p in ps], self.last_grad_norm)
        written = []
        for gi, (group, params) in enumerate(zip(self.param_groups, per_group)):
            if params:
                written += self._enqueue(gi, group, params, norm)
                written += params
        if self.skip_nonfinite and bool(self.last_grad_norm[1].item()):      # the one read-back, in this mode only
            self.skipped_steps += 1
            return loss
        for group, params in zip(self.param_groups, per_group):
            self._advance(group, params)
        _bump(written)
        return loss


class SGD(_DeviceOptimizer):
    """``torch.optim.SGD`` without dampening, one launch set per group (``ms_sgd_step``)."""

    def __init__(self, params, lr, momentum=0, weight_decay=0, nesterov=False, max_grad_norm=None, skip_nonfinite=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum")
        # (dampening 0: a constant kept in the group so that the state_dict loads into torch.optim.SGD and back)
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults, max_grad_norm, skip_nonfinite)

    def _enqueue(self, gi, group, params, norm):
        if group.get("dampening", 0) != 0:
            raise ValueError("SGD: dampening is not served")
        momentum = float(group["momentum"])
        bufs = None
        if momentum != 0:
            bufs = []
            for p in params:
                st = self.state[p]
                if st.get("momentum_buffer") is None:
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                _check_tensor(st["momentum_buffer"], "momentum_buffer")
                bufs.append(st["momentum_buffer"])
        li = self._cached_lists(gi, [params, [p.grad for p in params], bufs])
        _lib.check(_lib.load().ms_sgd_step(li.ptrs[0], li.ptrs[1], li.ptrs[2], li.numels, li.n, float(group["lr"]), momentum,
                                           float(group["weight_decay"]), int(bool(group["nesterov"])), _lib.ptr(norm),
                                           float(self.max_grad_norm or 0.0), int(self.skip_nonfinite), _lib.stream_ptr()),
                   "ms_sgd_step")
        return bufs or []


class Adam(_DeviceOptimizer):
    """``torch.optim.Adam`` (with ``amsgrad``), one launch set per group and step count (``ms_adam_step``)."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, max_grad_norm=None,
                 skip_nonfinite=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        super().__init__(params, defaults, max_grad_norm, skip_nonfinite)

    def _enqueue(self, gi, group, params, norm):
        amsgrad = bool(group["amsgrad"])
        # (the float32 values of the betas, which are what the kernel multiplies by: the bias corrections below must be those of
        # the recurrences that actually run)
        beta1, beta2 = (ctypes.c_float(b).value for b in group["betas"])
        by_step = {}
        for p in params:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if amsgrad and st.get("max_exp_avg_sq") is None:
                st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            for k in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ()):
                _check_tensor(st[k], k)
            by_step.setdefault(int(st["step"]), []).append(p)
        written = []
        lib = _lib.load()
        # (parameters of one group share a step count unless some sat steps out without a gradient: one launch set per count)
        for t0, ps in sorted(by_step.items()):
            t = t0 + 1
            m = [self.state[p]["exp_avg"] for p in ps]
            v = [self.state[p]["exp_avg_sq"] for p in ps]
            vmax = [self.state[p]["max_exp_avg_sq"] for p in ps] if amsgrad else None
            li = self._cached_lists((gi, len(by_step) > 1 and t0), [ps, [p.grad for p in ps], m, v, vmax])
            step_size = float(group["lr"]) / (1.0 - beta1 ** t)
            rsqrt_bc2 = math.sqrt(1.0 - beta2 ** t)
            _lib.check(lib.ms_adam_step(li.ptrs[0], li.ptrs[1], li.ptrs[2], li.ptrs[3], li.ptrs[4], li.numels, li.n, beta1, beta2,
                                        float(group["eps"]), float(group["weight_decay"]), step_size, rsqrt_bc2, _lib.ptr(norm),
                                        float(self.max_grad_norm or 0.0), int(self.skip_nonfinite), _lib.stream_ptr()),
                       "ms_adam_step")
            written += m + v + (vmax or [])
        return written

    def _advance(self, group, params):
        for p in params:
            self.state[p]["step"] += 1
