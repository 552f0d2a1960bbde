"""What tests/test_ds2_train_gpu.py takes from tests/ds2_train_ref.py, checked on the CPU: every clamp of both tiny models shows
its three regimes in live frames, every parameter has a gradient that is not all zero, and the float64 yardstick's loss falls
at every one of the SGD steps at ``LR``."""
import numpy as np
import pytest
import torch

import ds2_train_ref as M


@pytest.mark.parametrize("model", M.MODELS)
def test_every_clamp_shows_three_regimes_in_live_frames(model):
    w, d = M.make(model)
    acts = M.activations(model, w, d)
    assert len(acts) == 3
    for i, a in enumerate(acts):
        assert (a == 0.0).any() and (a == M.CLIP).any() and ((a > 0.0) & (a < M.CLIP)).any(), (model, i)


@pytest.mark.parametrize("model", M.MODELS)
def test_every_parameter_has_a_gradient_and_float32_is_close(model):
    w, d = M.make(model)
    loss, grads = M.yardstick(model, w, d)
    loss32, grads32 = M.torch_full(model, w, d, torch.float32)
    assert sorted(grads) == sorted(w) and np.isfinite(loss)
    assert abs(loss32 - loss) <= 1e-5 * abs(loss)
    for key, g in grads.items():
        assert np.isfinite(g).all() and np.abs(g).max() > 0, key
        assert np.abs(grads32[key] - g).max() <= 1e-4 * np.abs(g).max(), key
    assert M.logits(model, w, d).shape == (max(M.OUT_LENS), M.N, M.V)


@pytest.mark.parametrize("model", M.MODELS)
def test_yardstick_loss_falls_at_every_sgd_step(model):
    w, d = M.make(model)
    losses = M.sgd_losses(model, w, d)
    assert len(losses) == M.STEPS + 1
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
