"""The convolution front end's long-input kernels against the kernels they replace (``ms_conv_set_variant``: 0 = shipped
dispatch, 1 = the tiled kernel and layout passes) and against the CPU oracle.  Shapes are the smallest at which the new code
can still go wrong -- tile tails, SAME offsets, masks, row-block edges --, not the workload's own.  Needs an MI355X: -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conv_frontend_cases import ds2_cnn, handover_equals_two_calls, ragged_lens, run_cnn
from oracle import ds_oracle as O

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def cpu(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("same", [True, False])
@pytest.mark.parametrize("k,s", [([41, 11], [2, 2]), ([16, 3], [4, 3])])
def test_conv1_shared_window_equals_tiled_kernel_and_oracle(lib, monkeypatch, k, s, same):
    """Single-channel convolution, long input (``maskconv_fwin_shared_kernel``): output frames 128 (exact tiles), 129 (a tile of
    one frame) and 151 at T = 255 .. 301 for the DS2 filter; 80 / 81 features: 40 rows = four full row blocks, 41 = a block of
    one row; ragged lengths down to one shorter than the filter.  Bit-identical to the tiled kernel (same MFMAs in the same
    order per output element), and within the split-precision tolerance of the oracle."""
    from myrtlespeech_amd.model.cnn import MaskConv2d, PaddingMode
    monkeypatch.setenv("MS_CONV_MFMA_MIN_FLOPS", "0")
    torch.manual_seed(1)
    m = MaskConv2d(1, 32, k, s, PaddingMode.SAME if same else PaddingMode.NONE).eval()
    rng = np.random.default_rng(k[0] + same)
    for F in (80, 81):
        for tn in (255, 256, 257, 301):
            for N in (1, 3):
                x = rng.normal(size=(N, 1, F, tn)).astype(np.float32)
                lens = ragged_lens(tn, N, k[1])
                out = []
                try:
                    for variant in (0, 1):
                        lib.ms_conv_set_variant(variant)
                        out.append(m((T(x).cuda(), T(lens)), fused_activation=(0.0, 20.0)))
                finally:
                    lib.ms_conv_set_variant(0)
                (y0, nl0), (y1, nl1) = out
                case = str((k, s, same, F, tn, N))
                assert y0.shape[-1] > 48, case                       # a long input: the shared-window kernel's shapes
                assert torch.equal(y0, y1), (case, float((y0 - y1).abs().max()))
                want, wl = O.mask_conv2d(x, lens, cpu(m.weight), cpu(m.bias), tuple(s), same)
                np.testing.assert_allclose(cpu(y0), np.clip(want, 0.0, 20.0), rtol=1e-4, atol=3e-4, err_msg=case)
                np.testing.assert_array_equal(cpu(nl0), wl)
                np.testing.assert_array_equal(cpu(nl1), wl)


def test_handover_equals_two_calls():
    handover_equals_two_calls()


@pytest.mark.parametrize("mode", ["bf16x3", "fp16"])
def test_handover_equals_two_calls_in_other_precision_modes(mode):
    """The precision mode is read once per process: the same case in a child process."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_frontend_cases.py")
    r = subprocess.run([sys.executable, script, "handover"], env=dict(os.environ, MS_PRECISION=mode), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def test_pattern_that_must_not_match_runs_unfused(monkeypatch):
    """An activation between the convolutions that is not a plain clamp: the CNN loop calls the modules one by one."""
    from myrtlespeech_amd.model import deep_speech_2
    monkeypatch.setenv("MS_CONV_MFMA_MIN_FLOPS", "0")
    calls = []
    real = deep_speech_2.conv_pair_forward
    monkeypatch.setattr(deep_speech_2, "conv_pair_forward", lambda *a: calls.append(1) or real(*a))
    cnn = ds2_cnn(between=torch.nn.Softsign())
    rng = np.random.default_rng(7)
    x = (rng.normal(size=(3, 1, 80, 130)) * 3).astype(np.float32)
    lens = ragged_lens(130, 3, 11)
    got, got_lens = run_cnn(cnn, x, lens)
    assert not calls
    with torch.no_grad():
        y1, l1 = cnn[0]((T(x).cuda(), T(lens)))
        want, want_lens = cnn[2]((torch.nn.functional.softsign(y1), l1), fused_activation=(0.0, 20.0))
    assert torch.equal(got, want) and torch.equal(got_lens.cpu(), want_lens.cpu())
    # (and the pattern that does match goes through the pair)
    run_cnn(ds2_cnn(), x, lens)
    assert calls


def two_calls(cnn, x, lens):
    """The two convolutions of ``ds2_cnn`` called one after the other, clamps fused: ``(conv1's output, output, lengths)``."""
    with torch.no_grad():
        y1, l1 = cnn[0]((T(x).cuda(), T(lens)), fused_activation=(0.0, 20.0))
        y1_seen = y1.clone()                      # (conv2 masks its input in place)
        y2, l2 = cnn[2]((y1, l1), fused_activation=(0.0, 20.0))
    return y1_seen, y2, l2


def test_consumer_without_a_channels_last_tile_runs_unfused(lib, monkeypatch):
    """96 channels between the convolutions: conv1 (three channel tiles) is the shared-window kernel's, but the channels-last
    kernel has no tile for conv2 (96 channels x 11 taps staged: 179 712 B of LDS), whose call then falls through to the
    exact-float32 kernel -- which needs the float32 tensor.  The pair must see that before conv1 runs and leave the two calls."""
    from myrtlespeech_amd.model.cnn import conv_pair_forward
    monkeypatch.setenv("MS_CONV_MFMA_MIN_FLOPS", "0")
    cnn = ds2_cnn(channels=96)
    rng = np.random.default_rng(11)
    x = (rng.normal(size=(2, 1, 80, 130)) * 3).astype(np.float32)
    lens = ragged_lens(130, 2, 11)
    assert lib.ms_maskconv_fwin_planes_supported(2, 130, 96, 40, 65, 41, 11, 2, 2, 1) == 1
    assert lib.ms_maskconv_cl_supported(2, 96, 40, 32, 20, 65, 11, 1, 1) == 0
    assert lib.ms_maskconv_cl_supported(2, 32, 40, 32, 20, 65, 11, 1, 1) == 1
    with torch.no_grad():
        assert conv_pair_forward(cnn[0], (0.0, 20.0), cnn[2], (0.0, 20.0), (T(x).cuda(), T(lens))) is None
    got, got_lens = run_cnn(cnn, x, lens)
    _, want, want_lens = two_calls(cnn, x, lens)
    assert torch.equal(got, want) and torch.equal(got_lens.cpu(), want_lens.cpu())
    # conv1 at 96 output channels against the tiled kernel and the oracle (a channel tile index > 0 in the new kernel)
    out = []
    try:
        for variant in (0, 1):
            lib.ms_conv_set_variant(variant)
            out.append(cnn[0]((T(x).cuda(), T(lens)), fused_activation=(0.0, 20.0))[0])
    finally:
        lib.ms_conv_set_variant(0)
    assert torch.equal(out[0], out[1])
    ref, _ = O.mask_conv2d(x, lens, cpu(cnn[0].weight), cpu(cnn[0].bias), (2, 2), True)
    np.testing.assert_allclose(cpu(out[0]), np.clip(ref, 0.0, 20.0), rtol=1e-4, atol=3e-4)


def test_short_input_asks_no_kernel_and_launches_nothing(lib, monkeypatch):
    """At most 48 output frames (the tiled kernel's short-input tile): the pair is refused by the query, before any look-up."""
    from myrtlespeech_amd.model import cnn as cnn_module
    monkeypatch.setenv("MS_CONV_MFMA_MIN_FLOPS", "0")
    assert lib.ms_maskconv_fwin_planes_supported(3, 96, 32, 40, 48, 41, 11, 2, 2, 1) == 0
    assert lib.ms_maskconv_fwin_planes_supported(3, 98, 32, 40, 49, 41, 11, 2, 2, 1) == 1
    cnn = ds2_cnn()
    monkeypatch.setattr(cnn_module, "_mask_in_place", lambda *a: pytest.fail("the refused pair must not touch its input"))
    x = torch.randn(3, 1, 80, 96).cuda()
    with torch.no_grad():
        assert cnn_module.conv_pair_forward(cnn[0], (0.0, 20.0), cnn[2], (0.0, 20.0), (x, torch.tensor([96, 59, 7]))) is None


@pytest.mark.parametrize("on", [0, 2])
def test_forward_hooks_on_either_convolution_still_fire(monkeypatch, on):
    """A forward hook sees its module's call and output -- conv1's is the tensor the hand-over never makes: with a hook on either
    convolution the CNN loop makes the two calls, as it did before there was a pair."""
    monkeypatch.setenv("MS_CONV_MFMA_MIN_FLOPS", "0")
    cnn = ds2_cnn()
    rng = np.random.default_rng(13)
    x = (rng.normal(size=(3, 1, 80, 130)) * 3).astype(np.float32)
    lens = ragged_lens(130, 3, 11)
    y1, want, want_lens = two_calls(cnn, x, lens)
    seen = []
    handle = cnn[on].register_forward_hook(lambda mod, args, out: seen.append(out[0].clone()))
    try:
        got, got_lens = run_cnn(cnn, x, lens)
    finally:
        handle.remove()
    assert len(seen) == 1 and torch.equal(seen[0], y1 if on == 0 else want)
    assert torch.equal(got, want) and torch.equal(got_lens.cpu(), want_lens.cpu())
