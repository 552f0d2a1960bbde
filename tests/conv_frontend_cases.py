"""Cases of tests/test_gpu_conv_frontend.py that also have to run in another precision mode (``MS_PRECISION`` is read once
per process): ``python tests/conv_frontend_cases.py handover`` runs them in a process of its own and prints ``ok``."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def ragged_lens(tn: int, n: int, kt: int) -> np.ndarray:
    """One full sequence, one 37 frames shorter, one shorter than the filter's ``kt`` time taps."""
    return np.array([tn, tn - 37, max(1, kt - 4)][:n])


def ds2_cnn(between=None, channels=32):
    """DS2's two convolutions with their clamps; ``between`` replaces the activation between them, ``channels`` the 32
    channels between them."""
    from myrtlespeech_amd.model.cnn import MaskConv2d, PaddingMode
    from myrtlespeech_amd.model.seq_len_wrapper import SeqLenWrapper

    def act(m=None):
        return SeqLenWrapper(m if m is not None else torch.nn.Hardtanh(0.0, 20.0), torch.nn.Identity())

    torch.manual_seed(3)
    return torch.nn.Sequential(MaskConv2d(1, channels, [41, 11], [2, 2], PaddingMode.SAME), act(between),
                               MaskConv2d(channels, 32, [21, 11], [2, 1], PaddingMode.SAME), act()).eval()


def run_cnn(cnn, x, lens):
    """The CNN loop of ``DeepSpeech2`` on ``cnn`` (no recurrent or output layers are built)."""
    from myrtlespeech_amd.model.deep_speech_2 import DeepSpeech2
    model = DeepSpeech2(cnn, torch.nn.Identity(), None, torch.nn.Identity())
    with torch.no_grad():
        return model._run_cnn((torch.from_numpy(x).cuda(), torch.from_numpy(lens)))


def handover_equals_two_calls():
    """conv1 -> clamp -> conv2 with the planes handed over equals calling the two modules one after the other, bit for bit,
    and the pair really takes the fused entry points (``ms_conv_set_variant(1)`` turns them off)."""
    from myrtlespeech_amd import _lib
    from myrtlespeech_amd.model.cnn import conv_pair_forward
    os.environ["MS_CONV_MFMA_MIN_FLOPS"] = "0"
    lib = _lib.load()
    cnn = ds2_cnn()
    rng = np.random.default_rng(5)
    for tn in (130, 257):
        x = (rng.normal(size=(3, 1, 80, tn)) * 3).astype(np.float32)
        lens = ragged_lens(tn, 3, 11)
        with torch.no_grad():
            y1, l1 = cnn[0]((torch.from_numpy(x).cuda(), torch.from_numpy(lens)), fused_activation=(0.0, 20.0))
            want, want_lens = cnn[2]((y1, l1), fused_activation=(0.0, 20.0))
            pair = conv_pair_forward(cnn[0], (0.0, 20.0), cnn[2], (0.0, 20.0), (torch.from_numpy(x).cuda(), torch.from_numpy(lens)))
        assert pair is not None, "the DS2 pair must take the fused entry points"
        got, got_lens = run_cnn(cnn, x, lens)
        for y, nl in (pair, (got, got_lens)):
            assert y.shape == want.shape and torch.equal(y, want), (tn, float((y - want).abs().max()))
            assert torch.equal(nl.cpu(), want_lens.cpu()) and nl.dtype == want_lens.dtype
        lib.ms_conv_set_variant(1)
        try:
            with torch.no_grad():
                assert conv_pair_forward(cnn[0], (0.0, 20.0), cnn[2], (0.0, 20.0),
                                         (torch.from_numpy(x).cuda(), torch.from_numpy(lens))) is None
            old, old_lens = run_cnn(cnn, x, lens)
        finally:
            lib.ms_conv_set_variant(0)
        assert torch.equal(old, want) and torch.equal(old_lens.cpu(), want_lens.cpu())


if __name__ == "__main__":
    {"handover": handover_equals_two_calls}[sys.argv[1]]()
    print("ok")
