"""Dropout on the device: csrc/dropout.hip through the C ABI against the numpy restatement of tests/dropout_ref.py, BIT FOR BIT,
on every edge of the kernel: below / at / above one quad, the n % 4 tail, more than one workgroup, one size past the grid cap
(the stride loop's second trip), views that start one element into their allocation (the element-by-element path; the mask must
be the aligned one), in place, p at both ends, seeds and offsets with live high words, and NaN, Inf and negative values in kept
and in dropped positions.  Every input and output is a view into a larger buffer filled with a sentinel, checked after each run.

Bits of a NaN: IEEE 754 fixes neither the sign nor the payload of the NaN that Inf * 0 makes (the host's is negative, the
device's positive), so where the restatement gives a NaN the device must give a NaN, and everywhere else the same 32 bits.
"""
import ctypes

import numpy as np
import pytest
import torch

import dropout_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
PAD = 8                      # elements of sentinel either side (32 bytes: a view at PAD is 16-byte aligned)
CAP, BLOCK = 2048, 256       # csrc/dropout.hip: MAX_GRID, THREADS
SEED = 0x1234567890abcdef
OFFSET = (1 << 32) + 1
# (found on the CPU: at p = 1 - 2^-24 the mask of this offset keeps element 2563 of 4099 -- the one place the scale 2^24 shows)
OFFSET_KEEPS_ONE = (1 << 32) + 648


class View:
    """``n`` float32 elements ``lead`` elements past a 16-byte boundary inside a sentinel-filled device buffer."""

    def __init__(self, values=None, n=None, lead=0):
        n = len(values) if values is not None else n
        self.buf = torch.full((PAD + lead + n + PAD,), SENTINEL, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[PAD + lead:PAD + lead + n]
        assert self.t.data_ptr() % 16 == 4 * (lead % 4)
        self.edge = np.ones(self.buf.numel(), dtype=bool)
        self.edge[PAD + lead:PAD + lead + n] = False
        if values is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)))

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def read(self):
        got = self.buf.cpu().numpy()
        assert (got[self.edge] == np.float32(SENTINEL)).all(), "a sentinel was overwritten"
        return got[~self.edge].copy()


def same_bits(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaN in other places than the restatement's"
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)) & ~nan)[0]
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def gaussians(n, seed=0):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)      # (about half are negative)


def forward(lib, x, p, seed, offset, lead_x=0, lead_out=0, inplace=False):
    from myrtlespeech_amd import _lib
    xv = View(x, lead=lead_x)
    ov = xv if inplace else View(n=len(x), lead=lead_out)
    rc = lib.ms_dropout_forward(xv.ptr(), ov.ptr(), len(x), R.threshold(p), float(R.scale(p)), seed, offset, _lib.stream_ptr())
    assert rc == 0, _lib.load().ms_last_error()
    got = ov.read()
    if not inplace:
        assert xv.read().tobytes() == np.asarray(x, np.float32).tobytes()      # the input is only read
    return got


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1023, 4099, CAP * BLOCK * 4 + 5])
def test_forward_is_the_restatement_at_every_size(lib, n):
    x = gaussians(n, n)
    want = R.forward(x, 0.25, SEED, OFFSET)
    got = forward(lib, x, 0.25, SEED, OFFSET)
    same_bits(got, want)
    if n >= 255:
        dropped = float((got == 0).mean())
        assert 0.0 < dropped < 1.0 and abs(dropped - 0.25) <= 4 * np.sqrt(0.1875 / n)


@pytest.mark.parametrize("n", [5, 257, 4099])
@pytest.mark.parametrize("lead_x, lead_out", [(1, 0), (0, 1), (1, 1), (3, 2)])
def test_views_at_odd_offsets_get_the_aligned_mask(lib, n, lead_x, lead_out):
    x = gaussians(n, 3)
    aligned = forward(lib, x, 0.5, SEED, 7)
    same_bits(aligned, R.forward(x, 0.5, SEED, 7))
    assert forward(lib, x, 0.5, SEED, 7, lead_x=lead_x, lead_out=lead_out).tobytes() == aligned.tobytes()


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("n", [3, 4099, CAP * BLOCK * 4 + 5])
def test_in_place(lib, n, lead):
    x = gaussians(n, 4)
    same_bits(forward(lib, x, 0.25, SEED, OFFSET, lead_x=lead, inplace=True), R.forward(x, 0.25, SEED, OFFSET))


@pytest.mark.parametrize("p, offset", [(0.25, OFFSET), (0.5, OFFSET), (1.0 - 2.0 ** -24, OFFSET_KEEPS_ONE), (1.0, OFFSET),
                                       (2.0 ** -32, OFFSET)])
def test_every_probability(lib, p, offset):
    n = 4099
    x = gaussians(n, 5)
    want = R.forward(x, p, SEED, offset)
    got = forward(lib, x, p, SEED, offset)
    same_bits(got, want)
    kept = np.nonzero(R.mask(n, p, SEED, offset))[0]
    if p == 1.0:
        assert kept.size == 0 and not got.any()
    elif p > 0.9:
        assert kept.tolist() == [2563] and got[2563] == x[2563] * np.float32(2.0 ** 24) and np.count_nonzero(got) == 1
    elif p < 1e-6:
        assert kept.size == n and got.tobytes() == x.tobytes()      # thr = 1, scale rounds to 1: only the word 0 would drop


def test_high_words_of_seed_and_offset_are_live(lib):
    n = 1023
    x = np.ones(n, dtype=np.float32)
    runs = {}
    for seed, offset in ((SEED, OFFSET), (SEED & 0xFFFFFFFF, OFFSET), (SEED, OFFSET & 0xFFFFFFFF), (SEED, OFFSET + 1),
                         (SEED ^ (1 << 63), OFFSET), (SEED, OFFSET ^ (1 << 63)), (2 ** 64 - 1, 2 ** 64 - 1)):
        got = forward(lib, x, 0.5, seed, offset)
        same_bits(got, R.forward(x, 0.5, seed, offset))
        runs[(seed, offset)] = got.tobytes()
    assert len(set(runs.values())) == len(runs)


def specials(n, keep):
    """Gaussians with NaN, +Inf, -Inf and a negative value each in a kept and in a dropped position."""
    x = gaussians(n, 6)
    kept, dropped = np.nonzero(keep)[0], np.nonzero(~keep)[0]
    assert kept.size >= 4 and dropped.size >= 4
    for i, v in enumerate((np.nan, np.inf, -np.inf, -2.5)):
        x[kept[i]] = x[dropped[i]] = v
    return x, kept, dropped


@pytest.mark.parametrize("n", [13, 257])
def test_nan_inf_and_negative_values_in_kept_and_dropped_positions(lib, n):
    keep = R.mask(n, 0.5, SEED, OFFSET)
    x, kept, dropped = specials(n, keep)
    want = R.forward(x, 0.5, SEED, OFFSET)
    got = forward(lib, x, 0.5, SEED, OFFSET)
    same_bits(got, want)
    assert np.isnan(got[kept[0]]) and got[kept[1]] == np.inf and got[kept[2]] == -np.inf and got[kept[3]] == -5.0
    assert np.isnan(got[dropped[:3]]).all()                                 # NaN * 0, Inf * 0, -Inf * 0: all stay visible
    assert got[dropped[3]] == 0 and np.signbit(got[dropped[3]])             # -2.5 * +0 = -0


def clamp_backward(lib, dy, y, lo, hi, p, seed, offset, leads=(0, 0, 0)):
    from myrtlespeech_amd import _lib
    dv, yv, xv = View(dy, lead=leads[0]), View(y, lead=leads[1]), View(n=len(dy), lead=leads[2])
    rc = lib.ms_clamp_dropout_backward(dv.ptr(), yv.ptr(), xv.ptr(), len(dy), lo, hi, R.threshold(p), float(R.scale(p)), seed, offset,
                                       _lib.stream_ptr())
    assert rc == 0, _lib.load().ms_last_error()
    assert dv.read().tobytes() == dy.tobytes() and yv.read().tobytes() == y.tobytes()
    return xv.read()


@pytest.mark.parametrize("n", [3, 257, 4099, CAP * BLOCK * 4 + 5])
def test_clamp_dropout_backward_gates_and_masks(lib, n):
    lo, hi, p = 0.0, 1.0, 0.25
    rng = np.random.default_rng(n)
    dy = gaussians(n, 8)
    # y: the clamp's three regimes, exactly at lo, exactly at hi, strictly inside -- and NaN
    y = rng.choice(np.array([lo, hi, 0.25, 0.75, np.nextafter(np.float32(lo), np.float32(1)), np.nextafter(np.float32(hi), np.float32(0))],
                            dtype=np.float32), n).astype(np.float32)
    keep = R.mask(n, p, SEED, OFFSET)
    if n >= 257:
        inside = (y > lo) & (y < hi)
        kept_in, drop_in = np.nonzero(keep & inside)[0], np.nonzero(~keep & inside)[0]
        y[kept_in[0]] = np.nan          # a NaN y closes the gate
        y[drop_in[0]] = np.nan
        dy[drop_in[1]] = np.nan         # dy NaN in a dropped position, gate open: NaN * 0 stays visible
        dy[kept_in[1]] = np.nan
        shut = np.nonzero(~inside)[0]
        dy[shut[0]] = np.nan            # dy NaN behind a closed gate: 0
        dy[drop_in[2]] = np.inf
    want = R.clamp_backward(dy, y, lo, hi, p, SEED, OFFSET)
    got = clamp_backward(lib, dy, y, lo, hi, p, SEED, OFFSET)
    same_bits(got, want)
    assert not got[(y == lo) | (y == hi) | np.isnan(y)].any()
    if n >= 257:
        assert np.isnan(got[drop_in[1]]) and np.isnan(got[kept_in[1]]) and np.isnan(got[drop_in[2]]) and got[shut[0]] == 0
        assert got[kept_in[0]] == 0 and got[drop_in[0]] == 0
        assert clamp_backward(lib, dy, y, lo, hi, p, SEED, OFFSET, leads=(1, 2, 3)).tobytes() == got.tobytes()
    # with the gate wide open it is the forward kernel on dy
    wide = clamp_backward(lib, dy, np.full(n, 0.5, np.float32), lo, hi, p, SEED, OFFSET)
    assert wide.tobytes() == forward(lib, dy, p, SEED, OFFSET).tobytes()


def test_argument_checks_return_invalid_and_launch_nothing(lib):
    from myrtlespeech_amd import _lib
    n = 64
    x, out = View(gaussians(n)), View(n=n)
    null, st = ctypes.c_void_p(0), _lib.stream_ptr()
    thr, scale = R.threshold(0.25), float(R.scale(0.25))
    bad = [lib.ms_dropout_forward(null, out.ptr(), n, thr, scale, 0, 0, st),
           lib.ms_dropout_forward(x.ptr(), null, n, thr, scale, 0, 0, st),
           lib.ms_dropout_forward(x.ptr(), out.ptr(), n, 0, scale, 0, 0, st),
           lib.ms_dropout_forward(x.ptr(), out.ptr(), n, (1 << 32) + 1, scale, 0, 0, st),
           lib.ms_dropout_forward(x.ptr(), out.ptr(), n, thr, -1.0, 0, 0, st),
           lib.ms_dropout_forward(x.ptr(), out.ptr(), n, thr, float("inf"), 0, 0, st),
           lib.ms_dropout_forward(x.ptr(), out.ptr(), n, thr, float("nan"), 0, 0, st),
           lib.ms_dropout_forward(x.ptr(), out.ptr(), -1, thr, scale, 0, 0, st),
           lib.ms_clamp_dropout_backward(x.ptr(), null, out.ptr(), n, 0.0, 1.0, thr, scale, 0, 0, st),
           lib.ms_clamp_dropout_backward(null, x.ptr(), out.ptr(), n, 0.0, 1.0, thr, scale, 0, 0, st),
           lib.ms_clamp_dropout_backward(x.ptr(), x.ptr(), null, n, 0.0, 1.0, thr, scale, 0, 0, st),
           lib.ms_clamp_dropout_backward(x.ptr(), x.ptr(), out.ptr(), n, 0.0, 1.0, 0, scale, 0, 0, st),
           lib.ms_clamp_dropout_backward(x.ptr(), x.ptr(), out.ptr(), n, 0.0, 1.0, (1 << 32) + 1, scale, 0, 0, st),
           lib.ms_clamp_dropout_backward(x.ptr(), x.ptr(), out.ptr(), n, 0.0, 1.0, thr, float("nan"), 0, 0, st)]
    assert bad == [1] * len(bad)
    assert lib.ms_dropout_forward(null, null, 0, thr, scale, 0, 0, st) == 0      # n == 0: MS_OK, no launch
    assert lib.ms_clamp_dropout_backward(null, null, null, 0, 0.0, 1.0, thr, scale, 0, 0, st) == 0
    torch.cuda.synchronize()
    assert (out.buf.cpu().numpy() == np.float32(SENTINEL)).all()                  # nothing was written


def test_dropout_train_node_and_its_backward():
    """``dropout_train``: the forward kernel as an autograd node whose backward is the same kernel on the gradient."""
    from myrtlespeech_amd.model import dropout as D
    g = D.DropoutGenerator(SEED)
    g.offset = 5
    x = torch.tensor(gaussians(3 * 7 * 5, 9).reshape(3, 7, 5), device="cuda", requires_grad=True)
    out = D.dropout_train(x, 0.25, g)
    assert g.offset == 6 and out.shape == x.shape
    dy = gaussians(3 * 7 * 5, 10).reshape(3, 7, 5)
    out.backward(torch.tensor(dy, device="cuda"))
    same_bits(out.detach().cpu().numpy().reshape(-1), R.forward(x.detach().cpu().numpy(), 0.25, SEED, 5).reshape(-1))
    same_bits(x.grad.cpu().numpy().reshape(-1), R.forward(dy, 0.25, SEED, 5).reshape(-1))
