"""The LSTM backward on the device through the C ABI (``ms_lstm_recompute``, ``ms_lstm_backward_steps``,
``ms_embedding_backward``) against the float64 restatement tests/lstm_backward_ref.py, whose docstring derives the bounds the
device is held to: gates and c per element, dG per (t, n) row, d_h0 and d_c0 per n and d_b as a whole in the 2-norm.

Tiles.  The step kernel gives a workgroup 32 hidden units (one MFMA tile of columns) and walks the batch in passes of 32 rows
(one MFMA tile of rows); its K = 4H extent is dealt to eight waves in octets of k.  H in {8, 40, 72} is below a unit tile, a
tile and a tail, two tiles and a tail (and 4H / 8 = 4, 20, 36 octets: waves with nothing, and uneven shares); N in {1, 3, 33} is
one row, a partial row tile, a full tile and one more row.  The recompute's GEMM tiles are 128 rows by 32 / 64 / 128
columns: T N in {1 .. 297} and 4H in {32, 160, 288} lie on both sides.  T in {1, 2, 9}: the d_h0 launch directly after the
first step, one carried step, many.  In in {5, 33}: the GEMM's scalar and its 16-byte loads.

Every output is pre-filled with a sentinel and the workspace with 0xFF bytes.  The device feeds its own gates and c to its
backward, as the autograd node does.  Each case also prints the device's error on d_h0, d_c0 and d_b as a multiple of the
error of torch's float32 CPU autograd on the same case (both against float64, both relative to the tensor's largest
magnitude; an error of torch's below 2^-24 counts as 2^-24).  Measured on one MI355X over every case of this file -- worst
ratios to the bounds: gates 0.17, c 0.069, dG 0.029, d_h0 0.0092, d_c0 0.024, d_b 0.025 (MEASURED_RATIOS); worst multiples of
torch's float32 error: d_h0 1.28, d_c0 1.73, d_b 2.0 (MEASURED_MULTIPLES; all three on the one-row, eight-unit case, the
others are at or below 1.35); the asserted cap is four times each multiple (room for another reduction order on other
shapes; a wrong term shows as orders of magnitude).
"""
import numpy as np
import pytest
import torch

import lstm_backward_ref as L
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
CASES = L.cases()
U24 = 2.0 ** -24
# measured on one MI355X (this file, every case; tools/lstm_backward_time.py records them in profiles/lstm_backward_time.json)
MEASURED_RATIOS = dict(gates=0.17, c=0.069, dG=0.029, d_h0=0.0092, d_c0=0.024, d_b=0.025)
MEASURED_MULTIPLES = dict(d_h0=1.28, d_c0=1.73, d_b=2.0)
worst = {}
worst_mult = {}


def f32(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda().contiguous()


def i32(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a).reshape(-1), dtype=torch.int32).cuda()


def filled(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


class Device:
    """A case's tensors on the device and the two C-ABI calls on them."""

    def __init__(self, name):
        k = self.k = CASES[name]
        self.T, self.N, self.H, self.In = k["T"], k["N"], k["H"], k["In"]
        p = k["p"]
        self.x, self.h = f32(k["x"]), f32(L.reference(name)["h32"])
        self.h0, self.c0 = f32(k["h0"]), f32(k["c0"])
        self.w_ih, self.w_hh, self.b_ih, self.b_hh = f32(p["w_ih"]), f32(p["w_hh"]), f32(p["b_ih"]), f32(p["b_hh"])
        self.lens = i32(k["lens"])
        self.max_len = self.T if k["lens"] is None else int(k["lens"].max())
        self.d_out, self.d_hn, self.d_cn = f32(k["d_out"]), f32(k["d_hn"]), f32(k["d_cn"])

    def recompute(self, workspace_bytes=None, expect=None, **null):
        lib = _lib.load()
        T, N, H, In = self.T, self.N, self.H, self.In
        need = lib.ms_lstm_recompute_workspace_bytes(T, N, H)
        assert need >= 2 * T * N * 4 * H * 4
        nbytes = need if workspace_bytes is None else workspace_bytes
        ws = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device="cuda")
        self.gates, self.c = filled(T, N, 4 * H), filled(T, N, H)
        a = dict(x=self.x, h=self.h, w_ih=self.w_ih, w_hh=self.w_hh, gates=self.gates, c=self.c)
        a.update(null)
        rc = lib.ms_lstm_recompute(_lib.ptr(a["x"]), _lib.ptr(a["h"]), _lib.ptr(self.h0), _lib.ptr(self.c0), _lib.ptr(self.lens),
                                   _lib.ptr(a["w_ih"]), _lib.ptr(a["w_hh"]), _lib.ptr(self.b_ih), _lib.ptr(self.b_hh),
                                   _lib.ptr(a["gates"]), _lib.ptr(a["c"]), T, N, In, H, _lib.ptr(ws), nbytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        if expect is not None:
            assert _lib.ERR_NAMES[rc] == expect
            return None
        _lib.check(rc, "ms_lstm_recompute")
        return self.gates.cpu().numpy(), self.c.cpu().numpy()

    def backward(self, expect=None, **null):
        """After ``recompute()``: the device's own gates and c."""
        lib = _lib.load()
        T, N, H = self.T, self.N, self.H
        out = dict(dG=filled(T, N, 4 * H), d_h0=filled(N, H), d_c0=filled(N, H), d_b=filled(4 * H))
        a = dict(gates=self.gates, c=self.c, w_hh=self.w_hh, d_out=self.d_out, **out)
        a.update(null)
        rc = lib.ms_lstm_backward_steps(_lib.ptr(a["gates"]), _lib.ptr(a["c"]), _lib.ptr(self.c0), _lib.ptr(a["w_hh"]),
                                        _lib.ptr(a["d_out"]), _lib.ptr(self.d_hn), _lib.ptr(self.d_cn), _lib.ptr(self.lens),
                                        self.max_len, _lib.ptr(a["dG"]), _lib.ptr(a["d_h0"]), _lib.ptr(a["d_c0"]), _lib.ptr(a["d_b"]),
                                        T, N, H, _lib.stream_ptr())
        torch.cuda.synchronize()
        if expect is not None:
            assert _lib.ERR_NAMES[rc] == expect
            return None
        _lib.check(rc, "ms_lstm_backward_steps")
        return tuple(out[key].cpu().numpy() for key in ("dG", "d_h0", "d_c0", "d_b"))


def note(store, w, name, what):
    for key, v in w.items():
        store[key] = max(store.get(key, 0.0), v)
    print(f"{name}: {what} {({key: round(float(v), 4) for key, v in w.items()})}")
    print(f"worst {what} so far", {key: round(float(v), 4) for key, v in store.items()})


def multiples(name, d_h0, d_c0, d_b):
    """The device's error as a multiple of torch's float32 CPU autograd's, per tensor torch exposes."""
    k, r = CASES[name], L.reference(name)
    t64, t32 = L.torch_layer(k, np.float64), L.torch_layer(k, np.float32)
    out = {}
    for key, got in (("d_h0", d_h0), ("d_c0", d_c0), ("d_b", d_b)):
        if key not in t64 or not np.any(r[key]):
            continue
        out[key] = L.rel_err(got, r[key]) / max(L.rel_err(t32[key], t64[key]), U24)
    return out


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_case_within_the_bounds(name):
    r = L.reference(name)
    dev = Device(name)
    gates, c = dev.recompute()
    dG, d_h0, d_c0, d_b = dev.backward()
    live = L.live_mask(name)
    assert not np.any(np.where(live, 0, dG)), "rows of dG past a length must be exact zeros"
    for a in (dG, d_h0, d_c0, d_b, np.where(live, gates, 0), np.where(live, c, 0)):
        assert np.all(np.isfinite(a)) and not np.any(a == SENTINEL)
    w = dict(L.recompute_ratios(name, gates, c), **L.backward_ratios(name, dG, d_h0, d_c0, d_b))
    note(worst, w, name, "ratios to the bounds")
    m = multiples(name, d_h0, d_c0, d_b)
    note(worst_mult, m, name, "multiples of torch's float32 error")
    assert max(w.values()) <= 1.0, (name, w)
    if MEASURED_MULTIPLES is not None:
        for key, v in m.items():
            assert v <= 4.0 * MEASURED_MULTIPLES[key], (name, key, v)
    # the same inputs give the same bits
    gates2, c2 = dev.recompute()
    again = dev.backward()
    assert np.where(live, gates, 0).tobytes() == np.where(live, gates2, 0).tobytes()
    assert np.where(live, c, 0).tobytes() == np.where(live, c2, 0).tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip((dG, d_h0, d_c0, d_b), again))


def test_backward_from_the_reference_gates():
    """The step kernel alone, fed the float64 gates and c rounded to float32: inside the same bounds (which then allow for
    more than the rounding of its inputs), so an error of the recompute cannot hide one of the backward."""
    name = "t9_n33_h72_ragged"
    r = L.reference(name)
    dev = Device(name)
    dev.gates, dev.c = f32(r["gates"]), f32(r["c"])
    w = L.backward_ratios(name, *dev.backward())
    note(worst, w, name + " (reference gates)", "ratios to the bounds")
    assert max(w.values()) <= 1.0, w


@pytest.mark.parametrize("R,D,V1", [(1, 1, 1), (50, 6, 7), (300, 130, 9)])
def test_embedding_backward(R, D, V1):
    """Against numpy.add.at in float64: repeated indices, indices out of range on both sides (the look-up's clamp), a row that
    is never looked up; D on both sides of the 128 threads of a workgroup.  Bound: a float32 sum of at most R terms."""
    rng = np.random.default_rng(R + D)
    d_out = rng.standard_normal((R, D)).astype(np.float32)
    idx = rng.integers(-2, V1 + 2, size=R).astype(np.int32)
    unused = V1 // 2 if V1 > 2 else None
    if unused is not None:
        idx[idx == unused] = 0
    clamped = np.clip(idx, 0, V1 - 1)
    want, mag = np.zeros((V1, D)), np.zeros((V1, D))
    np.add.at(want, clamped, d_out.astype(np.float64))
    np.add.at(mag, clamped, np.abs(d_out.astype(np.float64)))
    lib = _lib.load()
    got = []
    d_out_dev, idx_dev = f32(d_out), i32(idx)
    for _ in range(2):
        d_table = filled(V1, D)
        _lib.check(lib.ms_embedding_backward(_lib.ptr(d_out_dev), _lib.ptr(idx_dev), _lib.ptr(d_table), R, D, V1, _lib.stream_ptr()),
                   "ms_embedding_backward")
        torch.cuda.synchronize()
        got.append(d_table.cpu().numpy())
    assert np.all(np.abs(got[0] - want) <= R * U24 * mag)
    assert got[0].tobytes() == got[1].tobytes()
    if unused is not None:
        assert not np.any(got[0][unused])
    if R > 1:
        assert len(set(clamped.tolist())) < R and idx.min() < 0 and idx.max() >= V1      # the case holds what it claims


def test_error_codes():
    lib = _lib.load()
    dev = Device("t2_n3_h40_equal")
    T, N, H, In = dev.T, dev.N, dev.H, dev.In
    assert lib.ms_lstm_recompute_workspace_bytes(0, N, H) == 0 and lib.ms_lstm_recompute_workspace_bytes(T, N, -1) == 0
    for key in ("x", "h", "w_ih", "w_hh", "gates", "c"):
        dev.recompute(expect="MS_ERR_INVALID", **{key: None})
    dev.recompute(workspace_bytes=lib.ms_lstm_recompute_workspace_bytes(T, N, H) - 1, expect="MS_ERR_WORKSPACE")
    dev.recompute()
    for key in ("gates", "c", "w_hh", "d_out", "dG", "d_h0", "d_c0", "d_b"):
        dev.backward(expect="MS_ERR_INVALID", **{key: None})
    null, st = _lib.ptr(None), _lib.stream_ptr()
    x = _lib.ptr(dev.x)         # any valid device pointer: the shape is refused before anything is read
    for shape in ((0, N, In, H), (T, 0, In, H), (T, N, 0, H), (T, N, In, 0)):
        assert lib.ms_lstm_recompute(x, x, null, null, null, x, x, null, null, x, x, *shape, x, 1 << 20, st) == 1
    for shape in ((0, N, H), (T, 0, H), (T, N, 0)):
        assert lib.ms_lstm_backward_steps(x, x, null, x, x, null, null, null, 1, x, x, x, x, *shape, st) == 1
    for max_len in (0, T + 1):
        assert lib.ms_lstm_backward_steps(x, x, null, x, x, null, null, x, max_len, x, x, x, x, T, N, H, st) == 1
    for args in ((null, x, x, 1, 1, 1), (x, null, x, 1, 1, 1), (x, x, null, 1, 1, 1), (x, x, x, 0, 1, 1), (x, x, x, 1, 0, 1),
                 (x, x, x, 1, 1, 0)):
        assert lib.ms_embedding_backward(*args, st) == 1
    torch.cuda.synchronize()
