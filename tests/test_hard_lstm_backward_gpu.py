"""The HardLSTM backward on the device through the C ABI (``ms_hard_lstm_recompute``, ``ms_hard_lstm_backward_steps``) against
tests/hard_lstm_backward_ref.py (``R``): the float64 restatement and its derived bounds, fed the device's OWN forward output.

  the kink table   one T = 1 step whose units sit on every kink and its float32 neighbours: dA, d_c0 and d_b are torch float32
                   autograd's bits (P closed, Q open, two roundings in z).
  the cases        ``R.cases()``, each the smallest shape that crosses one edge of the kernels.  The kink margin recomputed from
                   the device's h is asserted to be >= 8 x the largest bound on a recomputed value (the cases carry 16 x on the
                   CPU, so the device's forward cannot eat it); then gates (the pre-clamp plane), c, dA, d_h0, d_c0, d_b are
                   inside the bounds (ratio <= 1); direction 0 of ndir = 2 is BIT-equal to the ndir = 1 call; a second run gives
                   the same bits; guard zones around every output are intact and every output is fully written.
  NaN              a NaN in one sequence's x leaves the other sequences' rows of dA and d_h0 bit-identical.
  errors           the codes the header lists.
MEASURED_RATIOS: the worst ratios to the bounds over every case and direction, measured on one MI355X -- gates 0.34, c 0.41
(both on the 33 x 40 bidirectional case, whose bounds are the smallest), dA 0.053, d_h0 0.013, d_c0 0.020, d_b 0.037.  A record:
the criterion is the bound.  tools/hard_lstm_backward_time.py records them in profiles/hard_lstm_backward_time.json.
"""
import numpy as np
import pytest
import torch

import hard_lstm_backward_ref as R
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 64          # floats either side of an output: 256 bytes, so the outputs keep the allocator's alignment
CASES = R.cases()
MEASURED_RATIOS = dict(gates=0.34, c=0.41, dA=0.053, d_h0=0.013, d_c0=0.020, d_b=0.037)
worst = {}


def f32(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda().contiguous()


class Guarded:
    """An output buffer between two guard zones, everything pre-filled with the sentinel."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.raw = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.raw[GUARD:GUARD + n].view(*shape)

    def numpy(self):
        raw = self.raw.cpu().numpy()
        assert np.all(raw[:GUARD] == SENTINEL) and np.all(raw[-GUARD:] == SENTINEL), "a guard zone was written"
        out = self.t.cpu().numpy()
        assert not np.any(out == SENTINEL), "an output element was left unwritten"
        return out


def workspace(nbytes):
    return torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device="cuda")


def note(w, name):
    for key, v in w.items():
        worst[key] = max(worst.get(key, 0.0), v)
    print(f"{name}: ratios to the bounds {({key: round(float(v), 4) for key, v in w.items()})}")
    print("worst ratios to the bounds so far", {key: round(float(v), 4) for key, v in worst.items()})


def device_forward(k):
    """``HardLSTM.forward`` on the case: the layer's output [T, N, ndir H] as the device computes it (float32 numpy)."""
    from myrtlespeech_amd.model.hard_lstm import HardLSTM
    m = HardLSTM(k["In"], k["H"], 1, bidirectional=k["ndir"] == 2)
    with torch.no_grad():
        for d, params in enumerate(m._layer_params()[0]):
            for q, key in zip(params, ("w_ih", "w_hh", "b_ih", "b_hh")):
                v = k["p"][d][key]
                q.copy_(torch.zeros_like(q) if v is None else torch.as_tensor(v))
        hx = None if k["h0"] is None else (f32(k["h0"]), f32(k["c0"]))
        (out, _), _ = m((f32(k["x"]), torch.full((k["N"],), k["T"])), hx)
    return out.cpu().numpy()


class Device:
    """A case's tensors on the device and the two C-ABI calls on them.  ``ndir`` / ``x`` may be overridden."""

    def __init__(self, k, h, ndir=None, x=None):
        self.k = k
        self.T, self.N, self.H, self.In = k["T"], k["N"], k["H"], k["In"]
        nd = self.ndir = k["ndir"] if ndir is None else ndir
        H = self.H
        self.x = f32(k["x"] if x is None else x)
        self.h = [f32(h[..., d * H:(d + 1) * H]) for d in range(nd)]
        cut = lambda a: None if a is None else f32(a[:nd])      # noqa: E731
        self.h0, self.c0, self.d_hn, self.d_cn = cut(k["h0"]), cut(k["c0"]), cut(k["d_hn"]), cut(k["d_cn"])
        self.p = [{key: f32(v) for key, v in k["p"][d].items()} for d in range(nd)]
        self.d_out = f32(k["d_out"][..., :nd * H])
        self.gates, self.c = Guarded(nd, self.T, self.N, 4 * H), Guarded(nd, self.T, self.N, H)

    def recompute(self, d, workspace_bytes=None, expect=None, reverse=None, **null):
        lib = _lib.load()
        T, N, H, In = self.T, self.N, self.H, self.In
        need = lib.ms_lstm_recompute_workspace_bytes(T, N, H)
        nbytes = need if workspace_bytes is None else workspace_bytes
        ws = workspace(nbytes)
        p = self.p[d]
        a = dict(x=self.x, h=self.h[d], w_ih=p["w_ih"], w_hh=p["w_hh"], gates=self.gates.t[d], c=self.c.t[d])
        a.update(null)
        pick = lambda s: None if s is None else s[d]      # noqa: E731
        rc = lib.ms_hard_lstm_recompute(_lib.ptr(a["x"]), _lib.ptr(a["h"]), _lib.ptr(pick(self.h0)), _lib.ptr(pick(self.c0)),
                                        _lib.ptr(a["w_ih"]), _lib.ptr(a["w_hh"]), _lib.ptr(p["b_ih"]), _lib.ptr(p["b_hh"]),
                                        _lib.ptr(a["gates"]), _lib.ptr(a["c"]), T, N, In, H, d if reverse is None else reverse,
                                        _lib.ptr(ws), nbytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        if expect is not None:
            assert _lib.ERR_NAMES[rc] == expect, (_lib.ERR_NAMES[rc], expect)
            return
        _lib.check(rc, "ms_hard_lstm_recompute")

    def backward(self, expect=None, ndir=None, **null):
        """After every direction's ``recompute``: (dA, d_h0, d_c0, d_b), direction major."""
        lib = _lib.load()
        T, N, H, nd = self.T, self.N, self.H, self.ndir
        out = dict(dA=Guarded(nd, T, N, 4 * H), d_h0=Guarded(nd, N, H), d_c0=Guarded(nd, N, H), d_b=Guarded(nd, 4 * H))
        a = dict(gates=self.gates.t, c=self.c.t, w_hh_fwd=self.p[0]["w_hh"], w_hh_rev=self.p[1]["w_hh"] if nd == 2 else None,
                 d_out=self.d_out, **{key: v.t for key, v in out.items()})
        a.update(null)
        rc = lib.ms_hard_lstm_backward_steps(_lib.ptr(a["gates"]), _lib.ptr(a["c"]), _lib.ptr(self.c0), _lib.ptr(a["w_hh_fwd"]),
                                             _lib.ptr(a["w_hh_rev"]), _lib.ptr(a["d_out"]), _lib.ptr(self.d_hn), _lib.ptr(self.d_cn),
                                             _lib.ptr(a["dA"]), _lib.ptr(a["d_h0"]), _lib.ptr(a["d_c0"]), _lib.ptr(a["d_b"]), T, N, H,
                                             nd if ndir is None else ndir, _lib.stream_ptr())
        torch.cuda.synchronize()
        if expect is not None:
            assert _lib.ERR_NAMES[rc] == expect, (_lib.ERR_NAMES[rc], expect)
            return None
        _lib.check(rc, "ms_hard_lstm_backward_steps")
        return tuple(out[key].numpy() for key in ("dA", "d_h0", "d_c0", "d_b"))

    def run(self):
        """Both calls: (gates, c, dA, d_h0, d_c0, d_b), direction major, guards checked."""
        for d in range(self.ndir):
            self.recompute(d)
        return (self.gates.numpy(), self.c.numpy()) + self.backward()


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_kink_table_on_the_device_is_torch_float32_autograd_bit_for_bit():
    """w_ih is the identity on In = 4H, the biases are NULL and h0 is absent, so a = x exactly; c0, f and i are chosen so that
    c lands on +-1 and its neighbours (``R.kink_table``)."""
    kt = R.kink_table()
    H = kt["H"]
    want = R.kink_expected(np.float32)
    rng = np.random.default_rng(3)
    k = dict(T=1, N=1, In=4 * H, H=H, ndir=1, x=kt["a"].reshape(1, 1, 4 * H),
             p=(dict(w_ih=np.eye(4 * H, dtype=np.float32), w_hh=rng.uniform(-0.3, 0.3, (4 * H, H)).astype(np.float32), b_ih=None,
                     b_hh=None),),
             h0=None, c0=kt["c0"].reshape(1, 1, H), d_out=R.kink_d_out(H).reshape(1, 1, H), d_hn=None,
             d_cn=np.full((1, 1, H), 0.75, dtype=np.float32))
    dev = Device(k, np.zeros((1, 1, H), dtype=np.float32))
    gates, c, dA, d_h0, d_c0, d_b = dev.run()
    emu = R.kink_emulate()
    assert same_bits(c.reshape(-1), want["c"]) and same_bits(c.reshape(-1), emu["c"])
    bad = [kt["names"][j % H] for j in np.nonzero(dA.reshape(-1).view(np.uint32) != want["dA"].view(np.uint32))[0]]
    assert not bad, bad
    assert same_bits(d_c0.reshape(-1), want["d_c0"])
    assert same_bits(d_b.reshape(-1), want["dA"])          # one row: the column sums are the row
    # a = -2.5 is INSIDE (z == 0 after two roundings): the row a fused multiply-add gets wrong
    at = {n: j for j, n in enumerate(kt["names"])}
    for gate, name in ((0, "a_i"), (1, "a_f"), (3, "a_o")):
        j = at[f"{name}={np.float32(-2.5)!r}"]
        assert gates.reshape(4, H)[gate, j] == 0.0 and dA.reshape(4, H)[gate, j] != 0.0
    assert np.allclose(d_h0.reshape(-1), dA.reshape(-1).astype(np.float64) @ k["p"][0]["w_hh"].astype(np.float64), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_case_bounds_and_bits(name):
    k = CASES[name]
    nd, H = k["ndir"], k["H"]
    h = device_forward(k)
    r = R.reference(k, h)
    for d in range(nd):
        # asserted, never skipped: the device's own forward must leave the kinks their distance
        print(name, d, "margin from the device's h", r["margin"][d], "largest bound", r["e_kink"][d])
        assert r["margin"][d] >= 8.0 * r["e_kink"][d], (name, d, r["margin"][d], r["e_kink"][d])
    dev = Device(k, h)
    gates, c, dA, d_h0, d_c0, d_b = first = dev.run()
    for d in range(nd):
        for a in (gates[d], c[d], dA[d], d_h0[d], d_c0[d], d_b[d]):
            assert np.all(np.isfinite(a))
        w = R.ratios(r, d, gates[d], c[d], dA[d], d_h0[d], d_c0[d], d_b[d])
        note(w, f"{name} direction {d}")
        assert max(w.values()) <= 1.0, (name, d, w)
    if MEASURED_RATIOS is not None:      # (a record, not a criterion: the criterion is the bound)
        print("recorded worst ratios", MEASURED_RATIOS)
    # a second run gives the same bits
    assert all(same_bits(a, b) for a, b in zip(first, Device(k, h).run()))
    # direction 0 of the bidirectional call is the unidirectional call's bits
    if nd == 2:
        one = Device(k, h, ndir=1).run()
        for key, a, b in zip(("gates", "c", "dA", "d_h0", "d_c0", "d_b"), first, one):
            assert same_bits(a[0], b[0]), (name, key)


@pytest.mark.parametrize("name", [n for n in R.CASE_NAMES if CASES[n]["N"] > 1])
def test_a_nan_in_one_sequence_stays_in_its_rows(name):
    k = CASES[name]
    h = device_forward(k)
    clean = Device(k, h).run()
    bad = k["N"] // 2
    x = k["x"].copy()
    x[0, bad, 0] = np.nan
    dev = Device(k, h, x=x)
    for d in range(k["ndir"]):
        dev.recompute(d)
    dA, d_h0, _, _ = dev.backward()
    others = [n for n in range(k["N"]) if n != bad]
    assert same_bits(dA[:, :, others], clean[2][:, :, others])
    assert same_bits(d_h0[:, others], clean[3][:, others])


def test_error_codes():
    lib = _lib.load()
    k = CASES["t3_n2_h8_bidir"]
    h = R.case_reference("t3_n2_h8_bidir")
    h = np.concatenate(h["h32"], 2)
    dev = Device(k, h)
    T, N, H, In = dev.T, dev.N, dev.H, dev.In
    for key in ("x", "h", "w_ih", "w_hh", "gates", "c"):
        dev.recompute(1, expect="MS_ERR_INVALID", **{key: None})
    dev.recompute(1, reverse=2, expect="MS_ERR_INVALID")
    dev.recompute(1, reverse=-1, expect="MS_ERR_INVALID")
    dev.recompute(1, workspace_bytes=lib.ms_lstm_recompute_workspace_bytes(T, N, H) - 1, expect="MS_ERR_WORKSPACE")
    for d in (0, 1):
        dev.recompute(d)
    for key in ("gates", "c", "w_hh_fwd", "w_hh_rev", "d_out", "dA", "d_h0", "d_c0", "d_b"):
        dev.backward(expect="MS_ERR_INVALID", **{key: None})
    for ndir in (0, 3, -1):
        dev.backward(expect="MS_ERR_INVALID", ndir=ndir)
    null, st = _lib.ptr(None), _lib.stream_ptr()
    x = _lib.ptr(dev.x)         # any valid device pointer: the shape is refused before anything is read
    for shape in ((0, N, In, H), (T, 0, In, H), (T, N, 0, H), (T, N, In, 0), (-1, N, In, H)):
        assert lib.ms_hard_lstm_recompute(x, x, null, null, x, x, null, null, x, x, *shape, 1, x, 1 << 20, st) == 1
    for shape in ((0, N, H), (T, 0, H), (T, N, 0)):
        assert lib.ms_hard_lstm_backward_steps(x, x, null, x, x, x, null, null, x, x, x, x, *shape, 2, st) == 1
    torch.cuda.synchronize()
