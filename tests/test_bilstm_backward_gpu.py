"""The bidirectional LSTM backward on the device through the C ABI (``ms_lstm_recompute_dir``,
``ms_lstm_backward_steps_bidir``) against tests/bilstm_backward_ref.py: the float64 restatement of tests/lstm_backward_ref.py
applied per direction (the reverse one on the case flipped within its lengths), and that file's derived bounds evaluated the
same way.  The geometries are those of tests/test_lstm_backward_gpu.py (its docstring says which tile edges they straddle);
at length 1 the reverse direction's first and last step coincide.

Per case, with every output pre-filled with a sentinel and the workspace with 0xFF bytes:
  1. every output is finite, no sentinel survives, rows of dG past a length are exact zeros in both directions;
  2. both directions are inside the derived bounds (ratio <= 1);
  3. direction 0 is BIT-equal to ``ms_lstm_recompute`` + ``ms_lstm_backward_steps`` on the same inputs, in every output;
  4. direction 1 is BIT-equal, in the live rows of gates and c and in dG, d_h0, d_c0, to the unidirectional entries run on the
     flipped case and flipped back -- row-independent arithmetic, so a wrong index is a mismatch and not a tolerance question;
     d_b is bit-equal where all lengths are equal and held to its bound otherwise (another summation grouping);
  5. two runs give the same bits.
MEASURED_RATIOS: the worst ratios to the bounds over every case and both directions, measured on one MI355X -- gates 0.18,
c 0.069, dG 0.038, d_h0 0.0092, d_c0 0.024, d_b 0.025: the unidirectional file's figures, the reverse direction adding 0.038 on
dG (t9_n33_h8).
"""
import numpy as np
import pytest
import torch

import bilstm_backward_ref as B
import lstm_backward_ref as L
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
CASES = B.cases()
# measured on one MI355X (this file, every case, both directions; tools/bilstm_backward_time.py records them in
# profiles/bilstm_backward_time.json)
MEASURED_RATIOS = dict(gates=0.18, c=0.069, dG=0.038, d_h0=0.0092, d_c0=0.024, d_b=0.025)
worst = {}


def f32(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda().contiguous()


def i32(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a).reshape(-1), dtype=torch.int32).cuda()


def filled(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


def workspace(nbytes):
    return torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device="cuda")


def note(w, name, what):
    for key, v in w.items():
        worst[key] = max(worst.get(key, 0.0), v)
    print(f"{name}: {what} {({key: round(float(v), 4) for key, v in w.items()})}")
    print("worst ratios to the bounds so far", {key: round(float(v), 4) for key, v in worst.items()})


class Device:
    """A bidirectional case's tensors on the device and the two C-ABI calls on them."""

    def __init__(self, name):
        k = self.k = CASES[name]
        self.T, self.N, self.H, self.In = k["T"], k["N"], k["H"], k["In"]
        r = B.reference(name)
        self.x = f32(k["x"])
        self.h = [f32(r["h32"][d]) for d in (0, 1)]
        self.h0, self.c0 = f32(k["h0"]), f32(k["c0"])
        self.p = [{key: f32(v) for key, v in k["p"][d].items()} for d in (0, 1)]
        self.lens = i32(k["lens"])
        self.max_len = self.T if k["lens"] is None else int(k["lens"].max())
        self.d_out, self.d_hn, self.d_cn = f32(k["d_out"]), f32(k["d_hn"]), f32(k["d_cn"])
        self.gates, self.c = filled(2, self.T, self.N, 4 * self.H), filled(2, self.T, self.N, self.H)

    def recompute(self, d, workspace_bytes=None, expect=None, reverse=None, **null):
        lib = _lib.load()
        T, N, H, In = self.T, self.N, self.H, self.In
        need = lib.ms_lstm_recompute_workspace_bytes(T, N, H)
        nbytes = need if workspace_bytes is None else workspace_bytes
        ws = workspace(nbytes)
        self.gates[d].fill_(SENTINEL)
        self.c[d].fill_(SENTINEL)
        p = self.p[d]
        a = dict(x=self.x, h=self.h[d], w_ih=p["w_ih"], w_hh=p["w_hh"], gates=self.gates[d], c=self.c[d])
        a.update(null)
        pick = lambda s: None if s is None else s[d]      # noqa: E731
        rc = lib.ms_lstm_recompute_dir(_lib.ptr(a["x"]), _lib.ptr(a["h"]), _lib.ptr(pick(self.h0)), _lib.ptr(pick(self.c0)),
                                       _lib.ptr(self.lens), _lib.ptr(a["w_ih"]), _lib.ptr(a["w_hh"]), _lib.ptr(p["b_ih"]),
                                       _lib.ptr(p["b_hh"]), _lib.ptr(a["gates"]), _lib.ptr(a["c"]), T, N, In, H,
                                       d if reverse is None else reverse, _lib.ptr(ws), nbytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        if expect is not None:
            assert _lib.ERR_NAMES[rc] == expect
            return None
        _lib.check(rc, "ms_lstm_recompute_dir")
        return self.gates[d].cpu().numpy(), self.c[d].cpu().numpy()

    def backward(self, expect=None, max_len=None, **null):
        """After both ``recompute`` calls (or with ``self.gates`` / ``self.c`` set): (dG, d_h0, d_c0, d_b), direction major."""
        lib = _lib.load()
        T, N, H = self.T, self.N, self.H
        out = dict(dG=filled(2, T, N, 4 * H), d_h0=filled(2, N, H), d_c0=filled(2, N, H), d_b=filled(2, 4 * H))
        a = dict(gates=self.gates, c=self.c, w_hh_fwd=self.p[0]["w_hh"], w_hh_rev=self.p[1]["w_hh"], d_out=self.d_out, **out)
        a.update(null)
        rc = lib.ms_lstm_backward_steps_bidir(_lib.ptr(a["gates"]), _lib.ptr(a["c"]), _lib.ptr(self.c0), _lib.ptr(a["w_hh_fwd"]),
                                              _lib.ptr(a["w_hh_rev"]), _lib.ptr(a["d_out"]), _lib.ptr(self.d_hn),
                                              _lib.ptr(self.d_cn), _lib.ptr(self.lens), self.max_len if max_len is None else max_len,
                                              _lib.ptr(a["dG"]), _lib.ptr(a["d_h0"]), _lib.ptr(a["d_c0"]), _lib.ptr(a["d_b"]), T, N, H,
                                              _lib.stream_ptr())
        torch.cuda.synchronize()
        if expect is not None:
            assert _lib.ERR_NAMES[rc] == expect
            return None
        _lib.check(rc, "ms_lstm_backward_steps_bidir")
        return tuple(out[key].cpu().numpy() for key in ("dG", "d_h0", "d_c0", "d_b"))


def unidirectional(name, d):
    """The UNCHANGED entries (``ms_lstm_recompute``, ``ms_lstm_backward_steps``) on direction d's unidirectional view of the
    case -- for d = 1 the flipped case -- with the per-step results brought back to the layer's time order."""
    lib = _lib.load()
    k, u = CASES[name], B.dir_case(name, d)
    T, N, H, In = u["T"], u["N"], u["H"], u["In"]
    h = B.back(B.reference(name)["h32"][d], d, k["lens"])          # the direction's output in its own run's order
    x, h, h0, c0 = f32(u["x"]), f32(h), f32(u["h0"]), f32(u["c0"])
    p = {key: f32(v) for key, v in u["p"].items()}
    lens = i32(u["lens"])
    max_len = T if u["lens"] is None else int(u["lens"].max())
    ws = workspace(lib.ms_lstm_recompute_workspace_bytes(T, N, H))
    gates, c = filled(T, N, 4 * H), filled(T, N, H)
    _lib.check(lib.ms_lstm_recompute(_lib.ptr(x), _lib.ptr(h), _lib.ptr(h0), _lib.ptr(c0), _lib.ptr(lens), _lib.ptr(p["w_ih"]),
                                     _lib.ptr(p["w_hh"]), _lib.ptr(p["b_ih"]), _lib.ptr(p["b_hh"]), _lib.ptr(gates), _lib.ptr(c), T, N,
                                     In, H, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "ms_lstm_recompute")
    dG, d_h0, d_c0, d_b = filled(T, N, 4 * H), filled(N, H), filled(N, H), filled(4 * H)
    d_out, d_hn, d_cn = f32(u["d_out"]), f32(u["d_hn"]), f32(u["d_cn"])      # (named: they must outlive the call)
    _lib.check(lib.ms_lstm_backward_steps(_lib.ptr(gates), _lib.ptr(c), _lib.ptr(c0), _lib.ptr(p["w_hh"]), _lib.ptr(d_out),
                                          _lib.ptr(d_hn), _lib.ptr(d_cn), _lib.ptr(lens), max_len, _lib.ptr(dG),
                                          _lib.ptr(d_h0), _lib.ptr(d_c0), _lib.ptr(d_b), T, N, H, _lib.stream_ptr()),
               "ms_lstm_backward_steps")
    torch.cuda.synchronize()
    per_step = [B.back(a.cpu().numpy(), d, k["lens"]) for a in (gates, c, dG)]
    return per_step[0], per_step[1], per_step[2], d_h0.cpu().numpy(), d_c0.cpu().numpy(), d_b.cpu().numpy()


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_case_bounds_and_bits(name):
    k = CASES[name]
    dev = Device(name)
    rec = [dev.recompute(d) for d in (0, 1)]
    dG, d_h0, d_c0, d_b = dev.backward()
    live = B.live_mask(name)
    equal_lens = k["lens"] is None or len(set(k["lens"].tolist())) == 1
    for d in (0, 1):
        gates, c = rec[d]
        # 1. finite, fully written, exact zeros past a length
        assert not np.any(np.where(live, 0, dG[d])), "rows of dG past a length must be exact zeros"
        for a in (dG[d], d_h0[d], d_c0[d], d_b[d], np.where(live, gates, 0), np.where(live, c, 0)):
            assert np.all(np.isfinite(a)) and not np.any(a == SENTINEL)
        # 2. inside the derived bounds
        w = dict(B.recompute_ratios(name, d, gates, c), **B.backward_ratios(name, d, dG[d], d_h0[d], d_c0[d], d_b[d]))
        note(w, f"{name} direction {d}", "ratios to the bounds")
        assert max(w.values()) <= 1.0, (name, d, w)
        # 3. / 4. the bits of the unidirectional entries (direction 1: on the flipped case, flipped back)
        ug, uc, udG, ud_h0, ud_c0, ud_b = unidirectional(name, d)
        assert same_bits(np.where(live, gates, 0), np.where(live, ug, 0)), (name, d, "gates")
        assert same_bits(np.where(live, c, 0), np.where(live, uc, 0)), (name, d, "c")
        assert same_bits(dG[d], udG), (name, d, "dG")
        assert same_bits(d_h0[d], ud_h0), (name, d, "d_h0")
        assert same_bits(d_c0[d], ud_c0), (name, d, "d_c0")
        if d == 0 or equal_lens:
            assert same_bits(d_b[d], ud_b), (name, d, "d_b")
    if MEASURED_RATIOS is not None:      # (a record, not a criterion: the criterion is the bound)
        print("recorded worst ratios", MEASURED_RATIOS)
    # 5. the same inputs give the same bits
    rec2 = [dev.recompute(d) for d in (0, 1)]
    again = dev.backward()
    for d in (0, 1):
        assert same_bits(np.where(live, rec[d][0], 0), np.where(live, rec2[d][0], 0))
        assert same_bits(np.where(live, rec[d][1], 0), np.where(live, rec2[d][1], 0))
    assert all(same_bits(a, b) for a, b in zip((dG, d_h0, d_c0, d_b), again))


def test_reverse_zero_is_the_unidirectional_recompute():
    """``reverse = 0`` on the reverse direction's tensors: ``ms_lstm_recompute``'s bits (it is the same call)."""
    name = "t9_n33_h40_ragged"
    dev = Device(name)
    gates, c = dev.recompute(0)
    ug, uc = unidirectional(name, 0)[:2]
    live = B.live_mask(name)
    assert same_bits(np.where(live, gates, 0), np.where(live, ug, 0)) and same_bits(np.where(live, c, 0), np.where(live, uc, 0))


def test_backward_from_the_reference_gates():
    """The step kernel alone, fed the float64 gates and c rounded to float32, both directions: inside the same bounds, so an
    error of the recompute cannot hide one of the backward."""
    name = "t9_n33_h72_ragged"
    r = B.reference(name)
    dev = Device(name)
    dev.gates, dev.c = f32(np.stack(r["gates"])), f32(np.stack(r["c"]))
    dG, d_h0, d_c0, d_b = dev.backward()
    for d in (0, 1):
        w = B.backward_ratios(name, d, dG[d], d_h0[d], d_c0[d], d_b[d])
        note(w, f"{name} direction {d} (reference gates)", "ratios to the bounds")
        assert max(w.values()) <= 1.0, (d, w)


def test_error_codes():
    lib = _lib.load()
    dev = Device("t2_n3_h40_equal")
    T, N, H, In = dev.T, dev.N, dev.H, dev.In
    for key in ("x", "h", "w_ih", "w_hh", "gates", "c"):
        dev.recompute(1, expect="MS_ERR_INVALID", **{key: None})
    dev.recompute(1, reverse=2, expect="MS_ERR_INVALID")
    dev.recompute(1, reverse=-1, expect="MS_ERR_INVALID")
    dev.recompute(1, workspace_bytes=lib.ms_lstm_recompute_workspace_bytes(T, N, H) - 1, expect="MS_ERR_WORKSPACE")
    for d in (0, 1):
        dev.recompute(d)
    for key in ("gates", "c", "w_hh_fwd", "w_hh_rev", "d_out", "dG", "d_h0", "d_c0", "d_b"):
        dev.backward(expect="MS_ERR_INVALID", **{key: None})
    for max_len in (0, T + 1):
        dev.backward(expect="MS_ERR_INVALID", max_len=max_len)
    null, st = _lib.ptr(None), _lib.stream_ptr()
    x = _lib.ptr(dev.x)         # any valid device pointer: the shape is refused before anything is read
    for shape in ((0, N, In, H), (T, 0, In, H), (T, N, 0, H), (T, N, In, 0)):
        assert lib.ms_lstm_recompute_dir(x, x, null, null, null, x, x, null, null, x, x, *shape, 1, x, 1 << 20, st) == 1
    for shape in ((0, N, H), (T, 0, H), (T, N, 0)):
        assert lib.ms_lstm_backward_steps_bidir(x, x, null, x, x, x, null, null, null, 1, x, x, x, x, *shape, st) == 1
    # without lens every sequence has T steps
    assert lib.ms_lstm_backward_steps_bidir(x, x, null, x, x, x, null, null, null, T - 1, x, x, x, x, T, N, H, st) == 1
    torch.cuda.synchronize()
