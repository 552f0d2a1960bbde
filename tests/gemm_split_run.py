"""Device runner of tests/gemm_split_cases.py: ``ms_linear_split_forward``, ``ms_linear_split_pack`` and
``ms_linear_split_forward_packed`` through the C ABI on pre-filled buffers -- x and w inside NaN-filled buffers, y between
guard rows of 0xFFFFFFFF words, workspaces and packed planes filled with 0xFF bytes (NaN in both plane formats) with a guard of
their own -- and the checks that tests/test_gemm_split_gpu.py makes with it.  Every criterion is ``array_equal`` against the
exact expected values, a bit comparison between two calls, or a statement about NaN / Inf.  ``MS_PRECISION`` is read once per
process, so ``python tests/gemm_split_run.py exact nonfinite`` runs the whole list in a process of its own, stops at the first
failure and prints ``ok``."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import gemm_split_cases as C  # noqa: E402
from myrtlespeech_amd import _lib  # noqa: E402

GUARD_ROWS = 3                      # guard rows of N words before and after y
PAD = 64                            # NaN elements before and after x and w (a multiple of 4: the operands stay 16-byte aligned)
GUARD_BYTES = 256                   # behind a workspace or a packed buffer
NONFINITE_ACT = (-20.0, 20.0)


def mode():
    return os.environ.get("MS_PRECISION", "f16x3")


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def act_args(act):
    return (_lib.ACT_NONE, 0.0, 0.0) if act is None else (_lib.ACT_CLAMP, float(act[0]), float(act[1]))


def inside(a):
    """``a`` on the device inside a NaN-filled buffer; (buffer, dense view)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + 2 * PAD,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[PAD:PAD + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 0
    return buf, view


def scratch(nbytes):
    return torch.full((int(nbytes) + GUARD_BYTES,), 0xFF, dtype=torch.uint8, device="cuda")


def scratch_intact(buf, nbytes, what):
    assert bool((buf[int(nbytes):] == 0xFF).all()), (what, "wrote past its buffer")


class Out:
    """y [M, N] between guard rows; every word starts as 0xFFFFFFFF."""

    def __init__(self, M, N):
        self.M, self.N = M, N
        self.words = torch.full(((M + 2 * GUARD_ROWS) * N,), -1, dtype=torch.int32, device="cuda")
        self.y = self.words.view(torch.float32)[GUARD_ROWS * N:(GUARD_ROWS + M) * N].view(M, N)

    def guards_intact(self, what):
        g = GUARD_ROWS * self.N
        assert bool((self.words[:g] == -1).all()), (what, "wrote before y")
        assert bool((self.words[g + self.M * self.N:] == -1).all()), (what, "wrote past y (the row after M included)")

    def untouched(self, what):
        assert bool((self.words == -1).all()), (what, "a refused call wrote to y")

    def poison(self):
        self.words.fill_(-1)

    def take(self, what):
        self.guards_intact(what)
        return self.y.clone()


class Config:
    """``ms_gemm_set_variant`` and the two per-call switches for the duration of a call."""

    def __init__(self, lib, cfg):
        self.lib, self.cfg = lib, cfg

    def __enter__(self):
        v, t64, quarter = self.cfg
        self.saved = {k: os.environ.get(k) for k in ("MS_GEMM_TILE64", "MS_GEMM_QUARTER_TILE")}
        for k, val in (("MS_GEMM_TILE64", t64), ("MS_GEMM_QUARTER_TILE", quarter)):
            if val is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = val
        self.lib.ms_gemm_set_variant(v)

    def __exit__(self, *exc):
        self.lib.ms_gemm_set_variant(0)
        for k, val in self.saved.items():
            if val is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = val


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


class Call:
    """One (x, w, bias) on the device with an output and a workspace that every call of it reuses."""

    def __init__(self, lib, x, w, b):
        self.lib = lib
        (self.M, self.K), self.N = x.shape, w.shape[0]
        self.xbuf, self.x = inside(x)
        self.wbuf, self.w = inside(w)
        self.b = None if b is None else torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).cuda()
        self.zero = torch.zeros(self.N, dtype=torch.float32, device="cuda")
        self.out = Out(self.M, self.N)
        self.nws = lib.ms_linear_split_workspace_bytes(self.M, self.K, self.N)
        self.ws = scratch(self.nws)

    def forward(self, act, what, bias="own", cfg=C.CONFIGS[0]):
        a, lo, hi = act_args(act)
        bd = {"own": self.b, "null": None, "zero": self.zero}[bias]
        self.ws.fill_(0xFF)
        self.out.poison()                            # every call writes into 0xFFFFFFFF words, never over an earlier result
        with Config(self.lib, cfg):
            rc = self.lib.ms_linear_split_forward(_lib.ptr(self.x), _lib.ptr(self.w), _lib.ptr(bd), _lib.ptr(self.out.y), self.M,
                                                  self.K, self.N, a, lo, hi, _lib.ptr(self.ws), self.nws, _lib.stream_ptr())
        _lib.check(rc, str(what))
        got = self.out.take(what)
        scratch_intact(self.ws, self.nws, what)
        return got

    def forward_packed(self, act, what):
        lib, P = self.lib, _lib.ptr
        a, lo, hi = act_args(act)
        npk, nws = lib.ms_linear_split_packed_bytes(self.K, self.N), C.x_workspace_bytes(self.M, self.K)
        packed, ws = scratch(npk), scratch(nws)
        self.out.poison()
        _lib.check(lib.ms_linear_split_pack(P(self.w), P(packed), self.K, self.N, _lib.stream_ptr()), str((what, "pack")))
        # every plane word was written: 0xFFFF is a NaN in both formats and no finite weight gives one (one plane: hi only)
        nwords = self.N * self.K * (2 if C.two_planes(mode()) else 1)
        assert not bool((packed[:2 * nwords].view(torch.int16) == -1).any()), (what, "pack left plane words unwritten")
        _lib.check(lib.ms_linear_split_forward_packed(P(self.x), P(packed), P(self.b), P(self.out.y), self.M, self.K, self.N, a, lo, hi,
                                                      P(ws), nws, _lib.stream_ptr()), str((what, "forward_packed")))
        got = self.out.take(what)
        scratch_intact(packed, npk, (what, "pack"))
        scratch_intact(ws, nws, (what, "x planes"))
        return got


def exact(got, want, what):
    host = got.cpu().numpy()
    assert host.dtype == np.float32 and host.shape == want.shape, what
    bad = ~(host.astype(np.float64) == want)
    assert not bad.any(), (what, int(bad.sum()), "wrong; first at", np.argwhere(bad)[:4].tolist(), host[bad][:4].tolist(),
                           want[bad][:4].tolist())


def check_routes(c, md, cus):
    """The case must run on the kernels it was sized for: the restated launcher with the device's CU count."""
    assert cus == C.CUS, f"this device has {cus} compute units; the case list of gemm_split_cases.py is sized for {C.CUS}"
    have, want = C.routes(c, md, cus), C.routes(c, md, C.CUS)
    assert have == want and have[C.CONFIGS[0]] == C.INTENDED[c.group], (C.tag(c), md, "compute units", cus, have, want)
    return have


def check_case(lib, c, ran=None):
    """Every family of a case in this process's mode: exact values, a second call, every variant and switch, the packed path,
    bias NULL against a zero bias, the size queries.  ``ran`` collects {kernel: families}."""
    md = mode()
    rts = check_routes(c, md, cu_count())
    assert lib.ms_linear_split_workspace_bytes(c.M, c.K, c.N) == C.workspace_bytes(c.M, c.K, c.N) > 0
    assert lib.ms_linear_split_packed_bytes(c.K, c.N) == C.packed_bytes(c.K, c.N) > 0
    for fam in C.families(c.M, c.K, c.N, md):
        x, w, b = C.make(fam, c.M, c.K, c.N, md)
        act = C.act_of(fam)
        xw = C.Planes(x, w, md).product()
        what = (C.tag(c), md, fam)
        call = Call(lib, x, w, b)
        y0 = call.forward(act, what)
        exact(y0, C.clip(xw + b.astype(np.float64), act), what)
        assert same_bits(call.forward(act, (what, "second call")), y0), (what, "the second call differs")
        for cfg in C.CONFIGS[1:]:
            assert same_bits(call.forward(act, (what, cfg), cfg=cfg), y0), (what, cfg, rts[cfg], "differs from", rts[C.CONFIGS[0]])
        assert same_bits(call.forward_packed(act, what), y0), (what, "the packed path differs")
        y_null = call.forward(act, (what, "bias NULL"), bias="null")
        assert same_bits(y_null, call.forward(act, (what, "zero bias"), bias="zero")), (what, "bias NULL differs from a zero bias")
        if b.any():
            exact(y_null, C.clip(xw, act), (what, "bias NULL"))
        else:
            assert same_bits(y_null, y0), (what, "bias NULL differs from the zero bias of the family")
        if ran is not None:
            for k in set(rts.values()):
                ran.setdefault(k, set()).add(fam)


def check_nonfinite(lib, c, cfg):
    """The contract of include/ms_hotpath.h on one case and configuration, with and without the clamp: a NaN in x[m0, k0]
    makes row m0 NaN and leaves every other row's bits; an Inf makes it non-finite (through the clamp: NaN with two planes,
    whose lo plane is Inf - Inf; the bound that Hardtanh gives an Inf with one plane); the same for w and columns."""
    md = mode()
    check_routes(c, md, cu_count())
    x, w, b = C.make("lo", c.M, c.K, c.N, md)
    assert np.all(w != 0) and np.all(x != 0)
    for act in (None, NONFINITE_ACT):
        clean = Call(lib, x, w, b).forward(act, (C.tag(c), cfg, "clean"), cfg=cfg)
        exact(clean, C.expected(x, w, b, md, act), (C.tag(c), md, cfg, act, "clean"))
        for operand, rows, other in (("x", c.M, w), ("w", c.N, x)):
            for r0, k0 in C.nonfinite_positions(rows, c.K):
                for poison in (np.nan, np.inf, -np.inf):
                    what = (C.tag(c), md, cfg, act, operand, (r0, k0), poison)
                    a = (x if operand == "x" else w).copy()
                    a[r0, k0] = poison
                    got = Call(lib, a if operand == "x" else x, a if operand == "w" else w, b).forward(act, what, cfg=cfg)
                    line = got[r0] if operand == "x" else got[:, r0]
                    keep = torch.ones(rows, dtype=torch.bool, device="cuda")
                    keep[r0] = False
                    rest, rest0 = (got[keep], clean[keep]) if operand == "x" else (got[:, keep], clean[:, keep])
                    assert same_bits(rest, rest0), (what, "changed outputs that do not read it")
                    if np.isnan(poison) or (act is not None and C.two_planes(md)):
                        assert bool(torch.isnan(line).all()), (what, "not NaN", line[:8].tolist())
                    elif act is None:
                        assert not bool(torch.isfinite(line).any()), (what, "finite", line[:8].tolist())
                    else:
                        sign = np.sign(poison) * np.sign(C.plane(other[:, k0], C.fmt_of(md)))
                        want = np.where(sign > 0, act[1], act[0]).astype(np.float32)
                        assert np.array_equal(line.cpu().numpy(), want), (what, "Hardtanh of an Inf")


def run_exact(lib, ran=None):
    for c in C.cases():
        check_case(lib, c, ran)


def run_nonfinite(lib, ran=None):
    for c, cfg in C.nonfinite_cases():
        check_nonfinite(lib, c, cfg)


if __name__ == "__main__":
    the_lib = _lib.load()
    kernels = {}
    for job in sys.argv[1:]:
        {"exact": run_exact, "nonfinite": run_nonfinite}[job](the_lib, kernels)
    for k in sorted(kernels):
        print("mode", mode(), "kernel", k, "families", sorted(kernels[k]))
    print("ok")
