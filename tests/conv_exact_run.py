"""Device runner of tests/conv_exact_cases.py: every convolution entry point of include/ms_hotpath.h called through the C
ABI on pre-filled buffers -- a sentinel in every output element, a guard row of sentinels past the end, packed filters,
workspaces and planes buffers filled with 0xFF bytes (NaN as floats, NaN as fp16 / bf16 planes) with a guard of their own --
and the checks that tests/test_conv_exact_gpu.py makes with it.  ``MS_PRECISION`` is read once per process, so
``python tests/conv_exact_run.py exact|isolation|clamped`` runs the split-kernel checks in a process of its own and prints ``ok``."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_exact_cases as C  # noqa: E402
from myrtlespeech_amd import _lib  # noqa: E402

GUARD = 256                         # guard elements past y, guard bytes past a scratch buffer
SENTINEL = -7.25e33
SPLIT_ENTRIES = ("cl", "fwin", "gemm1d")


def one_plane():
    return os.environ.get("MS_PRECISION") == "fp16"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def act_args(act):
    return (_lib.ACT_NONE, 0.0, 0.0) if act is None else (_lib.ACT_CLAMP, float(act[0]), float(act[1]))


def lens_dev(lens):
    return None if lens is None else torch.tensor(list(lens), dtype=torch.int32, device="cuda")


def y_buffer(count):
    return torch.full((count + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")


def take(buf, shape, what):
    """The outputs of a finished call: the guard past them untouched, every one of them written."""
    host = buf.cpu().numpy()
    count = int(np.prod(shape))
    assert np.all(host[count:] == np.float32(SENTINEL)), (what, "wrote past the outputs")
    got = host[:count]
    assert not np.any(got == np.float32(SENTINEL)), (what, "outputs not written", int(np.sum(got == np.float32(SENTINEL))))
    return got.reshape(shape).copy()


def untouched(buf, what):
    assert bool((buf == SENTINEL).all()), (what, "a refused call wrote to y")


def scratch(nbytes):
    """``nbytes`` of 0xFF and a guard behind them; hand the kernel ``nbytes``."""
    return torch.full((int(nbytes) + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")


def scratch_intact(buf, nbytes, what):
    assert bool((buf[int(nbytes):] == 0xFF).all()), (what, "wrote past its scratch buffer")


def ok(rc, what):
    _lib.check(rc, str(what))


class Packed:
    """The packed filters of (case, w) for the case's entry point."""

    def __init__(self, lib, c, w):
        wd = dev(w)
        cg = c.Cin // c.groups
        if c.entry == "tap":
            self.bytes = lib.ms_maskconv_packed_bytes(c.Cout, cg, c.KF, c.KT, c.groups)
            self.buf = scratch(self.bytes)
            rc = lib.ms_maskconv_pack(_lib.ptr(wd), _lib.ptr(self.buf), c.Cout, cg, c.KF, c.KT, c.groups, _lib.stream_ptr())
        elif c.entry == "cl":
            self.bytes = lib.ms_maskconv_cl_packed_bytes(c.Cout, c.Cin, c.KF, c.KT)
            self.buf = scratch(self.bytes)
            rc = lib.ms_maskconv_cl_pack(_lib.ptr(wd), _lib.ptr(self.buf), c.Cout, c.Cin, c.KF, c.KT, _lib.stream_ptr())
        elif c.entry == "fwin":
            self.bytes = lib.ms_maskconv_fwin_packed_bytes(c.Cout, c.KF, c.KT)
            self.buf = scratch(self.bytes)
            rc = lib.ms_maskconv_fwin_pack(_lib.ptr(wd), _lib.ptr(self.buf), c.Cout, c.KF, c.KT, _lib.stream_ptr())
        elif c.entry == "gemm1d":
            self.bytes = lib.ms_maskconv1d_gemm_packed_bytes(c.Cout, c.Cin, c.KT)
            self.buf = scratch(self.bytes)
            rc = lib.ms_maskconv1d_gemm_pack(_lib.ptr(wd), _lib.ptr(self.buf), c.Cout, c.Cin, c.KT, _lib.stream_ptr())
        else:
            raise KeyError(c.entry)
        assert self.bytes > 0, (c.tag, "packed bytes")
        ok(rc, (c.tag, "pack"))
        torch.cuda.synchronize()
        scratch_intact(self.buf, self.bytes, (c.tag, "pack"))


def workspace_bytes(lib, c):
    if c.entry == "cl":
        return lib.ms_maskconv_cl_workspace_bytes(c.N, c.Cin, c.Fin, c.Tin)
    if c.entry == "fwin":
        return lib.ms_maskconv_fwin_workspace_bytes(c.N, c.Tin, c.KF, c.SF, c.Fout)
    if c.entry == "gemm1d":
        return lib.ms_maskconv1d_gemm_workspace_bytes(c.N, c.Cin, c.Tout, c.Cout, c.KT)
    return 0


def call(lib, c, xd, ld, packed, bd, yb, ws, ws_bytes, act_code=None):
    """The forward call of the case's entry point; returns its status.  ``act_code`` replaces the activation's code."""
    a, lo, hi = act_args(c.act)
    a = a if act_code is None else act_code
    P, S = _lib.ptr, _lib.stream_ptr()
    if c.entry == "tap":
        return lib.ms_maskconv_forward(P(xd), P(ld), P(packed.buf), P(bd), P(yb), c.N, c.Cin, c.Fin, c.Tin, c.Cout, c.Fout,
                                       c.Tout, c.KF, c.KT, c.SF, c.ST, c.DF, c.DT, c.pad_f, c.pad_t, c.groups, a, lo, hi, S)
    if c.entry == "cl":
        return lib.ms_maskconv_cl_forward(P(xd), P(ld), P(packed.buf), P(bd), P(yb), c.N, c.Cin, c.Fin, c.Tin, c.Cout, c.Fout,
                                          c.Tout, c.KF, c.KT, c.SF, c.ST, c.DF, c.DT, c.pad_f, c.pad_t, a, lo, hi, P(ws),
                                          ws_bytes, S)
    if c.entry == "fwin":
        return lib.ms_maskconv_fwin_forward(P(xd), P(ld), P(packed.buf), P(bd), P(yb), c.N, c.Fin, c.Tin, c.Cout, c.Fout, c.Tout,
                                            c.KF, c.KT, c.SF, c.ST, c.DT, c.pad_f, c.pad_t, a, lo, hi, P(ws), ws_bytes, S)
    if c.entry == "gemm1d":
        return lib.ms_maskconv1d_gemm_forward(P(xd), P(ld), P(packed.buf), P(bd), P(yb), c.N, c.Cin, c.Tin, c.Cout, c.Tout,
                                              c.KT, c.ST, c.DT, c.pad_t, a, lo, hi, P(ws), ws_bytes, S)
    raise KeyError(c.entry)


def run(lib, c, x, w, b, packed=None, what=None):
    """One forward of case ``c`` on (x, w, b): float32 [N, Cout, Fout, Tout]."""
    what = what or (c.entry, c.tag)
    packed = packed or Packed(lib, c, w)
    xd, ld = dev(x), lens_dev(c.lens)
    bd = dev(b) if c.bias else None
    shape = (c.N, c.Cout, c.Fout, c.Tout)
    yb = y_buffer(int(np.prod(shape)))
    nws = workspace_bytes(lib, c)
    ws = scratch(nws) if c.entry != "tap" else None
    ok(call(lib, c, xd, ld, packed, bd, yb, ws, nws), what)
    got = take(yb, shape, what)
    if ws is not None:
        scratch_intact(ws, nws, what)
    scratch_intact(packed.buf, packed.bytes, what)
    return got


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- the checks
def variants(c):
    return (0, 1) if c.entry == "fwin" else (0,)


def check_exact(lib, c, fams):
    """Every family of a case against the integer reference (``gauss``: its bound); a feature-window case under both
    variants of the dispatch, with the same bits."""
    for fam in fams:
        x, w, b = C.make(c, fam)
        got = {}
        for v in variants(c):
            lib.ms_conv_set_variant(v)
            try:
                got[v] = run(lib, c, x, w, b, what=(c.entry, c.tag, fam, "variant", v))
            finally:
                lib.ms_conv_set_variant(0)
            C.check(c, fam, got[v], (c.entry, c.tag, fam, "variant", v))
        if len(got) == 2:
            assert same_bits(got[0], got[1]), (c.tag, fam, "the two variants differ")


def check_routes(lib, c):
    """The library's own queries agree with the routes restated in conv_exact_cases.py."""
    if c.entry == "cl":
        assert lib.ms_maskconv_cl_supported(c.N, c.Cin, c.Fin, c.Cout, c.Fout, c.Tout, c.KT, c.ST, c.DT) == \
            int(C.cl_route(c) is not None), (c.tag, C.cl_route(c))
    if c.entry == "fwin":
        want = int(C.fwin_route(c) == "shared" and c.Cout % 16 == 0)
        assert lib.ms_maskconv_fwin_planes_supported(c.N, c.Tin, c.Cout, c.Fout, c.Tout, c.KF, c.KT, c.SF, c.ST, c.DT) == want, \
            (c.tag, C.fwin_route(c))
        lib.ms_conv_set_variant(1)
        try:
            assert lib.ms_maskconv_fwin_planes_supported(c.N, c.Tin, c.Cout, c.Fout, c.Tout, c.KF, c.KT, c.SF, c.ST, c.DT) == 0
        finally:
            lib.ms_conv_set_variant(0)


def check_padding_isolation(lib, c):
    """Part (a): +Inf, then NaN, in every frame t >= lens[n] of every utterance: every output keeps the clean run's bits."""
    x, w, b = C.make(c, "dense")
    L = C.eff_lens(c)
    assert any(v < c.Tin for v in L), (c.tag, "no padding to poison")
    for v in variants(c):
        lib.ms_conv_set_variant(v)
        try:
            packed = Packed(lib, c, w)
            clean = run(lib, c, x, w, b, packed)
            C.check(c, "dense", clean, (c.tag, "clean"))
            for poison in C.POISONS:
                xb = x.copy()
                for n in range(c.N):
                    xb[n, :, :, L[n]:] = poison
                got = run(lib, c, xb, w, b, packed)
                bad = bits(got) != bits(clean)
                assert not bad.any(), (c.entry, c.tag, "variant", v, "padding of", poison, "changed outputs",
                                       int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[bad][:6].tolist())
        finally:
            lib.ms_conv_set_variant(0)


def check_position_isolation(lib, c, seen=None):
    """Part (b): one non-finite input position at a time.  Outputs that ``reads`` does not mark keep the clean run's bits;
    on the float32 tap kernel the marked ones are non-finite.  ``seen`` collects, for the split kernels, what the marked
    outputs came out as."""
    x, w, b = C.make(c, "dense")
    assert c.act is None and np.all(w != 0)
    failures = []
    for v in variants(c):
        lib.ms_conv_set_variant(v)
        try:
            packed = Packed(lib, c, w)
            clean = run(lib, c, x, w, b, packed)
            C.check(c, "dense", clean, (c.tag, "clean"))
            for label, n, ch, f, t in C.isolation_positions(c):
                marked = C.reads(c, n, ch, f, t)
                for poison in C.POISONS:
                    xb = x.copy()
                    xb[n, ch, f, t] = poison
                    got = run(lib, c, xb, w, b, packed)
                    leak = ~marked & (bits(got) != bits(clean))
                    if leak.any():
                        failures.append((label, (n, ch, f, t), poison, "variant", v, int(leak.sum()), "outputs that do not read it "
                                         "changed, first", np.argwhere(leak)[:3].tolist(), got[leak][:3].tolist()))
                    if c.entry == "tap" and marked.any() and np.isfinite(got[marked]).any():
                        failures.append((label, (n, ch, f, t), poison, "an output that reads it is finite"))
                    if seen is not None and marked.any():
                        m = got[marked]
                        kind = "nan" if np.isnan(m).all() else "inf" if np.isinf(m).all() else \
                            "finite" if np.isfinite(m).all() else "mixed"
                        seen.setdefault((c.entry, str(poison)), set()).add(kind)
        finally:
            lib.ms_conv_set_variant(0)
    assert not failures, (c.entry, c.tag, len(failures), "failures", failures[:8])


def check_clamped_position_isolation(lib, c):
    """Part (b) under the clamp (lo, hi) of a case of ``clamped_isolation_cases``, as torch.clamp defines it.  Per poisoned
    position the same inputs run without the activation and with it: an output that reads the position is what np.clip makes
    of the unclamped run's value there (NaN -> NaN, +Inf -> hi, -Inf -> lo; with a NaN poison all of them are NaN), every
    other output keeps the clamped clean run's bits."""
    x, w, b = C.make(c, "dense")
    assert c.act is not None and np.all(w != 0)
    lo, hi = np.float32(c.act[0]), np.float32(c.act[1])
    raw_case = c._replace(act=None)
    failures, lost = [], []
    for v in variants(c):
        lib.ms_conv_set_variant(v)
        try:
            packed = Packed(lib, c, w)
            clean = run(lib, c, x, w, b, packed)
            C.check(c, "dense", clean, (c.tag, "clean"))
            for label, n, ch, f, t in C.isolation_positions(c):
                marked = C.reads(c, n, ch, f, t)
                for poison in C.POISONS + (-np.inf,):
                    xb = x.copy()
                    xb[n, ch, f, t] = poison
                    raw = run(lib, raw_case, xb, w, b, packed)
                    got = run(lib, c, xb, w, b, packed)
                    where = (label, (n, ch, f, t), poison, "variant", v)
                    leak = ~marked & (bits(got) != bits(clean))
                    if leak.any():
                        failures.append(where + (int(leak.sum()), "outputs that do not read it changed, first",
                                                 np.argwhere(leak)[:3].tolist(), got[leak][:3].tolist()))
                    want = np.clip(raw[marked], lo, hi)
                    if np.isnan(poison) and not np.isnan(got[marked]).all():
                        m = got[marked]
                        lost.append(where + (int((~np.isnan(m)).sum()), "of", int(m.size), "outputs that read the NaN are numbers, "
                                             "unclamped", raw[marked][~np.isnan(m)][:3].tolist(), "clamped", m[~np.isnan(m)][:3].tolist()))
                    same = (np.isnan(got[marked]) & np.isnan(want)) | (bits(got[marked]) == bits(want))
                    if not same.all():
                        failures.append(where + (int((~same).sum()), "clamped outputs differ from np.clip of the unclamped ones, "
                                                 "first", got[marked][~same][:3].tolist(), want[~same][:3].tolist()))
        finally:
            lib.ms_conv_set_variant(0)
    assert not failures, (c.entry, c.tag, len(failures), "failures", failures[:8])
    assert not lost, (c.entry, c.tag, len(lost), "positions whose NaN did not reach the outputs that read it", lost[:4])


def run_pair(lib, c1, c2, x, w1, b1, w2, b2):
    """(y2 by the hand-over, y1 and y2 by the two plain calls)."""
    P, S = _lib.ptr, _lib.stream_ptr()
    p1, p2 = Packed(lib, c1, w1), Packed(lib, c2, w2)
    y1 = run(lib, c1, x, w1, b1, p1)
    y2 = run(lib, c2, y1, w2, b2, p2)
    nplanes = lib.ms_maskconv_cl_workspace_bytes(c1.N, c1.Cout, c1.Fout, c1.Tout)
    nws = workspace_bytes(lib, c1)
    planes, ws = scratch(nplanes), scratch(nws)
    xd, l1, l2 = dev(x), lens_dev(c1.lens), lens_dev(c2.lens)
    b1d, b2d = (dev(b1) if c1.bias else None), (dev(b2) if c2.bias else None)
    a, lo, hi = act_args(c1.act)
    ok(lib.ms_maskconv_fwin_planes_forward(P(xd), P(l1), P(p1.buf), P(b1d), P(planes), nplanes, c1.N, c1.Fin, c1.Tin, c1.Cout,
                                           c1.Fout, c1.Tout, c1.KF, c1.KT, c1.SF, c1.ST, c1.DT, c1.pad_f, c1.pad_t, a, lo, hi,
                                           P(ws), nws, S), (c1.tag, "planes out"))
    shape = (c2.N, c2.Cout, c2.Fout, c2.Tout)
    yb = y_buffer(int(np.prod(shape)))
    a, lo, hi = act_args(c2.act)
    ok(lib.ms_maskconv_cl_planes_forward(P(l2), P(p2.buf), P(b2d), P(yb), c2.N, c2.Cin, c2.Fin, c2.Tin, c2.Cout, c2.Fout,
                                         c2.Tout, c2.KF, c2.KT, c2.SF, c2.ST, c2.DF, c2.DT, c2.pad_f, c2.pad_t, a, lo, hi,
                                         P(planes), nplanes, S), (c2.tag, "planes in"))
    got = take(yb, shape, (c2.tag, "planes in"))
    scratch_intact(planes, nplanes, c1.tag)
    scratch_intact(ws, nws, c1.tag)
    return got, y1, y2


def check_pair(lib, c1, c2, fams):
    assert lib.ms_maskconv_fwin_planes_supported(c1.N, c1.Tin, c1.Cout, c1.Fout, c1.Tout, c1.KF, c1.KT, c1.SF, c1.ST, c1.DT) == 1
    assert lib.ms_maskconv_cl_supported(c2.N, c2.Cin, c2.Fin, c2.Cout, c2.Fout, c2.Tout, c2.KT, c2.ST, c2.DT) == 1
    for fam in fams:
        x, w1, b1, w2, b2 = C.make_pair(c1, c2, fam)
        got, y1, y2 = run_pair(lib, c1, c2, x, w1, b1, w2, b2)
        want1, want2 = C.want_pair(c1, c2, fam)
        for name, g, wnt in (("conv1", y1, want1), ("conv2 after conv1", y2, want2), ("hand-over", got, want2)):
            bad = ~(g.astype(np.float64) == wnt)
            assert not bad.any(), (c1.tag, fam, name, int(bad.sum()), "wrong; first at", np.argwhere(bad)[:4].tolist(),
                                   g[bad][:4].tolist(), wnt[bad][:4].tolist())
        assert same_bits(got, y2), (c1.tag, fam, "the hand-over differs from the two plain calls")


def pair_families(i):
    """The one-plane fp16 mode runs ``dense`` only, and not the pair whose conv1 outputs (up to 4095) need a lo plane."""
    if not one_plane():
        return C.PAIR_FAMILIES
    return ("dense",) if i == 0 else ()


def split_exact(lib):
    for entry in SPLIT_ENTRIES:
        for c in C.cases(entry):
            check_routes(lib, c)
            check_exact(lib, c, C.families(c, one_plane()))
    for i, (c1, c2) in enumerate(C.handover_pairs()):
        if pair_families(i):
            check_pair(lib, c1, c2, pair_families(i))


def split_isolation(lib, seen=None):
    for entry in SPLIT_ENTRIES:
        for c in C.isolation_cases(entry):
            check_padding_isolation(lib, c)
            check_position_isolation(lib, c, seen)


def split_clamped(lib):
    """Every case is run; the cases that failed are reported together."""
    failed = []
    for entry in SPLIT_ENTRIES:
        for c in C.clamped_isolation_cases(entry):
            try:
                check_clamped_position_isolation(lib, c)
            except AssertionError as e:
                failed.append(c.tag)
                print("clamped isolation failed:", c.tag, str(e)[:400])
    assert not failed, ("clamped isolation failed on", failed)


if __name__ == "__main__":
    the_lib = _lib.load()
    observed = {}
    for job in sys.argv[1:]:
        {"exact": split_exact, "isolation": lambda l: split_isolation(l, observed), "clamped": split_clamped}[job](the_lib)
    for key in sorted(observed):
        print("marked outputs", key, sorted(observed[key]))
    print("ok")
