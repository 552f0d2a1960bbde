"""Every convolution entry point of include/ms_hotpath.h through the C ABI (tests/conv_exact_run.py) on the cases of
tests/conv_exact_cases.py (tests/test_conv_exact_cpu.py proves those): integer inputs against the integer reference with
``array_equal``, the gaussian family of the float32 tap kernel against its derived bound, non-finite values in the padding
and at single positions against the bits of the clean run, and the argument checks.  Every assertion is an exact equality,
that one bound, or a finiteness statement on the float32 kernel.  Needs a real MI355X: -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_exact_cases as C
import conv_exact_run as R
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

INVALID, WORKSPACE, UNSUPPORTED = 1, 3, 5
RUNNER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_exact_run.py")


def ident(c):
    return c.tag


# ----------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("c", C.cases("tap"), ids=ident)
def test_tap_kernel_gives_the_integers_and_keeps_the_gaussian_bound(lib, c):
    R.check_exact(lib, c, C.EXACT_FAMILIES + ("gauss",))


@pytest.mark.parametrize("c", C.cases("cl"), ids=ident)
def test_channels_last_kernels_give_the_integers(lib, c):
    R.check_routes(lib, c)
    R.check_exact(lib, c, C.EXACT_FAMILIES)


@pytest.mark.parametrize("c", C.cases("fwin"), ids=ident)
def test_feature_window_kernels_give_the_integers_under_both_variants(lib, c):
    R.check_routes(lib, c)
    R.check_exact(lib, c, C.EXACT_FAMILIES)


@pytest.mark.parametrize("c", C.cases("gemm1d"), ids=ident)
def test_im2col_gemm_gives_the_integers(lib, c):
    R.check_exact(lib, c, C.EXACT_FAMILIES)


@pytest.mark.parametrize("i", range(len(C.handover_pairs())), ids=lambda i: C.handover_pairs()[i][0].tag)
def test_handover_gives_the_bits_of_the_two_calls_and_the_integers(lib, i):
    R.check_pair(lib, *C.handover_pairs()[i], C.PAIR_FAMILIES)


# ----------------------------------------------------------------------------- isolation
ISO = [c for e in ("tap",) + R.SPLIT_ENTRIES for c in C.isolation_cases(e)]


@pytest.mark.parametrize("c", ISO, ids=ident)
def test_non_finite_padding_changes_no_output(lib, c):
    R.check_padding_isolation(lib, c)


@pytest.mark.parametrize("c", ISO, ids=ident)
def test_a_non_finite_input_reaches_only_the_outputs_that_read_it(lib, c):
    R.check_position_isolation(lib, c)


ISO_CLAMPED = [c for e in ("tap",) + R.SPLIT_ENTRIES for c in C.clamped_isolation_cases(e)]


@pytest.mark.parametrize("c", ISO_CLAMPED, ids=ident)
def test_a_non_finite_input_survives_the_clamp_of_the_epilogue(lib, c):
    """One NaN, +Inf or -Inf at an input position, under the clamp: the outputs that read a NaN are NaN; the outputs that read
    an Inf are np.clip of the unclamped run's values; every other output keeps the clamped clean run's bits.  On every route:
    the float32 tap kernel, the channels-last kernels, the im2col GEMM and the feature-window kernels, whose windows are
    padded with rows that belong to other outputs (cleared where they are read, csrc/conv_cl.hip granule_mask)."""
    R.check_clamped_position_isolation(lib, c)


def test_non_finite_padding_changes_no_output_of_the_handover(lib):
    c1, c2 = C.handover_pairs()[1]
    x, w1, b1, w2, b2 = C.make_pair(c1, c2, "dense")
    clean = R.run_pair(lib, c1, c2, x, w1, b1, w2, b2)[0]
    for poison in C.POISONS:
        xb = x.copy()
        for n, ln in enumerate(C.eff_lens(c1)):
            xb[n, :, :, ln:] = poison
        assert R.same_bits(R.run_pair(lib, c1, c2, xb, w1, b1, w2, b2)[0], clean), poison


# ----------------------------------------------------------------------------- the other precision modes
def child(precision, jobs):
    env = dict(os.environ, MS_PRECISION=precision)
    r = subprocess.run([sys.executable, RUNNER] + jobs, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (precision, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_split_kernels_exact_and_isolated_with_bf16_planes():
    child("bf16x3", ["exact", "isolation"])


def test_split_kernels_keep_a_non_finite_input_through_the_clamp_with_bf16_planes():
    """The same in a process with bf16 planes; the child runs every case and reports those that failed."""
    child("bf16x3", ["clamped"])


def test_split_kernels_exact_with_one_fp16_plane():
    child("fp16", ["exact"])


# ----------------------------------------------------------------------------- the ABI
def refused(lib, c, want_rc, x=True, packed=True, y=True, ws=True, lens=True, short=0, act_code=None, **change):
    """One forward call of case ``c`` with an argument taken away or changed: the status, and y untouched."""
    xh, w, b = C.make(c, "dense")
    pk = R.Packed(lib, c, w)
    c2 = c._replace(**change)
    yb = R.y_buffer(c.N * c.Cout * c.Fout * c.Tout)
    nws = R.workspace_bytes(lib, c)
    wsb = R.scratch(nws) if c.entry != "tap" else None

    class Gone:
        buf = None
    rc = R.call(lib, c2, R.dev(xh) if x else None, R.lens_dev(c.lens) if lens else None, pk if packed else Gone, R.dev(b),
                yb if y else None, wsb if ws else None, max(0, nws - short), act_code)
    torch.cuda.synchronize()
    assert rc == want_rc, (c.entry, dict(x=x, packed=packed, y=y, ws=ws, lens=lens, short=short, **change), rc,
                           lib.ms_last_error().decode())
    R.untouched(yb, (c.entry, change))


ABI_CASES = {e: C.cases(e)[1] for e in ("tap", "cl", "fwin", "gemm1d")}


@pytest.mark.parametrize("entry", list(ABI_CASES))
def test_bad_arguments_are_refused_and_nothing_is_written(lib, entry):
    c = ABI_CASES[entry]
    for gone in ("x", "packed", "y") + (("ws",) if entry != "tap" else ()) + (("lens",) if entry == "gemm1d" else ()):
        refused(lib, c, INVALID, **{gone: False})
    for field in ("N", "Tin", "Cout", "Tout", "KT", "ST", "DT") + (("Cin",) if entry != "fwin" else ("Fin",)):
        for v in (0, -1):
            refused(lib, c, INVALID, **{field: v})
    refused(lib, c, INVALID, pad_t=-1)
    refused(lib, c, INVALID, act_code=2)
    refused(lib, c, INVALID, act_code=-1)
    if entry == "cl":
        refused(lib, c, INVALID, Cin=c.Cin + 8)
    if entry == "fwin":
        refused(lib, c, INVALID, SF=3)
        refused(lib, c, INVALID, SF=1)
    if entry != "tap":
        refused(lib, c, WORKSPACE, short=1)


def test_short_planes_buffers_are_refused(lib):
    c1, c2 = C.handover_pairs()[1]
    x, w1, b1, w2, b2 = C.make_pair(c1, c2, "dense")
    P, S = _lib.ptr, _lib.stream_ptr()
    p1, p2 = R.Packed(lib, c1, w1), R.Packed(lib, c2, w2)
    nplanes = lib.ms_maskconv_cl_workspace_bytes(c1.N, c1.Cout, c1.Fout, c1.Tout)
    nws = R.workspace_bytes(lib, c1)
    planes, ws = R.scratch(nplanes), R.scratch(nws)
    xd, l1, l2, b1d, b2d = R.dev(x), R.lens_dev(c1.lens), R.lens_dev(c2.lens), R.dev(b1), R.dev(b2)
    a, lo, hi = R.act_args(c1.act)

    def producer(planes_bytes, ws_bytes, cout=c1.Cout):
        return lib.ms_maskconv_fwin_planes_forward(P(xd), P(l1), P(p1.buf), P(b1d), P(planes), planes_bytes, c1.N, c1.Fin, c1.Tin,
                                                   cout, c1.Fout, c1.Tout, c1.KF, c1.KT, c1.SF, c1.ST, c1.DT, c1.pad_f, c1.pad_t,
                                                   a, lo, hi, P(ws), ws_bytes, S)
    assert producer(nplanes - 1, nws) == WORKSPACE and producer(nplanes, nws - 1) == WORKSPACE
    assert producer(nplanes, nws, cout=c1.Cout + 8) == INVALID
    lib.ms_conv_set_variant(1)
    try:
        assert producer(nplanes, nws) == UNSUPPORTED
    finally:
        lib.ms_conv_set_variant(0)
    torch.cuda.synchronize()
    assert bool((planes == 0xFF).all()) and bool((ws == 0xFF).all()), "a refused producer wrote"
    yb = R.y_buffer(c2.N * c2.Cout * c2.Fout * c2.Tout)
    a, lo, hi = R.act_args(c2.act)
    rc = lib.ms_maskconv_cl_planes_forward(P(l2), P(p2.buf), P(b2d), P(yb), c2.N, c2.Cin, c2.Fin, c2.Tin, c2.Cout, c2.Fout, c2.Tout,
                                           c2.KF, c2.KT, c2.SF, c2.ST, c2.DF, c2.DT, c2.pad_f, c2.pad_t, a, lo, hi, P(planes),
                                           nplanes - 1, S)
    assert rc == WORKSPACE
    R.untouched(yb, "consumer")


def test_a_96_channel_consumer_at_11_taps_is_unsupported_and_writes_nothing(lib):
    c = C.mk("cl", "cin96_kt11", 2, 96, 20, 32, 21, 11, Tin=65, SF=2)
    assert C.cl_route(c) is None
    assert lib.ms_maskconv_cl_supported(c.N, c.Cin, c.Fin, c.Cout, c.Fout, c.Tout, c.KT, c.ST, c.DT) == 0
    assert lib.ms_maskconv_cl_supported(c.N, 32, c.Fin, c.Cout, c.Fout, c.Tout, c.KT, c.ST, c.DT) == 1
    refused(lib, c, UNSUPPORTED)


def test_size_and_support_queries_answer_0_on_bad_shapes(lib):
    for bad in (0, -1):
        assert lib.ms_maskconv_packed_bytes(bad, 3, 3, 3, 1) == 0 and lib.ms_maskconv_packed_bytes(4, 3, 3, bad, 1) == 0
        assert lib.ms_maskconv_packed_bytes(4, 3, 3, 3, bad) == 0
        assert lib.ms_maskconv_cl_packed_bytes(bad, 16, 3, 3) == 0 and lib.ms_maskconv_cl_packed_bytes(16, 16, bad, 3) == 0
        assert lib.ms_maskconv_cl_workspace_bytes(bad, 16, 3, 3) == 0 and lib.ms_maskconv_cl_workspace_bytes(1, 16, 3, bad) == 0
        assert lib.ms_maskconv_fwin_packed_bytes(bad, 41, 11) == 0 and lib.ms_maskconv_fwin_packed_bytes(32, 41, bad) == 0
        assert lib.ms_maskconv_fwin_workspace_bytes(bad, 100, 41, 2, 40) == 0
        assert lib.ms_maskconv_fwin_workspace_bytes(2, 100, 41, bad, 40) == 0
        assert lib.ms_maskconv1d_gemm_packed_bytes(bad, 16, 3) == 0 and lib.ms_maskconv1d_gemm_packed_bytes(16, 16, bad) == 0
        assert lib.ms_maskconv1d_gemm_workspace_bytes(bad, 16, 10, 16, 3) == 0
        assert lib.ms_maskconv_cl_supported(bad, 32, 20, 32, 10, 65, 11, 1, 1) == 0
        assert lib.ms_maskconv_fwin_planes_supported(bad, 130, 32, 40, 65, 41, 11, 2, 2, 1) == 0
    assert lib.ms_maskconv_packed_bytes(5, 3, 3, 3, 2) == 0                          # groups must divide Cout
    assert lib.ms_maskconv_cl_packed_bytes(16, 24, 3, 3) == 0                        # Cin % 16
    assert lib.ms_maskconv_cl_supported(2, 24, 20, 32, 10, 65, 11, 1, 1) == 0
    assert lib.ms_maskconv_fwin_planes_supported(2, 130, 32, 40, 65, 41, 11, 3, 2, 1) == 0      # odd SF
    assert lib.ms_maskconv_fwin_planes_supported(2, 130, 40, 40, 65, 41, 11, 2, 2, 1) == 0      # Cout % 16
    # the boundary of the shared-window kernel: more than 48 output frames
    assert lib.ms_maskconv_fwin_planes_supported(2, 96, 32, 40, 48, 41, 11, 2, 2, 1) == 0
    assert lib.ms_maskconv_fwin_planes_supported(2, 98, 32, 40, 49, 41, 11, 2, 2, 1) == 1
    # the exact sizes of the tap kernel's bank: [group][cout tile][Cin_g KF][KT rounded up to even][32] floats
    assert lib.ms_maskconv_packed_bytes(66, 2, 2, 3, 2) == 2 * 2 * 4 * 4 * 32 * 4
    assert lib.ms_maskconv_packed_bytes(32, 1, 1, 2, 1) == 1 * 1 * 1 * 2 * 32 * 4
