"""The exact-float32 GEMM through the C ABI (``ms_linear_forward``, ``ms_linear_splitk_forward``,
``ms_linear_splitk_workspace_bytes``) at tile, K-slice and alignment edges, against the float64 references and the three
input families of tests/gemm_f32_cases.py (tests/test_gemm_f32_cpu.py proves those).  The only criteria are exact equality
(integer families, bit comparisons between calls) and the derived gaussian bound.  Needs a real MI355X: -m gpu.

Every call writes into a y that has sentinel guard rows before and after it (they must survive) and runs twice (the same
bits).  ``test_linear_train_node`` is the one case that goes through Python: tests/test_rnnt_train_gpu.py reaches
``linear_train`` only inside ``RNNT.loss`` at 1e-3 of a tensor's largest magnitude, which is no equivalent."""
import numpy as np
import pytest
import torch

import gemm_f32_cases as C
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 3                           # guard rows on either side of y
SENTINEL = -7.25e33                 # no result of any family comes near it


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def act_args(act):
    return (_lib.ACT_NONE, 0.0, 0.0) if act is None else (_lib.ACT_CLAMP, act[0], act[1])


class Out:
    """y [M, N] inside a sentinel-filled buffer of GUARD + M + GUARD rows."""

    def __init__(self, M, N):
        self.buf = torch.full((M + 2 * GUARD, N), SENTINEL, dtype=torch.float32, device="cuda")
        self.y = self.buf[GUARD:GUARD + M]

    def untouched(self):
        return bool((self.buf == SENTINEL).all())

    def result(self, what):
        host = self.buf.cpu().numpy()
        assert np.all(host[:GUARD] == np.float32(SENTINEL)) and np.all(host[-GUARD:] == np.float32(SENTINEL)), (what, "guard rows")
        return host[GUARD:-GUARD].copy()


def linear(lib, x, w, b, M, K, N, act, what):
    """ms_linear_forward on device tensors, twice; the result as numpy."""
    a, lo, hi = act_args(act)
    runs = []
    for _ in range(2):
        out = Out(M, N)
        _lib.check(lib.ms_linear_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out.y), M, K, N, a, lo, hi,
                                         _lib.stream_ptr()), "ms_linear_forward")
        runs.append(out.result(what))
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), (what, "two runs differ")
    return runs[0]


def splitk(lib, x, w, b, M, K, N, act, flags, what, workspace=True):
    """ms_linear_splitk_forward with a workspace of exactly the queried size (``workspace=False``: NULL), twice."""
    a, lo, hi = act_args(act)
    need = lib.ms_linear_splitk_workspace_bytes(M, K, N, flags)
    runs = []
    for _ in range(2):
        out = Out(M, N)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda") if workspace else None
        _lib.check(lib.ms_linear_splitk_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out.y), M, K, N, a, lo, hi, flags,
                                                _lib.ptr(ws), need if workspace else 0, _lib.stream_ptr()), "ms_linear_splitk_forward")
        runs.append(out.result(what))
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), (what, "two runs differ")
    return runs[0]


def bits_equal(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ----------------------------------------------------------------------------- ms_linear_forward
@pytest.mark.parametrize("M,K,N", C.plain_shapes())
def test_linear_forward_edges(lib, M, K, N):
    for fam in C.FAMILIES:
        x, w, b = C.make(fam, M, K, N)
        ref = C.Ref(fam, x, w, b)
        xd, wd, bd = dev(x), dev(w), dev(b)
        for act in C.ACTS:
            for bias in (True, False):
                what = (fam, M, K, N, act, bias)
                ref.check(linear(lib, xd, wd, bd if bias else None, M, K, N, act, what), act, bias, what)


def test_all_three_tile_configurations(lib):
    """N = 1000 > 64: the configuration depends on the workgroup count against the compute units.  The dispatch arithmetic
    is restated in gemm_f32_cases.tile_regime; three ragged M must land in three DIFFERENT configurations on this part.
    Every configuration is the same k-ordered chain: a row's bits are the same in all three calls."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ms = C.regime_ms(cus)
    regimes = tuple(C.tile_regime(m, C.REGIME_N, cus) for m in ms)
    print("compute units", cus, "M", ms, "configurations", regimes)
    assert regimes == C.REGIMES and len(set(regimes)) == 3, (cus, ms, regimes)
    K, N = C.REGIME_K, C.REGIME_N
    for fam in C.FAMILIES:
        x, w, b = C.make(fam, max(ms), K, N)
        ref = C.Ref(fam, x, w, b)
        wd, bd = dev(w), dev(b)
        got = {}
        for m in ms:
            xd = dev(x[:m])
            for act in C.ACTS:
                for bias in (True, False):
                    what = (fam, m, K, N, act, bias)
                    got[m, act, bias] = linear(lib, xd, wd, bd if bias else None, m, K, N, act, what)
                    ref.check(got[m, act, bias], act, bias, what)
        for act in C.ACTS:
            for bias in (True, False):
                small, mid, big = (got[m, act, bias] for m in ms)
                assert bits_equal(small, mid[:ms[0]]) and bits_equal(small, big[:ms[0]]), (fam, act, bias, "128x32 rows")
                assert bits_equal(mid, big[:ms[1]]), (fam, act, bias, "128x64 rows")


@pytest.mark.parametrize("M,K,N", [(33, 36, 65), (129, 128, 31), (130, 64, 200)])
def test_misaligned_pointers_take_the_scalar_loads_and_give_the_same_bits(lib, M, K, N):
    """K % 4 == 0 but x, then w, then both start one float into a buffer: not 16-byte aligned, so the kernel must not use
    its 16-byte loads."""
    assert K % 4 == 0
    for fam in C.FAMILIES:
        x, w, b = C.make(fam, M, K, N)
        ref = C.Ref(fam, x, w, b)
        xd, wd, bd = dev(x), dev(w), dev(b)
        xo = torch.zeros(M * K + 1, dtype=torch.float32, device="cuda")
        wo = torch.zeros(N * K + 1, dtype=torch.float32, device="cuda")
        xo[1:].copy_(xd.reshape(-1))
        wo[1:].copy_(wd.reshape(-1))
        xm, wm = xo[1:].view(M, K), wo[1:].view(N, K)
        assert xd.data_ptr() % 16 == 0 and wd.data_ptr() % 16 == 0 and xm.data_ptr() % 16 == 4 and wm.data_ptr() % 16 == 4
        for act in C.ACTS:
            want = linear(lib, xd, wd, bd, M, K, N, act, (fam, "aligned"))
            ref.check(want, act, True, (fam, M, K, N, act))
            for xa, wa, name in ((xm, wd, "x"), (xd, wm, "w"), (xm, wm, "x and w")):
                got = linear(lib, xa, wa, bd, M, K, N, act, (fam, name))
                assert bits_equal(got, want), (fam, M, K, N, act, name, "misaligned")


# ----------------------------------------------------------------------------- split-K
def test_splitk_workspace_query(lib):
    for flags in (0, C.FEW_ROWS):
        for K in C.QUERY_K:
            for N in C.QUERY_N:
                for M in (1, 127, 300):
                    ks = C.splitk_slices(K, N, flags)
                    want = (ks * M * N * 4 + 255) // 256 * 256
                    assert lib.ms_linear_splitk_workspace_bytes(M, K, N, flags) == want, (M, K, N, flags, ks)
    assert lib.ms_linear_splitk_workspace_bytes(0, 1024, 29, 0) == 0


@pytest.mark.parametrize("K,N,flags", C.splitk_cases())
def test_splitk_forward(lib, K, N, flags):
    big = max(C.SPLITK_M)
    for fam in C.FAMILIES:
        x, w, b = C.make(fam, big, K, N)
        ref = C.Ref(fam, x, w, b)
        xd, wd, bd = dev(x), dev(w), dev(b)
        whole = {}
        for M in sorted(C.SPLITK_M, reverse=True):
            assert lib.ms_linear_splitk_workspace_bytes(M, K, N, flags) == C.splitk_workspace_bytes(M, K, N, flags) > 0
            xm = xd[:M].contiguous()
            for act in C.ACTS:
                for bias in (True, False):
                    what = (fam, M, K, N, flags, act, bias)
                    got = splitk(lib, xm, wd, bd if bias else None, M, K, N, act, flags, what)
                    ref.check(got, act, bias, what)
                    if M == big:
                        whole[act, bias] = got
                    # the slice count never depends on M: a row's bits do not depend on the rows it is batched with
                    assert bits_equal(got, whole[act, bias][:M]), (what, "rows of the M = 300 call")
            if M in (1, 129):
                # no workspace = the plain kernel, bit for bit
                for act in C.ACTS:
                    got = splitk(lib, xm, wd, bd, M, K, N, act, flags, (fam, M, "NULL workspace"), workspace=False)
                    assert bits_equal(got, linear(lib, xm, wd, bd, M, K, N, act, (fam, M, "plain"))), (fam, M, K, N, flags, act)
                    ref.check(got, act, True, (fam, M, K, N, flags, act, "NULL workspace"))


@pytest.mark.parametrize("K,N,flags", [(512, 29, 0), (641, 64, 0), (1000, 200, C.FEW_ROWS)])
def test_splitk_refuses_a_short_workspace_and_an_unknown_flag(lib, K, N, flags):
    M = 129
    x, w, b = C.make("gauss", M, K, N)
    xd, wd, bd = dev(x), dev(w), dev(b)
    need = lib.ms_linear_splitk_workspace_bytes(M, K, N, flags)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for fl, nbytes, why in ((flags, need - 1, "a workspace one byte short"), (flags | 2, need, "an unknown flag"),
                            (flags | 64, need, "an unknown flag")):
        out = Out(M, N)
        rc = lib.ms_linear_splitk_forward(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(out.y), M, K, N, _lib.ACT_NONE, 0.0, 0.0,
                                          fl, _lib.ptr(ws), nbytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc != _lib.MS_OK, why
        assert out.untouched(), (why, "y was written")


# ----------------------------------------------------------------------------- non-finite isolation
@pytest.mark.parametrize("M,K,N,flags", [(130, 100, 129, None), (129, 641, 29, 0)])
def test_a_non_finite_input_stays_in_its_row_or_column(lib, M, K, N, flags):
    """act none.  A NaN at x[m0, k0] makes exactly row m0 non-finite, an Inf at w[n0, k0] exactly column n0; every other
    element keeps the bits of the finite run (flags None: ms_linear_forward, else ms_linear_splitk_forward)."""
    x, w, b = C.make("gauss", M, K, N)
    wd, bd = dev(w), dev(b)

    def run(xa, wa, what):
        if flags is None:
            return linear(lib, dev(xa), dev(wa), bd, M, K, N, None, what)
        return splitk(lib, dev(xa), dev(wa), bd, M, K, N, None, flags, what)

    finite = run(x, w, "finite")
    assert np.isfinite(finite).all()
    C.check("gauss", finite, x, w, b, None, (M, K, N, flags))
    for m0, k0 in ((0, 0), (M - 1, K - 1), (M // 2 + 1, K // 2 + 1)):
        xn = x.copy()
        xn[m0, k0] = np.nan
        got = run(xn, w, ("NaN in x", m0, k0))
        assert not np.isfinite(got[m0]).any(), ("NaN in x", m0, k0, "its row")
        rest = np.arange(M) != m0
        assert bits_equal(got[rest], finite[rest]), ("NaN in x", m0, k0, "other rows")
    for n0, k0 in ((0, K - 1), (N - 1, 0), (N // 2 + 1, K // 2 + 1)):
        wn = w.copy()
        wn[n0, k0] = np.inf
        got = run(x, wn, ("Inf in w", n0, k0))
        assert not np.isfinite(got[:, n0]).any(), ("Inf in w", n0, k0, "its column")
        rest = np.arange(N) != n0
        assert bits_equal(np.ascontiguousarray(got[:, rest]), np.ascontiguousarray(finite[:, rest])), ("Inf in w", n0, k0, "other columns")


@pytest.mark.parametrize("M,K,N,flags", [(130, 100, 129, None), (129, 641, 29, 0)])
def test_a_nan_survives_the_clamp_in_its_row_or_column(lib, M, K, N, flags):
    """The same contract through MS_ACT_CLAMP, which is torch.nn.Hardtanh: a NaN stays a NaN (``fminf(fmaxf(v, lo), hi)``
    would make it ``lo``), in the tile kernel's epilogue and in the K-slice reduction; every other element keeps its bits."""
    x, w, b = C.make("gauss", M, K, N)
    bd, act = dev(b), (-0.5, 0.5)

    def run(xa, wa, what):
        if flags is None:
            return linear(lib, dev(xa), dev(wa), bd, M, K, N, act, what)
        return splitk(lib, dev(xa), dev(wa), bd, M, K, N, act, flags, what)

    finite = run(x, w, "finite")
    assert np.isfinite(finite).all() and (np.abs(finite) < 0.5).any() and (finite == 0.5).any() and (finite == -0.5).any()
    for m0, k0 in ((0, 0), (M - 1, K - 1), (M // 2 + 1, K // 2 + 1)):
        xn = x.copy()
        xn[m0, k0] = np.nan
        got = run(xn, w, ("NaN in x", m0, k0))
        assert np.isnan(got[m0]).all(), ("NaN in x", m0, k0, "its row")
        rest = np.arange(M) != m0
        assert bits_equal(got[rest], finite[rest]), ("NaN in x", m0, k0, "other rows")
    for n0, k0 in ((0, K - 1), (N - 1, 0), (N // 2 + 1, K // 2 + 1)):
        wn = w.copy()
        wn[n0, k0] = np.nan
        got = run(x, wn, ("NaN in w", n0, k0))
        assert np.isnan(got[:, n0]).all(), ("NaN in w", n0, k0, "its column")
        rest = np.arange(N) != n0
        assert bits_equal(np.ascontiguousarray(got[:, rest]), np.ascontiguousarray(finite[:, rest])), ("NaN in w", n0, k0, "other columns")


# ----------------------------------------------------------------------------- the training node
def test_linear_train_node(lib):
    """``linear_train`` forward and backward at (M, K, N) = (37, 20, 9) against float64 autograd: y and dx, dW, db are each
    one product of ms_linear_forward, so each is held to the gaussian bound of ITS product (contraction lengths K, N, M, M)."""
    from myrtlespeech_amd.model.rnn_autograd import linear_train
    M, K, N = 37, 20, 9
    x, w, b = C.make("gauss", M, K, N)
    dy = np.random.default_rng(7).standard_normal((M, N)).astype(np.float32)
    lin = torch.nn.Linear(K, N).cuda()
    with torch.no_grad():
        lin.weight.copy_(dev(w))
        lin.bias.copy_(dev(b))
    xd = dev(x).requires_grad_(True)
    y = linear_train(xd, lin)
    y.backward(dev(dy))
    got = dict(y=y.detach(), dx=xd.grad, dw=lin.weight.grad, db=lin.bias.grad)
    got = {k: v.cpu().numpy() for k, v in got.items()}

    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    w64 = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    b64 = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    y64 = x64 @ w64.t() + b64
    y64.backward(torch.tensor(dy, dtype=torch.float64))
    want = dict(y=y64.detach().numpy(), dx=x64.grad.numpy(), dw=w64.grad.numpy(), db=b64.grad.numpy())
    ones = np.ones((1, M), dtype=np.float32)
    # each result as the product a . b^T (+ bias) that the node computes it with
    operands = dict(y=(x, w, b), dx=(dy, np.ascontiguousarray(w.T), None), dw=(np.ascontiguousarray(dy.T), np.ascontiguousarray(x.T), None),
                    db=(ones, np.ascontiguousarray(dy.T), None))
    for key, (a_, b_, bias_) in operands.items():
        err = np.abs(got[key].astype(np.float64) - want[key])
        bound = C.gauss_bound(a_, b_, bias_).reshape(want[key].shape)
        assert got[key].shape == want[key].shape and np.all(err <= bound), (key, float((err / bound).max()))
