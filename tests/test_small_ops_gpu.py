"""The small operators through the C ABI on the cases of tests/small_ops_cases.py (tests/test_small_ops_cpu.py proves those):
ms_clamp, ms_mask_time_, ms_nct_to_tnc, ms_log_softmax_axis and its backward, ms_ctc_greedy_decode, ms_embedding_forward,
ms_rnnt_joint_forward, ms_rnnt_topk.  Every output (and every buffer an operator edits in place) lies between sentinel
guards that must survive; an output element that still holds the sentinel was never written.  The criteria are equality of
bits and the three derived bounds of the cases file.  Needs a real MI355X: -m gpu."""
import numpy as np
import pytest
import torch

import small_ops_cases as C
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7.25e33
ISENTINEL = -77777777
INVALID = 1


class Guarded:
    """``count`` elements between two guards, all filled with the sentinel, or holding ``init`` (an in-place operand)."""

    def __init__(self, count, dtype=torch.float32, init=None):
        self.count = int(count)
        self.sentinel = SENTINEL if dtype == torch.float32 else ISENTINEL
        self.buf = torch.full((self.count + 2 * GUARD,), self.sentinel, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + self.count]
        if init is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)))

    def take(self, shape, what, written=True):
        """The finished values: guards intact, and (``written``) no element left at the sentinel."""
        host = self.buf.cpu().numpy()
        s = host.dtype.type(self.sentinel)
        assert np.all(host[:GUARD] == s) and np.all(host[GUARD + self.count:] == s), (what, "wrote outside its buffer")
        got = host[GUARD:GUARD + self.count]
        if written:
            assert not np.any(got == s), (what, "elements never written", int(np.sum(got == s)))
        return got.reshape(shape).copy()

    def untouched(self, what):
        assert bool((self.buf == self.sentinel).all()), (what, "a call that should write nothing wrote")


def dev(a):
    """A device copy; the caller keeps it in a name until its call has been issued (a temporary's block goes back to the
    allocator at once and the next upload may land in it)."""
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ok(rc, what):
    _lib.check(rc, str(what))


def S():
    return _lib.stream_ptr()


# ----------------------------------------------------------------------------- ms_clamp
@pytest.mark.parametrize("lo,hi", C.CLAMP_LIMITS)
def test_clamp_matches_np_clip_bit_for_bit_and_keeps_nan(lib, lo, hi):
    """Out of place and in place (y == x) on every n; finite and infinite inputs come out with np.clip's bits, NaN stays NaN.
    n = 1 runs every special value on its own."""
    singles = [np.array([v], dtype=np.float32) for v in C.clamp_specials(lo, hi)]
    for x in singles + [C.clamp_input(n, lo, hi) for n in C.CLAMP_N[1:]]:
        n = x.size
        want = C.clamp_ref(x, lo, hi)
        xd = dev(x)
        y = Guarded(n)
        ok(lib.ms_clamp(_lib.ptr(xd), _lib.ptr(y.view), n, lo, hi, S()), ("clamp", n))
        got = y.take((n,), ("clamp", n, lo, hi))
        assert C.same_bits_or_both_nan(xd.cpu().numpy(), x).all(), "the input changed"
        nan = np.isnan(x)
        assert np.isnan(got[nan]).all(), ("clamp", n, lo, hi, "a NaN came out as", got[nan][:4].tolist())
        bad = ~nan & (C.bits(got) != C.bits(want))
        first = f"x {x[bad][:6].tolist()} gave {got[bad][:6].tolist()}, np.clip gives {want[bad][:6].tolist()}"
        assert not bad.any(), f"clamp n={n} ({lo}, {hi}): {int(bad.sum())} differ from np.clip; {first}"
        z = Guarded(n, init=x)
        ok(lib.ms_clamp(_lib.ptr(z.view), _lib.ptr(z.view), n, lo, hi, S()), ("clamp in place", n))
        same = C.same_bits_or_both_nan(z.take((n,), ("clamp in place", n), written=False), got)
        assert same.all(), ("clamp", n, lo, hi, "in place differs from out of place")


def test_clamp_of_nothing_is_ok_and_writes_nothing(lib):
    ok(lib.ms_clamp(None, None, 0, 0.0, 1.0, S()), "clamp n = 0, null pointers")
    y = Guarded(8)
    ok(lib.ms_clamp(_lib.ptr(y.view), _lib.ptr(y.view), 0, 0.0, 1.0, S()), "clamp n = 0")
    torch.cuda.synchronize()
    y.untouched("clamp n = 0")
    assert lib.ms_clamp(None, _lib.ptr(y.view), 4, 0.0, 1.0, S()) == INVALID
    y.untouched("clamp of a null input")


# ----------------------------------------------------------------------------- ms_mask_time_
@pytest.mark.parametrize("inner", C.MASK_INNER)
def test_mask_time_zeroes_the_tail_and_nothing_else(lib, inner):
    """lens 0, 1, T - 1, T, T + 5, -3 in one batch: the tail holds +0.0 bits also where the input held NaN or Inf, every other
    element keeps its bits (NaN payloads included), the guards around x survive."""
    for T in C.MASK_T:
        x, lens = C.mask_input(inner, T)
        want = C.mask_ref(x, lens)
        xb = Guarded(x.size, init=x)
        ld = dev(lens)
        ok(lib.ms_mask_time_(_lib.ptr(xb.view), _lib.ptr(ld), x.shape[0], inner, T, S()), ("mask", inner, T))
        got = xb.take(x.shape, ("mask", inner, T), written=False)
        bad = C.bits(got) != C.bits(want)
        assert not bad.any(), ("mask", inner, T, int(bad.sum()), "wrong; first at", np.argwhere(bad)[:4].tolist(),
                               got[bad][:4].tolist(), want[bad][:4].tolist())


# ----------------------------------------------------------------------------- ms_nct_to_tnc
@pytest.mark.parametrize("N", C.NCT_N)
def test_nct_to_tnc_is_the_transpose(lib, N):
    for CF in C.NCT_SIZES:
        for T in C.NCT_SIZES:
            x = C.nct_input(N, CF, T)
            y = Guarded(x.size)
            xd = dev(x)
            ok(lib.ms_nct_to_tnc(_lib.ptr(xd), _lib.ptr(y.view), N, CF, T, S()), ("nct", N, CF, T))
            got = y.take((T, N, CF), ("nct", N, CF, T))
            assert C.same_bits(got, C.nct_ref(x)), ("nct", N, CF, T, np.argwhere(got != C.nct_ref(x))[:4].tolist())


# ----------------------------------------------------------------------------- ms_log_softmax_axis (+ backward)
@pytest.mark.parametrize("shape", C.LSM_SHAPES)
def test_log_softmax_axis_keeps_its_bound_and_its_infinities(lib, shape):
    """-Inf entries give -Inf, a column of all -Inf, with a +Inf or with a NaN is NaN throughout, the rest obeys the bound."""
    outer, axis, inner = shape
    worst = 0.0
    for scale in C.LSM_SCALES:
        for variant in C.LSM_VARIANTS:
            x = C.lsm_input(shape, scale, variant)
            y = Guarded(x.size)
            xd = dev(x)
            ok(lib.ms_log_softmax_axis(_lib.ptr(xd), _lib.ptr(y.view), outer, axis, inner, S()), (shape, scale, variant))
            got = y.take(shape, (shape, scale, variant))
            worst = max(worst, C.check_toleranced(got, C.lsm_ref(x), C.lsm_bound(x), ("log_softmax", shape, scale, variant)))
    print("log_softmax", shape, "worst error / bound", worst)


@pytest.mark.parametrize("shape", C.LSM_SHAPES)
def test_log_softmax_axis_backward_keeps_its_bound_in_place_too(lib, shape):
    """On a y that contains -Inf (exp(y) = 0: the gradient passes through); the in-place call loss/ctc_loss.py makes
    (gx == g) gives the out-of-place call's bits."""
    outer, axis, inner = shape
    worst = 0.0
    for scale in C.LSM_SCALES:
        y, g = C.lsm_backward_input(shape, scale)
        yd, gd = dev(y), dev(g)
        gx = Guarded(g.size)
        ok(lib.ms_log_softmax_axis_backward(_lib.ptr(yd), _lib.ptr(gd), _lib.ptr(gx.view), outer, axis, inner, S()), (shape, scale))
        got = gx.take(shape, ("log_softmax backward", shape, scale))
        worst = max(worst, C.check_toleranced(got, C.lsm_backward_ref(y, g), C.lsm_backward_bound(y, g),
                                              ("log_softmax backward", shape, scale)))
        passes = np.isneginf(y)
        assert np.array_equal(C.bits(got)[passes], C.bits(g)[passes]), "exp(-Inf) = 0: the gradient passes through unchanged"
        inplace = Guarded(g.size, init=g)
        ok(lib.ms_log_softmax_axis_backward(_lib.ptr(yd), _lib.ptr(inplace.view), _lib.ptr(inplace.view), outer, axis, inner, S()),
           (shape, scale, "in place"))
        assert C.same_bits(inplace.take(shape, (shape, scale, "in place"), written=False), got), (shape, scale, "in place differs")
    print("log_softmax backward", shape, "worst error / bound", worst)


# ----------------------------------------------------------------------------- ms_ctc_greedy_decode
@pytest.mark.parametrize("T", C.GREEDY_T)
@pytest.mark.parametrize("V", C.GREEDY_V)
def test_greedy_decode_gives_the_chosen_paths(lib, V, T):
    """out_len and the first out_len[n] entries of every row, for both blanks and every path; the rest of a row is
    unspecified (the header says so) and is not looked at.  The guards around the [N, T] buffer survive."""
    N = C.GREEDY_N
    for blank in sorted({0, V - 1}):
        for path in C.GREEDY_PATHS:
            case = C.greedy_case(V, T, blank, path)
            if case is None:
                continue
            x, lens, want = case
            what = ("greedy", V, T, blank, path)
            out_idx, out_len = Guarded(N * T, torch.int32), Guarded(N, torch.int32)
            xd, ld = dev(x), dev(lens)
            ok(lib.ms_ctc_greedy_decode(_lib.ptr(xd), _lib.ptr(ld), _lib.ptr(out_idx.view), _lib.ptr(out_len.view), T, N, V,
                                        blank, S()), what)
            got_len = out_len.take((N,), what)
            got_idx = out_idx.take((N, T), what, written=False)
            assert got_len.tolist() == [len(w) for w in want], (what, got_len.tolist(), [len(w) for w in want])
            for n in range(N):
                got = got_idx[n, :got_len[n]].tolist()
                assert got == want[n], (what, n, "first difference at",
                                        next(i for i, (a, b) in enumerate(zip(got, want[n])) if a != b), got[:8], want[n][:8])


# ----------------------------------------------------------------------------- ms_embedding_forward
def test_embedding_copies_rows_and_clamps_indices(lib):
    for D in C.EMB_D:
        for V1 in C.EMB_V1:
            table, idx = C.embedding_input(D, V1)
            R = idx.size
            out = Guarded(R * D)
            td, idxd = dev(table), dev(idx)
            ok(lib.ms_embedding_forward(_lib.ptr(td), _lib.ptr(idxd), _lib.ptr(out.view), R, D, V1, S()), ("emb", D, V1))
            got = out.take((R, D), ("emb", D, V1))
            assert C.same_bits(got, C.embedding_ref(table, idx)), ("emb", D, V1)
            assert C.same_bits(got[2], table[0]) and C.same_bits(got[3], table[V1 - 1]), "out-of-range indices read the end rows"


# ----------------------------------------------------------------------------- ms_rnnt_joint_forward
@pytest.mark.parametrize("J", C.JOINT_J)
def test_joint_keeps_its_bound_and_normalises(lib, J):
    worst = 0.0
    for V1 in C.JOINT_V1:
        enc, row, pred, w, b = C.joint_input(J, V1)
        encd, rowd, predd, wd, bd = dev(enc), dev(row), dev(pred), dev(w), dev(b)
        for bias, biasd in ((b, bd), (None, None)):
            what = ("joint", J, V1, "bias" if bias is not None else "no bias")
            out = Guarded(C.JOINT_R * V1)
            ok(lib.ms_rnnt_joint_forward(_lib.ptr(encd), _lib.ptr(rowd), _lib.ptr(predd), _lib.ptr(wd), _lib.ptr(biasd),
                                         _lib.ptr(out.view), C.JOINT_R, J, V1, S()), what)
            got = out.take((C.JOINT_R, V1), what)
            bound = C.joint_bound(enc, row, pred, w, bias)
            worst = max(worst, C.check_toleranced(got, C.joint_ref(enc, row, pred, w, bias), bound, what))
            lse = C.logsumexp_rows(got)
            assert np.all(np.abs(lse) <= bound.max(axis=1)), (what, "a row does not sum to 1", lse.tolist())
    print("joint J =", J, "worst error / bound", worst)


def test_joint_wider_than_the_lds_is_refused_and_writes_nothing(lib):
    J, V1 = C.JOINT_REFUSED
    out = Guarded(V1)
    z, row = torch.zeros(J, dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib.ms_rnnt_joint_forward(_lib.ptr(z), _lib.ptr(row), _lib.ptr(z), _lib.ptr(z), None, _lib.ptr(out.view), 1, J, V1, S())
    torch.cuda.synchronize()
    assert rc == INVALID, rc
    out.untouched("joint refused")


# ----------------------------------------------------------------------------- ms_rnnt_topk
@pytest.mark.parametrize("Cn", C.TOPK_C)
def test_topk_is_the_stable_descending_order(lib, Cn):
    """Ties everywhere: the lowest index first.  Rows with fewer than k entries above -Inf end in (-1, -Inf); a NaN is never
    selected (the kernel's definition, written into the header)."""
    x = C.topk_input(Cn)
    xd = dev(x)
    for k in C.topk_ks(Cn):
        idx, val = Guarded(C.TOPK_B * k, torch.int32), Guarded(C.TOPK_B * k)
        ok(lib.ms_rnnt_topk(_lib.ptr(xd), _lib.ptr(idx.view), _lib.ptr(val.view), C.TOPK_B, Cn, k, S()), ("topk", Cn, k))
        got_idx, got_val = idx.take((C.TOPK_B, k), ("topk idx", Cn, k)), val.take((C.TOPK_B, k), ("topk val", Cn, k))
        want_idx, want_val = C.topk_ref(x, k)
        assert np.array_equal(got_idx, want_idx), ("topk", Cn, k, np.argwhere(got_idx != want_idx)[:4].tolist(),
                                                   got_idx[got_idx != want_idx][:4].tolist(), want_idx[got_idx != want_idx][:4].tolist())
        assert C.same_bits(got_val, want_val), ("topk values", Cn, k)
