"""tests/lookahead_cases.py proved without a GPU: its float64 reference IS the lookahead's definition (right-pad context - 1
frames, then a depthwise ``conv1d``), the exact family is exact in any order, a float32 chain stays inside the gaussian
bound, and the case lists reach the edges they are there for."""
import numpy as np
import pytest
import torch

import lookahead_cases as C


def definition(x, w, dtype=torch.float64):
    """The lookahead layer as the reference project defines it, restated: pad ``context - 1`` zero frames on the right of
    [N, F, T], then ``conv1d`` with one filter per feature (``groups = F``, weight [F, 1, context], no bias)."""
    xt, wt = torch.as_tensor(x, dtype=dtype), torch.as_tensor(w, dtype=dtype)
    ctx = wt.shape[1]
    padded = torch.nn.functional.pad(xt, (0, ctx - 1))
    return torch.nn.functional.conv1d(padded, wt[:, None, :], groups=wt.shape[0]).numpy()


@pytest.mark.parametrize("N,F,T,ctx", [(1, 1, 1, 1), (2, 3, 9, 4), (1, 5, 33, 20), (2, 4, 7, 17), (1, 2, 100, 80), (2, 1, 5, 80)])
def test_reference_is_the_definition(N, F, T, ctx):
    for fam in C.FAMILIES:
        x, w = C.make(fam, N, F, T, ctx)
        want = definition(x, w)
        got = C.reference(x, w)
        assert got.shape == (N, F, T)
        if fam == "exact":
            assert np.array_equal(got, want)
        else:
            # two float64 summations of the same ctx terms in two orders: the gaussian bound with float64's unit roundoff
            assert np.all(np.abs(got - want) <= 2 * C.gauss_bound(x, w) * (2.0 ** -53 / C.U))
        for T_out in {1, (T + 1) // 2, T}:
            assert np.array_equal(C.reference(x, w, T_out), got[:, :, :T_out])
        lo, hi = (float(np.float32(v)) for v in C.ACTS[1])        # the limits as the float arguments of the C ABI carry them
        assert lo != C.ACTS[1][0] and np.array_equal(C.reference(x, w, act=C.ACTS[1]), np.clip(got, lo, hi))


def all_cases():
    out = [(n, f, t, ctx, t) for n, f, t, ctx in C.tcontig_cases()] + [(n, f, t, ctx, t) for n, f, t, ctx, _ in C.fcontig_cases()]
    return out + [(2, 3, t_in, ctx, t_out) for t_in, t_out, ctx in C.window_cases()]


def test_exact_family_is_exact_in_any_order():
    for N, F, T, ctx, T_out in all_cases():
        x, w = C.make("exact", N, F, min(T, 300), ctx)
        assert np.array_equal(x, np.rint(x)) and np.array_equal(w, np.rint(w))
        assert np.abs(x).max() <= 1023 and np.abs(w).max() <= 7 and ctx * 1023 * 7 < 2 ** 24
        assert np.array_equal(definition(x, w, torch.float32), C.reference(x, w))       # float32 == float64


def test_float32_chain_stays_inside_the_gaussian_bound():
    worst = 0.0
    for N, F, T, ctx, T_out in all_cases():
        F = min(F, 8)
        x, w = C.make("gauss", N, F, T, ctx)
        assert np.all(w != 0)
        xp = np.zeros((N, F, T + ctx - 1), dtype=np.float32)
        xp[:, :, :T] = x
        acc = np.zeros((N, F, T_out), dtype=np.float32)
        for k in range(ctx):
            acc = acc + w[None, :, k, None] * xp[:, :, k:k + T_out]
        for act in C.ACTS:
            C.check("gauss", C.clip(acc, act), x, w, T_out, act, (N, F, T, ctx, T_out))
        bound = C.gauss_bound(x, w, T_out)
        worst = max(worst, float((np.abs(acc - C.reference(x, w, T_out)) / bound).max()))
    print("float32 chain: worst error / bound", worst)


def test_check_fails_on_a_wrong_element_and_on_a_shifted_tap():
    for fam in C.FAMILIES:
        x, w = C.make(fam, 2, 3, 40, 17)
        good = C.reference(x, w).astype(np.float32)
        C.check(fam, good, x, w, 40, None, fam)
        bad = good.copy()
        bad[1, 2, 30] += 1.0
        with pytest.raises(AssertionError):
            C.check(fam, bad, x, w, 40, None, fam)
        with pytest.raises(AssertionError):                       # one tap too many
            C.check(fam, C.reference(x, np.concatenate([w, w[:, :1]], axis=1)).astype(np.float32), x, w, 40, None, fam)
        with pytest.raises(AssertionError):                       # the taps one frame late
            C.check(fam, np.roll(good, 1, axis=2), x, w, 40, None, fam)


def test_case_lists_reach_the_edges():
    tc = C.tcontig_cases()
    assert len(tc) == 24 and {c[2] for c in tc} == {1, 255, 256, 257, 300, 513} and {c[3] for c in tc} == {1, 2, 17, 80}
    assert {c[0] for c in tc} == {1, 2} and {c[1] for c in tc} == {1, 3}
    assert (300, 80) in {(c[2], c[3]) for c in tc}                                 # the halo across the 256-frame block
    for ctx in (1, 2, 17, 80):
        assert {(c[0], c[1]) for c in tc if c[3] == ctx} == {(1, 1), (2, 3), (1, 3), (2, 1)}
    fc = C.fcontig_cases()
    assert len(fc) == 42 and {c[1] for c in fc} == {1, 255, 256, 257, 300} and {c[2] for c in fc} == {1, 16, 17, 32, 33, 70}
    assert {c[3] for c in fc} == {1, 15, 16, 17, 32, 33, 80} and all(c[0] == 2 for c in fc)
    assert any(c[4] for c in fc) and not all(c[4] for c in fc)
    assert any(c[4] and c[1] > 256 for c in fc) and any(c[1] > 256 and c[3] % 16 for c in fc)
    wc = C.window_cases()
    assert {c[1] for c in wc} >= {1, 16, 17} and any(c[0] == c[1] for c in wc)
    assert any(0 < c[0] - c[1] < c[2] - 1 for c in wc) and any(c[0] - c[1] > c[2] - 1 for c in wc)
    assert all(1 <= c[1] <= c[0] for c in wc)
