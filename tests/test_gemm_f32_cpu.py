"""What tests/gemm_f32_cases.py promises, proved without a GPU for every case of its lists: the caps that make the two exact
families exact in ANY order of float32 accumulation, that a hi + lo three-pass product is wrong on the one-hot family, that
a plain float32 chain stays inside the gaussian bound, and the shape lists and dispatch arithmetic themselves."""
import numpy as np
import pytest

import gemm_f32_cases as C


def all_data_shapes():
    """Every (M, K, N) the GPU test draws data for (the K-slice cases draw their largest M; fewer rows are its leading rows)."""
    shapes = list(C.plain_shapes())
    shapes += [(m, C.REGIME_K, C.REGIME_N) for m in C.regime_ms(256)]
    shapes += [(max(C.SPLITK_M), k, n) for k, n, _ in C.splitk_cases()]
    return shapes


def test_shape_lists_cover_the_edges():
    plain = C.plain_shapes()
    assert len(plain) == len(set(plain)) and len(plain) <= 62
    for vals, axis in ((C.EDGE_M, 0), (C.EDGE_K, 1), (C.EDGE_N, 2)):
        assert set(vals) <= {s[axis] for s in plain}, axis
    assert all(s in plain for s in C.TRAINING_SHAPES)
    # K % 4 != 0 and == 0; one, two, three trips of the 32-wide K tile; N on both sides of the 32- and 64-column tiles
    ks = {s[1] for s in plain}
    assert {1, 32, 33, 64, 100} <= ks and any(k % 4 for k in ks) and any(k % 4 == 0 for k in ks)
    assert {"128x32", "128x64"} <= {C.tile_regime(m, n, 256) for m, _, n in plain if n <= 64}
    sk = C.splitk_cases()
    assert len(sk) * len(C.SPLITK_M) <= 100 and len(sk) == 25
    assert all(C.splitk_slices(k, n, fl) > 0 for k, n, fl in sk)
    # slices that do not divide the 32-wide tiles evenly, and slices whose K is no multiple of 4
    assert any(C.cdiv(k, 32) % C.splitk_slices(k, n, fl) for k, n, fl in sk) and any(k % 4 for k, _, _ in sk)


def test_slice_count_and_workspace_restated_from_the_header():
    assert C.splitk_slices(511, 29, 0) == 0 and C.splitk_slices(512, 29, 0) == 4 and C.splitk_slices(641, 64, 0) == 5
    assert C.splitk_slices(1024, 64, 0) == 8 and C.splitk_slices(4100, 1, 0) == 8
    assert C.splitk_slices(1024, 65, 0) == 0 and C.splitk_slices(1024, 65, C.FEW_ROWS) == 8
    assert C.splitk_slices(1024, 4096, C.FEW_ROWS) == 8 and C.splitk_slices(1024, 4097, C.FEW_ROWS) == 0
    assert C.splitk_workspace_bytes(3, 512, 29, 0) == 1536 and C.splitk_workspace_bytes(1, 512, 1, 0) == 256
    assert C.splitk_workspace_bytes(300, 511, 29, 0) == 0


@pytest.mark.parametrize("cus", [256, 304, 228, 128, 64, 32])
def test_three_ragged_row_counts_land_in_three_tile_configurations(cus):
    ms = C.regime_ms(cus)
    assert tuple(C.tile_regime(m, C.REGIME_N, cus) for m in ms) == C.REGIMES
    assert all(m % 128 for m in ms)
    if cus == 256:
        assert ms == (100, 128 * 8 + 37, 128 * 16 + 37)


def test_dense_family_is_exact_in_any_order():
    assert C.dense_x_max(1) == C.dense_x_max(1024) == 2047 and 7 * 1024 * 2047 + 1000 < 2 ** 24
    for M, K, N in all_data_shapes():
        x, w, b = C.make("dense", M, K, N)
        assert np.array_equal(x, np.rint(x)) and np.array_equal(w, np.rint(w)) and np.array_equal(b, np.rint(b))
        assert np.abs(x).max() <= C.dense_x_max(K) <= 2047 and np.abs(w).max() <= 7 and np.abs(b).max() <= 1000
        assert K <= 1024 or 7 * K * C.dense_x_max(K) + 1000 < 2 ** 24
        # every partial sum of every order is bounded by this, so it is an integer below 2^24: exact in float32
        assert C.abs_sum(x, w, b).max() < 2 ** 24, (M, K, N)
        want = C.reference(x, w, b)
        assert np.array_equal(x @ w.T + b, want), (M, K, N)                                    # float32 == float64
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)


def test_onehot_family_is_exact_and_rejects_three_pass_products():
    for M, K, N in all_data_shapes():
        x, w, b = C.make("onehot", M, K, N)
        km = C.onehot_k(M, K)
        assert np.array_equal(np.count_nonzero(x, axis=1), np.ones(M)) and np.all(x[np.arange(M), km] != 0)
        for v in (x[np.arange(M), km], w.ravel()):
            a = np.abs(v).astype(np.int64)
            assert np.array_equal(a, np.abs(v)) and a.min() >= 2049 and a.max() <= 2895 and np.all(a % 2 == 1)
        assert 2895 * 2895 < 2 ** 23 and C.abs_sum(x, w, b).max() < 2 ** 24
        want = C.reference(x, w, b)
        assert np.array_equal(want, x[np.arange(M), km][:, None].astype(np.float64) * w[:, km].T + b)
        assert np.array_equal(x @ w.T + b, want), (M, K, N)                                    # float32 == float64
        if M * K * N < 2e7:                    # (a Python loop over k)
            assert np.array_equal(C.chain_f32(x, w, b), want), (M, K, N)
        for rnd in (C.round_fp16, C.round_bf16):
            # the emulation's halves are exact here, so all it loses is lo.lo: wrong at EVERY element
            assert np.all(C.three_pass(x, w, b, rnd) != want), (M, K, N, rnd.__name__)


def test_bf16_rounding_emulation_is_round_to_nearest_even():
    import torch
    a = np.concatenate([np.arange(2049, 2896, dtype=np.float32), np.random.default_rng(0).standard_normal(4096).astype(np.float32)])
    assert np.array_equal(C.round_bf16(a), torch.from_numpy(a).to(torch.bfloat16).double().numpy())


def test_float32_chain_stays_inside_the_gaussian_bound():
    worst = 0.0
    for M, K, N in all_data_shapes():
        x, w, b = C.make("gauss", M, K, N)
        if M * N > 70000:                      # the chain emulation is a Python loop over k: the leading rows are enough
            x = x[:64]
        got = C.chain_f32(x, w, b)
        C.check("gauss", got, x, w, b, None, (M, K, N))
        C.check("gauss", C.clip(got, C.ACTS[1]), x, w, b, C.ACTS[1], (M, K, N))
        worst = max(worst, float((np.abs(got - C.reference(x, w, b)) / C.gauss_bound(x, w, b)).max()))
    print("float32 chain: worst error / bound", worst)


def test_check_fails_on_a_wrong_element():
    for fam in C.FAMILIES:
        x, w, b = C.make(fam, 33, 36, 31)
        good = C.reference(x, w, b).astype(np.float32)
        C.check(fam, good, x, w, b, None, fam)
        bad = good.copy()
        bad[7, 5] += 1.0 if fam != "gauss" else 1e-3
        with pytest.raises(AssertionError):
            C.check(fam, bad, x, w, b, None, fam)
        bad = good.copy()
        bad[0, 0] = np.nan
        with pytest.raises(AssertionError):
            C.check(fam, bad, x, w, b, None, fam)
