"""tests/small_ops_cases.py proven without a GPU: every reference against torch on the CPU in float64 (torch.clamp,
F.hardtanh, torch.log_softmax and its autograd, argmax + collapse + blank removal, torch.topk where no ties occur,
F.embedding, log_softmax(W tanh(e + p) + b)), the case lists against the edges they were written for, and, for the three
toleranced operators, a float32 restatement of the kernel's arithmetic (its summation order, float32 exp / log / tanh) against
the derived bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_ops_cases as C

f32 = np.float32


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


# ----------------------------------------------------------------------------- references against torch
@pytest.mark.parametrize("lo,hi", C.CLAMP_LIMITS)
def test_clamp_reference_is_torch_clamp_and_hardtanh(lo, hi):
    """Bit for bit in float32, NaN staying NaN, -0.0 staying -0.0; every special value is in every input that has room."""
    for n in C.CLAMP_N[:4] + (5000,):
        x = C.clamp_input(n, lo, hi)
        want = C.clamp_ref(x, lo, hi)
        xt = torch.from_numpy(x)
        assert C.same_bits_or_both_nan(want, torch.clamp(xt, float(f32(lo)), float(f32(hi))).numpy()).all()
        if np.isfinite(hi):
            assert C.same_bits_or_both_nan(want, F.hardtanh(xt, float(f32(lo)), float(f32(hi))).numpy()).all()
        assert np.array_equal(np.isnan(want), np.isnan(x))
        if n >= 17:
            sp = C.clamp_specials(lo, hi)
            assert C.same_bits(x[:len(sp)], sp) and np.isnan(x).sum() >= 2 and np.isinf(x).sum() >= 4
            assert (x[~np.isnan(x)] < f32(lo)).any() and (x[~np.isnan(x)] > f32(hi)).any() == bool(np.isfinite(hi))
    assert C.CLAMP_N[-1] > 2048 * 256


def test_mask_reference_and_lengths():
    for inner in C.MASK_INNER:
        for T in C.MASK_T:
            x, lens = C.mask_input(inner, T)
            assert sorted(lens.tolist()) == sorted([0, 1, T - 1, T, T + 5, -3])
            want = C.mask_ref(x, lens)
            t = np.arange(T)[None, None, :]
            dead = t >= np.maximum(lens, 0)[:, None, None]
            dead = np.broadcast_to(dead, x.shape).copy()
            assert np.all(C.bits(want)[dead] == 0), "the tail is +0.0"
            assert np.array_equal(C.bits(want)[~dead], C.bits(x)[~dead])
            assert C.same_bits_or_both_nan(want, torch.where(torch.from_numpy(dead), torch.zeros(()), torch.from_numpy(x)).numpy()).all()
            if T > 2:
                assert np.isnan(x[dead]).any() and np.isinf(x[dead]).any()
    assert 64 in C.MASK_INNER and 65 in C.MASK_INNER and 256 in C.MASK_T and 257 in C.MASK_T


def test_transpose_reference():
    for N in C.NCT_N:
        for CF in C.NCT_SIZES:
            for T in C.NCT_SIZES:
                x = C.nct_input(N, CF, T)
                want = C.nct_ref(x)
                assert want.shape == (T, N, CF) and len(np.unique(x)) == x.size
                assert np.array_equal(want, torch.from_numpy(x).permute(2, 0, 1).contiguous().numpy())


@pytest.mark.parametrize("shape", C.LSM_SHAPES)
def test_log_softmax_reference_is_torch_and_its_autograd(shape):
    """Forward: within 1e-12 (absolute, on values of order 100) of torch.log_softmax in float64 where finite, the same -Inf
    and NaN entries.  Backward: torch's autograd of log_softmax at the x that gave y, on the draws without -Inf (autograd of
    a -Inf entry is NaN in torch; the kernel's formula, which starts from y, passes the gradient through)."""
    for scale in C.LSM_SCALES:
        for variant in C.LSM_VARIANTS:
            x = C.lsm_input(shape, scale, variant)
            ref = C.lsm_ref(x)
            want = torch.log_softmax(t64(x), dim=1).numpy()
            assert np.array_equal(np.isnan(ref), np.isnan(want)), (shape, scale, variant)
            inf = np.isinf(want)
            assert np.array_equal(ref[inf], want[inf])
            fin = np.isfinite(want)
            assert np.all(np.abs(ref[fin] - want[fin]) <= 1e-12)
            if variant == "neg_inf_entries" and shape[1] > 1:
                assert np.isneginf(ref).any() and not np.isnan(ref).any()
            if variant == "bad_columns":
                cols = [(o, i) for o in range(shape[0]) for i in range(shape[2])][:3]
                assert all(np.isnan(ref[o, :, i]).all() for o, i in cols)
                assert np.isnan(ref).sum() == len(cols) * shape[1]
        xt = t64(C.lsm_input(shape, scale, "plain")).requires_grad_()
        y = torch.log_softmax(xt, dim=1)
        g = C.rng_of(("g", shape)).standard_normal(shape)
        y.backward(t64(g))
        ours = C.lsm_backward_ref(y.detach().numpy(), g)
        assert np.all(np.abs(ours - xt.grad.numpy()) <= 1e-12 * (1 + np.abs(g).sum(axis=1, keepdims=True)))
        yb, gb = C.lsm_backward_input(shape, scale)
        passes = np.isneginf(yb)
        assert np.array_equal(C.lsm_backward_ref(yb, gb)[passes], gb.astype(np.float64)[passes])
    assert any(o * i > 256 for o, _, i in C.LSM_SHAPES) and (1, 1, 1) in C.LSM_SHAPES


def collapse_torch(x, lens, blank):
    T = x.shape[0]
    sym = torch.argmax(torch.from_numpy(x), dim=2)
    out = []
    for n in range(x.shape[1]):
        s = sym[:min(max(int(lens[n]), 0), T), n]
        s = torch.unique_consecutive(s)
        out.append(s[s != blank].tolist())
    return out


@pytest.mark.parametrize("V", C.GREEDY_V)
def test_greedy_reference_is_argmax_collapse_and_blank_removal(V):
    """torch.argmax + unique_consecutive + blank removal on every path.  torch.argmax treats a NaN as the maximum; which of
    several equal maxima or several NaNs it returns is not documented, so the ``ties_and_non_finite`` frames are proven
    against the rule itself (``first_max``: asserted frame by frame in ``greedy_case``) and against torch only where the
    arg max is unique."""
    made = 0
    for T in (1, 257):
        for blank in sorted({0, V - 1}):
            for path in C.GREEDY_PATHS:
                case = C.greedy_case(V, T, blank, path)
                if case is None:
                    assert path == "no_blank_no_repeat" and V < 3
                    continue
                x, lens, want = case
                made += 1
                assert lens.tolist() == [T, T // 2 + 1, 0, T + 5] and want[2] == []
                if path != "ties_and_non_finite":
                    assert want == collapse_torch(x, lens, blank), (V, T, blank, path)
                if path == "all_blank" or V == 1:
                    assert all(w == [] for w in want)
                if path == "no_blank_no_repeat":
                    assert [len(w) for w in want] == [T, T // 2 + 1, 0, T]
                if path == "blank_on_edges" and T == 257 and V > 1:
                    assert len(want[0]) == 2 and len(set(want[0])) == 1      # ... blank at 64 ... blank at 256, the last frame
                if path == "run_across_edges" and T == 257 and V > 1:
                    assert len(want[0]) == 3 and len(want[1]) == 2      # frames 0-1, 60-67, 250-261: each run once
    assert made >= 8
    rows = np.array([[1, np.inf, np.nan, 5], [np.nan, 3, np.nan, 9], [-np.inf] * 4, [2, 7, 7, 1]], dtype=f32)
    assert [C.first_max(r) for r in rows] == [2, 0, 0, 1]
    assert torch.argmax(torch.from_numpy(rows[[0, 3]]), dim=1).tolist() == [2, 1]


def test_embedding_reference_is_f_embedding_on_clamped_indices():
    for D in C.EMB_D:
        for V1 in C.EMB_V1:
            table, idx = C.embedding_input(D, V1)
            assert idx[:4].tolist() == [0, V1 - 1, -1, V1 + 3]
            want = C.embedding_ref(table, idx)
            got = F.embedding(torch.from_numpy(idx).long().clamp(0, V1 - 1), torch.from_numpy(table)).numpy()
            assert C.same_bits(want, got)
            assert C.same_bits(want[2], table[0]) and C.same_bits(want[3], table[V1 - 1])


def test_topk_reference_is_torch_topk_where_no_ties_occur_and_stable_where_they_do():
    r = C.rng_of("topk-distinct")
    x = r.permutation(300).astype(f32).reshape(3, 100)
    for k in (1, 5, 100):
        idx, val = C.topk_ref(x, k)
        tv, ti = torch.topk(torch.from_numpy(x), k, dim=1)
        assert np.array_equal(idx, ti.numpy()) and np.array_equal(val, tv.numpy())
    for Cn in C.TOPK_C:
        x = C.topk_input(Cn)
        for k in C.topk_ks(Cn):
            idx, val = C.topk_ref(x, k)
            for b in range(C.TOPK_B):
                live = idx[b] >= 0
                n_live = int(np.sum(x[b] > -np.inf))
                assert live.sum() == min(k, n_live) and np.all(live[:live.sum()])
                assert np.all(idx[b][~live] == -1) and np.all(np.isneginf(val[b][~live]))
                order = np.argsort(-np.where(x[b] > -np.inf, x[b], -np.inf), kind="stable")[:live.sum()]
                assert np.array_equal(idx[b][live], order) and np.array_equal(val[b][live], x[b][order])
                assert not np.isnan(val[b]).any()
        if Cn >= 255:
            assert np.isnan(x[2]).any() and np.isneginf(x[1]).any() and len(np.unique(x[0])) <= 5
    assert C.topk_ks(3)[-1] == 5 and C.topk_ks(1000)[-1] == 1002


@pytest.mark.parametrize("J", C.JOINT_J)
def test_joint_reference_is_log_softmax_of_the_projected_tanh(J):
    for V1 in C.JOINT_V1:
        enc, row, pred, w, b = C.joint_input(J, V1)
        assert np.isnan(enc[2]).all() and np.isnan(enc[4]).all() and len(set(row.tolist())) < len(row)
        for bias in (b, None):
            ref = C.joint_ref(enc, row, pred, w, bias)
            z = torch.tanh(t64(enc)[torch.from_numpy(row).long()] + t64(pred))
            logits = z @ t64(w).T + (0 if bias is None else t64(bias))
            want = torch.log_softmax(logits, dim=1).numpy()
            assert np.all(np.abs(ref - want) <= 1e-12), (J, V1)
            assert np.all(np.abs(C.logsumexp_rows(ref)) <= 1e-12)
    assert (C.JOINT_REFUSED[0] + C.JOINT_REFUSED[1]) * 4 > 64 * 1024


# ----------------------------------------------------------------------------- float32 restatements against the bounds
def lsm_f32(x):
    """log_softmax_axis_kernel in float32 numpy: running fmax, sum of exp(x - m) in the order of a, log(sum) + m, x - lz."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        A = x.shape[1]
        m = np.full((x.shape[0], x.shape[2]), -np.inf, dtype=f32)
        for a in range(A):
            m = np.fmax(m, x[:, a])
        s = np.zeros_like(m)
        for a in range(A):
            s = s + np.exp(x[:, a] - m)
        lz = np.log(s) + m
        y = x - lz[:, None, :]
    assert y.dtype == f32
    return y


def lsm_backward_f32(y, g):
    s = np.zeros((y.shape[0], y.shape[2]), dtype=f32)
    for a in range(y.shape[1]):
        s = s + g[:, a]
    out = g - np.exp(y) * s[:, None, :]
    assert out.dtype == f32
    return out


def wave_sum_f32(lanes):
    """The xor butterfly of 64 lanes over the last axis; every lane ends with the total, lane 0's is returned."""
    v = lanes.astype(f32)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def strided_lane_sums_f32(terms):
    """terms [..., n] float32 -> [..., 64]: lane l adds its terms l, l + 64, ... in that order."""
    n = terms.shape[-1]
    lanes = np.zeros(terms.shape[:-1] + (64,), dtype=f32)
    for k0 in range(0, n, 64):
        chunk = terms[..., k0:k0 + 64]
        lanes[..., :chunk.shape[-1]] = lanes[..., :chunk.shape[-1]] + chunk
    return lanes


def joint_f32(enc, row, pred, w, b):
    """rnnt_joint_kernel in float32 numpy: tanh of the float32 sum, per-lane strided dot products, the butterfly, the bias,
    then the log-softmax of wave 0 with lane-strided maxima and sums."""
    z = np.tanh(enc[row] + pred)                                  # [R, J] float32
    prod = w[None, :, :] * z[:, None, :]                          # [R, V1, J]
    lg = wave_sum_f32(strided_lane_sums_f32(prod))
    if b is not None:
        lg = lg + b[None, :]
    m = np.max(lg, axis=1, keepdims=True)
    s = wave_sum_f32(strided_lane_sums_f32(np.exp(lg - m)))
    lz = np.log(s)[:, None] + m
    out = lg - lz
    assert out.dtype == f32
    return out


def test_log_softmax_restated_in_float32_stays_inside_the_bound():
    """Largest error / bound over all shapes, scales and variants: 0.33 (forward), 0.25 (backward)."""
    worst_f = worst_b = 0.0
    for shape in C.LSM_SHAPES:
        for scale in C.LSM_SCALES:
            for variant in C.LSM_VARIANTS:
                x = C.lsm_input(shape, scale, variant)
                worst_f = max(worst_f, C.check_toleranced(lsm_f32(x), C.lsm_ref(x), C.lsm_bound(x), (shape, scale, variant)))
            y, g = C.lsm_backward_input(shape, scale)
            worst_b = max(worst_b, C.check_toleranced(lsm_backward_f32(y, g), C.lsm_backward_ref(y, g),
                                                      C.lsm_backward_bound(y, g), (shape, scale, "backward")))
    print("log-softmax worst error / bound: forward", worst_f, "backward", worst_b)
    assert 0 < worst_f <= 0.5 and 0 < worst_b <= 0.5, (worst_f, worst_b)


def test_joint_restated_in_float32_stays_inside_the_bound():
    """Largest error / bound over all (J, V1), with and without the bias: 0.09; each row's logsumexp within the row's
    largest bound of 0."""
    worst = 0.0
    for J in C.JOINT_J:
        for V1 in C.JOINT_V1:
            enc, row, pred, w, b = C.joint_input(J, V1)
            for bias in (b, None):
                got = joint_f32(enc, row, pred, w, bias)
                bound = C.joint_bound(enc, row, pred, w, bias)
                worst = max(worst, C.check_toleranced(got, C.joint_ref(enc, row, pred, w, bias), bound, (J, V1, bias is None)))
                assert np.all(np.abs(C.logsumexp_rows(got)) <= bound.max(axis=1)), (J, V1)
    print("joint worst error / bound", worst)
    assert 0 < worst <= 0.5, worst
