"""Proofs, without a GPU, of what tests/gemm_split_cases.py promises: the restated roundings against torch's CPU casts, the
exact split of the ``lo`` family, the exactness bound of every case, family and mode, the float64 reference against integer
arithmetic, the restated launcher's reach on 256 CUs with every tile edge and K-block count per kernel, the coded families'
separation, and four mutations that each move an expected output (so the device suite can fail)."""
import numpy as np
import pytest
import torch

import gemm_split_cases as C

SMALL = C.cases("small")


def all_family_values(mode):
    vals = []
    for c in SMALL[:5]:
        for fam in C.families(c.M, c.K, c.N, mode):
            x, w, _ = C.make(fam, c.M, c.K, c.N, mode)
            vals += [x.ravel(), w.ravel()]
    v = np.concatenate(vals)
    return np.concatenate([v, v - C.plane(v, C.fmt_of(mode))])           # and what the lo planes are rounded from


@pytest.mark.parametrize("mode", C.MODES)
def test_restated_roundings_match_torch_cpu_casts(mode):
    v = all_family_values(mode)
    t = torch.from_numpy(v)
    assert np.array_equal(C.rn_bf16(v), t.to(torch.bfloat16).float().numpy())
    inside = np.abs(v) <= C.F16_MAX
    assert np.array_equal(C.rn_f16(v[inside]), t[torch.from_numpy(inside)].to(torch.float16).float().numpy())
    # a spread of other values: subnormal results, ties, the top of the range
    rng = np.random.default_rng(0)
    u = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-9, 5, 4096), [65504.0, -65504.0, 65519.0, 2.0 ** -24,
                        2.0 ** -25, 3 * 2.0 ** -25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8]]).astype(np.float32)
    u = u[np.abs(u) < 65520.0]
    assert np.array_equal(C.rn_bf16(u), torch.from_numpy(u).to(torch.bfloat16).float().numpy())
    assert np.array_equal(C.rn_f16(u), torch.from_numpy(u).to(torch.float16).float().numpy())


def test_fp16_planes_saturate_as_documented():
    big = np.array([65504.0, -65504.0, 65536.0, 131008.0, 1.0e6, -3.0e5, 70000.0], dtype=np.float32)
    hi, lo = C.split(big, "f16")
    assert hi.tolist() == [65504.0, -65504.0, 65504.0, 65504.0, 65504.0, -65504.0, 65504.0]
    assert lo.tolist() == [0.0, 0.0, 32.0, 65504.0, 65504.0, -65504.0, 4496.0]
    tiny = np.array([2.0 ** -10 + 2.0 ** -24, -(2.0 ** -10 + 3 * 2.0 ** -24)], dtype=np.float32)
    hi, lo = C.split(tiny, "f16")
    assert hi.tolist() == [2.0 ** -10, -2.0 ** -10] and lo.tolist() == [2.0 ** -24, -3 * 2.0 ** -24]
    assert np.all(np.abs(lo) < 2.0 ** -14)                               # fp16-subnormal


@pytest.mark.parametrize("fmt,mode", [("f16", "f16x3"), ("bf16", "bf16x3")])
def test_lo_family_splits_exactly(fmt, mode):
    s = C.LO_SHIFT[fmt]
    for K in (32, 288, 640, 2048):
        x, w, _ = C.make("lo", 70, K, 50, mode)
        for a in (x, w):
            hi, lo = C.split(a, fmt)
            assert np.array_equal(hi, np.rint(a)) and np.all(hi != 0) and np.abs(hi).max() == C.lo_amax(K, fmt)
            assert np.array_equal(lo.astype(np.float64), a.astype(np.float64) - hi) and set(np.unique(lo * 2.0 ** s)) == {-1.0, 0.0, 1.0}
            assert np.mean(lo != 0) >= 0.25


@pytest.mark.parametrize("mode", C.MODES)
def test_exactness_bound_holds_for_every_small_case(mode):
    for c in SMALL:
        for fam in C.families(c.M, c.K, c.N, mode):
            x, w, b = C.make(fam, c.M, c.K, c.N, mode)
            r = C.exactness(C.Planes(x, w, mode), b)
            assert r.max() < 2 ** 24, (C.tag(c), fam, mode, float(r.max()))


def finite_min(g):
    return float(np.min(g[np.isfinite(g)])) if np.isfinite(g).any() else 1.0


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("group", ["quarter", "half", "full"])
def test_exactness_bound_holds_for_every_large_case(group, mode):
    """Millions of outputs a case, so an upper bound of the per-output ratio instead of the ratio itself: with one grid for
    the whole matrix (the smallest of the three products' grids) and the largest magnitudes of the planes,
    sum_k |term| + |bias| <= K (|xh||wh| + |xl||wh| + |xh||wl|)_max + |b|_max.  The ``range`` family has rows on other grids:
    its eight special rows and columns are checked output by output against everything, and all other rows and columns are
    integers of magnitude <= 3 on grid 1 (9 K < 2^24)."""
    for c in C.cases(group):
        for fam in C.families(c.M, c.K, c.N, mode):
            if mode == "fp16" and fam in ("hi", "lo", "clamp"):
                if c.K == 32:                                             # f16x3's operands and a subset of its terms:
                    for a_, b_ in zip(C.make(fam, c.M, c.K, c.N, "fp16"), C.make(fam, c.M, c.K, c.N, "f16x3")):
                        assert np.array_equal(a_, b_)                     # the same draw, and the same plane format
                    assert C.fmt_of("fp16") == C.fmt_of("f16x3")
                continue
            x, w, b = C.make(fam, c.M, c.K, c.N, mode)
            if fam == "range":
                sr, sc = [C.range_row(c.M, j) for j in range(8)], [C.range_row(c.N, j) for j in range(8)]
                assert len(set(sr)) == 8 and len(set(sc)) == 8 and not b.any()
                for a_, special in ((x, sr), (w, sc)):
                    rest = np.delete(a_, special, axis=0)
                    assert np.array_equal(rest, np.rint(rest)) and np.abs(rest).max() <= 3 and 9 * c.K < 2 ** 24
                for xs, ws, bs in ((x[sr], w, b), (x, w[sc], b[sc])):
                    r = C.exactness(C.Planes(xs, ws, mode), bs)
                    assert r.max() < 2 ** 24, (C.tag(c), fam, mode, float(r.max()))
                continue
            p = C.Planes(x, w, mode)
            gxh, gxl, gwh, gwl = (finite_min(C.grid(a_)) for a_ in (p.xh, p.xl, p.wh, p.wl))
            g = min(gxh * gwh, gxl * gwh if p.xl.any() else np.inf, gxh * gwl if p.wl.any() else np.inf)
            mx = [np.abs(a_).max() for a_ in (p.xh, p.xl, p.wh, p.wl)]
            per_k = mx[0] * mx[2] + mx[1] * mx[2] + mx[0] * mx[3]
            if fam.startswith("coded"):
                per_k = per_k / c.K                                       # one-hot against codes: one non-zero term per output
                assert np.all((p.xh != 0).sum(axis=1) == 1) or np.all((p.wh != 0).sum(axis=1) == 1)
            assert np.all(np.floor(np.abs(b) / g) == np.abs(b) / g)
            assert (c.K * per_k + np.abs(b).max()) / g < 2 ** 24, (C.tag(c), fam, mode)


def int_eval(p, b):
    """The product in int64 on the planes scaled to integers, every row of x and of w by its own grid."""
    def row_grid(hi, lo):
        g = np.minimum(C.grid(hi), C.grid(lo))
        return np.where(np.isinf(g), 1.0, g)[:, None]
    gx, gw = row_grid(p.xh, p.xl), row_grid(p.wh, p.wl)
    ints = [np.rint(a / g).astype(np.int64) for a, g in ((p.xh, gx), (p.xl, gx), (p.wh, gw), (p.wl, gw))]
    assert all(np.array_equal(i * g, a) for i, a, g in zip(ints, (p.xh, p.xl, p.wh, p.wl), (gx, gx, gw, gw)))
    xh, xl, wh, wl = ints
    assert all(np.abs(a_).max() < 2 ** 20 for a_ in ints) and p.xh.shape[1] <= 2 ** 11          # no int64 overflow
    y = xh @ wh.T + xl @ wh.T + xh @ wl.T
    return y.astype(np.float64) * (gx * gw.T) + b.astype(np.float64)


@pytest.mark.parametrize("mode", C.MODES)
def test_float64_reference_equals_integer_arithmetic_on_the_small_cases(mode):
    for c in SMALL:
        for fam in C.families(c.M, c.K, c.N, mode):
            x, w, b = C.make(fam, c.M, c.K, c.N, mode)
            p = C.Planes(x, w, mode)
            assert np.array_equal(C.expected(x, w, b, mode, planes=p), int_eval(p, b)), (C.tag(c), fam)


def test_one_plane_mode_differs_from_two_where_a_lo_plane_exists():
    c = SMALL[4]
    x, w, b = C.make("lo", c.M, c.K, c.N, "fp16")
    assert not np.array_equal(C.expected(x, w, b, "fp16"), C.expected(x, w, b, "f16x3"))


# ----------------------------------------------------------------------------- the launcher
@pytest.mark.parametrize("mode", C.MODES)
def test_route_reaches_every_kernel_with_every_edge(mode):
    got = C.reached(mode)
    assert set(got) == set(C.kernels_of(mode)), (mode, sorted(got))
    for c in C.cases():
        want = C.INTENDED[c.group]
        assert C.route(c.M, c.K, c.N, mode) == want, (C.tag(c), mode)
    for kernel, hits in got.items():
        tm, tn = C.TILES[kernel]
        ms, ns = {c.M for c, _ in hits}, {c.N for c, _ in hits}
        nks = {c.K // 32 for c, _ in hits}
        assert set(C.KBLOCKS) <= nks and max(nks) >= 16, (mode, kernel, sorted(nks))
        for name, vals, t in (("M", ms, tm), ("N", ns, tn)):
            res = {v % t for v in vals}
            assert {1, t - 1, 0} <= res, (mode, kernel, name, sorted(vals))
            assert any(v > t and v % t == 1 for v in vals), (mode, kernel, name, "tile + 1")
        assert any(n % 4 for n in ns) and any(n % 4 == 0 and n % tn for n in ns), (mode, kernel, sorted(ns))
        if kernel in ("tile64", "kernel") or (mode == "fp16" and kernel in ("kernel2", "kernel4", "kernel4n")):
            # reachable at small outputs: the literal 1, tile - 1, tile, tile + 1
            assert {1, tm - 1, tm, tm + 1} <= ms, (mode, kernel, sorted(ms))
            assert tn == 256 or {1, tn - 1, tn, tn + 1} <= ns, (mode, kernel, sorted(ns))


def test_route_candidates_of_the_issue():
    assert C.route(300, 64, 4200, "f16x3") == "kernel4q" and C.route(300, 64, 4200, "f16x3", quarter_env="0") == "kernel4h"
    assert C.route(100, 64, 10500, "f16x3") == "kernel4h"
    assert C.route(3330, 64, 3330, "f16x3") == "kernel4" and C.route(3330, 64, 3330, "f16x3", 2) == "kernel2"
    assert C.route(3330, 64, 3330, "f16x3", 9) == "kernel4n" and C.route(3330, 64, 3330, "bf16x3", 9) == "kernel4n<6>"
    assert C.route(64, 64, 64, "f16x3") == "tile64" and C.route(64, 64, 64, "f16x3", tile64_env="0") == "kernel"
    assert C.route(64, 64, 64, "fp16", tile64_env="0") == "kernel4"
    # the shapes of the existing bit-equality tests
    assert C.route(1024, 2048, 8192, "f16x3") == "kernel4h" and C.route(4100, 64, 4100, "f16x3") == "kernel4"
    assert C.route(512, 2560, 1024, "f16x3") == "tile64" and C.route(2100, 96, 2052, "f16x3") == "kernel4h"


def test_nonfinite_cases_reach_one_kernel_each():
    for mode in C.MODES:
        got = [C.route(c.M, c.K, c.N, mode, *cfg) for c, cfg in C.nonfinite_cases()]
        assert set(C.kernels_of(mode)) - set(got) <= {"kernel4n<2>", "kernel4n<3,spaced>", "kernel4n<2,spaced>"}, (mode, got)


def test_sizes_restated():
    assert C.workspace_bytes(3, 32, 5) == 512 + 768 and C.packed_bytes(32, 5) == 768 and C.x_workspace_bytes(3, 32) == 512
    assert C.workspace_bytes(0, 32, 5) == 0 and C.packed_bytes(32, 0) == 0


# ----------------------------------------------------------------------------- the coded families
@pytest.mark.parametrize("mode", C.MODES)
def test_coded_families_separate_every_position(mode):
    R = C.code_rows(mode)
    cd = C.codes(512, 2048, mode)
    assert len(np.unique(cd[:R, :64])) == R * 64                          # distinct over (row mod R, k mod 64)
    hi, lo = C.split(cd, C.fmt_of(mode))
    total = hi.astype(np.float64) + (lo if C.two_planes(mode) else 0)
    assert np.array_equal(total, cd)                                      # exact in the format
    for group in C.SHAPES:
        for c in C.cases(group):
            for rows in (c.M, c.N):
                k = C.onehot_k(rows, c.K)
                if rows >= max(32, 2 * (c.K // 32)):
                    assert set(k % 32) == set(range(32)) and set(k // 32) == set(range(c.K // 32)), (C.tag(c), rows)
                if rows >= c.K:
                    assert set(k) == set(range(c.K))
        # every K-block count of the group has such a case for x's rows and for w's
        for nk in {c.K // 32 for c in C.cases(group)}:
            assert any(c.K // 32 == nk and min(c.M, c.N) >= max(32, 2 * nk) for c in C.cases(group)), (group, nk)
    c = SMALL[5]
    x, w, b = C.make("coded-w", c.M, c.K, c.N, mode)
    y = C.expected(x, w, b, mode)
    assert np.array_equal(y, w[:, C.onehot_k(c.M, c.K)].T.astype(np.float64))
    x, w, b = C.make("coded-x", c.M, c.K, c.N, mode)
    assert np.array_equal(C.expected(x, w, b, mode), x[:, C.onehot_k(c.N, c.K)].astype(np.float64))


def test_clamp_family_reaches_both_bounds_and_all_three_regions():
    lo, hi = C.CLAMP_ACT
    for mode in C.MODES:
        for c in C.cases():
            if c.M * c.N < 64 or c.group == "full" and mode != "f16x3":
                continue
            x, w, b = C.make("clamp", c.M, c.K, c.N, mode)
            y = C.expected(x, w, b, mode)
            assert (y < lo).any() and (y > hi).any() and ((y > lo) & (y < hi)).any() and (y == lo).any() and (y == hi).any(), C.tag(c)


# ----------------------------------------------------------------------------- mutations
def moved(p, b, q):
    return not np.array_equal(p.product() + b, q.product() + b)


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3"])
def test_each_mutation_moves_an_expected_output(mode):
    import copy
    hits = {"swap": 0, "cross": 0, "lolo": 0, "row": 0}
    for c in SMALL[2:]:
        x, w, b = C.make("lo", c.M, c.K, c.N, mode)
        p = C.Planes(x, w, mode)
        base = p.product()
        # a lo element swapped with its neighbour (one granule of one row)
        q = copy.deepcopy(p)
        k = int(np.argmax(q.xl[1, :-1] != q.xl[1, 1:]))
        q.xl[1, [k, k + 1]] = q.xl[1, [k + 1, k]]
        hits["swap"] += not np.array_equal(q.product(), base)
        # the x_lo . w_hi term lost for the last K-block
        q = copy.deepcopy(p)
        lost = base - q.xl[:, -32:] @ q.wh[:, -32:].T
        hits["cross"] += not np.array_equal(lost, base)
        # an added x_lo . w_lo term
        hits["lolo"] += not np.array_equal(p.product(lolo=True), base)
        # a row read at m + 1
        q = copy.deepcopy(p)
        q.xh[0], q.xl[0] = p.xh[1], p.xl[1]
        hits["row"] += not np.array_equal(q.product(), base)
    assert all(v == len(SMALL) - 2 for v in hits.values()), hits
    # ... and the coded families see a neighbouring element, row or K-block by construction
    c = SMALL[5]
    x, w, b = C.make("coded-w", c.M, c.K, c.N, mode)
    for shifted in (np.roll(w, 1, axis=1), np.roll(w, 1, axis=0), np.roll(w, 32, axis=1)):
        assert not np.array_equal(C.expected(x, shifted, b, mode), C.expected(x, w, b, mode))
