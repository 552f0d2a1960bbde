"""What tests/conv_exact_cases.py promises, proved without a GPU: the reference against torch and the numpy oracle, the cap
and the plane-exactness of every family, that the families can fail, the edges the case lists must contain, the routes, and
the reads predicate."""
import numpy as np
import pytest
import torch

import conv_exact_cases as C
from oracle import ds_oracle as O

ENTRIES = ("tap", "cl", "fwin", "gemm1d")
ALL_CASES = [c for e in ENTRIES for c in C.cases(e)]
ISO_CASES = [c for e in ENTRIES for c in C.isolation_cases(e)]
PAIRS = C.handover_pairs()


def work(c):
    return c.N * c.Cout * c.Fout * c.Tout * C.terms(c)


SMALL = [c for c in ALL_CASES + ISO_CASES if work(c) < 3e7]


def ident(c):
    return f"{c.entry}-{c.tag}"


def torch_conv(c, x, w, b):
    """float64 torch.nn.functional.conv2d on the masked input, padded by hand (left pads as given, zeros to the right)."""
    xm = torch.from_numpy(np.asarray(x, dtype=np.float64)).clone()
    for n, ln in enumerate(C.eff_lens(c)):
        xm[n, :, :, ln:] = 0
    hf = (c.Fout - 1) * c.SF + (c.KF - 1) * c.DF + 1
    ht = (c.Tout - 1) * c.ST + (c.KT - 1) * c.DT + 1
    xp = torch.nn.functional.pad(xm, (c.pad_t, max(0, ht - c.pad_t - c.Tin), c.pad_f, max(0, hf - c.pad_f - c.Fin)))
    y = torch.nn.functional.conv2d(xp, torch.from_numpy(w.astype(np.float64)),
                                   torch.from_numpy(b.astype(np.float64)) if c.bias else None,
                                   (c.SF, c.ST), 0, (c.DF, c.DT), c.groups)[:, :, :c.Fout, :c.Tout].numpy()
    return y if c.act is None else np.clip(y, c.act[0], c.act[1])


@pytest.mark.parametrize("c", SMALL, ids=ident)
def test_reference_equals_torch_conv2d_in_float64(c):
    for fam in ("dense", "gauss") if c.entry == "tap" else ("dense",):
        x, w, b = C.make(c, fam)
        got, ref = C.want(c, fam), torch_conv(c, x, w, b)
        assert got.shape == ref.shape
        if fam == "dense":
            assert np.array_equal(got, ref)
        else:
            assert np.allclose(got, ref, rtol=0, atol=1e-9)


@pytest.mark.parametrize("c", [c for c in SMALL if (c.pad_f, c.Fout) == C.pad_same(c.Fin, c.KF, c.SF, c.DF)
                               and (c.pad_t, c.Tout) == C.pad_same(c.Tin, c.KT, c.ST, c.DT) and (c.KF > 1 or c.KT > 1)][::3],
                         ids=ident)
def test_reference_equals_the_numpy_oracle_under_same_padding(c):
    x, w, b = C.make(c, "dense")
    lens = np.array(C.eff_lens(c))
    y, _ = O.mask_conv2d(x, lens, w, b if c.bias else None, (c.SF, c.ST), True, (c.DF, c.DT), c.groups)
    if c.act is not None:
        y = np.clip(y, c.act[0], c.act[1])
    assert np.array_equal(np.asarray(y, dtype=np.float64), C.want(c, "dense"))


@pytest.mark.parametrize("c", ALL_CASES + ISO_CASES, ids=ident)
def test_the_cap_holds_for_every_family(c):
    for fam in C.EXACT_FAMILIES:
        x, w, b = C.make(c, fam)
        s = C.abs_sum(c, x, w, b if c.bias else None)
        assert s.max() < C.CAP, (fam, s.max())
        assert np.all(x == np.rint(x)) and np.all(w == np.rint(w)) and np.all(b == np.rint(b))


def test_the_cap_holds_for_the_pairs():
    for c1, c2 in PAIRS:
        for fam in C.PAIR_FAMILIES:
            x, w1, b1, w2, b2 = C.make_pair(c1, c2, fam)
            y1, _ = C.want_pair(c1, c2, fam)
            assert C.abs_sum(c1, x, w1, b1).max() < C.CAP and C.abs_sum(c2, y1, w2, b2).max() < C.CAP
            assert y1.min() >= c1.act[0] and y1.max() <= c1.act[1] and np.all(y1 == np.rint(y1))
    s1 = PAIRS[1][0]
    for fam in C.PAIR_FAMILIES:
        y1, _ = C.want_pair(*PAIRS[1], fam)
        need_lo = (y1 > 2048) & (y1 % 2 == 1)
        assert s1.act == (0.0, 4095.0) and need_lo.sum() > 100, "the small pair's conv1 outputs must need a lo plane"
        for rnd in (C.round_fp16, C.round_bf16):
            hi, lo = C.split(y1, rnd)
            assert np.array_equal(hi + lo, y1) and np.all(lo[need_lo] != 0)
        # every channel and feature row of conv2's input holds such a value
        assert need_lo.any(axis=(0, 3)).all(), fam
    # DS2's pair at 80 x 130 with the clamp (0, 20)
    c1, c2 = PAIRS[0]
    assert (c1.Fin, c1.Tin, c1.KF, c1.KT, c1.SF, c1.ST, c1.act) == (80, 130, 41, 11, 2, 2, (0.0, 20.0))
    assert (c2.Cin, c2.KF, c2.KT, c2.SF, c2.ST, c2.act) == (32, 21, 11, 2, 1, (0.0, 20.0)) and C.terms(PAIRS[1][1]) <= 585


@pytest.mark.parametrize("fam", C.EXACT_FAMILIES)
def test_every_value_is_exact_as_hi_plus_lo_and_the_lo_planes_are_needed(fam):
    """fp16 and bf16 planes, the weights under the restated power-of-two scale, the activations also doubled."""
    for c in SMALL:
        x, w, b = C.make(c, fam)
        for rnd, half in ((C.round_fp16, True), (C.round_bf16, False)):
            s = C.weight_scale(w, half)
            assert s == (1.0 if not half else 1024.0 if fam != "wlo" else 2.0)
            assert 2.0 ** 12 <= np.abs(w).max() * s < 2.0 ** 13 or not half
            for name, v in (("x", x), ("2x", 2.0 * x), ("w", w * s)):
                hi, lo = C.split(v, rnd)
                assert np.array_equal(hi + lo, v.astype(np.float64)), (c.tag, fam, name)
                big = np.abs(v) > 2048 * (s if name == "w" else 2 if name == "2x" else 1)
                if fam == "dense" or (fam, name[-1]) in (("xlo", "w"), ("wlo", "x")):
                    assert not big.any() and np.all(lo == 0), (c.tag, fam, name, "must fit one plane")
                else:
                    assert big.any() and np.all(lo[big] != 0), (c.tag, fam, name, "a 12-bit value without a lo")


def without_lo(a, rnd):
    return C.split(a, rnd)[0].astype(np.float32)


@pytest.mark.parametrize("c", [c for e in ENTRIES for c in C.cases(e)[:3]], ids=ident)
def test_a_product_without_the_lo_plane_is_wrong_on_its_family(c):
    for rnd in (C.round_fp16, C.round_bf16):
        x, w, b = C.make(c, "xlo")
        assert not np.array_equal(C.case_reference(c, without_lo(x, rnd), w, b, act=None), C.case_reference(c, x, w, b, act=None))
        x, w, b = C.make(c, "wlo")
        assert not np.array_equal(C.case_reference(c, x, without_lo(w, rnd), b, act=None), C.case_reference(c, x, w, b, act=None))


@pytest.mark.parametrize("c", [c for c in ALL_CASES if C.terms(c) > 1], ids=ident)
def test_the_12_bit_values_visit_every_channel_lane_tap_and_window_row(c):
    """xlo: for every (channel mod 16, kf, kt) some output's window holds an in-length 12-bit x there."""
    x, _, _ = C.make(c, "xlo")
    big = np.abs(x) > 2048
    for n, ln in enumerate(C.eff_lens(c)):
        big[n, :, :, ln:] = False
    hf = (c.Fout - 1) * c.SF + (c.KF - 1) * c.DF + 1
    ht = (c.Tout - 1) * c.ST + (c.KT - 1) * c.DT + 1
    bp = np.zeros((c.N, c.Cin, max(hf, c.pad_f + c.Fin), max(ht, c.pad_t + c.Tin)), dtype=bool)
    bp[:, :, c.pad_f:c.pad_f + c.Fin, c.pad_t:c.pad_t + c.Tin] = big
    cg = c.Cin // c.groups
    for lane in range(min(16, cg)):
        for kf in range(c.KF):
            for kt in range(c.KT):
                sl = bp[:, :, kf * c.DF:kf * c.DF + (c.Fout - 1) * c.SF + 1:c.SF, kt * c.DT:kt * c.DT + (c.Tout - 1) * c.ST + 1:c.ST]
                rows_in = [f for f in range(c.Fout) if 0 <= f * c.SF - c.pad_f + kf * c.DF < c.Fin]
                if not rows_in or not any(0 <= t * c.ST - c.pad_t + kt * c.DT < max(C.eff_lens(c)) for t in range(c.Tout)):
                    continue                      # a tap that only ever meets padding
                chans = [ch for ch in range(c.Cin) if (ch % cg) % 16 == lane]
                assert sl[:, chans].any(), (c.tag, lane, kf, kt)


def test_the_case_lists_contain_every_edge():
    def has(cs, **want):
        for k, vals in want.items():
            got = {getattr(c, k) if not callable(k) else k(c) for c in cs}
            assert set(vals) <= got, (k, sorted(set(vals) - got))

    tap, cl, fw, g1 = (C.cases(e) for e in ENTRIES)
    has(tap, Tout=(1, 31, 32, 33, 127, 128, 129), KT=(1, 2, 3, 4, 5, 11), ST=(1, 2, 3), DT=(1, 2), SF=(1, 2, 3), DF=(1, 2, 3))
    assert {1, 31, 32, 33, 40} <= {c.Cout // c.groups for c in tap}
    assert {1, 15, 16, 17, 33} <= {c.Cin // c.groups * c.KF for c in tap}
    assert {1, 2} <= {c.groups for c in tap} and any(c.groups == c.Cin > 1 for c in tap)
    assert any(c.pad_f == 0 and c.pad_t == 0 and c.KF > 1 for c in tap) and any(c.pad_f > 0 and c.pad_t > 0 for c in tap)
    # feature rows above and below the input
    assert any(c.pad_f > 0 and (c.Fout - 1) * c.SF - c.pad_f + (c.KF - 1) * c.DF >= c.Fin for c in tap)
    assert any(c.lens is None for c in tap) and any(not c.bias for c in tap)
    assert any(c.lens and 1 in c.lens and max(c.lens) > c.Tin for c in tap)
    cut = [c for c in tap if c.act is not None]
    assert cut
    for c in cut:
        raw = C.case_reference(c, *C.make(c, "dense"), act=None)
        assert (raw < c.act[0]).any() and (raw > c.act[1]).any() and ((raw > c.act[0]) & (raw < c.act[1])).any()
    has(cl, Cin=(16, 32, 48), Cout=(16, 29, 32, 33, 40, 64), Tout=(47, 48, 49, 127, 128, 129), Fout=(1, 2, 3, 8, 9),
        KT=(1, 2, 3, 5, 11), ST=(1, 2, 3), DT=(1, 2), KF=(1, 3, 5), SF=(1, 2), DF=(1, 2), N=(1, 5, 70))
    short = [c for c in cl if C.cl_route(c) == "short"]
    assert {1, 15, 16} <= {c.Tout for c in short} and {16, 29, 33} <= {c.Cout for c in short} and {1, 5, 70} <= {c.N for c in short}
    assert any(c.Tout == 17 and c.Cin == 32 and C.cl_route(c) == "tile32" for c in cl)
    has(fw, KF=(15, 16, 17, 41), SF=(2, 4), KT=(1, 3, 11), Tout=(48, 49, 128, 129), Fin=(80, 81), Cout=(32, 40, 96))
    assert max(c.N * c.Cin * c.Fin * c.Tin for c in ALL_CASES) == 3 * 81 * 301
    assert {31, 32, 33, 55, 96} <= {c.Cin * c.KT for c in g1}
    has(g1, Tout=(1, 31, 32, 33), Cout=(1, 63, 64, 65), ST=(1, 2), DT=(1, 2), pad_t=(0, 5))
    assert any(not c.bias for c in g1) and all(c.lens is not None and c.Fin == c.KF == c.SF == 1 for c in g1)
    assert all(c.Cin == 1 and c.DF == 1 and c.SF % 2 == 0 and c.groups == 1 for c in fw)
    assert all(c.Cin % 16 == 0 and c.groups == 1 for c in cl)


def test_the_routes_the_cases_are_meant_to_take():
    cl = {c.tag: C.cl_route(c) for c in C.cases("cl")}
    assert cl["cin16_cout16_t47_kt1"] == cl["cin32_cout32_t48_kt2"] == cl["fout9_t48_kt11"] == cl["n5_t47_st2_dt2"] == "tile32"
    assert cl["cin48_cout33_t49_kt3"] == cl["cout40_t127_kt5_dt2"] == cl["cout64_t128_st2"] == cl["cout29_t129_kt11_st3"] == "tile128"
    assert cl["short_t1"] == cl["short_t15_cout29"] == cl["short_t16_cout33_n70"] == cl["short_t16_fout26"] == "short"
    assert cl["tile32_t17"] == cl["cin16_t16_not_short"] == "tile32"
    assert set(cl.values()) == {"short", "tile32", "tile128"}
    fw = {c.tag: (C.fwin_route(c, 0), C.fwin_route(c, 1)) for c in C.cases("fwin")}
    assert fw["kf15_sf2_t48"] == ("tile32", "tile32") and fw["kf41_t48_dt2"] == ("tile32", "tile32")
    assert fw["kf16_sf4_t49"] == ("shared", "tile128") and fw["kf41_sf4_fin81_nopad"] == ("shared", "tile128")
    assert fw["kf17_sf2_t128_st2"] == fw["kf41_sf2_t129_fin80"] == fw["ds2_fin81_tin301"] == ("shared", "tile128")
    for c1, c2 in PAIRS:
        assert C.fwin_route(c1) == "shared" and c1.Cout % 16 == 0 and C.cl_route(c2) in ("tile32", "tile128")
    # a 96-channel consumer at 11 taps has no tile
    assert C.cl_tile(2, 96 // 8, 20, 65, 11, 1, 1, 32) == 0
    iso = {c.tag: (C.cl_route(c) if c.entry == "cl" else C.fwin_route(c)) for e in ("cl", "fwin") for c in C.isolation_cases(e)}
    assert iso == {"iso_cl_kt11": "tile128", "iso_cl_short": "short", "iso_cl_t40_st2": "tile32", "iso_fwin_kf41": "shared",
                   "iso_fwin_kf17_t40": "tile32"}


@pytest.mark.parametrize("c", ISO_CASES, ids=ident)
def test_reads_marks_exactly_the_outputs_that_an_input_changes(c):
    x, w, b = C.make(c, "dense")
    assert c.act is None and np.all(w != 0) and any(v < c.Tin for v in C.eff_lens(c))
    base = C.want(c, "dense")
    pos = C.isolation_positions(c)
    labels = " ".join(p[0] for p in pos)
    assert "last_real_frame" in labels and "utterance0" in labels and "last_channel" in labels
    if c.KT % 2:
        assert "one_tap_past" in labels
    if c.entry == "fwin":
        assert "row_under_window" in labels
    unmarked_neighbour = 0
    for label, n, ch, f, t in pos:
        xb = x.copy()
        xb[n, ch, f, t] += 1
        marked = C.reads(c, n, ch, f, t)
        assert np.array_equal(C.case_reference(c, xb, w, b) != base, marked), label
        assert marked.any() and not marked[[m for m in range(c.N) if m != n]].any()
        if label.startswith("one_tap_past"):
            to = int(label.split("to")[-1])
            assert not marked[:, :, :, to].any()
            unmarked_neighbour += 1
    assert unmarked_neighbour or c.KT % 2 == 0
    # a masked frame is read by nobody
    n = c.N - 1
    assert not C.reads(c, n, 0, 0, C.eff_lens(c)[n]).any()
    xb = x.copy()
    xb[n, :, :, C.eff_lens(c)[n]:] += 1
    assert np.array_equal(C.case_reference(c, xb, w, b), base)


@pytest.mark.parametrize("c", [c for e in ENTRIES for c in C.clamped_isolation_cases(e)], ids=ident)
def test_the_isolation_clamp_cuts_some_outputs_and_not_all(c):
    """The clamped isolation cases share the draw of the unclamped ones; np.clip, which their device check uses as the
    definition, keeps NaN and maps the infinities to the limits."""
    plain = [p for p in C.isolation_cases(c.entry) if p.tag + "_clamp" == c.tag][0]
    assert all(np.array_equal(a, b) for a, b in zip(C.make(c, "dense"), C.make(plain, "dense")))
    raw, lo, hi = C.want(plain, "dense"), c.act[0], c.act[1]
    assert (raw < lo).any() and (raw > hi).any() and ((raw > lo) & (raw < hi)).any()
    assert np.array_equal(C.want(c, "dense"), np.clip(raw, lo, hi))
    out = np.clip(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), np.float32(lo), np.float32(hi))
    assert out.dtype == np.float32 and np.isnan(out[0]) and out[1] == hi and out[2] == lo
