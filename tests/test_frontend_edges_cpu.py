"""tests/frontend_cases.py proven without a GPU: every float64 reference against oracle/frontend_oracle.py and against torch
where torch has the operation (std, reflect pad, clamp / max), the case tables against the edges they were written for, a
float32 restatement of each toleranced operator against at most HALF of its derived bound, and the non-finite rule of the
MFCC pinned on the oracle."""
import numpy as np
import pytest
import torch

import frontend_cases as C
from oracle import frontend_oracle as FO

f32 = np.float32


# ----------------------------------------------------------------------------- MFCC: tables, reference, rule
def test_mfcc_tables_are_the_oracles_and_the_products():
    from myrtlespeech_amd.data.preprocess import MFCC
    for n_fft, win, n_mels, n_mfcc in ((32, 32, 8, 8), (32, 20, 8, 5), (33, 33, 8, 8), (400, 400, 128, 80), (400, 320, 128, 13),
                                       (32, 32, 128, 13)):
        window, dft, fb, dct = C.mfcc_tables(n_fft, win, n_mels, n_mfcc)
        nf = n_fft // 2 + 1
        want_w = np.zeros(n_fft, dtype=f32)
        want_w[(n_fft - win) // 2:(n_fft - win) // 2 + win] = FO.hann_window(win)
        assert C.same_bits(window, want_w)
        assert C.same_bits(fb, np.ascontiguousarray(FO.mel_filterbank(nf, 0.0, 8000.0, n_mels).T))
        assert C.same_bits(dct, np.ascontiguousarray(FO.create_dct(n_mfcc, n_mels).T))
        x = C.rng_of(("dft", n_fft)).standard_normal(n_fft)
        spec, ref = dft.astype(np.float64) @ x, np.fft.rfft(x)
        assert np.allclose(spec[:nf], ref.real, atol=1e-4) and np.allclose(spec[nf:], ref.imag, atol=1e-4)
        tw, td, tf, tc = MFCC(n_mfcc=n_mfcc, melkwargs=dict(n_fft=n_fft, win_length=win, hop_length=8, n_mels=n_mels)).tables()
        assert np.allclose(window, tw.numpy(), atol=1e-6) and np.array_equal(dft, td.numpy())
        assert np.allclose(fb, tf.numpy(), atol=1e-4) and np.allclose(dct, tc.numpy(), atol=1e-6)
    assert (C.mfcc_tables(32, 32, 128, 13)[2].sum(1) == 0).any(), "n_mels = 128 over 17 bins has empty triangles"


def test_mfcc_frame_index_is_torch_reflect_pad():
    for n_fft, hop, L in ((32, 8, 17), (32, 8, 64), (32, 8, 65), (32, 8, 71), (400, 160, 201), (400, 160, 1120), (33, 8, 61)):
        x = torch.arange(L, dtype=torch.float32)
        padded = torch.nn.functional.pad(x[None, None], (n_fft // 2, n_fft // 2), mode="reflect")[0, 0].numpy()
        nfr = 1 + L // hop
        idx = C._frame_index(L, nfr, n_fft, hop)
        want = np.stack([padded[t * hop:t * hop + n_fft] for t in range(nfr)])
        assert np.array_equal(idx, want.astype(np.int64)), (n_fft, hop, L)
    # an odd n_fft with len % hop == 0: the last frame's last tap lies one sample beyond torch's padding and mirrors on
    idx = C._frame_index(64, 9, 33, 8)
    assert idx[8, 32] == 2 * 63 - (64 - 16 + 32) and idx.min() >= 0 and idx.max() <= 63


def test_mfcc_case_table_covers_its_edges():
    for cid, (g, lens, ms, top_db, kind) in C.MFCC_CASES.items():
        assert min(lens) > g["n_fft"] // 2 and max(lens) <= ms and g["n_mfcc"] <= g["n_mels"] and g["win"] <= g["n_fft"], cid
    g, lens, ms, _, _ = C.MFCC_CASES["reflect32"]
    assert lens[0] == g["n_fft"] // 2 + 1 and sorted(l % g["hop"] for l in lens[1:]) == [0, 1, g["hop"] - 1]
    assert g["n_mfcc"] == g["n_mels"]
    g, lens, _, _, _ = C.MFCC_CASES["full400"]
    assert {0, 1, g["hop"] - 1} <= {l % g["hop"] for l in lens} and lens[0] == 201
    shapes = {(C.mfcc_frames(ms, g["hop"]), g["n_mfcc"]) for cid, (g, _, ms, _, _) in C.MFCC_CASES.items() if cid.startswith("tile_")}
    assert shapes == {(T, c) for T in C.TILE_SIZES for c in C.TILE_SIZES}
    assert C.MFCC_CASES["tile_T33_c33"][0]["n_mfcc"] == C.MFCC_CASES["tile_T33_c33"][0]["n_mels"]
    assert C.MFCC_CASES["odd_nfft"][0]["n_fft"] % 2 == 1 and C.MFCC_CASES["win_lt_nfft"][0]["win"] < 32
    w = C.mfcc_case("zero_utterance")[1]
    assert not w[0, :60].any() and np.isnan(w[0, 60:]).all()
    for cid, (g, lens, ms) in C.OVERSIZE_CASES.items():
        assert max(lens) > ms and C.mfcc_frames(max(lens), g["hop"]) > C.mfcc_frames(ms, g["hop"])


def oracle_mfcc(wave, L, g, top_db):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return FO.mfcc(wave[None, :L], g["n_mfcc"], g["win"], g["hop"], n_fft=g["n_fft"], n_mels=g["n_mels"],
                       top_db=top_db if top_db >= 0 else None)[0]


def mfcc_f32(wave, L, tables, hop, top_db):
    """The kernels' arithmetic in float32 numpy: window product, three float32 matrix products (in the order of the BLAS at
    hand), re^2 + im^2, 10 log10(select) , the floor by select, all rounded to float32 at every step."""
    window, dft, fb, dct = tables
    nf = fb.shape[1]
    fr = window[None, :] * wave[C._frame_index(L, 1 + L // hop, window.size, hop)]
    spec = fr @ dft.T
    re, im = spec[:, :nf], spec[:, nf:]
    pw = re * re + im * im
    mel = pw @ fb.T
    db = f32(10.0) * np.log10(np.where(mel < C.AMIN, C.AMIN, mel))
    if top_db >= 0:
        floor = db.max() - f32(top_db)
        db = np.where(db > floor, db, floor)
    cep = db @ dct.T
    assert cep.dtype == f32
    return cep.T


def test_mfcc_reference_against_the_oracle_and_the_float32_restatement_inside_half_the_bound():
    """The oracle (float64 rfft, float32 everywhere else) and the stage-by-stage float32 restatement both stay within half of
    the derived bound of the float64 reference on every case, every element, padding included; every bound is finite.
    Largest share: see the cases file's docstring."""
    worst_o = worst_r = 0.0
    for cid in C.MFCC_CASES:
        tables, wave, lens, hop, top_db = C.mfcc_case(cid)
        g = C.MFCC_CASES[cid][0]
        ref, bound = C.mfcc_ref(wave, lens, tables, hop, top_db, with_bound=True)
        assert np.isfinite(ref).all() and np.isfinite(bound).all(), cid
        scale = np.abs(ref).max()          # cepstra of dB values: hundreds
        assert bound.max() < 1e-2 * scale and np.median(bound[bound > 0]) < 1e-3 * scale, (cid, "a bound this wide checks little")
        got_o, got_r = np.zeros_like(ref), np.zeros_like(ref)
        for n, L in enumerate(lens):
            nfr = 1 + L // hop
            assert not ref[n, :, nfr:].any() and not bound[n, :, nfr:].any()
            got_r[n, :, :nfr] = mfcc_f32(wave[n], L, tables, hop, top_db)
            got_o[n, :, :nfr] = oracle_mfcc(wave[n], L, g, top_db) if cid != "odd_nfft_extra_frame" else got_r[n, :, :nfr]
        valid = bound > 0
        worst_o = max(worst_o, float(np.max(np.abs(got_o - ref)[valid] / bound[valid])))
        worst_r = max(worst_r, float(np.max(np.abs(got_r - ref)[valid] / bound[valid])))
        assert np.all(np.abs(got_o - ref) <= 0.5 * bound), (cid, "oracle")
        assert np.all(np.abs(got_r - ref) <= 0.5 * bound), (cid, "restatement")
    print("MFCC worst error / bound: oracle", worst_o, "float32 restatement", worst_r)
    assert 0 < worst_r <= 0.5 and 0 < worst_o <= 0.5


def test_mfcc_floors_are_active_in_the_cases_written_for_them():
    tables, wave, lens, hop, top_db = C.mfcc_case("silent_stretch")
    with_floor = C.mfcc_ref(wave, lens, tables, hop, 80.0)
    without = C.mfcc_ref(wave, lens, tables, hop, -1.0)
    assert np.abs(with_floor - without).max() > 1.0, "the silent stretch lies below max - 80 dB"
    tables, wave, lens, hop, _ = C.mfcc_case("empty_triangles_no_floor")
    db0 = C.mfcc_ref(wave, lens, tables, hop, -1.0)
    assert np.isfinite(db0).all()
    mel = (tables[2].sum(1) == 0)
    assert mel.sum() > 50, "most of 128 triangles over 17 bins are empty: amin decides their dB"
    tables, wave, lens, hop, _ = C.mfcc_case("zero_utterance")
    z = C.mfcc_ref(wave, lens, tables, hop, 80.0)
    want = (np.full((1, 8), -100.0) @ tables[3].astype(np.float64).T)[0]
    assert np.allclose(z[0, :, :1 + 60 // 8], want[:, None], atol=1e-4), "silence is -100 dB in every band"


@pytest.mark.parametrize("cid", sorted(C.POISON_CASES))
def test_a_non_finite_sample_makes_its_whole_utterance_nan_in_the_oracle_and_the_reference(cid):
    """The rule the device is held to: for NaN, +Inf, -Inf and an overflowing 3e38 at the first, a middle and the last
    sample, torchaudio's pipeline as the oracle restates it (np.maximum and np.max, like torch.clamp and torch.max) gives NaN in
    EVERY feature of that utterance -- no kind or position is an exception.  The float64 reference agrees for NaN and +-Inf;
    3e38 overflows only in float32, so for it the rule is the oracle's and the reference stays finite."""
    g, lens, ms = C.POISON_CASES[cid]
    tables = C.mfcc_tables(g["n_fft"], g["win"], g["n_mels"], g["n_mfcc"])
    clean = C.mfcc_wave(cid, lens, ms)
    L = lens[1]
    assert np.isfinite(oracle_mfcc(clean[1], L, g, 80.0)).all()
    for kind, value in C.POISON_KINDS.items():
        for where in C.POISON_AT:
            w = clean.copy()
            w[1, C.poison_position(L, where)] = value
            assert np.isnan(oracle_mfcc(w[1], L, g, 80.0)).all(), (cid, kind, where, "oracle")
            ref = C.mfcc_ref(w, np.array(lens), tables, g["hop"], 80.0)
            nfr = 1 + L // g["hop"]
            if kind == "big":       # 3e38 squared overflows float32 (the oracle's and the device's power), not float64
                assert np.isfinite(ref).all()
            else:
                assert np.isnan(ref[1, :, :nfr]).all() and not ref[1, :, nfr:].any(), (cid, kind, where)
            assert np.isfinite(ref[0]).all() and np.isfinite(ref[2]).all()
    # torch agrees on the two selects: clamp(min) and max keep a NaN, fmaxf would drop it
    t = torch.tensor([float("nan"), 1e-12, 3.0])
    assert torch.isnan(torch.clamp(t, min=1e-10)[0]) and torch.isnan(torch.max(t, torch.tensor(0.5))[0]) and torch.isnan(t.max())


def test_oversized_lengths_mean_max_samples_in_the_reference():
    for cid, (g, lens, ms) in C.OVERSIZE_CASES.items():
        tables = C.mfcc_tables(g["n_fft"], g["win"], g["n_mels"], g["n_mfcc"])
        wave = C.mfcc_wave(cid, lens, ms)
        assert np.isfinite(wave[int(np.argmax(lens))]).all()
        a = C.mfcc_ref(wave, np.array(lens), tables, g["hop"], 80.0)
        b = C.mfcc_ref(wave, np.minimum(np.array(lens), ms), tables, g["hop"], 80.0)
        assert np.array_equal(a, b) and np.isfinite(a).all()


# ----------------------------------------------------------------------------- Standardize
@pytest.mark.filterwarnings("ignore:std", "ignore:Degrees of freedom")      # the one-element utterances: NaN on purpose
def test_standardize_reference_is_torch_std_and_the_oracle_inside_half_the_bound():
    """float64 torch ((x - mean) / std, unbiased) within 1e-9 relative of the reference; the oracle (float32 mean and std,
    float32 subtraction and division: the kernel's arithmetic) within half of the bound on every case."""
    worst = 0.0
    for cid, (N, inner, T, _, mean, dev) in C.STD_CASES.items():
        x, lens = C.standardize_input(cid)
        ref, bound = C.standardize_ref(x, lens, with_bound=True)
        got = np.zeros_like(ref)
        for n in range(N):
            L = min(int(lens[n]), T)
            assert not ref[n, :, max(L, 0):].any()
            if L <= 0:
                continue
            v = x[n, :, :L]
            assert np.isfinite(v).all() and (L == T or np.isnan(x[n, :, L:]).all())
            t = torch.from_numpy(v.astype(np.float64))
            want = ((t - t.mean()) / t.std()).numpy()
            if v.size == 1:
                assert np.isnan(want).all() and np.isnan(ref[n, :, :L]).all()
            else:
                assert np.all(np.abs(ref[n, :, :L] - want) <= 1e-9 * (1 + np.abs(want))), (cid, n)
            with np.errstate(invalid="ignore", divide="ignore"):
                got[n, :, :L] = FO.standardize(v)
        worst = max(worst, C.check(got, ref, 0.5 * bound, ("standardize", cid)))
    print("Standardize worst error / half bound", worst, "-> of the bound", worst / 2)
    assert 0 < worst <= 1.0
    x, lens = C.standardize_input("lens_inner1")
    assert lens.tolist() == [0, 1, 8, 9, 14, -3] and np.isnan(C.standardize_ref(x, lens)[1, 0, 0])
    sizes = {cid: inner * T for cid, (_, inner, T, _, _, _) in C.STD_CASES.items()}
    assert sizes["one_element"] == 1 and sizes["below_one_block"] == 4095 and sizes["above_one_block"] == 4097
    assert sizes["above_block_cap"] > 512 * 4096
    x, _ = C.standardize_input("offset_far_above_spread")
    assert abs(x[0].mean() - 1e4) < 1 and 5e-3 < x[0].std() < 2e-2


# ----------------------------------------------------------------------------- AddContextFrames
def test_context_reference_is_the_oracle_on_every_utterance():
    seen_T, seen = set(), set()
    for F, T, c in C.CTX_CASES:
        x, lens = C.context_input(F, T, c)
        assert sorted(lens.tolist()) == sorted([0, 1, T - 1, T, T + 5, -3])
        want = C.context_ref(x, lens, c)
        assert want.shape == (6, 2 * c + 1, F, T)
        for n in range(6):
            L = min(max(int(lens[n]), 0), T)
            assert np.all(C.bits(want[n, :, :, L:]) == 0), "every t >= len is +0.0"
            if L:
                solo = FO.add_context_frames(x[n:n + 1, :, :L], c)
                assert C.same_bits(np.ascontiguousarray(want[n, :, :, :L]), solo), (F, T, c, n)
            assert not np.any(C.bits(want[n]) == C.bits(np.array([C.NAN_PAYLOAD]))[0]), "the padding's poison never appears"
        if T > 30:
            assert np.isnan(want).any() and np.isinf(want).any()
        seen_T.add(T)
        seen.add((c == 0, c >= T, F == 1))
    assert {255, 256, 257} <= seen_T and any(s[0] for s in seen) and any(s[1] for s in seen) and any(s[2] for s in seen)


# ----------------------------------------------------------------------------- SpecAugment
def test_spec_reference_is_the_oracles_zeroing_and_the_cases_hold_their_edges():
    for cid, (Cn, F, T, fb, tb) in C.SPEC_CASES.items():
        x = C.spec_input(cid)
        want = C.spec_ref(x, fb, tb)
        for n in range(2):
            y = x[n].copy()
            for s, w in (fb[n] if fb else ()):           # FO.spec_augment's two loops on the drawn bands
                y[:, s:s + w, :] = 0
            for s, w in (tb[n] if tb else ()):
                y[:, :, s:s + w] = 0
            assert C.same_bits(want[n], y), cid
        changed = C.bits(want) != C.bits(x)
        assert np.all(C.bits(want)[changed] == 0), "what changes becomes +0.0"
        if cid == "zero_width":
            assert not changed.any()
        if cid in ("overlapping", "past_T"):
            assert np.isnan(x[changed]).any() and np.isnan(want[~changed]).any()
    assert C.SPEC_CASES["start_at_the_end"][3][0][0][0] == C.SPEC_CASES["start_at_the_end"][1]
    assert C.SPEC_CASES["start_at_the_end"][4][0][0][0] == C.SPEC_CASES["start_at_the_end"][2]
    assert {C.SPEC_CASES[c][0] for c in C.SPEC_CASES} == {1, 3}


# ----------------------------------------------------------------------------- MFCCLegacy
def legacy_f64_other_order(wave, L, tables, frame_len, frame_step, nfft, preemph=0.97):
    """The kernel's float64 arithmetic in another order (numpy's rfft instead of the direct sums), rounded to float32."""
    twiddle, fbank, dct, lifter = tables
    x = C.legacy_int16(wave[:L])
    sig = np.append(x[0], x[1:] - preemph * x[:-1])
    nfr = C.legacy_frames(L, frame_len, frame_step)
    padded = np.concatenate([sig, np.zeros((nfr - 1) * frame_step + frame_len - L)])
    frames = np.stack([padded[t * frame_step:t * frame_step + frame_len] for t in range(nfr)])
    p = np.square(np.abs(np.fft.rfft(frames, nfft))) / nfft
    eps = np.finfo(float).eps
    energy = p.sum(1)
    feat = p @ fbank.T
    cep = (np.log(np.where(feat == 0, eps, feat)) @ dct.T) * lifter
    cep[:, 0] = np.log(np.where(energy == 0, eps, energy))
    return cep.astype(f32).T


def test_legacy_reference_against_the_oracle_and_inside_half_the_bound():
    """On the shipped geometry the oracle (python_speech_features restated, its own tables) is within half of the bound; on
    every geometry, nfft < frame_len included, so is the same arithmetic in numpy's rfft order.  Every bound is finite and
    below 1e-4: nothing is excused by a wide bound."""
    worst = 0.0
    for cid, (frame_len, frame_step, nfft, nfilt, numcep, lens, ms) in C.LEGACY_CASES.items():
        tables = C.legacy_tables(nfft, nfilt, numcep)
        wave = C.legacy_wave(cid)
        ref, bound = C.legacy_ref(wave, lens, tables, frame_len, frame_step, nfft, with_bound=True)
        assert np.isfinite(ref).all() and np.isfinite(bound).all() and bound.max() < 1e-4, (cid, bound.max())
        got = np.zeros_like(ref)
        for n, L in enumerate(lens):
            L = min(L, ms)
            nfr = C.legacy_frames(L, frame_len, frame_step)
            assert not ref[n, :, nfr:].any()
            got[n, :, :nfr] = legacy_f64_other_order(wave[n], L, tables, frame_len, frame_step, nfft)
            if cid == "shipped":
                o = FO.mfcc_legacy(wave[n:n + 1, :L], numcep, frame_len, frame_step)[0]
                assert np.all(np.abs(o - ref[n, :, :nfr]) <= 0.5 * bound[n, :, :nfr]), (cid, n, "oracle")
        valid = bound > 0
        worst = max(worst, float(np.max(np.abs(got - ref)[valid] / bound[valid])))
        assert np.all(np.abs(got - ref) <= 0.5 * bound), cid
    print("MFCCLegacy worst error / bound", worst)
    assert 0 < worst <= 0.5


def test_legacy_cases_hold_their_edges():
    frame_len, frame_step, nfft, nfilt, numcep, lens, ms = C.LEGACY_CASES["small"]
    assert lens[:3] == (1, frame_len, frame_len + 1) and (lens[3] - frame_len) % frame_step != 0
    assert C.LEGACY_CASES["rfft_truncates"][2] < C.LEGACY_CASES["rfft_truncates"][0]
    assert np.array_equal(C.legacy_tables(512, 26, 13)[1], FO.psf_filterbanks(26, 512, 16000))
    assert C.legacy_int16(np.array([1.0, -1.0, 1e-5, -2e-5, 0.5], dtype=f32)).tolist() == [-32768.0, -32768.0, 0.0, 0.0, 16384.0]
    for cid in C.LEGACY_CASES:
        frame_len, frame_step, nfft, nfilt, numcep, lens, ms = C.LEGACY_CASES[cid]
        w = C.legacy_wave(cid)
        assert (np.abs(w) == 1.0).any() and ((w != 0) & (np.abs(w) < 1 / 32768)).any()
        for n, L in enumerate(lens):
            assert np.all(w[n, min(L, ms):] == C.LEGACY_PAD)
        if len(lens) > 3:      # an all-zero frame (both eps branches) next to frames with signal
            tables = C.legacy_tables(nfft, nfilt, numcep)
            ref = C.legacy_ref(w, lens, tables, frame_len, frame_step, nfft)
            assert np.any(np.isclose(ref[3, 0], np.log(np.finfo(float).eps))), cid
    assert (C.legacy_tables(32, 8, 8)[1].sum(1) == 0).any(), "an empty filter: the feat == 0 branch inside a live frame"
    # a leak of the 0.999 padding into any frame changes the features: the reference on a zero-padded copy differs where
    # the padding is read, and equals where it is not
    frame_len, frame_step, nfft, nfilt, numcep, lens, ms = C.LEGACY_CASES["oversize"]
    w = C.legacy_wave("oversize")
    tables = C.legacy_tables(nfft, nfilt, numcep)
    assert np.array_equal(C.legacy_ref(w, lens, tables, frame_len, frame_step, nfft),
                          C.legacy_ref(w, np.minimum(lens, ms), tables, frame_len, frame_step, nfft))
