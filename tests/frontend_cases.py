"""Cases, inputs, float64 references and error bounds of the feature front end (csrc/frontend.hip):

    ms_mfcc_forward, ms_standardize_forward, ms_context_frames_forward, ms_spec_augment_, ms_mfcc_legacy_forward

numpy only; imports nothing from the package (the shared helpers come from tests/small_ops_cases.py, whose rules hold here:
E = 2^-23 is charged per float32 operation, G(k) bounds k stacked operations and a sum of k terms in ANY order, SECOND carries
the neglected second-order terms).  tests/test_frontend_edges_cpu.py proves the references against oracle/frontend_oracle.py and
torch and holds a float32 restatement of each toleranced operator to half of its bound; tests/test_frontend_edges_gpu.py runs the
cases through the C ABI.  AddContextFrames and SpecAugment move values without arithmetic: equality of bits.

MFCC (mfcc_ref, mfcc_bound).  The reference takes the float32 tables the device gets (window, DFT basis, mel filterbank, DCT),
widened to float64, so the bound measures the kernels' arithmetic and not the construction of the tables.  It follows the ABI's
own definitions: 1 + len / hop frames, sample index t hop + j - n_fft / 2 mirrored at 0 and at len - 1 (for an even n_fft that is
torch.stft(center=True, pad_mode="reflect"); an odd n_fft with len % hop == 0 has one frame more than torch.stft, whose last
tap lies one sample beyond torch's padding), lengths above max_samples count as max_samples.  Stage by stage, D. being the
bound of the stage's error:

    f_j   = w_j x_s                                  one product:             D f_j  = E |f_j|
    re_k  = sum_j f_j c_kj   (im_k alike)            K = n_fft:               D re_k = G(n_fft + 1) sum_j |f_j| |c_kj|
    p_k   = re_k^2 + im_k^2                          two roundings per term:  D p_k  = 2 |re_k| D re_k + 2 |im_k| D im_k
                                                                                       + G(2) p_k   (+ D re^2 + D im^2: re may
                                                                                       cancel to nothing, so not second order)
    mel_m = sum_k p_k b_mk,  b >= 0                  K = n_fft / 2 + 1:       D mel_m = sum_k b_mk D p_k + G(n_fft / 2 + 1) mel_m
    db_m  = 10 log10f(max(mel_m, amin))              max is 1-Lipschitz, so the clamped value c' lies in
                                                     [max(amin, c - D mel), c + D mel]; log10 turns that relative error into
                                                     the absolute 10 max(log10((c + D) / c), log10(c / max(amin, c - D))),
                                                     finite whatever D is, so the amin clamp needs no exclusion list; log10f
                                                     (2 ulp in the HIP math documentation), the product and the offset add
                                                     G(ULP_LOG10 + 2) |db_m|
    floor = max_valid db - top_db                    max is 1-Lipschitz, and only a candidate (db_i + D db_i >= max_j (db_j -
                                                     D db_j)) can be the other side's maximum, while the reference's own
                                                     arg max is one: D floor = max_candidates D db + E |floor|
    db'_m = max(db_m, floor)                         |max(a, b) - max(a', b')| <= max(|a - a'|, |b - b'|); where db_m - D db_m >
                                                     floor + D floor both sides take db_m and D db'_m = D db_m, elsewhere
                                                     D db'_m = max(D db_m, D floor): no exclusion list for the floor either
    cep_c = sum_m db'_m d_cm                         K = n_mels:              D cep_c = sum_m |d_cm| D db'_m
                                                                                        + G(n_mels) sum_m |db'_m| |d_cm|

every sum in any order, fused or not; each stage's absolute allowance also carries 2^-126 per operation for results that
underflow.  SECOND is applied to D mel before the logarithm and to D cep.  Non-finite rule (pinned on the oracle by the CPU
test): a NaN, a +-Inf or an overflowing 3e38 sample makes every valid feature of its utterance NaN under a top_db floor
(the poisoned frame is NaN after the mel product, 0 Inf being NaN; np.max and np.maximum carry it to every frame), and leaves
every other utterance alone.  3e38 overflows in the float32 power only, so mfcc_ref (float64) stays finite for it: the rule
is the float32 oracle's, and the GPU test asserts the rule itself, not mfcc_ref, on the poisoned utterance.

Standardize (standardize_ref, standardize_bound).  mean and variance are accumulated in float64 over count = inner len
elements (two passes, any order: relative errors of order count 2^-52), then mean and sd are rounded to float32 and
y = (x - mean) / sd takes a subtraction and a division: with mu, sigma the exact moments

    |y - ref| <= SECOND (E |mu| / sigma + G(3) |y|) + 2^-52 (count + 4) (mean |x| / sigma + |y|)

the first term is the float32 rounding of the mean, which torch's own float32 path pays too (at mean 1e4, deviation 1e-2 it is
0.12: the input itself is quantised to a tenth of sigma).  inner len == 1 is NaN like torch (0 / 0), len <= 0 is all zeros.

MFCCLegacy (legacy_ref, legacy_bound): float64 on the device, float32 only at the store: E |ref| plus the float64 terms with
D64 = 2^-52 per operation: re_k over `used` taps G64(used + 1) sum |frame| |tw|; p_k as above (with its square term) / nfft;
feat_m = sum_k p_k fb_mk: sum fb D p + G64(nbins) feat; log: D feat / (feat - D feat) + ULP_LOG D64 |log feat| (double log:
1 ulp); cep_c = lifter_c sum_m feat_m dct_cm: |lifter_c| (sum |dct| D logfeat + G64(nfilt + 2) sum |logfeat| |dct|);
c0 = log(energy) alike.  The two eps branches compare with exactly 0.0, which both sides reach only through exact zeros
(an all-zero frame, an empty filter); the inputs contain no frame that cancels to nearly nothing, and the CPU test asserts
that every bound of every case is finite and small, so nothing is left out through an infinite bound.  NaN samples are outside
this path's contract and are not tested.

Measured shares (largest error / bound over all cases of an operator):
    float32 restatement on the CPU (must stay <= 0.5):   MFCC 0.088 (the oracle: 0.088)   Standardize 0.42   MFCCLegacy 0.485
    kernels on the MI355X:                               MFCC 0.088                       Standardize 0.42   MFCCLegacy 0.485
The MFCC's largest share is the all-zero utterance (10 log10f(1e-10f) times the DCT, the same roundings on both machines);
at n_fft = 400 the any-order bound of a 400-term sum is far from a real summation (0.003 used).  Standardize's is the rounding
of the mean, MFCCLegacy's the rounding of the float32 store: a correctly rounded result uses half of the charged ulp, which is
why both sit just below one half.
"""
import numpy as np

from small_ops_cases import E, G, SECOND, ULP_LOG, bits, check_toleranced, rng_of, same_bits, same_bits_or_both_nan  # noqa: F401

D64 = 2.0 ** -52
UNDER = 2.0 ** -126
ULP_LOG10 = 2                                  # maximum ulp error of log10f in the HIP math documentation
AMIN = np.float32(1e-10)
POISON_KINDS = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf, "big": 3e38}
POISON_AT = ("first", "middle", "last")
NAN_PAYLOAD = np.array([0x7fc0dead], dtype=np.uint32).view(np.float32)[0]     # padding poison with a payload of its own


def G64(k):
    return k * D64 / (1.0 - k * D64)


def check(got, ref, bound, what):
    """check_toleranced on EVERY element (where the bound is 0, the padding, that means equality; and there the bits must be
    +0.0); returns the largest error / bound over the elements whose bound is positive (0 if there is none)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        check_toleranced(got, ref, bound, what)
    exact = bound == 0
    assert not np.any(bits(np.asarray(got))[exact & (ref == 0)]), (what, "a padding element is not +0.0")
    live = np.isfinite(ref) & (bound > 0) & np.isfinite(bound)
    if not live.any():
        return 0.0
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)[live] / bound[live]))


# ----------------------------------------------------------------------------- MFCC
def mfcc_tables(n_fft, win_length, n_mels, n_mfcc, sample_rate=16000):
    """(window [n_fft], dft [2 (n_fft/2+1), n_fft], mel_fb [n_mels, n_fft/2+1], dct [n_mfcc, n_mels]) float32, laid out as the
    ABI takes them: the periodic Hann window centred in n_fft, cos rows then -sin rows with the angle reduced exactly, HTK mel
    triangles over 0 .. sample_rate / 2, the orthonormal DCT-II."""
    f = np.float32
    nf = n_fft // 2 + 1
    window = np.zeros(n_fft, dtype=f)
    left = (n_fft - win_length) // 2
    window[left:left + win_length] = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)).astype(f)
    kj = (np.arange(nf)[:, None] * np.arange(n_fft)[None, :]) % n_fft
    ang = kj * (2.0 * np.pi / n_fft)
    dft = np.concatenate([np.cos(ang), -np.sin(ang)]).astype(f)
    all_freqs = np.linspace(0.0, sample_rate // 2, nf, dtype=f)
    m_pts = np.linspace(0.0, 2595.0 * np.log10(1.0 + (sample_rate // 2) / 700.0), n_mels + 2, dtype=f)
    f_pts = (f(700.0) * (np.power(f(10.0), m_pts / f(2595.0)) - f(1.0))).astype(f)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    fb = np.maximum(f(0.0), np.minimum((f(-1.0) * slopes[:, :-2]) / f_diff[:-1], slopes[:, 2:] / f_diff[1:])).astype(f)
    n = np.arange(n_mels, dtype=f)
    k = np.arange(n_mfcc, dtype=f)[:, None]
    dct = np.cos(f(np.pi / float(n_mels)) * (n + f(0.5)) * k).astype(f)
    dct[0] *= f(1.0 / np.sqrt(2.0))
    dct *= f(np.sqrt(2.0 / float(n_mels)))
    return window, np.ascontiguousarray(dft), np.ascontiguousarray(fb.T), np.ascontiguousarray(dct)


def mfcc_frames(max_samples, hop):
    return 1 + max_samples // hop


def _frame_index(L, nfr, n_fft, hop):
    s = np.arange(nfr)[:, None] * hop + np.arange(n_fft)[None, :] - n_fft // 2
    s = np.where(s < 0, -s, s)
    s = np.where(s >= L, 2 * (L - 1) - s, s)
    return np.clip(s, 0, L - 1)


def _mfcc_stages(x, L, tables, hop, top_db, with_bound):
    """One utterance (x float32 [>= L]) in float64: (cep [nfr, n_mfcc], its bound or None)."""
    window, dft, fb, dct = (t.astype(np.float64) for t in tables)
    n_fft, nf, n_mels = window.size, fb.shape[1], fb.shape[0]
    nfr = 1 + L // hop
    amin = np.float64(AMIN)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        fr = window[None, :] * x.astype(np.float64)[_frame_index(L, nfr, n_fft, hop)]
        spec = fr @ dft.T
        re, im = spec[:, :nf], spec[:, nf:]
        pw = re * re + im * im
        mel = pw @ fb.T
        c = np.maximum(mel, amin)
        db = 10.0 * np.log10(c)
        floor = np.max(db) - top_db if top_db >= 0 else -np.inf
        dbf = np.maximum(db, floor) if top_db >= 0 else db
        cep = dbf @ dct.T
        if not with_bound:
            return cep, None
        aspec = np.abs(fr) @ np.abs(dft).T
        d_spec = G(n_fft + 1) * aspec + (n_fft + 1) * UNDER
        d_re, d_im = d_spec[:, :nf], d_spec[:, nf:]
        d_pw = 2 * np.abs(re) * d_re + 2 * np.abs(im) * d_im + d_re ** 2 + d_im ** 2 + G(2) * pw + 3 * UNDER
        d_mel = SECOND * (d_pw @ fb.T + G(nf) * mel + nf * UNDER)
        d_db = 10.0 * np.maximum(np.log10((c + d_mel) / c), np.log10(c / np.maximum(amin, c - d_mel))) \
            + G(ULP_LOG10 + 2) * np.abs(db)
        if top_db >= 0:
            candidates = db + d_db >= np.max(db - d_db)               # only these can be the maximum on the other side
            d_floor = np.max(d_db[candidates]) + E * abs(floor)
            d_dbf = np.where(db - d_db > floor + d_floor, d_db, np.maximum(d_db, d_floor))
        else:
            d_dbf = d_db
        d_cep = SECOND * (d_dbf @ np.abs(dct).T + G(n_mels) * (np.abs(dbf) @ np.abs(dct).T))
    return cep, d_cep


def mfcc_ref(wave, lens, tables, hop, top_db, with_bound=False):
    """wave float32 [N, max_samples], lens [N] -> float64 [N, n_mfcc, T] (and the bound, alike): frames at and beyond
    1 + len / hop are 0, lengths above max_samples count as max_samples."""
    N, max_samples = wave.shape
    T = mfcc_frames(max_samples, hop)
    n_mfcc = tables[3].shape[0]
    out = np.zeros((N, n_mfcc, T))
    bound = np.zeros((N, n_mfcc, T))
    for n in range(N):
        L = min(int(lens[n]), max_samples)
        cep, d = _mfcc_stages(wave[n], L, tables, hop, top_db, with_bound)
        out[n, :, :cep.shape[0]] = cep.T
        if with_bound:
            bound[n, :, :cep.shape[0]] = d.T
    return (out, bound) if with_bound else out


def mfcc_wave(case_id, lens, max_samples, kind="speechlike", pad=NAN_PAYLOAD):
    """float32 [N, max_samples]: gaussians of deviation 0.1 whose middle third is 300 times quieter (so the top_db floor is
    active); ``silent_stretch``: that third is exactly zero; ``zero``: utterance 0 is all zeros.  Beyond each length: ``pad``."""
    r = rng_of(("mfcc", case_id))
    w = np.full((len(lens), max_samples), pad, dtype=np.float32)
    for n, L in enumerate(lens):
        L = min(L, max_samples)
        x = r.standard_normal(L) * 0.1
        a, b = L // 3, 2 * L // 3
        x[a:b] *= 0.0 if kind in ("silent_stretch", "zero") else 1.0 / 300
        if kind == "zero" and n == 0:
            x[:] = 0.0
        w[n, :L] = x.astype(np.float32)
    return w


def geometry(n_fft, win, hop, n_mels, n_mfcc):
    return dict(n_fft=n_fft, win=win, hop=hop, n_mels=n_mels, n_mfcc=n_mfcc)


# id -> (geometry, lens, max_samples, top_db, kind)
MFCC_CASES = {
    # the smallest legal length (both mirrors in one frame), len % hop = 0, 1, hop - 1; n_mfcc == n_mels
    "reflect32": (geometry(32, 32, 8, 8, 8), (17, 64, 65, 71), 75, 80.0, "speechlike"),
    "win_lt_nfft": (geometry(32, 20, 8, 8, 5), (17, 50, 77), 77, 80.0, "speechlike"),
    "odd_nfft": (geometry(33, 33, 8, 8, 8), (17, 61, 67), 70, 80.0, "speechlike"),
    "odd_nfft_extra_frame": (geometry(33, 33, 8, 8, 8), (64, 24), 64, 80.0, "speechlike"),
    "full400": (geometry(400, 400, 160, 128, 80), (201, 1119, 1120, 1121, 640), 1300, 80.0, "speechlike"),
    "win_lt_400": (geometry(400, 320, 100, 128, 13), (201, 999, 1000, 1001), 1001, 80.0, "speechlike"),
    # n_mels = 128 over 17 bins: most triangles are empty, their energy is 0 and amin decides
    "empty_triangles": (geometry(32, 32, 8, 128, 13), (90, 41, 17), 90, 80.0, "speechlike"),
    "empty_triangles_no_floor": (geometry(32, 32, 8, 128, 13), (90, 41, 17), 90, -1.0, "speechlike"),
    "zero_utterance": (geometry(32, 32, 8, 8, 8), (60, 75, 41), 75, 80.0, "zero"),
    "zero_utterance_no_floor": (geometry(32, 32, 8, 8, 8), (60, 75, 41), 75, -1.0, "zero"),
    "silent_stretch": (geometry(32, 32, 8, 8, 8), (120, 75, 41), 120, 80.0, "silent_stretch"),
    "silent_stretch_no_floor": (geometry(400, 400, 160, 128, 80), (1600, 900), 1600, -1.0, "silent_stretch"),
    "silent_stretch400": (geometry(400, 400, 160, 128, 80), (1600, 900), 1600, 80.0, "silent_stretch"),
}
# the 32 x 32 transpose tile of the [frames, coefficients] -> [coefficients, T] pass: T and n_mfcc at 1, 31, 32, 33
TILE_SIZES = (1, 31, 32, 33)
for _T in TILE_SIZES:
    for _c in TILE_SIZES:
        _ms = 19 if _T == 1 else 20 * (_T - 1) + 3
        MFCC_CASES[f"tile_T{_T}_c{_c}"] = (geometry(32, 32, 20, 33, _c), (_ms, max(_ms - 23, 18)), _ms, 80.0, "speechlike")

# poison and oversized lengths: (geometry, lens, max_samples); utterance 1 is the victim
POISON_CASES = {"poison32": (geometry(32, 32, 8, 8, 8), (60, 75, 41), 75),
                "poison400": (geometry(400, 400, 160, 128, 80), (500, 700, 330), 700)}
OVERSIZE_CASES = {"oversize32": (geometry(32, 32, 8, 8, 8), (60, 75 + 9, 41), 75),
                  "oversize400": (geometry(400, 400, 160, 128, 80), (500, 330, 700 + 161), 700)}


def mfcc_case(case_id):
    """(tables, wave with NaN beyond every length, lens int32, hop, top_db)."""
    g, lens, max_samples, top_db, kind = MFCC_CASES[case_id]
    tables = mfcc_tables(g["n_fft"], g["win"], g["n_mels"], g["n_mfcc"])
    return tables, mfcc_wave(case_id, lens, max_samples, kind), np.array(lens, dtype=np.int32), g["hop"], top_db


def poison_position(L, where):
    return {"first": 0, "middle": L // 2, "last": L - 1}[where]


# ----------------------------------------------------------------------------- Standardize
def ragged_lens(T):
    return np.array([0, 1, T - 1, T, T + 5, -3], dtype=np.int32)


# id -> (N, inner, T, lens or None for ragged_lens(T), mean, deviation)
STD_CASES = {
    "lens_inner1": (6, 1, 9, None, 3.0, 5.0),                    # inner len == 1 at len 1: NaN like torch
    "lens_inner3": (6, 3, 40, None, 3.0, 5.0),
    "one_element": (2, 1, 1, (1, 1), 0.0, 1.0),
    "below_one_block": (2, 3, 1365, (1365, 1300), -2.0, 0.5),    # 4095 elements: one block of 256 threads x 16
    "above_one_block": (2, 1, 4097, (4097, 4000), -2.0, 0.5),
    "above_block_cap": (2, 2, 1048600, (1048600, 1048593), 1.0, 2.0),   # > 512 x 4096: the grid-stride loop runs again
    "offset_far_above_spread": (2, 4, 500, (500, 333), 1e4, 1e-2),
}


def standardize_input(case_id):
    """(x float32 [N, inner, T] with NaN (payload NAN_PAYLOAD) wherever t >= len, lens int32 [N])."""
    N, inner, T, lens, mean, dev = STD_CASES[case_id]
    lens = ragged_lens(T) if lens is None else np.array(lens, dtype=np.int32)
    x = (rng_of(("std", case_id)).standard_normal((N, inner, T)) * dev + mean).astype(np.float32)
    for n in range(N):
        x[n, :, max(int(lens[n]), 0):] = NAN_PAYLOAD
    return x, lens


def standardize_ref(x, lens, with_bound=False):
    """float64 [N, inner, T]: (x - mean) / std (unbiased) over t < min(len, T), +0.0 beyond; NaN where inner len == 1."""
    N, inner, T = x.shape
    out, bound = np.zeros(x.shape), np.zeros(x.shape)
    for n in range(N):
        L = min(int(lens[n]), T)
        if L <= 0:
            continue
        v = x[n, :, :L].astype(np.float64)
        count = v.size
        with np.errstate(invalid="ignore", divide="ignore"):
            mu = v.mean()
            sigma = np.sqrt(np.sum((v - mu) ** 2) / (count - 1.0)) if count > 1 else np.nan
            y = (v - mu) / sigma
            out[n, :, :L] = y
            bound[n, :, :L] = SECOND * (E * abs(mu) / sigma + G(3) * np.abs(y)) \
                + D64 * (count + 4) * (np.mean(np.abs(v)) / sigma + np.abs(y))
    return (out, bound) if with_bound else out


# ----------------------------------------------------------------------------- AddContextFrames
CTX_CASES = tuple((F, T, c) for T in (255, 256, 257) for F, c in ((1, 0), (3, 2))) + ((3, 5, 7), (1, 4, 4), (2, 1, 1), (1, 40, 3))


def context_input(F, T, c):
    """(x float32 [6, F, T], lens): gaussians with NaN and +-Inf in about one element of eight inside the utterance, and
    NaN with the payload NAN_PAYLOAD everywhere beyond it."""
    r = rng_of(("ctx", F, T, c))
    x = r.standard_normal((6, F, T)).astype(np.float32)
    kind = r.integers(0, 24, size=x.shape)
    x[kind == 0] = np.nan
    x[kind == 1] = np.inf
    x[kind == 2] = -np.inf
    lens = ragged_lens(T)
    for n in range(6):
        x[n, :, max(int(lens[n]), 0):] = NAN_PAYLOAD
    return x, lens


def context_ref(x, lens, c):
    """y[n, w, f, t] = x[n, f, t + w - c] where t and t + w - c lie in [0, min(len, T)), +0.0 elsewhere."""
    N, F, T = x.shape
    y = np.zeros((N, 2 * c + 1, F, T), dtype=np.float32)
    for n in range(N):
        L = min(max(int(lens[n]), 0), T)
        for w in range(2 * c + 1):
            lo, hi = max(0, c - w), min(L, L + c - w)              # t in [lo, hi): t < L and 0 <= t + w - c < L
            if hi > lo:
                y[n, w, :, lo:hi] = x[n, :, lo + w - c:hi + w - c]
    return y


# ----------------------------------------------------------------------------- SpecAugment
# id -> (C, F, T, f_bands per utterance, t_bands per utterance); bands are (start, width)
SPEC_CASES = {
    "zero_width": (1, 5, 9, [[(2, 0)], [(0, 0)]], [[(3, 0)], [(8, 0)]]),
    "start_at_the_end": (3, 5, 9, [[(5, 2)], [(4, 1)]], [[(9, 3)], [(8, 1)]]),
    "overlapping": (1, 7, 300, [[(1, 3), (2, 4)], [(0, 1), (0, 7)]], [[(250, 10), (255, 3)], [(0, 2), (1, 1)]]),
    "past_T": (3, 4, 257, [[(3, 5)], [(1, 1)]], [[(250, 20)], [(256, 1000)]]),
    "no_f_table": (1, 5, 9, None, [[(3, 2)], [(0, 9)]]),
    "no_t_table": (3, 5, 9, [[(2, 2)], [(0, 5)]], None),
    "one_frame_F1": (1, 1, 1, [[(0, 1)], [(1, 1)]], [[(1, 1)], [(0, 0)]]),
    "block_edge": (1, 2, 513, [[(1, 1)], [(2, 1)]], [[(255, 2)], [(511, 2)]]),
}


def spec_input(case_id):
    """x float32 [N, C, F, T] with NaN and +-Inf in about one element of six, so bands hold some and the rest keeps some."""
    C, F, T = SPEC_CASES[case_id][:3]
    r = rng_of(("spec", case_id))
    x = r.standard_normal((2, C, F, T)).astype(np.float32)
    kind = r.integers(0, 12, size=x.shape)
    x[kind == 0] = NAN_PAYLOAD
    x[kind == 1] = -np.inf
    return x


def spec_ref(x, f_bands, t_bands):
    y = x.copy()
    for n in range(x.shape[0]):
        for s, w in (f_bands[n] if f_bands else ()):
            y[n, :, s:s + w, :] = np.float32(0.0)
        for s, w in (t_bands[n] if t_bands else ()):
            y[n, :, :, s:s + w] = np.float32(0.0)
    return y


# ----------------------------------------------------------------------------- MFCCLegacy
def legacy_frames(samples, frame_len, frame_step):
    return 1 if samples <= frame_len else 1 + -(-(samples - frame_len) // frame_step)


def legacy_tables(nfft, nfilt, numcep, sample_rate=16000, ceplifter=22):
    """(twiddle [nfft, 2], fbank [nfilt, nfft/2+1], dct [numcep, nfilt], lifter [numcep]) float64, python_speech_features'."""
    j = np.arange(nfft) * (2.0 * np.pi / nfft)
    twiddle = np.stack([np.cos(j), np.sin(j)], axis=1)
    mel = np.linspace(0.0, 2595.0 * np.log10(1.0 + (sample_rate / 2) / 700.0), nfilt + 2)
    bins = np.floor((nfft + 1) * (700.0 * (10.0 ** (mel / 2595.0) - 1.0)) / sample_rate)
    fbank = np.zeros((nfilt, nfft // 2 + 1))
    for m in range(nfilt):
        for i in range(int(bins[m]), int(bins[m + 1])):
            fbank[m, i] = (i - bins[m]) / (bins[m + 1] - bins[m])
        for i in range(int(bins[m + 1]), int(bins[m + 2])):
            fbank[m, i] = (bins[m + 2] - i) / (bins[m + 2] - bins[m + 1])
    n = np.arange(nfilt)
    dct = np.cos(np.pi * (n[None, :] + 0.5) * n[:, None] / nfilt) * np.sqrt(2.0 / nfilt)
    dct[0] *= 1.0 / np.sqrt(2.0)
    lifter = 1.0 + (ceplifter / 2.0) * np.sin(np.pi * np.arange(numcep) / ceplifter)
    return np.ascontiguousarray(twiddle), fbank, np.ascontiguousarray(dct[:numcep]), lifter


LEGACY_PAD = np.float32(0.999)       # a NaN converts to the integer 0 on both sides and would hide a leak
# id -> (frame_len, frame_step, nfft, nfilt, numcep, lens, max_samples)
LEGACY_CASES = {
    # lengths 1, frame_len, frame_len + 1, a partly filled last frame
    "small": (25, 10, 32, 8, 8, (1, 25, 26, 48, 39), 48),
    "rfft_truncates": (40, 16, 32, 8, 6, (1, 40, 41, 77), 77),           # nfft < frame_len: Python cannot reach it
    "shipped": (400, 320, 512, 26, 13, (1, 400, 401, 1000), 1000),
    "oversize": (25, 10, 32, 8, 8, (30, 48 + 7, 48 + 100), 48),          # lengths above max_samples
}


def legacy_wave(case_id):
    """float32 [N, max_samples]: clipped gaussians of deviation 0.3; from the first third on, one sample in eight is exactly
    +1.0 or -1.0 (the int16 wrap) and one in eight truncates to 0; utterance 3 (if any) has a stretch of exact zeros long
    enough for all-zero frames (both eps branches).  Beyond each length: 0.999."""
    frame_len, frame_step, _, _, _, lens, max_samples = LEGACY_CASES[case_id]
    r = rng_of(("legacy", case_id))
    w = np.full((len(lens), max_samples), LEGACY_PAD, dtype=np.float32)
    for n, L in enumerate(lens):
        L = min(L, max_samples)
        x = np.clip(r.standard_normal(L) * 0.3, -1, 1).astype(np.float32)
        kind = r.integers(0, 8, size=L)
        kind[:L // 3] = 7
        x[kind == 0] = np.where(r.random(int(np.sum(kind == 0))) < 0.5, 1.0, -1.0)
        x[kind == 1] = (r.random(int(np.sum(kind == 1))) - 0.5) * np.float32(1.9 / 32768)
        if n == 3:
            x[L // 2:L // 2 + 2 * frame_len + frame_step] = 0.0
        w[n, :L] = x
    return w


def legacy_int16(x):
    """(double)(int16_t)(int)(x * 32768.0f): truncation towards zero, then the two's-complement wrap (1.0 -> -32768)."""
    return (x.astype(np.float32) * np.float32(32768)).astype(np.int32).astype(np.int16).astype(np.float64)


def legacy_ref(wave, lens, tables, frame_len, frame_step, nfft, preemph=0.97, with_bound=False):
    """float64 [N, numcep, T] (and the bound): python_speech_features.mfcc as MFCCLegacy drives it, lengths above max_samples
    counting as max_samples, frames past an utterance's own count 0."""
    twiddle, fbank, dct, lifter = tables
    N, max_samples = wave.shape
    T = legacy_frames(max_samples, frame_len, frame_step)
    nbins, nfilt, numcep = nfft // 2 + 1, fbank.shape[0], dct.shape[0]
    used = min(frame_len, nfft)
    idx = (np.arange(nbins)[:, None] * np.arange(used)[None, :]) % nfft
    cosm, sinm = twiddle[idx, 0], twiddle[idx, 1]                     # [nbins, used]
    eps = np.finfo(np.float64).eps
    out, bound = np.zeros((N, numcep, T)), np.zeros((N, numcep, T))
    for n in range(N):
        L = min(int(lens[n]), max_samples)
        x = legacy_int16(wave[n, :L])
        sig = np.append(x[0], x[1:] - preemph * x[:-1])
        nfr = legacy_frames(L, frame_len, frame_step)
        padded = np.concatenate([sig, np.zeros((nfr - 1) * frame_step + frame_len - L)])
        fr = np.stack([padded[t * frame_step:t * frame_step + used] for t in range(nfr)])       # [nfr, used]
        re, im = fr @ cosm.T, -(fr @ sinm.T)
        p = (re * re + im * im) / nfft
        energy = p.sum(1)
        feat = p @ fbank.T
        e1, f1 = np.where(energy == 0, eps, energy), np.where(feat == 0, eps, feat)
        logf = np.log(f1)
        cep = (logf @ dct.T) * lifter[None, :]
        cep[:, 0] = np.log(e1)
        out[n, :, :nfr] = cep.T
        if with_bound:
            with np.errstate(invalid="ignore", divide="ignore"):
                d_fr = 2 * D64 * np.abs(fr)                           # the pre-emphasis: a product and a difference
                d_re = G64(used + 1) * (np.abs(fr) @ np.abs(cosm).T) + d_fr @ np.abs(cosm).T
                d_im = G64(used + 1) * (np.abs(fr) @ np.abs(sinm).T) + d_fr @ np.abs(sinm).T
                d_p = (2 * np.abs(re) * d_re + 2 * np.abs(im) * d_im + d_re ** 2 + d_im ** 2) / nfft + G64(3) * p
                d_feat = d_p @ fbank.T + G64(nbins) * feat
                d_en = d_p.sum(1) + G64(nbins) * energy
                rel = lambda d, v: np.where(v == 0, 0.0, np.where(d < v, d / (v - d), np.inf))       # noqa: E731
                d_logf = rel(d_feat, feat) + ULP_LOG * D64 * np.abs(logf)
                d_cep = np.abs(lifter)[None, :] * (d_logf @ np.abs(dct).T + G64(nfilt + 2) * (np.abs(logf) @ np.abs(dct).T))
                d_cep[:, 0] = rel(d_en, energy) + ULP_LOG * D64 * np.abs(np.log(e1))
                bound[n, :, :nfr] = (SECOND * (E * np.abs(cep) + d_cep)).T
    return (out, bound) if with_bound else out
