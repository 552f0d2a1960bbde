"""The feature front end through the C ABI on the cases of tests/frontend_cases.py (tests/test_frontend_edges_cpu.py proves
those): ms_mfcc_forward, ms_standardize_forward, ms_context_frames_forward, ms_spec_augment_, ms_mfcc_legacy_forward.  Every
output and every workspace lies between sentinel guards that must survive; every waveform lies inside a larger allocation
filled with the padding's poison, so an index that leaves the utterance reads poison the test owns.  The criteria are
equality of bits and the derived bounds of the cases file, on every element.  Needs a real MI355X: -m gpu."""
import numpy as np
import pytest
import torch

import frontend_cases as C
from myrtlespeech_amd import _lib
from test_small_ops_gpu import GUARD, INVALID, Guarded, S, dev, ok

pytestmark = pytest.mark.gpu

WORKSPACE = 3          # MS_ERR_WORKSPACE
TAIL = 1024            # poison elements behind a waveform batch: more than any oversized length reaches


class Waves:
    """A [N, max_samples] float32 batch inside an allocation of ``fill`` (GUARD elements before it, TAIL behind it)."""

    def __init__(self, wave, fill):
        self.buf = torch.full((GUARD + wave.size + TAIL,), float(fill), dtype=torch.float32, device="cuda")
        self.view = self.buf[GUARD:GUARD + wave.size]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(wave).reshape(-1)))


def run_mfcc(lib, tables, wave, lens, hop, top_db, what):
    """(out [N, n_mfcc, T]) of one guarded call; the workspace's guards are checked too."""
    window, dft, fb, dct = tables
    N, max_samples = wave.shape
    n_fft, n_mels, n_mfcc = window.size, fb.shape[0], dct.shape[0]
    T = C.mfcc_frames(max_samples, hop)
    td = [dev(t) for t in tables]
    wd, ld = Waves(wave, np.nan), dev(np.asarray(lens, dtype=np.int32))
    nbytes = lib.ms_mfcc_workspace_bytes(N, T, n_fft, n_mels, n_mfcc)
    assert nbytes > 0 and nbytes % 4 == 0
    out, ws = Guarded(N * n_mfcc * T), Guarded(nbytes // 4)
    ok(lib.ms_mfcc_forward(_lib.ptr(wd.view), _lib.ptr(ld), *[_lib.ptr(t) for t in td], _lib.ptr(out.view), N, max_samples, T,
                           n_fft, hop, n_mels, n_mfcc, top_db, _lib.ptr(ws.view), nbytes, S()), what)
    got = out.take((N, n_mfcc, T), what)
    ws.take((nbytes // 4,), (what, "workspace"), written=False)
    return got


# ----------------------------------------------------------------------------- ms_mfcc_forward
def mfcc_case_groups():
    plain = [cid for cid in C.MFCC_CASES if not cid.startswith("tile_")]
    return [(cid,) for cid in plain] + [tuple(f"tile_T{T}_c{c}" for c in C.TILE_SIZES) for T in C.TILE_SIZES]


@pytest.mark.parametrize("cids", mfcc_case_groups(), ids=lambda g: g[0] if len(g) == 1 else g[0].rsplit("_", 1)[0])
def test_mfcc_keeps_its_bound_and_every_utterance_equals_its_solo_run(lib, cids):
    """Ragged batches whose padding is NaN: every element within the bound of the float64 reference, frames past an
    utterance's own count +0.0, and every utterance bit for bit what it gives alone (its own length as max_samples)."""
    worst = 0.0
    for cid in cids:
        tables, wave, lens, hop, top_db = C.mfcc_case(cid)
        got = run_mfcc(lib, tables, wave, lens, hop, top_db, cid)
        ref, bound = C.mfcc_ref(wave, lens, tables, hop, top_db, with_bound=True)
        worst = max(worst, C.check(got, ref, bound, cid))
        for n, L in enumerate(lens):
            nfr = 1 + int(L) // hop
            solo = run_mfcc(lib, tables, wave[n:n + 1, :L], [L], hop, top_db, (cid, "solo", n))
            assert solo.shape[2] == nfr
            assert C.same_bits(np.ascontiguousarray(got[n, :, :nfr]), solo[0]), (cid, n, "differs from its solo run")
    print("mfcc", cids[0], "worst error / bound", worst)


@pytest.mark.parametrize("cid", sorted(C.POISON_CASES))
def test_mfcc_poisoned_utterance_is_nan_and_its_neighbours_keep_their_bits(lib, cid):
    """NaN, +-Inf and an overflowing 3e38 at the first, a middle and the last valid sample of utterance 1: all of its valid
    features are NaN (torchaudio's result, pinned on the oracle by the CPU test), its padding frames stay +0.0, and the other
    utterances are bit for bit what the clean batch gives."""
    g, lens, max_samples = C.POISON_CASES[cid]
    tables = C.mfcc_tables(g["n_fft"], g["win"], g["n_mels"], g["n_mfcc"])
    clean = C.mfcc_wave(cid, lens, max_samples)
    base = run_mfcc(lib, tables, clean, lens, g["hop"], 80.0, cid)
    ref, bound = C.mfcc_ref(clean, lens, tables, g["hop"], 80.0, with_bound=True)
    C.check(base, ref, bound, cid)
    L = lens[1]
    nfr = 1 + L // g["hop"]
    for kind, value in C.POISON_KINDS.items():
        for where in C.POISON_AT:
            w = clean.copy()
            w[1, C.poison_position(L, where)] = value
            got = run_mfcc(lib, tables, w, lens, g["hop"], 80.0, (cid, kind, where))
            bad = ~np.isnan(got[1, :, :nfr])
            assert not bad.any(), (cid, kind, where, int(bad.sum()), "valid features are not NaN, e.g.", got[1, :, :nfr][bad][:4].tolist())
            assert not np.any(C.bits(np.ascontiguousarray(got[1, :, nfr:]))), (cid, kind, where, "padding frames are not +0.0")
            for n in (0, 2):
                assert C.same_bits(got[n], base[n]), (cid, kind, where, "utterance", n, "changed")


@pytest.mark.parametrize("cid", sorted(C.OVERSIZE_CASES))
def test_mfcc_length_above_max_samples_counts_as_max_samples(lib, cid):
    """The oversized utterance would read the next row or the NaN behind the batch; the result is that of the clamped length."""
    g, lens, max_samples = C.OVERSIZE_CASES[cid]
    tables = C.mfcc_tables(g["n_fft"], g["win"], g["n_mels"], g["n_mfcc"])
    wave = C.mfcc_wave(cid, lens, max_samples)
    got = run_mfcc(lib, tables, wave, lens, g["hop"], 80.0, cid)
    clamped = run_mfcc(lib, tables, wave, np.minimum(lens, max_samples), g["hop"], 80.0, (cid, "clamped"))
    bad = C.bits(got) != C.bits(clamped)
    assert not bad.any(), (cid, int(bad.sum()), "elements differ from the clamped call; NaN among them:", bool(np.isnan(got).any()))
    ref, bound = C.mfcc_ref(wave, lens, tables, g["hop"], 80.0, with_bound=True)
    C.check(got, ref, bound, cid)


def test_mfcc_refusals_return_their_codes_and_write_nothing(lib):
    tables, wave, lens, hop, top_db = C.mfcc_case("reflect32")
    N, max_samples = wave.shape
    n_fft, n_mels, n_mfcc = 32, 8, 8
    T = C.mfcc_frames(max_samples, hop)
    td = [dev(t) for t in tables]
    wd, ld = Waves(wave, np.nan), dev(lens)
    nbytes = lib.ms_mfcc_workspace_bytes(N, T, n_fft, n_mels, n_mfcc)
    out, ws = Guarded(N * (n_mels + 1) * (T + 1)), Guarded(nbytes // 4)
    ptrs = [_lib.ptr(wd.view), _lib.ptr(ld)] + [_lib.ptr(t) for t in td] + [_lib.ptr(out.view)]

    def call(ptrs=ptrs, T=T, n_mfcc=n_mfcc, ws_ptr=_lib.ptr(ws.view), ws_bytes=nbytes, refused=True):
        rc = lib.ms_mfcc_forward(*ptrs, N, max_samples, T, n_fft, hop, n_mels, n_mfcc, top_db, ws_ptr, ws_bytes, S())
        torch.cuda.synchronize()
        if refused:
            out.untouched(("refused call wrote its output", rc))
            ws.untouched(("refused call wrote its workspace", rc))
        return rc

    for i in range(len(ptrs)):
        assert call(ptrs=ptrs[:i] + [None] + ptrs[i + 1:]) == INVALID, ("null pointer", i)
    assert call(ws_ptr=None) == INVALID
    assert call(T=T + 1) == INVALID and call(T=T - 1) == INVALID, "T != 1 + max_samples / hop"
    assert call(n_mfcc=n_mels + 1) == INVALID, "n_mfcc > n_mels"
    assert call(ws_bytes=nbytes - 1) == WORKSPACE, "a workspace one byte short"
    assert lib.ms_mfcc_workspace_bytes(0, T, n_fft, n_mels, n_mfcc) == 0
    assert call(refused=False) == 0, "and the same arguments unharmed are accepted"


# ----------------------------------------------------------------------------- ms_standardize_forward
def run_standardize(lib, x, lens, what, in_place=False):
    N, inner, T = x.shape
    xd = Guarded(x.size, init=x)
    ld = None if lens is None else dev(np.asarray(lens, dtype=np.int32))
    y = xd if in_place else Guarded(x.size)
    nbytes = lib.ms_standardize_workspace_bytes(N)
    assert nbytes == 16 * N
    ws = Guarded(nbytes // 4)
    ok(lib.ms_standardize_forward(_lib.ptr(xd.view), _lib.ptr(ld), _lib.ptr(y.view), N, inner, T, _lib.ptr(ws.view), nbytes, S()), what)
    got = y.take(x.shape, what, written=not in_place)
    ws.take((nbytes // 4,), (what, "workspace"), written=False)
    if not in_place:
        assert C.same_bits(xd.take(x.shape, (what, "input"), written=False), x), (what, "the input changed")
    return got


@pytest.mark.parametrize("cid", sorted(C.STD_CASES))
def test_standardize_keeps_its_bound_ignores_nan_padding_and_works_in_place(lib, cid):
    """Padding of NaN: the valid region within the bound (NaN where inner len == 1, like torch), the tail +0.0; the same
    input padded with zeros gives the same bits; y == x gives the same bits."""
    x, lens = C.standardize_input(cid)
    got = run_standardize(lib, x, lens, cid)
    ref, bound = C.standardize_ref(x, lens, with_bound=True)
    print("standardize", cid, "worst error / bound", C.check(got, ref, bound, cid))
    zero_padded = np.where(np.isnan(x), np.float32(0.0), x)
    assert C.same_bits_or_both_nan(run_standardize(lib, zero_padded, lens, (cid, "zero padded")), got).all()
    assert C.same_bits_or_both_nan(run_standardize(lib, x, lens, (cid, "in place"), in_place=True), got).all()


def test_standardize_without_lengths_and_with_a_short_workspace(lib):
    x, lens = C.standardize_input("below_one_block")
    x = np.where(np.isnan(x), np.float32(1.5), x)
    full = np.full(x.shape[0], x.shape[2], dtype=np.int32)
    got = run_standardize(lib, x, None, "lens == NULL")
    ref, bound = C.standardize_ref(x, full, with_bound=True)
    C.check(got, ref, bound, "lens == NULL")
    assert C.same_bits(got, run_standardize(lib, x, full, "lens == T"))
    y, ws, xd = Guarded(x.size), Guarded(8), dev(x)
    assert lib.ms_standardize_forward(_lib.ptr(xd), None, _lib.ptr(y.view), 2, 3, 1365, _lib.ptr(ws.view), 31, S()) == WORKSPACE
    assert lib.ms_standardize_forward(None, None, _lib.ptr(y.view), 2, 3, 1365, _lib.ptr(ws.view), 32, S()) == INVALID
    torch.cuda.synchronize()
    y.untouched("standardize refused")
    ws.untouched("standardize refused")


def test_standardize_nan_inside_an_utterance_stays_inside_it(lib):
    """The utterance's valid region is NaN throughout, its tail +0.0, and its neighbours bit for bit the clean batch's."""
    r = C.rng_of("std-nan")
    lens = np.array([30, 25, 40], dtype=np.int32)
    x = (r.standard_normal((3, 3, 40)) * 2 + 1).astype(np.float32)
    for n in range(3):
        x[n, :, lens[n]:] = C.NAN_PAYLOAD
    base = run_standardize(lib, x, lens, "clean")
    for pos in ((0, 0), (1, 12), (2, 24)):
        xp = x.copy()
        xp[1][pos] = np.nan
        got = run_standardize(lib, xp, lens, ("NaN at", pos))
        assert np.isnan(got[1, :, :25]).all(), ("NaN at", pos, "valid region is not NaN throughout")
        assert not np.any(C.bits(np.ascontiguousarray(got[1, :, 25:]))), "the tail is +0.0"
        assert C.same_bits(got[0], base[0]) and C.same_bits(got[2], base[2]), "a neighbour changed"


# ----------------------------------------------------------------------------- ms_context_frames_forward
@pytest.mark.parametrize("F,T,c", C.CTX_CASES)
def test_context_frames_moves_bits_and_never_the_padding(lib, F, T, c):
    """lens 0, 1, T - 1, T, T + 5, -3 in one batch: NaN and +-Inf inside an utterance keep their bits, the NaN beyond it never
    appears, every t >= len is +0.0; without lengths every utterance is T frames long."""
    x, lens = C.context_input(F, T, c)
    xd, ld = dev(x), dev(lens)
    for lens_arg, lens_ref in ((ld, lens), (None, np.full(6, T))):
        what = ("context", F, T, c, "lens" if lens_arg is not None else "no lens")
        y = Guarded(6 * (2 * c + 1) * F * T)
        ok(lib.ms_context_frames_forward(_lib.ptr(xd), _lib.ptr(lens_arg), _lib.ptr(y.view), 6, F, T, c, S()), what)
        got = y.take((6, 2 * c + 1, F, T), what, written=False)
        want = C.context_ref(x, lens_ref, c)
        bad = C.bits(got) != C.bits(want)
        assert not bad.any(), (what, int(bad.sum()), "wrong; first at", np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(),
                               want[bad][:4].tolist())


# ----------------------------------------------------------------------------- ms_spec_augment_
@pytest.mark.parametrize("cid", sorted(C.SPEC_CASES))
def test_spec_augment_zeroes_its_bands_and_nothing_else(lib, cid):
    """In place between guards: NaN inside a band becomes +0.0, everything outside keeps its bits (NaN payloads included)."""
    Cn, F, T, fb, tb = C.SPEC_CASES[cid]
    x = C.spec_input(cid)
    xb = Guarded(x.size, init=x)
    fd = None if fb is None else dev(np.array(fb, dtype=np.int32))
    tbd = None if tb is None else dev(np.array(tb, dtype=np.int32))
    n_f, n_t = (0 if fb is None else len(fb[0])), (0 if tb is None else len(tb[0]))
    ok(lib.ms_spec_augment_(_lib.ptr(xb.view), _lib.ptr(fd), _lib.ptr(tbd), 2, Cn, F, T, n_f, n_t, S()), cid)
    got = xb.take(x.shape, cid, written=False)
    want = C.spec_ref(x, fb, tb)
    bad = C.bits(got) != C.bits(want)
    assert not bad.any(), (cid, int(bad.sum()), "wrong; first at", np.argwhere(bad)[:4].tolist())


def test_spec_augment_without_bands_writes_nothing_and_null_tables_are_refused(lib):
    x = C.spec_input("overlapping")
    xb = Guarded(x.size, init=x)
    ok(lib.ms_spec_augment_(_lib.ptr(xb.view), None, None, 2, 1, 7, 300, 0, 0, S()), "no bands")
    assert lib.ms_spec_augment_(_lib.ptr(xb.view), None, None, 2, 1, 7, 300, 1, 0, S()) == INVALID
    assert lib.ms_spec_augment_(_lib.ptr(xb.view), None, None, 2, 1, 7, 300, 0, 1, S()) == INVALID
    assert lib.ms_spec_augment_(None, None, None, 2, 1, 7, 300, 0, 0, S()) == INVALID
    assert C.same_bits(xb.take(x.shape, "no bands", written=False), x)


# ----------------------------------------------------------------------------- ms_mfcc_legacy_forward
@pytest.mark.parametrize("cid", sorted(C.LEGACY_CASES))
def test_mfcc_legacy_keeps_its_bound_and_never_reads_the_padding(lib, cid):
    """The padding, and the allocation around the batch, hold 0.999 (a NaN would convert to the integer 0 and hide a leak);
    lengths above max_samples count as max_samples."""
    frame_len, frame_step, nfft, nfilt, numcep, lens, max_samples = C.LEGACY_CASES[cid]
    tables = C.legacy_tables(nfft, nfilt, numcep)
    wave = C.legacy_wave(cid)
    N = len(lens)
    T = C.legacy_frames(max_samples, frame_len, frame_step)
    td = [dev(t) for t in tables]
    wd, ld = Waves(wave, C.LEGACY_PAD), dev(np.array(lens, dtype=np.int32))
    out = Guarded(N * numcep * T)
    ok(lib.ms_mfcc_legacy_forward(_lib.ptr(wd.view), _lib.ptr(ld), *[_lib.ptr(t) for t in td], _lib.ptr(out.view), N, max_samples, T,
                                  frame_len, frame_step, nfft, nfilt, numcep, 0.97, S()), cid)
    got = out.take((N, numcep, T), cid)
    ref, bound = C.legacy_ref(wave, lens, tables, frame_len, frame_step, nfft, with_bound=True)
    print("mfcc_legacy", cid, "worst error / bound", C.check(got, ref, bound, cid))
