"""``ms_edit_distance`` (through the C ABI) and ``post_process.edit_distance`` against the restatement of the specification
(tests/edit_distance_ref.py) on every case of tests/edit_distance_cases.py.  Every assertion is integer equality.

Each case runs with rows as narrow as its longest row and with wider, poisoned rows: the kernels choose their path and size
their buffers by the row width, so the two runs of a case near a gate take different paths to the same answer.  The last
test asserts that the table reaches every path."""
import numpy as np
import pytest
import torch

import edit_distance_cases as C
import edit_distance_ref as R
from myrtlespeech_amd import _lib
from myrtlespeech_amd.post_process import EditCounts, edit_distance
from myrtlespeech_amd.post_process.edit_distance import MAX_UNITS, WAVE_UNITS, max_row_length, unit_capacity

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
paths_taken = set()      # ("wave" | "block", mode, lane axis / strided loop) of every ABI launch of this module


def guarded(nbytes_or_array, dtype=None):
    """A device buffer with 256 sentinel bytes on either side: (whole uint8 buffer, view of the payload)."""
    if isinstance(nbytes_or_array, np.ndarray):
        payload = np.ascontiguousarray(nbytes_or_array)
        nbytes = payload.nbytes
    else:
        payload, nbytes = None, int(nbytes_or_array)
    padded = -(-max(nbytes, 1) // 256) * 256
    whole = torch.full((256 + padded + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
    if payload is not None and nbytes:
        whole[256:256 + nbytes] = torch.from_numpy(payload.view(np.uint8).reshape(-1)).cuda()
    return whole, whole[256:256 + max(nbytes, 1)], nbytes


def intact(whole, nbytes):
    host = whole.cpu().numpy()
    return bool((host[:256] == SENTINEL).all() and (host[256 + max(nbytes, 1):] == SENTINEL).all())


def run_abi(case, extra=0, variant=None, totals=None, ws_short=0):
    """One ``ms_edit_distance`` call.  Returns (rc, out [N, 6] numpy, the guards' verdict)."""
    lib = _lib.load()
    h, hl, r, rl = C.matrices(case, extra, variant)
    n = h.shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    h_d, hl_d, r_d, rl_d = dev(h), dev(hl), dev(r), dev(rl)
    out_whole, out, out_bytes = guarded(n * 6 * 4)
    nbytes = lib.ms_edit_distance_workspace_bytes(n, h.shape[1], r.shape[1])
    assert nbytes > 0
    ws_whole, ws, ws_bytes = guarded(nbytes - ws_short)
    words = case.mode == R.WORDS
    cap_h, cap_r = unit_capacity(h.shape[1], words), unit_capacity(r.shape[1], words)
    if not ws_short:
        if min(cap_h, cap_r) <= WAVE_UNITS:
            paths_taken.add(("wave", case.mode, "ref" if cap_r < cap_h else "hyp"))
        else:
            m_max = int(C.expected(case.name)[:, 4].max())
            paths_taken.add(("block", case.mode, "strided" if m_max + 1 > C.BLOCK else "single"))
    rc = lib.ms_edit_distance(_lib.ptr(h_d), h.shape[1], _lib.ptr(hl_d), _lib.ptr(r_d), r.shape[1], _lib.ptr(rl_d), n, case.mode,
                              case.separator, case.n_symbols, out.data_ptr(), _lib.ptr(totals), ws.data_ptr(),
                              nbytes - ws_short, _lib.stream_ptr())
    torch.cuda.synchronize()
    ok = intact(out_whole, out_bytes) and intact(ws_whole, ws_bytes)
    return rc, out_whole[256:256 + out_bytes].cpu().numpy().view(np.int32).reshape(n, 6), ok


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_abi_equals_restatement(case):
    want = C.expected(case.name)
    rc, got, ok = run_abi(case)
    assert rc == 0, _lib.load().ms_last_error()
    assert ok, "a sentinel around out or the workspace was overwritten"
    assert got.tolist() == want.tolist()
    # a second run gives the same bits; wider rows with poisoned padding change no output word (and may change the path)
    assert run_abi(case)[1].tolist() == got.tolist()
    for extra, variant in ((3, 0), (5, 2), (70, 1)):
        rc, padded, ok = run_abi(case, extra, variant)
        assert rc == 0 and ok
        assert padded.tolist() == want.tolist(), (extra, variant)


@pytest.mark.parametrize("name", ["tok_zero_mid_batch", "wrd_n70", "tok_hyp_256_shorter", "wrd_ref_64_shorter"])
def test_totals_accumulate_and_are_optional(name):
    case = C.BY_NAME[name]
    want = C.expected(name)
    tot_whole, tot, _ = guarded(np.zeros(6, dtype=np.int64))
    totals = tot.view(torch.int64)
    for _ in range(2):
        rc, got, ok = run_abi(case, totals=totals)
        assert rc == 0 and ok and got.tolist() == want.tolist()
    assert totals.cpu().tolist() == (2 * want.sum(axis=0)).tolist()
    assert intact(tot_whole, 48)
    rc, got, ok = run_abi(case, totals=None)
    assert rc == 0 and ok and got.tolist() == want.tolist()
    assert totals.cpu().tolist() == (2 * want.sum(axis=0)).tolist()


def test_totals_beyond_int32():
    """The sums are 64-bit: a total that starts near 2^31 keeps counting."""
    case = C.BY_NAME["tok_1_vs_300"]
    totals = torch.full((6,), 2 ** 31 - 5, dtype=torch.int64, device="cuda")
    rc, got, ok = run_abi(case, totals=totals)
    assert rc == 0 and ok
    assert totals.cpu().tolist() == (C.expected(case.name).sum(axis=0) + (2 ** 31 - 5)).tolist()


def test_short_workspace_and_limit_are_refused_without_a_launch():
    lib = _lib.load()
    case = C.BY_NAME["wrd_separators"]
    rc, got, ok = run_abi(case, ws_short=1)
    assert rc == 3 and ok                                         # MS_ERR_WORKSPACE
    assert (got.view(np.uint8) == SENTINEL).all()                 # nothing was launched: out still holds the sentinel
    n = 2
    out = torch.full((n, 6), -77, dtype=torch.int32, device="cuda")
    lens = torch.zeros(n, dtype=torch.int32, device="cuda")
    for mode in (R.TOKENS, R.WORDS):
        over = max_row_length(mode == R.WORDS) + 1
        for hs, rs in ((over, 8), (8, over)):
            rows_h = torch.zeros((n, hs), dtype=torch.int32, device="cuda")
            rows_r = torch.zeros((n, rs), dtype=torch.int32, device="cuda")
            ws = torch.empty(max(lib.ms_edit_distance_workspace_bytes(n, hs, rs), 256), dtype=torch.uint8, device="cuda")
            rc = lib.ms_edit_distance(_lib.ptr(rows_h), hs, _lib.ptr(lens), _lib.ptr(rows_r), rs, _lib.ptr(lens), n, mode, 1, 3,
                                      _lib.ptr(out), None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
            assert rc == 5                                        # MS_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == -77).all()
    with pytest.raises(ValueError):                               # the Python layer refuses before any launch
        edit_distance(torch.zeros((n, MAX_UNITS + 1), dtype=torch.int32, device="cuda"), lens, [[1], [2]], None)
    with pytest.raises(ValueError):
        edit_distance(torch.zeros((n, 2 * MAX_UNITS), dtype=torch.int32, device="cuda"), lens, [[1], [2]], None,
                      separator_index=0, n_symbols=3)


def test_the_limit_itself_is_served():
    """4096 tokens against 4096: hypothesis = reference shifted by one (labels of period 251), so the answer is known without
    a 16 M cell loop on the host.  One insertion and one deletion around 4095 matches cost 2.  Equal unit counts force I = D, so
    the only other way to cost 2 is two substitutions around 4094 matches on the main diagonal, where no position matches:
    (2, 0, 1, 1) whatever the ties inside the matrix."""
    n_tok = MAX_UNITS
    base = (np.arange(n_tok + 1) % 251).astype(np.int32)
    hyp, ref = base[:-1].tolist(), base[1:].tolist()
    got = edit_distance([hyp], None, [ref], None).cpu().numpy()
    assert got.tolist() == [[2, 0, 1, 1, n_tok, n_tok]]
    same = edit_distance([hyp], None, [hyp], None).cpu().numpy()
    assert same.tolist() == [[0, 0, 0, 0, n_tok, n_tok]]
    # the same shift in one-letter words: 4096 words in 8191 labels a side, separator 251, the widest word scan
    n_words = MAX_UNITS

    def packed(letters):
        row = np.full(2 * len(letters) - 1, 251, dtype=np.int32)
        row[0::2] = letters
        return row.tolist()

    got = edit_distance([packed(base[:n_words])], None, [packed(base[1:n_words + 1])], None, separator_index=251, n_symbols=252)
    assert got.cpu().tolist() == [[2, 0, 1, 1, n_words, n_words]]


@pytest.mark.parametrize("name", ["tok_n70", "wrd_n70", "wrd_out_of_range", "wrd_no_separator", "tok_hyp_257_longer",
                                  "wrd_scan_steps", "wrd_zero_mid_batch"])
def test_python_entry_point_in_every_input_form(name):
    case = C.BY_NAME[name]
    want = C.expected(name).tolist()
    kw = dict(separator_index=case.separator, n_symbols=case.n_symbols) if case.mode == R.WORDS else {}
    h, hl, r, rl = C.matrices(case, extra=4, variant=3)
    t = torch.from_numpy
    forms = [
        (case.hyp, None, case.ref, None),                                                  # lists of lists
        (t(h), t(hl), t(r), t(rl)),                                                        # host tensors
        (t(h).to(torch.int64), t(hl).to(torch.int64), t(r).cuda(), t(rl).cuda()),          # mixed, int64 host side
        (t(h).cuda(), t(hl).cuda(), t(r).cuda(), t(rl).cuda()),                            # device tensors as they are
        (t(h).cuda(), hl.tolist(), case.ref, None),
    ]
    totals = torch.zeros(6, dtype=torch.int64, device="cuda")
    for hyp, hyp_lens, ref, ref_lens in forms:
        got = edit_distance(hyp, hyp_lens, ref, ref_lens, totals=totals, **kw)
        assert got.is_cuda and got.dtype == torch.int32 and got.shape == (len(want), 6)
        assert got.cpu().tolist() == want
    assert totals.cpu().tolist() == (len(forms) * C.expected(name).sum(axis=0)).tolist()
    row = EditCounts(*got[0].tolist())
    assert row.substitutions + row.deletions + row.insertions == row.distance


def test_python_entry_point_empty_batch_and_empty_rows():
    assert edit_distance([], None, [], None).shape == (0, 6)
    assert edit_distance([[], []], None, [[], [1]], None).cpu().tolist() == [[0, 0, 0, 0, 0, 0], [1, 0, 1, 0, 0, 1]]
    empty = torch.zeros((2, 0), dtype=torch.int32, device="cuda")
    lens = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert edit_distance(empty, lens, [[1, 2], []], None).cpu().tolist() == [[2, 0, 2, 0, 0, 2], [0, 0, 0, 0, 0, 0]]


def test_every_path_is_reached_by_the_table():
    """The table holds a case on both sides of every gate of the kernels, in both modes (``run_abi`` records the path the
    host arithmetic on the row widths selects, as the entry point does)."""
    paths_taken.clear()
    for name in ("tok_hyp_63_shorter", "tok_ref_63_shorter", "tok_hyp_64_shorter", "tok_hyp_257_longer",
                 "wrd_hyp_tight_63", "wrd_ref_tight_63", "wrd_hyp_tight_64", "wrd_hyp_257_longer"):
        rc, got, ok = run_abi(C.BY_NAME[name])
        assert rc == 0 and ok and got.tolist() == C.expected(name).tolist()
    assert paths_taken == {(path, mode, how) for mode in (R.TOKENS, R.WORDS)
                           for path, how in (("wave", "hyp"), ("wave", "ref"), ("block", "single"), ("block", "strided"))}
