"""tests/rnnt_decode_cases.py proved without a GPU: the float64 reference agrees with the float32 oracle on every case, every
case has its decision margin and the statistics it claims, the table hits every value of every dispatch dimension of
``ms_rnnt_decode``, and the workspace query refuses exactly the unsupported shapes."""
import numpy as np
import pytest

import rnnt_decode_cases as C
import rnnt_decode_ref as R64
from oracle import rnnt_oracle as RO

IDS = [c.id for c in C.CASES]


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_reference_agrees_with_the_float32_oracle(c):
    _, _, psd, jsd, enc = C.parts(c)
    if c.zero_bias:
        psd = {k: np.zeros_like(v) if ".bias_" in k else v for k, v in psd.items()}
    ref = C.reference(c)
    if c.greedy:
        want = RO.greedy_decode(enc, c.lengths, psd, jsd, c.H, c.L, c.V, c.ms)
    else:
        want, scores = RO.beam_decode(enc, c.lengths, psd, jsd, c.H, c.L, c.V, c.w, c.ms)
        live = [n for n in range(c.N) if c.lengths[n] > 0]            # (both give 0.0 for an utterance without frames)
        np.testing.assert_allclose([ref[n]["score"] for n in live], [scores[n] for n in live], rtol=1e-4, atol=1e-4)
    assert [u["hyp"] for u in ref] == want


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_margin_and_claims(c):
    ref = C.reference(c)
    margin = min(u["margin"] for u in ref)
    print(f"{c.id}: margin {margin:.2e}, dispatch {c.dispatch}")
    assert margin >= C.MARGIN
    assert C.failed_claims(c, ref) == []
    assert len(set(c.lengths.tolist())) > 1, "ragged lengths in every batch"
    assert int(c.lengths.max()) == c.T


def test_every_dispatch_value_is_hit():
    seen = {k: set() for k in C.DIMENSIONS}
    for c in C.CASES:
        for k, v in c.dispatch.items():
            if v is not None:
                seen[k].add(v)
    assert seen == C.DIMENSIONS
    # ... and by the entry the table says: the sequence is in the id, the named gates are where they are meant to be
    for c in C.CASES:
        assert c.dispatch["sequence"] == c.id.split("_")[0], c.id
    d = {c.id: c.dispatch for c in C.CASES}
    assert d["recut_L1"]["top_g"] == "with_joint_only" and d["recut_H128_L1"]["rgj"] == 1 and d["recut_L3_exact"]["rgj"] == 2
    for name in ("L3_fused_R16", "L3_fused_R40", "D192"):
        for seq in ("greedy", "round4"):
            assert d[f"{seq}_{name}"]["predictor"] == "fused", (seq, name)
    assert d["greedy_L3_fused_R16"]["fused_form"] == 1 and d["greedy_L3_fused_R40"]["fused_form"] == 2
    assert d["round4_L3_fused_R16"]["fused_form"] == 1 and d["round4_L3_fused_R40"]["fused_form"] == 2
    for name in ("L1", "L3_exact", "H40", "H128_L1"):
        assert d[f"round4_{name}"]["predictor"] == d[f"greedy_{name}"]["predictor"] == "exact", name
    assert d["recut_w32"]["gate_row_blocks"] == 2 and d["round4_w24_fused"]["fused_form"] == 2
    assert d["recut_J1056"]["move"] == d["recut_LH2240"]["move"] == "slow" and d["recut_L3_fused_R16"]["move"] == "fast"
    for seq in ("greedy", "round4"):
        assert d[f"{seq}_V40"]["joint_slots"] == d[f"{seq}_J528"]["joint_slots"] == "v64/regs"
        assert d[f"{seq}_J1040"]["joint_slots"] == "v64/loop" and d[f"{seq}_L1"]["joint_slots"] == "tile/regs"
    assert d["round4_V479_w32"]["joint_slots"] == "vloop/regs" and d["greedy_joint_64KB"]["joint_slots"] == "vloop/loop"
    assert d["greedy_N70"]["init_blocks"] == d["recut_N70_w2"]["init_blocks"] == 2
    # the limits sit exactly on their legal side
    c = C.BY_ID["round4_V479_w32"]
    assert c.w * (c.V + 1) * 4 == 60 * 1024
    c = C.BY_ID["greedy_joint_64KB"]
    assert (c.J + c.V + 1) * 4 == 64 * 1024
    c = C.BY_ID["recut_w32_ms4"]
    assert c.w * c.ms == 128


def test_chunked_walk():
    assert R64.chunked_walk([], 4) == (0, [])
    assert R64.chunked_walk([0] * 32, 4) == (1, [])
    assert R64.chunked_walk([0] * 33, 4) == (2, [])
    assert R64.chunked_walk([0] * 320, 4) == (10, [])
    assert R64.chunked_walk([0] * 31 + [1], 4) == (2, [])            # the label ends the first walk, the frame's blank the second
    assert R64.chunked_walk([0] * 31 + [2], 2) == (2, [0])           # ... and the quota is reached in row 0 of the second
    # one label per iteration: a frame with its quota of 2 takes two iterations and is left without a blank
    assert R64.chunked_walk([2] * 33, 2) == (66, [0] * 33)
    assert R64.chunked_walk([0] * 31 + [1, 0], 1) == (2, [31])


def test_event_driven_exit_cases_need_about_ten_iterations():
    for name in ("greedy_exit_len0", "greedy_exit_len1"):
        c = C.BY_ID[name]
        ref = C.reference(c)
        assert [u["iterations"] for u in ref] == [10, 7, int(c.lengths[2]), 2]
        assert c.T * c.ms + (c.T + 31) // 32 + 1 == 1291


BASE = dict(T=8, N=4, V=6, D=8, H=64, L=2, J=32, beam_width=4, max_symbols=3, greedy=0)


def ws_bytes(lib, **kw):
    a = dict(BASE, **kw)
    return lib.ms_rnnt_decode_workspace_bytes(a["T"], a["N"], a["V"], a["D"], a["H"], a["L"], a["J"], a["beam_width"],
                                              a["max_symbols"], a["greedy"])


def test_workspace_bytes_is_zero_exactly_for_unsupported_shapes(lib):
    assert ws_bytes(lib) > 0 and ws_bytes(lib, greedy=1) > 0
    assert ws_bytes(lib, L=8) > 0 and ws_bytes(lib, L=9) == 0 and ws_bytes(lib, L=9, greedy=1) == 0
    assert ws_bytes(lib, beam_width=32) > 0 and ws_bytes(lib, beam_width=33) == 0 and ws_bytes(lib, beam_width=0) == 0
    assert ws_bytes(lib, beam_width=33, greedy=1) > 0 and ws_bytes(lib, beam_width=0, greedy=1) > 0    # greedy ignores the width
    for name in ("T", "N", "V", "D", "H", "L", "J", "max_symbols"):
        for greedy in (0, 1):
            assert ws_bytes(lib, **{name: 1, "greedy": greedy}) > 0, name
            assert ws_bytes(lib, **{name: 0, "greedy": greedy}) == 0, name
            assert ws_bytes(lib, **{name: -1, "greedy": greedy}) == 0, name
    for c in C.CASES:
        assert ws_bytes(lib, T=c.T, N=c.N, V=c.V, D=c.D, H=c.H, L=c.L, J=c.J, beam_width=c.w, max_symbols=c.ms,
                        greedy=int(c.greedy)) > 0, c.id


def test_workspace_bytes_does_not_decrease_in_T_and_N(lib):
    for greedy in (0, 1):
        for kw in (dict(), dict(beam_width=32, max_symbols=4), dict(H=448, L=5), dict(V=479, J=48)):
            by_t = [ws_bytes(lib, T=t, greedy=greedy, **kw) for t in range(1, 70)]
            by_n = [ws_bytes(lib, N=n, greedy=greedy, **kw) for n in range(1, 140)]
            assert all(a <= b for a, b in zip(by_t, by_t[1:])) and all(a <= b for a, b in zip(by_n, by_n[1:]))
            assert by_n[0] < by_n[-1]
            if not greedy:
                assert by_t[0] < by_t[-1]          # (the trie grows with T; the greedy decode keeps nothing per frame)
