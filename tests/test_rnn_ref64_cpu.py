"""The float64 reference of the recurrent layers (tests/rnn_ref64.py) against two independent witnesses, without a GPU:
the reference project's own outputs (tests/golden/rnn_*.npz, hard_lstm_*.npz) within the suite's tolerance, and the float32
oracle on every case of the length / padding lattice (tests/rnn_length_cases.py) within a QUARTER of that tolerance -- so that
three quarters of it remain for the kernels when tests/test_gpu_rnn_lengths.py holds them to the same reference."""
import numpy as np
import pytest

import rnn_length_cases as LC
import rnn_ref64 as R64
from oracle import ds_oracle as O
from util import Golden, golden_names

TOL = dict(rtol=1e-4, atol=1e-4)      # tests/test_gpu_parity.py


@pytest.mark.parametrize("name", golden_names("rnn_"))
def test_ref64_reproduces_the_reference_rnn_outputs(name):
    g = Golden(name)
    c = g.cfg
    hx = None
    if g.has("in/h0"):
        hx = (g["in/h0"], g["in/c0"]) if c["rnn_type"] == 0 else g["in/h0"]
    sd = {k[len("rnn."):]: v for k, v in g.sd().items()}
    out, hid = R64.rnn_forward(c["rnn_type"], g["in/x"], g["in/lens"], sd, c["hidden_size"], c["num_layers"],
                               c["bidirectional"], hx, c["batch_first"])
    assert out.dtype == np.float64
    np.testing.assert_allclose(out, g["out/y"], **TOL)
    if c["rnn_type"] == 0:
        np.testing.assert_allclose(hid[0], g["out/hn"], **TOL)
        np.testing.assert_allclose(hid[1], g["out/cn"], **TOL)
    else:
        np.testing.assert_allclose(hid, g["out/hn"], **TOL)


@pytest.mark.parametrize("name", golden_names("hard_lstm_"))
def test_ref64_reproduces_the_reference_hard_lstm_outputs(name):
    g = Golden(name)
    c = g.cfg
    sd = {k[len("rnn."):]: v for k, v in g.sd().items()}
    out, (hn, cn) = R64.hard_lstm_forward(g["in/x"], sd, c["hidden_size"], c["num_layers"], c["bidirectional"],
                                          (g["in/h0"], g["in/c0"]), c["batch_first"])
    np.testing.assert_allclose(out, g["out/y"], **TOL)
    np.testing.assert_allclose(hn, g["out/hn"], **TOL)
    np.testing.assert_allclose(cn, g["out/cn"], **TOL)


def test_ref64_never_reads_a_padded_row():
    """The property the GPU tests pin, on the reference itself: NaN in every padded frame, and a longer buffer, change nothing."""
    case = LC.BY_ID["S7-lstm200bi-L2"]
    x, lens, hx = LC.make_inputs(case)
    sd = LC.make_params(case)
    want = reference(case, x, lens, hx, sd)
    xn = x.copy()
    xn[LC.padding_mask(case)] = np.nan
    got = reference(case, xn, lens, hx, sd)
    for a, b in zip(want, got):
        np.testing.assert_array_equal(a, b)
    short = reference(case, x[:max(case.lens)], lens, hx, sd)
    np.testing.assert_array_equal(short[0], want[0][:max(case.lens)])
    assert not want[0][LC.padding_mask(case)].any()


def reference(case, x, lens, hx, sd):
    """-> (out, h_n, c_n | None) float64."""
    D = case.bidir
    if case.kind == "HARD":
        out, (hn, cn) = R64.hard_lstm_forward(x, sd, case.H, case.nl, D, hx)
        return out, hn, cn
    if case.kind == "LSTM":
        out, (hn, cn) = R64.rnn_forward(R64.LSTM, x, lens, sd, case.H, case.nl, D, hx)
        return out, hn, cn
    out, hn = R64.rnn_forward(R64.GRU if case.kind == "GRU" else R64.RNN_TANH, x, lens, sd, case.H, case.nl, D, hx)
    return out, hn, None


def oracle(case, x, lens, hx, sd):
    if case.kind == "HARD":
        out, (hn, cn) = O.hard_lstm_forward(x, sd, case.H, case.nl, case.bidir, hx)
        return out, hn, cn
    if case.kind == "LSTM":
        out, (hn, cn) = O.rnn_forward(O.LSTM, x, lens, sd, case.H, case.nl, case.bidir, hx)
        return out, hn, cn
    out, hn = O.rnn_forward(O.GRU if case.kind == "GRU" else O.BASIC_RNN, x, lens, sd, case.H, case.nl, case.bidir, hx)
    return out, hn, None


@pytest.mark.parametrize("case", [c for c in LC.CASES if c.gain == 1.0], ids=lambda c: c.id)
def test_float32_oracle_is_within_a_quarter_of_the_tolerance_of_ref64(case):
    """A condition on the case, not a measurement: a case that misses it is reshaped, never given a wider bound."""
    x, lens, hx = LC.make_inputs(case)
    sd = LC.make_params(case)
    want = reference(case, x, lens, hx, sd)
    got = oracle(case, x, lens, hx, sd)
    for name, a, b in zip(("out", "h_n", "c_n"), got, want):
        if b is None:
            continue
        assert a.shape == b.shape
        print(case.id, name, "max |f32 - f64| =", float(np.abs(a - b).max()))
        np.testing.assert_allclose(a, b, err_msg=f"{case.id} {name}", **LC.QUARTER_TOL)
    if case.lens is not None:
        assert not want[0][LC.padding_mask(case)].any()
    assert float(np.abs(want[0]).max()) > 0.01          # a live network (one step from a zero state at H = 1024 gives ~0.04)


def test_the_lattice_covers_what_it_says():
    ids = [c.id for c in LC.CASES]
    for sched in ("S1", "S2", "S4", "S5", "S6", "S7", "S8", "S9"):
        for pat in ("L0", "L1odd", "L1even", "L2", "L3"):
            assert any(i.startswith(sched) and i.endswith(pat) for i in ids), (sched, pat)
    for c in LC.CASES:
        if c.lens is None:
            continue
        lens = np.asarray(c.lens)
        assert len(lens) == c.N and lens.min() >= 1 and lens.max() <= c.T and np.all(np.diff(lens) <= 0), c.id
        pat = c.id.rsplit("-", 1)[1]
        M = int(lens.max())
        if pat == "L0":
            assert M == c.T and lens.min() == 1
        elif pat.startswith("L1"):
            assert M < c.T and lens.min() == M and M % 2 == (1 if pat == "L1odd" else 0)
        elif pat == "L2":
            assert M < c.T and lens.min() == 1 and len(set(lens.tolist())) < c.N
        elif pat == "L3":
            assert M == 1 and c.T > 1
    given = sum(c.hx for c in LC.CASES)
    assert abs(2 * given - len(LC.CASES)) <= 1
    for ids_ in LC.GATE_SETS.values():
        assert all(i in LC.BY_ID for i in ids_)
    assert {c.sched for c in LC.CASES if c.gain != 1.0} == {"S1", "S2", "S5"}
