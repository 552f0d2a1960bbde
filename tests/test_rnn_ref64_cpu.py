"""The float64 reference of the recurrent layers (tests/rnn_ref64.py) against two independent witnesses, without a GPU:
the reference project's own outputs (tests/golden/rnn_*.npz, hard_lstm_*.npz) within the suite's tolerance, and the float32
oracle on every case of the length / padding lattice (tests/rnn_length_cases.py) within a QUARTER of that tolerance -- so that
three quarters of it remain for the kernels when tests/test_gpu_rnn_lengths.py holds them to the same reference.

The operand-rounding emulation (``operands=``, the yardstick of the MS_PRECISION=bf16x3 and =fp16 children): the default
path is untouched; on every case of a mode's subset the emulation's distance E from the reference meets the mode's condition
(bf16x3: E <= 0.5e-4, so the device is held to exactly the suite's 1e-4; fp16: 2 E <= 3e-3, the bound of the older fp16
checks); the emulation passes the accuracy check as a stand-in for the device, and three planted faults fail it."""
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


def reference(case, x, lens, hx, sd, **kw):
    """-> (out, h_n, c_n | None) float64 (``operands=...``: the emulation of a mode instead)."""
    D = case.bidir
    if case.kind == "HARD":
        out, (hn, cn) = R64.hard_lstm_forward(x, sd, case.H, case.nl, D, hx, **kw)
        return out, hn, cn
    if case.kind == "LSTM":
        out, (hn, cn) = R64.rnn_forward(R64.LSTM, x, lens, sd, case.H, case.nl, D, hx, **kw)
        return out, hn, cn
    out, hn = R64.rnn_forward(R64.GRU if case.kind == "GRU" else R64.RNN_TANH, x, lens, sd, case.H, case.nl, D, hx, **kw)
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
    for sched in ("S1", "S2", "S4", "S5", "S6", "S7", "S8", "S9", "S10"):
        for pat in ("L0", "L1odd", "L1even", "L2", "L3"):
            assert any(i.startswith(sched + "-") and i.endswith(pat) for i in ids), (sched, pat)
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


# ---------------------------------------------------------------------------------- the operand-rounding emulation
MODE_BOUND = {"bf16x3": lambda e: e <= 0.5e-4, "fp16": lambda e: 2.0 * e <= 3e-3}
MODES_OF = {}
for _mode, _entries in LC.MODE_CHILD.items():
    for _cid, _ in _entries:
        MODES_OF.setdefault(_cid, []).append(_mode)


def run_case(case, sd=None, **kw):
    """-> (out[:M], h_n, c_n | None) of the case as the GPU child computes it: on the buffer cut to the longest sequence."""
    x, lens, hx = LC.make_inputs(case)
    return reference(case, x[:LC.steps_of(case)], lens, hx, LC.make_params(case) if sd is None else sd, **kw)


def test_operands_none_is_the_reference_and_never_enters_the_rounding_code(monkeypatch):
    """The default path is the float64 reference it was: the argument left out and ``operands=None`` give the same bits, and
    neither reaches a line of the emulation (the plan and every plane function raise).  One case per cell kind."""
    def boom(*a, **k):
        raise AssertionError("the float64 reference entered the operand-rounding code")
    for name in ("S7-lstm200bi-L2", "S8-gru64bi-L2", "S8-tanh48uni-L2", "S10-lstm64bi-L0"):
        case = LC.BY_ID[name]
        want = run_case(case)
        with monkeypatch.context() as mp:
            for fn in ("_layer_plan", "_planes", "_w_planes", "_h_planes", "_tagged", "_product"):
                mp.setattr(R64, fn, boom)
            got = run_case(case, operands=None)
        for a, b in zip(want, got):
            assert (a is None and b is None) or np.array_equal(a, b)
        assert any(not np.array_equal(a, b) for a, b in zip(want, run_case(case, operands="bf16x3")) if a is not None)


def test_the_layer_plan_restates_the_modes():
    P, O = R64._PAIR, R64._ONE
    plan = R64._layer_plan
    for H in (256, 512, 768, 1024, 200, 1000):          # fp16: one plane at the two-stream widths, padded widths included
        assert plan(R64.LSTM, H, 64, True, "fp16") == (O, O) and plan(R64.HARD_LSTM, H, 64, True, "bf16x3") == (P, P)
    assert plan(R64.LSTM, 64, 24, True, "fp16") == (None, P)        # 64 stays 64: float32 GEMM for 24 features, bf16 pairs
    assert plan(R64.LSTM, 64, 128, False, "fp16") == (P, P)
    assert plan(R64.LSTM, 100, 24, True, "bf16x3") == (P, P)        # padded to 128: the input is padded to 32 with it
    assert plan(R64.LSTM, 2048, 32, True, "bf16x3") == (P, P) and plan(R64.LSTM, 2048, 32, True, "fp16") == (P, None)
    assert plan(R64.LSTM, 2100, 32, True, "bf16x3") == (P, None)
    assert plan(R64.GRU, 512, 32, True, "fp16") == (P, P) and plan(R64.GRU, 512, 24, True, "fp16") == (None, P)
    assert plan(R64.GRU, 64, 24, True, "bf16x3") == (P, P)          # padded to 512
    assert plan(R64.RNN_TANH, 2600, 32, True, "bf16x3") == (P, None)   # a launch per step: float32 h . W_hh
    with pytest.raises(ValueError):
        plan(R64.LSTM, 256, 64, True, "f16x3")


def test_tagged_words_restate_publish_split():
    h = np.array([0.3333333, -0.7071068, 1.0, 2.0 ** -9, 0.0], dtype=np.float32)
    for tag in (0, 1):
        hi, lo = R64._h_planes(h, ("bf16", 2), tag)
        bits = hi.astype(np.float32).view(np.uint32)
        assert np.all(bits & 0xFFFF == 0) and np.all((bits >> 16) & 1 == tag)
        assert np.all((lo.astype(np.float32).view(np.uint32) >> 16) & 1 == tag)
        # lo recovers hi's bit; its own costs <= 2^-7 of lo
        assert np.all(np.abs(hi + lo - h) <= 2.0 ** -14 * np.abs(h) + 2.0 ** -120)
        one, none = R64._h_planes(h, ("f16", 1), tag)
        assert none is None and np.all(one.astype(np.float16).view(np.uint16) & 1 == tag)
        assert np.all(np.abs(one - h) <= 2.0 ** -10 * np.abs(h) + 2.0 ** -24)          # at most one fp16 ulp


@pytest.mark.parametrize("cid", [c.id for c in LC.CASES if c.id in MODES_OF and c.gain == 1.0])
def test_mode_conditions_hold_and_the_emulation_passes_as_the_device(cid):
    """Two conditions on the case, not measurements (a case that misses one is replaced by the same row at fewer steps, never
    given a wider bound), and the accuracy check with the emulation standing in for the device."""
    case = LC.BY_ID[cid]
    sd = LC.make_params(case)
    ref = run_case(case, sd)
    for mode in MODES_OF[cid]:
        emu = run_case(case, sd, operands=mode)
        for name, err, _, tol in LC.check_mode_accuracy(case, mode, emu, ref, emu):
            assert MODE_BOUND[mode](err), (mode, cid, name, err)
            assert tol == (1e-4 if mode == "bf16x3" else max(1e-4, 2.0 * err))
        if case.lens is not None:
            assert not emu[0][LC.padding_mask(case)[:LC.steps_of(case)]].any()


def test_every_mode_case_exists_and_sat_cases_stay_bit_comparisons():
    for mode, entries in LC.MODE_CHILD.items():
        ids = [i for i, _ in entries]
        assert len(set(ids)) == len(ids) and all(i in LC.BY_ID for i in ids)
        assert all(p in ("overlap", "packed", "loop") for _, p in entries)
        assert len(LC.MODE_EXCLUDED[mode]) <= 2 and all(i in ids for i in LC.MODE_EXCLUDED[mode])
        assert "S1-lstm1024bi-sat" in ids
    assert all(p == LC.BY_ID[i].path for i, p in LC.BF16X3_CHILD)
    assert dict(LC.FP16_CHILD)["S1-lstm1024bi-L2"] == "overlap" and dict(LC.FP16_CHILD)["S5-lstm1024bi-n40-L2"] == "loop"
    assert sum(i.startswith("S10-") for i, _ in LC.BF16X3_CHILD) == 15


def fails(case, mode, got, ref, emu):
    try:
        LC.check_mode_accuracy(case, mode, got, ref, emu)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mode, cid", [("bf16x3", "S4-lstm512bi-L2"), ("fp16", "S4-lstm512bi-L2"), ("bf16x3", "S6-gru512uni-L2"),
                                       ("fp16", "S7-lstm200bi-L2")])
def test_planted_faults_fail_the_accuracy_check(mode, cid, monkeypatch):
    """The emulation with a fault planted in it stands in for a faulty device; the tolerance comes from the clean emulation."""
    case = LC.BY_ID[cid]
    ref, emu = run_case(case), run_case(case, operands=mode)
    assert not fails(case, mode, emu, ref, emu)
    # 1. one 32-wide k-slice of W_hh zeroed in one direction of one layer
    sd = LC.make_params(case)
    name = "weight_hh_l1" + ("_reverse" if case.bidir else "")
    sd[name] = sd[name].copy()
    sd[name][:, 32:64] = 0.0
    assert fails(case, mode, run_case(case, sd, operands=mode), ref, emu)
    # 2. h_n of a ragged batch taken at step M instead of at step len_n: the last layer's forward state read from the
    #    output's last frame, which is zero for every shorter sequence
    assert min(case.lens) < max(case.lens)
    h_n = emu[1].copy()
    h_n[(case.nl - 1) * (2 if case.bidir else 1)] = emu[0][LC.steps_of(case) - 1][:, :case.H]
    assert fails(case, mode, (emu[0], h_n, emu[2]), ref, emu)
    # 3. the lo planes dropped in bf16x3
    if mode == "bf16x3":
        monkeypatch.setattr(R64, "_PAIR", ("bf16", 1))
        assert fails(case, mode, run_case(case, operands=mode), ref, emu)
