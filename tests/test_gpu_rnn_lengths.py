"""Recurrent stacks on over-padded and short batches: every schedule of ``run_layers`` (the overlapped stack, packed rows,
chained planes with one exchange initialisation, two batch groups per launch, the persistent GRU, zero-padded widths, the
tanh-RNN as a GRU, a launch per step, the exact-f32 kernels) through the public ``RNN.forward`` / ``HardLSTM.forward`` on
buffers whose longest sequence ends before the buffer does.  The reference (``pack_padded_sequence -> RNN ->
pad_packed_sequence(total_length)``) never reads a padded row and is indifferent to how much padding there is; per case:

  1. out, h_n, c_n against the float64 reference (tests/rnn_ref64.py) within the suite's tolerance;
  2. out[t >= len_n, n] is exactly 0, the whole block out[M:] included;
  3. the amount of padding does not matter: the same module on x[:M] gives the same bits;
  4. the content of the padding does not matter: 1e4 * randn, then NaN, in every padded frame -- the same bits;
  5. no time-out word is left in the module's workspace.

The other two split modes -- MS_PRECISION=bf16x3 and MS_PRECISION=fp16, read once per process -- run their subsets of the
lattice (``LC.BF16X3_CHILD``, ``LC.FP16_CHILD``) in one child process each.  Checks 2 to 5 and the stack-against-loop bit
comparisons are the same and take no tolerance; check 1 holds the device to rtol = atol = max(1e-4, 2 E), E being the distance
of the operand-rounding emulation (rnn_ref64, ``operands=``) from the same float64 reference, computed in the child from the
reference side alone (``LC.check_mode_accuracy``).

The cases, their inputs and weights: tests/rnn_length_cases.py (shared with tests/test_rnn_ref64_cpu.py, which shows on the CPU
that the float32 oracle stays within a quarter of the tolerance of the float64 reference on each of them).  Needs a real
MI355X: -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rnn_length_cases as LC
import rnn_ref64 as R64

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-4, atol=1e-4)      # the suite's (tests/test_gpu_parity.py)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def cpu(t):
    return t.detach().cpu().numpy()


def reference(case, x, lens, hx, sd, operands=None):
    """-> (out, h_n, c_n | None) float64; only the M steps that exist are computed (the rest of ``out`` is zero by definition).
    ``operands``: the emulation of a mode's operand rounding instead of the reference itself (rnn_ref64)."""
    if case.kind == "HARD":
        out, (hn, cn) = R64.hard_lstm_forward(x, sd, case.H, case.nl, case.bidir, hx, operands=operands)
        return out, hn, cn
    if case.kind == "LSTM":
        out, (hn, cn) = R64.rnn_forward(R64.LSTM, x, lens, sd, case.H, case.nl, case.bidir, hx, operands=operands)
        return out, hn, cn
    out, hn = R64.rnn_forward(R64.GRU if case.kind == "GRU" else R64.RNN_TANH, x, lens, sd, case.H, case.nl, case.bidir, hx,
                              operands=operands)
    return out, hn, None


def build_module(case):
    from myrtlespeech_amd.model.hard_lstm import HardLSTM
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    if case.kind == "HARD":
        m = HardLSTM(case.In, case.H, num_layers=case.nl, bidirectional=case.bidir)
    else:
        kind = {"LSTM": RNNType.LSTM, "GRU": RNNType.GRU, "TANH": RNNType.BASIC_RNN}[case.kind]
        m = RNN(kind, case.In, case.H, num_layers=case.nl, bidirectional=case.bidir)
    sd = LC.make_params(case)
    m.load_state_dict({"rnn." + k: T(v) for k, v in sd.items()}, strict=True)
    assert m.check_status
    return m.eval(), sd


def forward(m, case, x, lens, hx):
    """-> (out, h_n, c_n | None) on the device, through the module's public forward."""
    if case.kind in ("LSTM", "HARD"):
        (out, _), (hn, cn) = m((x, lens), hx)
        return out, hn, cn
    (out, _), hn = m((x, lens), hx)
    return out, hn, None


def same_bits(want, got, what):
    for name, a, b in zip(("out", "h_n", "c_n"), want, got):
        if a is not None:
            assert torch.equal(a, b), f"{what}: {name} differs"


def cell_of(case):
    from myrtlespeech_amd import _lib
    return {"LSTM": _lib.CELL_LSTM, "GRU": _lib.CELL_GRU, "TANH": _lib.CELL_RNN_TANH, "HARD": _lib.CELL_HARD_LSTM}[case.kind]


def predicates(case, steps=None):
    """What the library's predicates say about the case when it runs ``steps`` steps (default: its longest sequence)."""
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    cell, ndir = cell_of(case), 2 if case.bidir else 1
    M = LC.steps_of(case) if steps is None else steps
    ragged = case.lens is not None and min(case.lens) < max(case.lens)
    in_sizes = [case.In] + [ndir * case.H] * (case.nl - 1)
    p = dict(chains=lib.ms_rnn_layer_chains_planes(cell, case.H, ndir), wide=lib.ms_rnn_layer_is_wide(cell, case.H, ndir, min(case.N, 64)),
             padded=lib.ms_rnn_padded_hidden(cell, case.H, ndir),
             packs=int(ragged and all(lib.ms_rnn_layer_packs_rows(cell, M, case.N, k, case.H, ndir) for k in in_sizes)),
             overlap=lib.ms_rnn_stack_overlap_ok(cell, M, case.N, case.In, case.H, ndir, case.nl))
    p["path"] = "packed" if p["packs"] else ("overlap" if p["overlap"] else "loop")
    return p


def assert_intended_path(case):
    """The case reaches the schedule it was written for (so it cannot silently move to another kernel)."""
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    p = predicates(case)
    ndir = 2 if case.bidir else 1
    assert p["path"] == case.path, (case.id, p)
    if case.sched in ("S1", "S2", "S3"):
        assert p["chains"] == 1 and p["wide"] == 1 and p["padded"] == case.H, (case.id, p)
    elif case.sched == "S4":
        assert p["chains"] == 1 and p["wide"] == 0 and p["overlap"] == 0 and p["padded"] == case.H, (case.id, p)
    elif case.sched == "S5":
        assert p["chains"] == 1 and p["wide"] == 1 and p["overlap"] == 0 and case.N > 32, (case.id, p)
    elif case.sched == "S6":
        assert p["chains"] == 1 and p["padded"] == case.H and p["wide"] == 0, (case.id, p)
    elif case.sched == "S7":
        assert p["padded"] == {200: 256, 800: 1024}[case.H], (case.id, p)
    elif case.sched == "S8":
        hp = lib.ms_rnn_padded_hidden(_lib.CELL_GRU, case.H, ndir)
        as_gru = lib.ms_rnn_layer_chains_planes(_lib.CELL_GRU, hp, ndir)
        if case.H == 2600:      # wider than every persistent GRU: a launch per step at the next multiple of 64
            assert (hp, as_gru, p["padded"]) == (2624, 0, 2624), (case.id, hp, as_gru, p)
        else:                   # zero-padded onto the persistent GRU-512 (the tanh-RNN written as a GRU)
            assert (hp, as_gru) == (512, 1), (case.id, hp, as_gru)
    elif case.sched == "S9":
        assert not _lib.split_precision() and p["overlap"] == 0 and p["packs"] == 0, (case.id, p)
    elif case.sched == "S10":
        if case.H == 64:        # the one-stream split kernel at its own width: not padded, planes not chained
            assert (p["padded"], p["chains"], p["wide"]) == (64, 0, 0), (case.id, p)
        else:                   # the two-stream kernel beyond 1 024 units: chained planes, 8-unit workgroups, never overlapped
            assert (p["padded"], p["chains"], p["wide"], p["overlap"]) == (case.H, 1, 0, 0), (case.id, p)
    return p


def assert_mode_path(case, mode, path):
    """(in a mode's child) the process runs that mode, and the case reaches the path recorded for it there."""
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    assert os.environ.get("MS_PRECISION") == mode and _lib.split_precision(), mode
    p = assert_intended_path(case._replace(path=path))
    if mode == "fp16":          # rows never pack in this mode, whatever the lengths
        cell, ndir = cell_of(case), 2 if case.bidir else 1
        for k in (case.In, ndir * case.H):
            assert lib.ms_rnn_layer_packs_rows(cell, LC.steps_of(case), case.N, k, case.H, ndir) == 0, (case.id, k)
        assert p["packs"] == 0 and path != "packed", (case.id, p)
    return p


def check_case(case, mode=None, path=None):
    """``mode`` / ``path`` (a mode's child): the path the case takes in that mode, and check 1 by the mode's criterion."""
    from myrtlespeech_amd import _lib
    from myrtlespeech_amd.model import rnn as R
    lib = _lib.load()
    if mode is None:
        assert_intended_path(case)
        path = case.path
    else:
        assert_mode_path(case, mode, path)
    m, sd = build_module(case)
    x, lens, hx = LC.make_inputs(case)
    xd = T(x).cuda()
    lens_t = torch.full((case.N,), case.T, dtype=torch.int64) if lens is None else T(lens)
    hxd = None if hx is None else (tuple(T(a).cuda() for a in hx) if isinstance(hx, tuple) else T(hx).cuda())
    got = forward(m, case, xd, lens_t, hxd)
    M = LC.steps_of(case)
    # 1. against the float64 reference
    if case.gain == 1.0 and mode is not None:
        want = reference(case, x[:M], lens, hx, sd)
        dev = tuple(None if a is None else cpu(a) for a in got)
        LC.check_mode_accuracy(case, mode, (dev[0][:M],) + dev[1:], want, reference(case, x[:M], lens, hx, sd, mode))
    elif case.gain == 1.0:
        want = reference(case, x[:M], lens, hx, sd)
        for name, a, b in zip(("out", "h_n", "c_n"), got, want):
            if b is None:
                continue
            a = cpu(a)
            if name == "out":
                a = a[:M]
            print(case.id, name, "max |kernel - f64| =", float(np.abs(a - b).max()), "max |f64| =", float(np.abs(b).max()))
            np.testing.assert_allclose(a, b, err_msg=f"{case.id} {name}", **TOL)
    if path == "overlap":           # ... and the layer loop's bits
        prev = R._OVERLAP
        R._OVERLAP = False
        try:
            same_bits(got, forward(m, case, xd, lens_t, hxd), "layer loop")
        finally:
            R._OVERLAP = prev
    for segs in case.segs:          # ... whatever segment count is asked for
        prev = R._OVERLAP_SEGMENTS
        R._OVERLAP_SEGMENTS = segs
        try:
            same_bits(got, forward(m, case, xd, lens_t, hxd), f"{segs} segments")
        finally:
            R._OVERLAP_SEGMENTS = prev
    if case.lens is not None:
        mask = T(LC.padding_mask(case)).cuda()
        # 2. padded rows are exactly zero
        assert got[0].shape[0] == case.T
        assert not bool(got[0][mask].any()), f"{case.id}: a padded output row is not zero"
        assert not bool(got[0][M:].any())
        # 3. the amount of padding does not matter
        if M < case.T:
            short = forward(m, case, xd[:M].contiguous(), lens_t, hxd)
            same_bits((got[0][:M], got[1], got[2]), short, "buffer cut to the longest sequence")
        # 4. the content of the padding does not matter
        if bool(mask.any()):
            gen = torch.Generator(device="cuda").manual_seed(7)
            for what, fill in (("1e4 * randn", 1e4 * torch.randn(xd.shape, device="cuda", generator=gen)),
                               ("NaN", torch.full_like(xd, float("nan")))):
                dirty = torch.where(mask[:, :, None], fill, xd)
                same_bits(got, forward(m, case, dirty, lens_t, hxd), f"padding filled with {what}")
    # 5. no sticky status
    assert lib.ms_rnn_status(_lib.ptr(m._workspace.buf), _lib.stream_ptr()) == 0
    return got


@pytest.mark.parametrize("case", [c for c in LC.IN_PROCESS if c.sched != "S3"], ids=lambda c: c.id)
def test_rnn_lengths_and_padding(case):
    check_case(case)


@pytest.mark.parametrize("case", [c for c in LC.IN_PROCESS if c.sched == "S3"], ids=lambda c: c.id)
def test_hard_lstm_stack_on_both_sides_of_its_gate(case):
    """The hard LSTM takes no lengths: buffer lengths on both sides of its own gate, against the float64 reference and
    ``torch.equal`` to the layer loop (``check_case``: every case whose path is the overlapped stack is run on both)."""
    from myrtlespeech_amd.model import rnn as R
    got = check_case(case)
    m, _ = build_module(case)
    x, _, hx = LC.make_inputs(case)
    prev = R._OVERLAP
    R._OVERLAP = False
    try:
        hxd = None if hx is None else tuple(T(a).cuda() for a in hx)
        same_bits(got, forward(m, case, T(x).cuda(), torch.full((case.N,), case.T, dtype=torch.int64), hxd), "R._OVERLAP = False")
    finally:
        R._OVERLAP = prev


@pytest.mark.parametrize("name", sorted(LC.GATE_SETS))
def test_gate_cases_probe_the_gate(name):
    """L4's self-check: among the cases of a set that reach the gate (rows not packed), the predicate asked with the steps that
    run and with the buffer length must disagree for at least one and say 1 twice for at least one; otherwise the set no longer
    probes the gate and has to be chosen again."""
    disagree = both = 0
    for cid in LC.GATE_SETS[name]:
        case = LC.BY_ID[cid]
        by_steps, by_buffer = predicates(case), predicates(case, case.T)
        print(cid, "steps:", by_steps, "buffer:", by_buffer["overlap"])
        if min(case.lens) < max(case.lens) and case.path != "packed":
            assert by_steps["packs"] == 0, cid       # a ragged case that is relied on to reach the gate
        if by_steps["packs"]:
            continue
        disagree += by_steps["overlap"] != by_buffer["overlap"]
        both += by_steps["overlap"] == 1 and by_buffer["overlap"] == 1
    assert disagree >= 1 and both >= 1, (name, disagree, both)


def run_f32_cases():
    """(in a child process started with MS_PRECISION=f32) every S9 case."""
    for case in LC.F32_CHILD:
        check_case(case)
    print("f32 lengths ok", len(LC.F32_CHILD))


def run_mode_cases(mode):
    """(in a child process started with MS_PRECISION=<mode>) every case of the mode's subset; the first failure ends the child."""
    cases = LC.MODE_CHILD[mode]
    for cid, path in cases:
        check_case(LC.BY_ID[cid], mode, path)
    print(f"{mode} lengths ok", len(cases))


@pytest.mark.parametrize("mode", sorted(LC.MODE_CHILD))
def test_split_mode_lengths_in_subprocess(mode):
    """MS_PRECISION=bf16x3 / fp16: the mode's subset of the lattice in one fresh child, once, under its own time limit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_rnn_lengths as G; G.run_mode_cases(%r)\n") % (root, os.path.join(root, "tests"), mode)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MS_PRECISION=mode), capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-20000:])      # E, the device's distance and their ratio, per case and quantity
    assert r.returncode == 0 and f"{mode} lengths ok {len(LC.MODE_CHILD[mode])}" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_exact_f32_mode_lengths_in_subprocess():
    """MS_PRECISION=f32 is read once per process: the S9 cases run in one fresh child, once, under its own time limit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_rnn_lengths as G; G.run_f32_cases()\n") % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MS_PRECISION="f32"), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and f"f32 lengths ok {len(LC.F32_CHILD)}" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
