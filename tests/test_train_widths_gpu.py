"""Training stacks at the widths the persistent kernels serve: ``rnn_train`` / ``gru_train`` on one case per FORWARD schedule
(tests/train_width_cases.py: unpadded, padded, two-stream, wide with one and two batch groups, packed rows, H > 1024, the 8- and
10-unit persistent GRU, the tanh-RNN as a GRU, a launch per step, and -- in a child process with MS_PRECISION=f32 -- the
exact-f32 kernels), each in a buffer three steps longer than its longest sequence.  The training counterpart of
tests/test_gpu_rnn_lengths.py: that file checks what the forward hands the backward on every schedule, this one that gradients
survive it.  Per case (``W.check`` holds b .. e; tests/test_train_widths_cpu.py runs the same function on a stand-in):

  a. the library's predicates say the case reaches the schedule it names, before anything runs;
  b. out, h_n, c_n against the torch float64 yardstick within the suite's 1e-4; rows past a length exactly 0; the default forward
     gives the same bits before and after the training call; no time-out word is left;
  c. every gradient within 1e-3 of its tensor's largest magnitude of the yardstick (the criterion of tests/test_ds1_train_gpu.py
     and its siblings, for the reason given there), printed as a multiple of torch float32's error (floored at 2^-24); dx exactly
     0 in every row past a length;
  d. single-layer cases, both precision modes: every gradient against the project's float64 restatement of the backward FED THE
     DEVICE'S OWN OUTPUT, as a multiple of the float32 restatement's error on the same inputs (floored at 2^-24).  The cap is not
     measured: K / log2(K), K the longest sum in the case (``W.emulation_cap``);
  e. padding does not matter, bit for bit: the same batch in a buffer of exactly M steps, NaN in every row of x past a length,
     NaN in every row of d_out past a length, and a second run all give the same bits;
  f. (one LSTM and one GRU case) x without a gradient, and a loss on ``out`` alone, change no bit of the others.

MEASURED: the worst multiples of one run on one MI355X, per mode and case (DESIGN 4 holds the same table).  Needs a real
MI355X: -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_width_cases as W

pytestmark = pytest.mark.gpu

# (mode, case) -> (worst gradient error against the yardstick, worst multiple of torch float32's error, worst multiple of the
# emulation's error | None for a stack of two layers), one run on one MI355X; "f32": the child under MS_PRECISION=f32.  Every
# case passes c in both modes, none is excluded (W.C_EXCLUDED_DEFAULT is empty).  The worst tensor is L1024's dx: one k-ordered
# chain over the 8 192 gate rows of both directions, the same 2.42e-6 in both modes.  Caps of d: 232 .. 416.
MEASURED = {
    ("default", "L64"): (4.48e-07, 1.7, None),
    ("default", "L200"): (5.59e-07, 3.7, None),
    ("default", "L256"): (5.79e-07, 2.6, None),
    ("default", "L1024"): (2.42e-06, 7.8, 5.0),
    ("default", "L1024g"): (1.60e-06, 5.5, 3.6),
    ("default", "L1024p"): (1.68e-06, 5.7, 3.7),
    ("default", "L1280"): (1.50e-06, 2.3, 3.7),
    ("default", "G512"): (8.57e-07, 4.1, None),
    ("default", "G1280"): (8.50e-07, 2.5, 2.0),
    ("default", "G200"): (7.53e-07, 3.0, None),
    ("default", "T200"): (7.87e-07, 2.7, None),
    ("default", "T2600"): (1.48e-06, 1.9, 2.8),
    ("f32", "L256"): (6.59e-07, 3.0, None),
    ("f32", "L1024"): (2.42e-06, 7.8, 4.8),
    ("f32", "G512"): (5.28e-07, 2.0, None),
}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def cpu(t):
    return t.detach().cpu().numpy()


def cell_of(case):
    from myrtlespeech_amd import _lib
    return {"LSTM": _lib.CELL_LSTM, "GRU": _lib.CELL_GRU, "TANH": _lib.CELL_RNN_TANH}[case.kind]


def predicates(case):
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    cell, ndir = cell_of(case), W.ndir_of(case)
    in_sizes = [case.In] + [ndir * case.H] * (case.nl - 1)
    hp = lib.ms_rnn_padded_hidden(_lib.CELL_GRU, case.H, ndir)
    return dict(padded=lib.ms_rnn_padded_hidden(cell, case.H, ndir), wide=lib.ms_rnn_layer_is_wide(cell, case.H, ndir, min(case.N, 64)),
                chains=lib.ms_rnn_layer_chains_planes(cell, case.H, ndir),
                packs=int(all(lib.ms_rnn_layer_packs_rows(cell, case.M, case.N, k, case.H, ndir) for k in in_sizes)),
                gru=(hp, lib.ms_rnn_layer_chains_planes(_lib.CELL_GRU, hp, ndir)))


def assert_intended_schedule(case, mode):
    """a.  The table's answers hold in the default mode; the f32 child asserts what distinguishes its kernels."""
    from myrtlespeech_amd import _lib
    p = predicates(case)
    print(case.id, mode, p)
    if mode == "default":
        assert _lib.split_precision()
        for key, want in case.expect.items():
            assert p[key] == want, (case.id, key, p)
    else:
        assert not _lib.split_precision() and p["packs"] == 0, (case.id, p)
        if case.id == "G512":       # the exact-f32 mode has no persistent GRU
            assert p["chains"] == 0, (case.id, p)


def build_module(case):
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    kind = {"LSTM": RNNType.LSTM, "GRU": RNNType.GRU, "TANH": RNNType.BASIC_RNN}[case.kind]
    m = RNN(kind, case.In, case.H, num_layers=case.nl, bidirectional=case.bidir)
    m.load_state_dict({"rnn." + k: T(v) for k, v in W.make_params(case).items()}, strict=True)
    assert m.check_status
    return m.eval()


def states(case, hx, grad):
    if hx is None:
        return None
    mk = lambda a: T(a).cuda().requires_grad_(grad)      # noqa: E731
    return tuple(mk(a) for a in hx) if case.kind == "LSTM" else mk(hx)


def default_forward(m, case, inp):
    with torch.no_grad():
        (out, _), hid = m((T(inp["x"]).cuda(), T(inp["lens"])), states(case, inp["hx"], False))
    res = dict(out=out, h_n=hid[0], c_n=hid[1]) if case.kind == "LSTM" else dict(out=out, h_n=hid)
    return {k: cpu(v).copy() for k, v in res.items()}


def train(m, case, inp, x_grad=True, out_only=False):
    """One forward and one backward through the public entry point -> ``yardstick``'s keys as numpy arrays."""
    from myrtlespeech_amd.model.rnn_autograd import gru_train, rnn_train
    lstm = case.kind == "LSTM"
    for p in m.parameters():
        p.grad = None
    x = T(inp["x"]).cuda().requires_grad_(x_grad)
    hx = states(case, inp["hx"], True)
    if lstm:
        out, (hn, cn) = rnn_train(m, x, T(inp["lens"]), hx)
    else:
        (out, hn), cn = gru_train(m, x, T(inp["lens"]), hx), None
    loss = (out * T(inp["d_out"]).cuda()).sum()
    if not out_only:
        loss = loss + (hn * T(inp["d_hn"]).cuda()).sum()
        if lstm:
            loss = loss + (cn * T(inp["d_cn"]).cuda()).sum()
    loss.backward()
    res = dict(out=out, h_n=hn)
    if lstm:
        res["c_n"] = cn
    if x_grad:
        res["x"] = x.grad
    if hx is not None:
        res.update(dict(hx=hx[0].grad, cx=hx[1].grad) if lstm else dict(hx=hx.grad))
    res.update({k: p.grad for k, p in m.rnn.named_parameters()})
    assert all(v is not None for v in res.values()), [k for k, v in res.items() if v is None]
    return {k: cpu(v) for k, v in res.items()}


def run_case(case, mode):
    from myrtlespeech_amd import _lib
    assert_intended_schedule(case, mode)
    m = build_module(case)
    inp = W.make_inputs(case)
    got = {"before/" + k: v for k, v in default_forward(m, case, inp).items()}
    runs = dict(main=inp, again=inp, short=W.cut(inp, case.M), nan_x=dict(inp, x=W.poisoned(inp["x"], case)),
                nan_dout=dict(inp, d_out=W.poisoned(inp["d_out"], case)))
    for run, variant in runs.items():
        for key, v in train(m, case, variant).items():
            if run == "main" or key not in W.FORWARD_KEYS:
                got[f"{run}/{key}"] = v
    got.update({"after/" + k: v for k, v in default_forward(m, case, inp).items()})
    got["status"] = np.asarray(_lib.load().ms_rnn_status(_lib.ptr(m._workspace.buf), _lib.stream_ptr()))
    res = W.check(case, got, mode, inp, exclude_c=(mode == "default" and case.id in W.C_EXCLUDED_DEFAULT))
    worst = (max(v[0] for v in res.values()), max(v[1] for v in res.values()),
             max(v[2] for v in res.values()) if case.nl == 1 else None)
    print(f"MEASURED {mode} {case.id}: worst error {worst[0]:.2e}, {worst[1]:.1f} x torch float32"
          + ("" if worst[2] is None else f", {worst[2]:.1f} x emulation (cap {W.emulation_cap(case):.0f})"))
    return m, inp, got


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.id)
def test_training_at_a_served_width(case):
    m, inp, got = run_case(case, "default")
    if case.id not in ("L256", "G512"):
        return
    # f. optional inputs: x without a gradient, a loss on out alone -- the other gradients keep their bits
    skip = W.FORWARD_KEYS + ("x",)
    frozen = train(m, case, inp, x_grad=False)
    assert "x" not in frozen
    for key, v in frozen.items():
        if key not in skip:
            assert v.tobytes() == got["main/" + key].tobytes(), f"{case.id} {key}: x without a gradient changes bits"
    zero = dict(inp, d_hn=np.zeros_like(inp["d_hn"]), d_cn=None if inp["d_cn"] is None else np.zeros_like(inp["d_cn"]))
    want, alone = train(m, case, zero), train(m, case, zero, out_only=True)
    for key, v in alone.items():
        assert v.tobytes() == want[key].tobytes(), f"{case.id} {key}: a loss on out alone is not the loss with d_hn = 0"


def run_f32_cases():
    """(in a child process started with MS_PRECISION=f32) the three cases of ``W.F32_CHILD``."""
    for case in W.F32_CHILD:
        run_case(case, "f32")
    print("f32 training widths ok", len(W.F32_CHILD))


def test_exact_f32_mode_in_subprocess():
    """MS_PRECISION=f32 is read once per process: L256, L1024 and G512 run in one fresh child, once, under its own time limit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_train_widths_gpu as G; G.run_f32_cases()\n") % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MS_PRECISION="f32"), capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-20000:])
    assert r.returncode == 0 and f"f32 training widths ok {len(W.F32_CHILD)}" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
