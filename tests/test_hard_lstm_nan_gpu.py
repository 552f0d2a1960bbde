"""A NaN in one sequence of a HardLSTM batch stays a NaN: through every kernel of csrc/rnn.hip that contains the hard cell
(hard sigmoid clamp(0.2 v + 0.5, 0, 1), hard tanh clamp(v, -1, 1)), by the public ``HardLSTM.forward``.

The reference cell (model/hard_lstm.py, restated in float64 by tests/rnn_ref64.py with np.minimum / np.maximum, which keep a
NaN) propagates a NaN gate to c and h; a clamp spelled fminf(fmaxf(v, lo), hi) returns ``lo`` for it, so a diverged sequence
would come out of the layer as finite numbers.

One NaN at x[T0, N0, 0], shapes T = 6, N = 3.  Expected:
  * the float64 reference's NaN pattern, element for element: in a forward direction sequence N0 is NaN in every unit at
    t >= T0, in a reverse direction at t <= T0, its h_n and c_n are NaN (a second layer above a bidirectional first one sees a
    NaN in every frame of N0);
  * sequences 0 and 2, and the frames of N0 on the other side of T0, keep the clean run's bits.

The smallest (H, directions, environment) that reaches each kernel, read off the dispatch of ms_rnn_layer_forward_ex and
asserted with the library's predicates where they exist:

  kernel                          H     dirs  environment           why
  lstm_persistent_split_kernel    64    1     default               split operands, a multiple of 64 that is no two-stream width
  lstm_persistent_split2_kernel   256   1     default               the smallest two-stream width (chains planes, not wide)
  wide2_wave                      1024  2     default               the wide-workgroup kernel serves H = 1024 only
  rnn_step_generic_kernel         8     1     MS_RNN_PAD_HIDDEN=0   not a multiple of 32; the module would pad it to 64
  lstm_persistent_kernel          32    1     MS_RNN_PAD_HIDDEN=0   a multiple of 32 but not of 64; the module would pad it to 64
  rnn_step_mfma_kernel            1088  1     MS_RNN_PAD_HIDDEN=0   a multiple of 64 above 1024 that is no wide width (padded: 1280)
  lstm_persistent_f32x2_kernel    256   1     MS_PRECISION=f32      the smallest two-stream width in exact-f32 mode

Both variables are read once per process, so those cases run in one child process each.  Needs a real MI355X: -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rnn_length_cases as LC
import rnn_ref64 as R64

pytestmark = pytest.mark.gpu

T_STEPS, N_SEQ, T0, N0 = 6, 3, 2, 1


def case(tag, H, bidir, nl, In=8):
    return LC.Case(f"hardnan-{tag}", "NAN", "HARD", In, H, bidir, nl, N_SEQ, T_STEPS, None, False, 1.0, "loop", ())


#        (case, predicates that hold for it in its environment: padded width, chains planes, wide)
DEFAULT = [(case("split64", 64, False, 1), (64, 0, 0)),
           (case("split64-bi-2layers", 64, True, 2), (64, 0, 0)),
           (case("split2-256", 256, False, 1), (256, 1, 0)),
           (case("split2-256-bi-2layers", 256, True, 2, In=32), (256, 1, 0)),
           (case("wide1024-bi", 1024, True, 1, In=32), (1024, 1, 1))]
PAD_OFF = [(case("scalar8", 8, False, 1), (8, 0, 0)),
           (case("scalar8-bi-2layers", 8, True, 2), (8, 0, 0)),
           (case("persistent32", 32, False, 1), (32, 0, 0)),
           (case("persistent32-bi", 32, True, 1), (32, 0, 0)),
           (case("stepmfma1088", 1088, False, 1), (1088, 0, 0))]
F32 = [(case("f32x2-256", 256, False, 1), (256, 0, 0)),
       (case("f32x2-256-bi", 256, True, 1), (256, 0, 0))]
CHILDREN = {"pad_off": (PAD_OFF, {"MS_RNN_PAD_HIDDEN": "0"}), "f32": (F32, {"MS_PRECISION": "f32"})}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def build_module(c):
    from myrtlespeech_amd.model.hard_lstm import HardLSTM
    m = HardLSTM(c.In, c.H, num_layers=c.nl, bidirectional=c.bidir)
    sd = LC.make_params(c)
    m.load_state_dict({"rnn." + k: T(v) for k, v in sd.items()}, strict=True)
    return m.eval(), sd


def forward(m, x):
    (out, _), (hn, cn) = m((T(x).cuda(), torch.full((N_SEQ,), T_STEPS, dtype=torch.int64)), None)
    return [t.detach().cpu().numpy() for t in (out, hn, cn)]


def check_predicates(c, want):
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    ndir = 2 if c.bidir else 1
    got = (lib.ms_rnn_padded_hidden(_lib.CELL_HARD_LSTM, c.H, ndir), lib.ms_rnn_layer_chains_planes(_lib.CELL_HARD_LSTM, c.H, ndir),
           lib.ms_rnn_layer_is_wide(_lib.CELL_HARD_LSTM, c.H, ndir, N_SEQ))
    assert got == want, (c.id, "padded width, chains planes, wide", got, want)


def check_case(c, want_predicates):
    check_predicates(c, want_predicates)
    m, sd = build_module(c)
    x, _, _ = LC.make_inputs(c)
    clean = forward(m, x)
    assert all(np.isfinite(a).all() for a in clean), c.id
    xb = x.copy()
    xb[T0, N0, 0] = np.nan
    got = forward(m, xb)
    ref_out, (ref_hn, ref_cn) = R64.hard_lstm_forward(xb, sd, c.H, c.nl, c.bidir, None)
    H, D = c.H, 2 if c.bidir else 1
    if c.nl == 1:   # the pattern the reference must show, spelled out
        want = np.zeros((T_STEPS, N_SEQ, D * H), dtype=bool)
        want[T0:, N0, :H] = True
        if c.bidir:
            want[:T0 + 1, N0, H:] = True
        assert np.array_equal(np.isnan(ref_out), want), c.id
    assert np.isnan(ref_hn[:, N0]).all() and np.isnan(ref_cn[:, N0]).all(), c.id
    for name, g, r, cl in zip(("out", "h_n", "c_n"), got, (ref_out, ref_hn, ref_cn), clean):
        nan = np.isnan(r)
        assert nan.any() and not nan[:, [0, 2]].any(), (c.id, name)
        lost = nan & ~np.isnan(g)
        assert not lost.any(), (c.id, name, int(lost.sum()), "of", int(nan.sum()), "values that are NaN in the reference came out as "
                                "numbers; first at", np.argwhere(lost)[:4].tolist(), g[lost][:4].tolist())
        changed = ~nan & (g.view(np.uint32) != cl.view(np.uint32))
        assert not changed.any(), (c.id, name, int(changed.sum()), "values outside the NaN's reach differ from the clean run; first "
                                   "at", np.argwhere(changed)[:4].tolist(), g[changed][:4].tolist(), cl[changed][:4].tolist())
    from myrtlespeech_amd import _lib
    assert _lib.load().ms_rnn_status(_lib.ptr(m._workspace.buf), _lib.stream_ptr()) == 0, c.id


@pytest.mark.parametrize("c,want", DEFAULT, ids=[c.id for c, _ in DEFAULT])
def test_a_nan_stays_a_nan_through_the_split_kernels(c, want):
    check_case(c, want)


def run_child(name):
    """(in a child process started with the environment of CHILDREN[name])"""
    cases, _ = CHILDREN[name]
    failed = []
    for c, want in cases:
        try:
            check_case(c, want)
        except AssertionError as e:
            failed.append(c.id)
            print("failed:", c.id, str(e)[:300])
    assert not failed, failed
    print("hard lstm nan ok", name, len(cases))


@pytest.mark.parametrize("name", sorted(CHILDREN))
def test_a_nan_stays_a_nan_through_the_kernels_of_another_environment(name):
    cases, env = CHILDREN[name]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_hard_lstm_nan_gpu as G; G.run_child(%r)\n") % (root, os.path.join(root, "tests"), name)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"hard lstm nan ok {name} {len(cases)}" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
