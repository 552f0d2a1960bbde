"""The training counterpart of tests/rnn_length_cases.py: one case per FORWARD schedule of the recurrent stacks, for the autograd
nodes ``rnn_train`` / ``gru_train`` (myrtlespeech_amd/model/rnn_autograd.py), which consume what that forward hands them.
tests/test_train_widths_gpu.py runs the cases on the device, tests/test_train_widths_cpu.py runs the same assertions
(``check``) on a stand-in.  numpy, plus torch on the CPU for the yardstick; nothing of the package under test is imported.

A case: cell, In, H, directions, layers, N, the longest sequence M, a buffer of T = M + 3 steps (always longer than the longest
sequence), lengths sorted in decreasing order with longest M and shortest 1, hx given or absent (alternating over the list),
and ``expect``: what the library's predicates must say for the case to reach the schedule it was written for (asserted on
the device before anything runs).  The S-row batch sizes and widths are those of tests/rnn_length_cases.py, whose forward
tests run them on the schedule named.

Weights: uniform(-1 / sqrt(H), 1 / sqrt(H)) drawn with numpy, seeded from the case id; x, hx, d_out, d_hn, d_cn likewise.

``yardstick(case, dtype)``       torch.nn.LSTM / GRU / RNN under pack_padded_sequence, loss sum(out d_out) + sum(h_n d_hn)
                                 [+ sum(c_n d_cn)]: out, h_n, c_n and every gradient -- ``x``, ``hx`` (and ``cx``: the LSTM's c0)
                                 and each parameter under its module name.  float64 is the reference, float32 the error a float32
                                 implementation is expected to make.
``given_h(case, out, dtype)``    single-layer cases: the project's own restatement of the backward (``recompute``,
                                 ``backward_steps``, ``batch_products`` of tests/lstm_backward_ref.py, tests/bilstm_backward_ref.py,
                                 tests/gru_backward_ref.py, used as they are) fed a GIVEN output, as the specification says.  In
                                 float32 the three batch products are numpy float32 matmuls on the emulation's float32 dG (the
                                 refs' ``batch_products`` is float64 only).
``check(case, got, mode)``       every assertion of the GPU test over a dict of numpy arrays (see its docstring).
"""
import zlib
from collections import namedtuple

import numpy as np

import bilstm_backward_ref as B
import gru_backward_ref as G
import lstm_backward_ref as L

Case = namedtuple("Case", "id kind In H bidir nl N M T lens hx in32 expect")

FWD_TOL = dict(rtol=1e-4, atol=1e-4)      # the suite's forward tolerance (tests/test_gpu_parity.py)
REL = 1e-3                                # the training tests' criterion (tests/test_ds1_train_gpu.py gives the reason)
U24 = 2.0 ** -24
GATE_SATURATED = 1.0e4                    # a tanh layer written as a GRU: input biases that hold r at exactly 1 and z at exactly 0
FORWARD_KEYS = ("out", "h_n", "c_n")
RUNS = ("main", "again", "short", "nan_x", "nan_dout")


def _seed(case_id):
    return zlib.crc32(("train-" + case_id).encode())


def _ragged(rng, N, M):
    """Sorted in decreasing order, longest M (twice when there is room), shortest 1."""
    lens = np.sort(rng.integers(1, M + 1, size=N))[::-1].copy()
    lens[0] = M
    if N > 2:
        lens[1] = M
    lens[-1] = 1
    return tuple(int(v) for v in lens)


_cases = []


def _add(cid, kind, In, H, ndir, nl, N, M, in32, **expect):
    hx = len(_cases) % 2 == 0                       # hx given and absent alternate over the list
    lens = _ragged(np.random.default_rng(_seed(cid) ^ 0x1E45), N, M)
    _cases.append(Case(cid, kind, In, H, ndir == 2, nl, N, M, M + 3, lens, hx, in32, expect))


# ``expect``: padded = ms_rnn_padded_hidden, wide = ms_rnn_layer_is_wide, chains = ms_rnn_layer_chains_planes, packs =
# ms_rnn_layer_packs_rows on every layer (all in the default precision mode); gru = (ms_rnn_padded_hidden(GRU), whether that
# width chains planes) for a tanh stack: (512, 1) runs as a GRU on the persistent GRU-512, (2624, 0) takes a launch per step.
_add("L64", "LSTM", 24, 64, 2, 2, 6, 6, False, padded=64, chains=0, wide=0, packs=0)        # smallest width that runs unpadded
_add("L200", "LSTM", 40, 200, 1, 2, 5, 6, False, padded=256, wide=0, packs=0)               # every saved layer output is a slice
_add("L256", "LSTM", 64, 256, 2, 2, 5, 6, True, padded=256, chains=1, wide=0, packs=0)      # two-stream kernel, unpadded
_add("L1024", "LSTM", 64, 1024, 2, 1, 3, 6, True, padded=1024, wide=1, packs=0)             # wide-workgroup kernel, one batch group
_add("L1024g", "LSTM", 64, 1024, 2, 1, 40, 6, True, padded=1024, wide=1, packs=0)           # ... two batch groups; two 32-row passes
# packed rows, unidirectional: the projection takes its row count from the device only where M N rows fill 192 tiles of 256 x 256
# of the [M N, 4 H] gate buffer (ms::gemm_rows_from_device_ok: not "starved" on 256 CUs) -- 12 rows of 16 tiles, M N > 2 816,
# so M = 45 is the shortest batch of 64 that packs (at M = 26 only a bidirectional layer, 8 H wide, does)
_add("L1024p", "LSTM", 64, 1024, 1, 1, 64, 45, True, padded=1024, wide=1, packs=1)
_add("L1280", "LSTM", 32, 1280, 2, 1, 3, 5, True, padded=1280, chains=1, wide=0, packs=0)   # H > 1024 two-stream kernel
_add("G512", "GRU", 32, 512, 1, 2, 32, 6, True, padded=512, chains=1, wide=0, packs=0)      # 8-unit persistent GRU, unpadded
_add("G1280", "GRU", 64, 1280, 2, 1, 9, 6, True, padded=1280, chains=1, wide=0, packs=0)    # 10-unit persistent GRU
_add("G200", "GRU", 40, 200, 2, 2, 6, 6, False, padded=512, packs=0)                        # padded to 512
_add("T200", "TANH", 40, 200, 2, 2, 6, 6, False, gru=(512, 1), packs=0)                     # tanh as a GRU on the padded GRU-512
_add("T2600", "TANH", 32, 2600, 1, 1, 6, 5, True, padded=2624, gru=(2624, 0), packs=0)      # launch per step, at width 2624

CASES = tuple(_cases)
BY_ID = {c.id: c for c in CASES}
SINGLE_LAYER = tuple(c for c in CASES if c.nl == 1)
# MS_PRECISION=f32 is read once per process: these run again in one child process.  There L256 is the exact-f32 two-stream
# kernel (its h carries an epoch tag in the mantissa LSB) and G512 has no persistent GRU.
F32_CHILD = tuple(BY_ID[i] for i in ("L256", "L1024", "G512"))
# default-mode cases taken out of criterion c because of the split-precision forward alone (d passes in both modes and c passes
# in the f32 child; such a case stays in the f32 child and under d, and DESIGN 4 states its error): id -> error.  None so far.
C_EXCLUDED_DEFAULT = {}


def gates_of(kind):
    return {"LSTM": 4, "GRU": 3, "TANH": 1}[kind]


def ndir_of(case):
    return 2 if case.bidir else 1


def param_names(case):
    return [f"{n}_l{layer}{sfx}" for layer in range(case.nl) for sfx in ("", "_reverse")[:ndir_of(case)]
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def make_params(case):
    """The case's parameters as float32 arrays under the module's names (``weight_ih_l0`` ...)."""
    rng = np.random.default_rng(_seed(case.id) ^ 0x5EED)
    H, D, g = case.H, ndir_of(case), gates_of(case.kind)
    k = 1.0 / np.sqrt(H)
    sd = {}
    for name in param_names(case):
        layer = int(name.split("_l")[1].split("_")[0])
        in_size = case.In if layer == 0 else D * H
        shape = (g * H, in_size) if name.startswith("weight_ih") else ((g * H, H) if name.startswith("weight_hh") else (g * H,))
        sd[name] = rng.uniform(-k, k, size=shape).astype(np.float32)
    return sd


def make_inputs(case):
    """dict: x [T, N, In], lens int64 [N], hx (None | h0 | (h0, c0)), d_out [T, N, ndir H], d_hn, d_cn (LSTM) -- float32."""
    rng = np.random.default_rng(_seed(case.id))
    f32 = lambda *s: rng.normal(size=s).astype(np.float32)      # noqa: E731
    states = (case.nl * ndir_of(case), case.N, case.H)
    lstm = case.kind == "LSTM"
    x = f32(case.T, case.N, case.In)
    h0, c0 = 0.4 * f32(*states), 0.4 * f32(*states)
    hx = None if not case.hx else ((h0, c0) if lstm else h0)
    return dict(x=x, lens=np.asarray(case.lens, dtype=np.int64), hx=hx, d_out=f32(case.T, case.N, ndir_of(case) * case.H),
                d_hn=f32(*states), d_cn=f32(*states) if lstm else None)


def live_mask(case, T=None):
    """[T, N, 1] bool: True where a frame exists."""
    return (np.arange(case.T if T is None else T)[:, None] < np.asarray(case.lens)[None, :])[..., None]


def poisoned(a, case):
    """``a`` [T, N, ...] with NaN in every row past its sequence's length."""
    return np.where(live_mask(case, a.shape[0]), a, np.float32(np.nan)).astype(np.float32)


def cut(inp, M):
    """The same batch in a buffer of exactly M steps."""
    return dict(inp, x=np.ascontiguousarray(inp["x"][:M]), d_out=np.ascontiguousarray(inp["d_out"][:M]))


def grad_keys(case, res):
    """The gradient tensors of a result dict (everything but the forward outputs)."""
    return [k for k in res if k not in FORWARD_KEYS]


_yard = {}


def yardstick(case, dtype=np.float64, inp=None, params=None):
    """See the module docstring.  ``inp`` / ``params``: other inputs than ``make_inputs(case)`` / ``make_params(case)`` (not
    cached).  The gradients of hx are returned only where the case gives hx."""
    key = (case.id, np.dtype(dtype).name)
    if inp is None and params is None and key in _yard:
        return _yard[key]
    import torch
    cache = inp is None and params is None
    inp = make_inputs(case) if inp is None else inp
    sd = make_params(case) if params is None else params
    td = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    lstm = case.kind == "LSTM"
    cls = {"LSTM": torch.nn.LSTM, "GRU": torch.nn.GRU, "TANH": torch.nn.RNN}[case.kind]
    m = cls(case.In, case.H, num_layers=case.nl, bidirectional=case.bidir).to(td)
    with torch.no_grad():
        for name, w in sd.items():
            getattr(m, name).copy_(torch.from_numpy(w).to(td))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(td)      # noqa: E731
    T = inp["x"].shape[0]
    x = t(inp["x"]).requires_grad_(True)
    states = (case.nl * ndir_of(case), case.N, case.H)
    hx = inp["hx"]
    h0 = (torch.zeros(states, dtype=td) if hx is None else t(hx[0] if lstm else hx)).requires_grad_(True)
    c0 = (torch.zeros(states, dtype=td) if hx is None else t(hx[1])).requires_grad_(True) if lstm else None
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.from_numpy(inp["lens"]), enforce_sorted=True)
    if lstm:
        out, (hn, cn) = m(packed, (h0, c0))
    else:
        (out, hn), cn = m(packed, h0), None
    out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
    total = (out * t(inp["d_out"])).sum() + (hn * t(inp["d_hn"])).sum()
    if lstm:
        total = total + (cn * t(inp["d_cn"])).sum()
    total.backward()
    res = dict(out=out, h_n=hn)
    if lstm:
        res["c_n"] = cn
    res["x"] = x.grad
    if hx is not None:
        res["hx"] = h0.grad
        if lstm:
            res["cx"] = c0.grad
    for name in sd:
        res[name] = getattr(m, name).grad
    res = {k: v.detach().numpy() for k, v in res.items()}
    if cache:
        _yard[key] = res
    return res


def _as_gru(p, H):
    """A tanh layer's parameters as those of the GRU that computes it (r held at exactly 1, z at exactly 0)."""
    z = lambda *s: np.zeros(s, dtype=np.float32)      # noqa: E731
    return dict(w_ih=np.concatenate([z(2 * H, p["w_ih"].shape[1]), p["w_ih"]]), w_hh=np.concatenate([z(2 * H, H), p["w_hh"]]),
                b_ih=np.concatenate([np.full(H, GATE_SATURATED, np.float32), np.full(H, -GATE_SATURATED, np.float32), p["b_ih"]]),
                b_hh=np.concatenate([z(2 * H), p["b_hh"]]))


def _dir_params(case, sd, d):
    sfx = "_l0" + ("_reverse" if d else "")
    p = {k: sd[n + sfx] for k, n in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh"))}
    return _as_gru(p, case.H) if case.kind == "TANH" else p


def given_h_parts(case, out, dtype=np.float64, inp=None, params=None):
    """Per direction of a single-layer case, everything the restatement makes of the GIVEN output ``out`` [T, N, ndir H], per-step
    tensors in the LAYER's time order: dict(p, x, h_prev, dGi, dGh, dx, d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_h0[, d_c0])."""
    assert case.nl == 1
    inp = make_inputs(case) if inp is None else inp
    sd = make_params(case) if params is None else params
    f = np.dtype(dtype).type
    lens, H, lstm = inp["lens"], case.H, case.kind == "LSTM"
    hx = inp["hx"]
    parts = []
    with np.errstate(over="ignore"):      # (exp(1e4) of the saturated gates of a tanh layer written as a GRU)
        for d in range(ndir_of(case)):
            p = _dir_params(case, sd, d)
            view = (lambda a: B.flip_time(a, lens)) if d == 1 else (lambda a: a)
            x = view(np.where(live_mask(case, inp["x"].shape[0]), inp["x"], 0).astype(np.float32))
            h = view(np.ascontiguousarray(out[..., d * H:(d + 1) * H]))
            d_out = view(np.ascontiguousarray(inp["d_out"][..., d * H:(d + 1) * H]))
            h0 = None if hx is None else (hx[0][d] if lstm else hx[d])
            c0 = None if (hx is None or not lstm) else hx[1][d]
            r = dict(p=p)
            if lstm:
                gates, c, _ = L.recompute(p, x, h, h0, c0, lens, dtype=f)
                dG, r["d_h0"], r["d_c0"], d_b = L.backward_steps(p, gates, c, c0, d_out, inp["d_hn"][d], inp["d_cn"][d], lens, dtype=f)
                dGi = dGh = dG
                r["d_b_ih"] = r["d_b_hh"] = d_b
                h_prev = L.h_prev_of(h, h0, lens)
            else:
                gates, q, _ = G.recompute(p, x, h, h0, lens, dtype=f)
                dGi, dGh, r["d_h0"], r["d_b_ih"], r["d_b_hh"] = G.backward_steps(p, gates, q, h, h0, d_out, inp["d_hn"][d], lens, dtype=f)
                h_prev = G.h_prev_of(h, h0, lens)
            if f is np.float64:
                if lstm:
                    dx, r["d_w_ih"], r["d_w_hh"] = L.batch_products(p, dG, x, h, h0, lens)
                else:
                    dx, r["d_w_ih"], r["d_w_hh"] = G.batch_products(p, dGi, dGh, x, h, h0, lens)
            else:       # the refs' batch_products are float64 only: the same three products as float32 matmuls
                gi2, gh2 = dGi.reshape(-1, dGi.shape[2]), dGh.reshape(-1, dGh.shape[2])
                dx = (gi2 @ p["w_ih"]).reshape(x.shape)
                r["d_w_ih"], r["d_w_hh"] = gi2.T @ x.reshape(-1, x.shape[2]), gh2.T @ h_prev.astype(np.float32).reshape(-1, H)
            r.update(x=view(x), h_prev=view(h_prev), dGi=view(dGi), dGh=view(dGh), dx=view(dx))
            parts.append(r)
    return parts


def given_h(case, out, dtype=np.float64, inp=None, params=None):
    """Every gradient of a single-layer case from the GIVEN output ``out``, keyed like ``yardstick``'s."""
    inp = make_inputs(case) if inp is None else inp
    parts = given_h_parts(case, out, dtype, inp, params)
    rows = slice(2 * case.H, 3 * case.H) if case.kind == "TANH" else slice(None)      # a tanh layer's own rows of the GRU's
    res = dict(x=sum(r["dx"] for r in parts))
    if inp["hx"] is not None:
        res["hx"] = np.stack([r["d_h0"] for r in parts])
        if case.kind == "LSTM":
            res["cx"] = np.stack([r["d_c0"] for r in parts])
    for d, r in enumerate(parts):
        sfx = "_l0" + ("_reverse" if d else "")
        for name, key in (("weight_ih", "d_w_ih"), ("weight_hh", "d_w_hh"), ("bias_ih", "d_b_ih"), ("bias_hh", "d_b_hh")):
            res[name + sfx] = r[key][rows]
    return res


def rel_err(got, ref):
    """max |got - ref| relative to the tensor's largest magnitude; NaN counts as infinite."""
    ref = np.asarray(ref, dtype=np.float64)
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    d = np.where(np.isnan(d), np.inf, d)
    return float(np.max(d) / max(float(np.max(np.abs(ref))), 1e-300))


def longest_sum(case):
    """K of criterion d: the longest sum in the case -- the recurrent product over the G H gate rows (``dG w_hh``), a
    pre-activation over In + H terms, or a weight gradient over the live rows.  (A tanh layer counts its own H rows: the two
    gate blocks the GRU form adds are exact zeros.)"""
    return max(gates_of(case.kind) * case.H, case.In + case.H, int(sum(case.lens)))


def emulation_cap(case):
    """K / log2(K): the ratio between the worst-case rounding bound of one k-ordered float32 chain of K terms (K u: the
    kernels) and that of numpy's pairwise and blocked sums (about log2(K) u: the emulation)."""
    K = longest_sum(case)
    return K / np.log2(K)


def check(case, got, mode, inp=None, exclude_c=False):
    """Every assertion of tests/test_train_widths_gpu.py on one case, over ``got``: a dict of numpy arrays keyed ``run/tensor``.
    Runs: ``main`` (the case as it stands), ``again`` (the same once more), ``short`` (the buffer cut to M steps), ``nan_x`` and
    ``nan_dout`` (NaN in every row of x / of d_out past its sequence's length); tensors: ``out``, ``h_n``, ``c_n`` (main only)
    and every gradient under ``yardstick``'s key.  ``before/*`` and ``after/*``: the module's default forward around the
    training call; ``status``: the workspace's time-out word.  ``mode``: "default" | "f32" | a label for a stand-in.
    ``exclude_c``: the case is out of criterion c in this mode (``C_EXCLUDED_DEFAULT``).  -> {tensor: (error against the
    yardstick, multiple of torch float32's error, multiple of the emulation's error | None)}."""
    inp = make_inputs(case) if inp is None else inp
    want, t32 = yardstick(case, np.float64), yardstick(case, np.float32)
    T, M, lens = case.T, case.M, inp["lens"]
    main = {k[len("main/"):]: v for k, v in got.items() if k.startswith("main/")}
    grads = grad_keys(case, want)
    assert sorted(main) == sorted(want), (case.id, sorted(main), sorted(want))
    live = live_mask(case)
    # b. forward
    for key in FORWARD_KEYS:
        if key in want:
            assert main[key].shape == want[key].shape, (case.id, key, main[key].shape)
            np.testing.assert_allclose(main[key], want[key], err_msg=f"{case.id} {mode} {key}", **FWD_TOL)
    assert main["out"].shape[0] == T and not np.any(np.where(live, 0, main["out"])), f"{case.id}: a padded output row is not zero"
    assert not np.any(main["out"][M:])
    for key in FORWARD_KEYS:
        if key in want:
            assert got["before/" + key].tobytes() == got["after/" + key].tobytes(), f"{case.id}: the default forward's {key} changed"
    assert int(got["status"]) == 0, f"{case.id}: a time-out word is left in the workspace"
    # c. gradients against the yardstick
    res = {}
    for key in grads:
        assert main[key].shape == want[key].shape, (case.id, key, main[key].shape, want[key].shape)
        err = rel_err(main[key], want[key])
        res[key] = [err, err / max(rel_err(t32[key], want[key]), U24), None]
    assert not np.any(np.where(live, 0, main["x"])), f"{case.id}: dx is not zero in a row past a length"
    # d. single-layer cases: against the restatement fed the device's own output
    cap = emulation_cap(case)
    if case.nl == 1:
        g64, g32 = given_h(case, main["out"], np.float64, inp), given_h(case, main["out"], np.float32, inp)
        assert sorted(g64) == sorted(grads)
        for key in grads:
            res[key][2] = rel_err(main[key], g64[key]) / max(rel_err(g32[key], g64[key]), U24)
    for key in grads:
        e, m32, memu = res[key]
        print(f"{case.id} {mode} {key}: error {e:.2e}, {m32:.2f} x torch float32" + ("" if memu is None else f", {memu:.2f} x emulation (cap {cap:.0f})"))
    for key in grads:
        if not exclude_c:
            assert res[key][0] <= REL, (case.id, mode, key, res[key][0])
        if res[key][2] is not None:
            assert res[key][2] <= cap, (case.id, mode, key, res[key][2], cap)
    # e. padding does not matter, bit for bit
    for key in grads:
        a = main[key]
        assert got["again/" + key].tobytes() == a.tobytes(), f"{case.id} {key}: two runs differ"
        short = got["short/" + key]
        if key == "x":
            assert short.shape[0] == M and not np.any(a[M:]), f"{case.id}: dx[M:] of the long buffer is not zero"
            a = np.ascontiguousarray(a[:M])
        assert short.tobytes() == a.tobytes(), f"{case.id} {key}: the buffer cut to the longest sequence gives other bits"
        for run in ("nan_x", "nan_dout"):
            assert got[f"{run}/{key}"].tobytes() == main[key].tobytes(), f"{case.id} {key}: {run} changes bits"
    return {k: tuple(v) for k, v in res.items()}
