"""The length / padding lattice of the recurrent-stack tests, defined once: tests/test_rnn_ref64_cpu.py (float32 oracle
against the float64 reference, no GPU) and tests/test_gpu_rnn_lengths.py (the kernels against the float64 reference) import
the same cases, inputs and weights from here.  numpy only: nothing of the package under test is imported.

A case = a schedule row (cell, width, directions, layers, batch) x a length pattern in a buffer of ``T`` steps whose longest
sequence has ``M = max(lens)`` steps:

  L0  M = T, ragged, shortest 1                    (the pattern every older test has: the control)
  L1  M < T, all lengths M (one odd M, one even M)
  L2  M < T, ragged with ties, shortest 1
  L3  every length 1, T > 1
  L4  (S1, S2) M on both sides of the overlapped stack's gate in a buffer well past it, equal lengths and ragged

``path`` is the schedule the case is meant to reach and the GPU test asserts through the library's predicates:
  "overlap"  ms_rnn_stack_forward (ms_rnn_stack_overlap_ok(M) == 1, rows not packed)
  "packed"   the layer loop on packed rows (ms_rnn_layer_packs_rows(M) == 1)
  "loop"     the layer loop, every row computed
What the gate arithmetic gives (segments of 1024 / N steps that must be shorter than the steps that run; rows packed from
about 1 280 rows up) is worked out in the comments next to the rows; the GPU test re-derives it at run time.

``BF16X3_CHILD`` / ``FP16_CHILD``: the cases that run once more under MS_PRECISION=bf16x3 / fp16, each with the path it takes
in that mode, and the accuracy criterion of those runs (``mode_tolerance``, ``check_mode_accuracy``), shared by the GPU children
and by the CPU test that shows the criterion's conditions.

Weights: uniform(-1 / sqrt(H), 1 / sqrt(H)), the default initialisation of torch's recurrent modules and of the hard LSTM,
drawn with numpy so that a machine without the package's device gets the same numbers.  ``gain`` = 8 multiplies weight_ih
(saturated gates); those cases are compared bit for bit only, never against a tolerance.
"""
import zlib
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "id sched kind In H bidir nl N T lens hx gain path segs")
# kind: "LSTM" | "GRU" | "TANH" | "HARD"; lens: tuple of N lengths (None for HARD: it takes none); hx: initial state given;
# path: see above; segs: extra segment counts (R._OVERLAP_SEGMENTS) under which the case must give the same bits

QUARTER_TOL = dict(rtol=2.5e-5, atol=2.5e-5)      # float32 oracle against float64 reference: a quarter of the suite's TOL


def _seed(case_id):
    return zlib.crc32(case_id.encode())


def _ragged(rng, N, M):
    """Sorted in decreasing order, longest M (twice when there is room: a tie at the top), shortest 1, ties likely."""
    lens = np.sort(rng.integers(1, M + 1, size=N))[::-1].copy()
    lens[0] = M
    if N > 2:
        lens[1] = M
    if N > 1:
        lens[-1] = 1
    if N > 3:
        lens[-2] = lens[-3]
    return tuple(int(v) for v in lens)


def _equal(N, M):
    return (int(M),) * N


_cases = []


def _add(cid, sched, kind, In, H, bidir, nl, N, T, lens, path, gain=1.0, segs=()):
    hx = len(_cases) % 2 == 0                       # half of the cases are given an initial state
    _cases.append(Case(cid, sched, kind, In, H, bidir, nl, N, T, lens, hx, gain, path, tuple(segs)))


def _patterns(sched, tag, kind, In, H, bidir, nl, N, l0, l1, l2, l3=5, paths=("loop",) * 5):
    """The patterns L0 .. L3 for one schedule row.  l0 = T (= M); l1 = (T, odd M, even M); l2 = (T, M)."""
    rng = np.random.default_rng(_seed(f"{sched}-{tag}"))
    base = f"{sched}-{tag}"
    _add(f"{base}-L0", sched, kind, In, H, bidir, nl, N, l0, _ragged(rng, N, l0), paths[0])
    _add(f"{base}-L1odd", sched, kind, In, H, bidir, nl, N, l1[0], _equal(N, l1[1]), paths[1])
    _add(f"{base}-L1even", sched, kind, In, H, bidir, nl, N, l1[0], _equal(N, l1[2]), paths[2])
    _add(f"{base}-L2", sched, kind, In, H, bidir, nl, N, l2[0], _ragged(rng, N, l2[1]), paths[3])
    _add(f"{base}-L3", sched, kind, In, H, bidir, nl, N, l3, _equal(N, 1), paths[4])


# ---- S1: LSTM 1024 bidirectional, 3 layers, 32 sequences -- the overlapped stack at the config-2 shape.  Segments are 32 steps:
# the stack overlaps from M = 33 on.  A ragged batch is packed from about 1 280 rows (M = 41): L0 stays below that, L2 above.
_patterns("S1", "lstm1024bi", "LSTM", 64, 1024, True, 3, 32, 36, (44, 35, 36), (56, 50),
          paths=("overlap", "overlap", "overlap", "packed", "loop"))
_rng = np.random.default_rng(_seed("S1-L4"))
for _M in (32, 33, 65):
    # (M = 32: the segment is not shorter than the run -> the layer loop, while the buffer's 130 steps would say "overlap")
    _add(f"S1-lstm1024bi-L4-eq{_M}", "S1", "LSTM", 64, 1024, True, 3, 32, 130, _equal(32, _M), "loop" if _M == 32 else "overlap",
         segs=(3, 16) if _M == 65 else ())
    # (ragged: 32 x 65 = 2 080 rows are packed -- that case does not reach the gate, and says so)
    _add(f"S1-lstm1024bi-L4-rag{_M}", "S1", "LSTM", 64, 1024, True, 3, 32, 130, _ragged(_rng, 32, _M),
         "loop" if _M == 32 else ("overlap" if _M == 33 else "packed"))
_add("S1-lstm1024bi-sat", "S1", "LSTM", 64, 1024, True, 3, 32, 60, _ragged(_rng, 32, 34), "overlap", gain=8.0)

# ---- S2: LSTM 1024 bidirectional, 2 layers, 4 sequences -- an 8-rank shard of a batch of 32: segments of 256 steps, the stack
# overlaps from M = 257 on; 4 sequences never reach the row count that packs.
_patterns("S2", "lstm1024bi-n4", "LSTM", 64, 1024, True, 2, 4, 260, (270, 259, 260), (270, 261),
          paths=("overlap", "overlap", "overlap", "overlap", "loop"))
_rng = np.random.default_rng(_seed("S2-L4"))
for _M in (256, 257):
    _add(f"S2-lstm1024bi-n4-L4-eq{_M}", "S2", "LSTM", 64, 1024, True, 2, 4, 501, _equal(4, _M), "loop" if _M == 256 else "overlap")
    _add(f"S2-lstm1024bi-n4-L4-rag{_M}", "S2", "LSTM", 64, 1024, True, 2, 4, 501, _ragged(_rng, 4, _M),
         "loop" if _M == 256 else "overlap")
_add("S2-lstm1024bi-n4-sat", "S2", "LSTM", 64, 1024, True, 2, 4, 300, _ragged(_rng, 4, 258), "overlap", gain=8.0)

# ---- S3: the hard LSTM takes no lengths (max_len = T); 17 sequences: segments of 60 steps, the stack overlaps from T = 61 on
for _T in (60, 61, 121):
    _add(f"S3-hard1024bi-T{_T}", "S3", "HARD", 32, 1024, True, 2, 17, _T, None, "loop" if _T == 60 else "overlap")

# ---- S4: the two-stream kernel: chained planes + one exchange initialisation per stack, no overlap
_patterns("S4", "lstm512bi", "LSTM", 64, 512, True, 2, 32, 12, (12, 7, 8), (12, 9))
_patterns("S4", "lstm768uni", "LSTM", 96, 768, False, 2, 7, 12, (12, 7, 8), (12, 9))

# ---- S5: LSTM 1024 bidirectional beyond 32 sequences: two batch groups per launch (40, 64), launches of 64 rows (96); never
# overlapped.  L2 is sized above the row count that packs (1 640 / 1 664 / 1 632 rows).
for _N, _M2 in ((40, 41), (64, 26), (96, 17)):
    _patterns("S5", f"lstm1024bi-n{_N}", "LSTM", 64, 1024, True, 2, _N, 10, (12, 7, 8), (_M2 + 4, _M2),
              paths=("loop", "loop", "loop", "packed", "loop"))
_rng = np.random.default_rng(_seed("S5-sat"))
_add("S5-lstm1024bi-n64-sat", "S5", "LSTM", 64, 1024, True, 2, 64, 14, _ragged(_rng, 64, 9), "loop", gain=8.0)

# ---- S6: the persistent GRU, chained planes
_patterns("S6", "gru1280bi", "GRU", 64, 1280, True, 2, 9, 12, (12, 7, 8), (12, 9))
_patterns("S6", "gru512uni", "GRU", 32, 512, False, 2, 32, 12, (12, 7, 8), (12, 9))

# ---- S7: hidden sizes that run zero-padded at the next width with a persistent kernel (200 -> 256, 800 -> 1024)
_patterns("S7", "lstm200bi", "LSTM", 40, 200, True, 2, 5, 12, (12, 7, 8), (12, 9))
_patterns("S7", "gru800uni", "GRU", 64, 800, False, 2, 5, 12, (12, 7, 8), (12, 9))

# ---- S8: the small widths and the tanh-RNN.  In the default precision mode a GRU of 64 units and a tanh-RNN of 48 or 200 run
# zero-padded on the persistent GRU-512 (the tanh-RNN written as a GRU); a tanh-RNN wider than every persistent GRU (2 600
# units, run at 2 624) is the one that takes a launch per step.
_patterns("S8", "gru64bi", "GRU", 24, 64, True, 2, 6, 12, (12, 7, 8), (12, 9))
_patterns("S8", "tanh200bi", "TANH", 40, 200, True, 2, 6, 12, (12, 7, 8), (12, 9))
_patterns("S8", "tanh48uni", "TANH", 24, 48, False, 2, 6, 12, (12, 7, 8), (12, 9))
_patterns("S8", "tanh2600uni", "TANH", 32, 2600, False, 2, 6, 8, (9, 5, 6), (9, 7), l3=3)

# ---- S9: MS_PRECISION=f32, read once per process: these run in one child process (test_gpu_rnn_lengths.py)
_patterns("S9", "lstm256bi-f32", "LSTM", 64, 256, True, 2, 8, 12, (12, 7, 8), (12, 9))

# ---- S10 (appended after S9 so that every earlier case keeps its place, and with it its initial state): two kernel forms no
# earlier row reaches.  lstm64bi: the one-stream split kernel at an unpadded small width (64 stays 64, planes not chained; its
# first layer's 24 features are no multiple of 32 and go through the float32 GEMM).  lstm1280bi / lstm2048uni: the two-stream
# kernel beyond 1 024 units -- 10 and 16 k-steps per wave; at 1 280 the directions run as two launches (2 x 160 workgroups
# do not fit 256 CUs), at 2 048 the lo plane of W_hh lives in 128 KB of LDS.  About 200 MB of float32 weights per case at these
# two widths.
_patterns("S10", "lstm64bi", "LSTM", 24, 64, True, 2, 6, 12, (12, 7, 8), (12, 9))
_patterns("S10", "lstm1280bi", "LSTM", 32, 1280, True, 2, 5, 12, (12, 7, 8), (12, 9))
_patterns("S10", "lstm2048uni", "LSTM", 32, 2048, False, 2, 4, 12, (12, 7, 8), (12, 9))

CASES = tuple(_cases)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
IN_PROCESS = tuple(c for c in CASES if c.sched != "S9")
F32_CHILD = tuple(c for c in CASES if c.sched == "S9")

# ---- the other two split modes, read once per process like f32: one child process each (test_gpu_rnn_lengths.py).  An entry is
# (case id, the path the case takes IN THAT MODE).  MS_PRECISION=bf16x3 changes operand formats only, so every case keeps its
# path.  Under MS_PRECISION=fp16 rows never pack (the one-plane kernels read dense rows): a case whose default path is
# "packed" takes the overlapped stack where the stack gate admits it (S1-L2: 32 sequences, 50 steps > 32) and the layer loop
# elsewhere (S5: more than 32 sequences are never overlapped).
_L = ("L0", "L1odd", "L1even", "L2", "L3")
_S1 = tuple(f"S1-lstm1024bi-{p}" for p in ("L0", "L1odd", "L2", "L3", "L4-eq33", "L4-eq65", "sat"))
_S4 = tuple(f"S4-lstm512bi-{p}" for p in _L) + ("S4-lstm768uni-L2",)
_S5 = tuple(f"S5-lstm1024bi-n40-{p}" for p in _L)
_S7 = ("S7-lstm200bi-L0", "S7-lstm200bi-L2")
_BF16X3_IDS = (_S1 + ("S3-hard1024bi-T61",) + _S4 + _S5 + ("S6-gru1280bi-L0", "S6-gru1280bi-L2", "S6-gru512uni-L2") + _S7
               + ("S7-gru800uni-L2", "S8-gru64bi-L2", "S8-tanh200bi-L2", "S8-tanh2600uni-L2")
               + tuple(f"S10-{t}-{p}" for t in ("lstm64bi", "lstm1280bi", "lstm2048uni") for p in _L))
_FP16_IDS = (_S1 + ("S3-hard1024bi-T61",) + _S4 + _S5 + ("S5-lstm1024bi-n96-L0", "S5-lstm1024bi-n96-L2") + _S7
             + ("S10-lstm64bi-L2", "S6-gru512uni-L2"))
_FP16_UNPACKED = {"S1-lstm1024bi-L2": "overlap", "S5-lstm1024bi-n40-L2": "loop", "S5-lstm1024bi-n96-L2": "loop"}
BF16X3_CHILD = tuple((i, BY_ID[i].path) for i in _BF16X3_IDS)
FP16_CHILD = tuple((i, _FP16_UNPACKED.get(i, BY_ID[i].path)) for i in _FP16_IDS)
MODE_CHILD = {"bf16x3": BF16X3_CHILD, "fp16": FP16_CHILD}
assert all(p != "packed" for _, p in FP16_CHILD)
assert {i for i in _FP16_IDS if BY_ID[i].path == "packed"} == set(_FP16_UNPACKED)
# Cases that show a documented property of a mode instead of a fault: kept under every bit check, left out of the accuracy
# check (mode -> {case id: reason}); more than two per mode would mean the criterion is wrong, not the cases.
MODE_EXCLUDED = {"bf16x3": {}, "fp16": {}}
MODE_FLOOR = 1e-4      # the suite's tolerance: a mode is never held tighter than the default mode


def mode_tolerance(emu, ref):
    """The accuracy criterion of the mode children, from the reference side alone: E = max |emu - ref| / (1 + |ref|) of the
    operand-rounding emulation (rnn_ref64, ``operands=``) against the float64 reference -> (E, rtol = atol = max(1e-4, 2 E)).
    The emulation and the device are two realisations of one rounding process (float64 against float32 sums, so near-ties on
    the operand grids fall differently); their distances from the reference are expected to be equal and the factor allows
    one to be twice the other."""
    emu, ref = np.asarray(emu, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    e = float((np.abs(emu - ref) / (1.0 + np.abs(ref))).max())
    return e, max(MODE_FLOOR, 2.0 * e)
GATE_SETS = {      # L4: the cases of one gate, by the form of their lengths
    "S1-eq": tuple(f"S1-lstm1024bi-L4-eq{m}" for m in (32, 33, 65)), "S1-rag": tuple(f"S1-lstm1024bi-L4-rag{m}" for m in (32, 33, 65)),
    "S2-eq": tuple(f"S2-lstm1024bi-n4-L4-eq{m}" for m in (256, 257)), "S2-rag": tuple(f"S2-lstm1024bi-n4-L4-rag{m}" for m in (256, 257)),
}


def steps_of(case):
    return case.T if case.lens is None else max(case.lens)


def gates_of(kind):
    return {"LSTM": 4, "HARD": 4, "GRU": 3, "TANH": 1}[kind]


def make_params(case):
    """The case's parameters as float32 arrays under the module's state_dict names (without the ``rnn.`` prefix)."""
    rng = np.random.default_rng(_seed(case.id) ^ 0x5EED)
    H, D, G = case.H, 2 if case.bidir else 1, gates_of(case.kind)
    k = 1.0 / np.sqrt(H)
    sd = {}
    for layer in range(case.nl):
        in_size = case.In if layer == 0 else D * H
        for d in range(D):
            if case.kind == "HARD":
                pre = f"layers.{layer}." + (("fwd." if d == 0 else "bwd.") if case.bidir else "") + "cell."
                names = [pre + n for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            else:
                sfx = f"_l{layer}" + ("_reverse" if d else "")
                names = [n + sfx for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            for name, shape in zip(names, ((G * H, in_size), (G * H, H), (G * H,), (G * H,))):
                w = rng.uniform(-k, k, size=shape).astype(np.float32)
                if "weight_ih" in name:
                    w *= np.float32(case.gain)
                sd[name] = w
    return sd


def make_inputs(case):
    """-> (x [T, N, In] float32, lens int64 [N] | None, hx): hx is None, an array (GRU, tanh) or a pair (LSTM, hard)."""
    rng = np.random.default_rng(_seed(case.id))
    x = rng.normal(size=(case.T, case.N, case.In)).astype(np.float32)
    lens = None if case.lens is None else np.asarray(case.lens, dtype=np.int64)
    hx = None
    if case.hx:
        shape = (case.nl * (2 if case.bidir else 1), case.N, case.H)
        h0 = (rng.normal(size=shape) * 0.4).astype(np.float32)
        hx = (h0, (rng.normal(size=shape) * 0.4).astype(np.float32)) if case.kind in ("LSTM", "HARD") else h0
    return x, lens, hx


def padding_mask(case):
    """[T, N] bool: True where a frame lies at or beyond its sequence's length."""
    return np.arange(case.T)[:, None] >= np.asarray(case.lens)[None, :]


def check_mode_accuracy(case, mode, got, ref, emu):
    """Check 1 of a mode's child: ``got``, ``ref``, ``emu`` are (out[:M], h_n, c_n | None) of the device, the float64 reference
    and the emulation.  Prints E, the device's distance and their ratio per quantity; -> [(name, E, device, tolerance)]."""
    rows = []
    for name, g, r, e in zip(("out", "h_n", "c_n"), got, ref, emu):
        if r is None:
            continue
        g = np.asarray(g, dtype=np.float64)
        assert g.shape == r.shape == e.shape, (case.id, name, g.shape, r.shape)
        err, tol = mode_tolerance(e, r)
        dev = float((np.abs(g - r) / (1.0 + np.abs(r))).max())
        print(f"{mode} {case.id} {name}: E = {err:.3e}  device = {dev:.3e}  device / E = {dev / max(err, 1e-300):.2f}"
              f"  tolerance = {tol:.3e}")
        if case.id not in MODE_EXCLUDED[mode]:
            np.testing.assert_allclose(g, r, rtol=tol, atol=tol, err_msg=f"{mode} {case.id} {name}")
        rows.append((name, err, dev, tol))
    return rows
