"""The RNN-T decode on the device at every kernel gate (tests/rnnt_decode_cases.py) against the float64 reference with decision
margins (tests/rnnt_decode_ref.py).

Every case's smallest decision gap is at least 1e-3 (asserted on the CPU, test_rnnt_decode_cpu.py), ten times the 1e-4 the
beam's scores are held to, so the transcripts are asserted EQUAL with no escape clause: a mismatch is a finding about a kernel,
never a near-tie."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnnt_decode_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-4, atol=1e-4)       # test_rnnt_device_decode_sweep's tolerance on the beam's scores
SENTINEL = -77


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def built(c):
    pred, joint, _, _, enc = C.parts(c)
    return pred, joint, enc


def raw_decode(pred, joint, enc, lens, w, ms, greedy, null_bias=False, V=None, short_by=0, ws_bytes=None):
    """``ms_rnnt_decode`` called directly (what ``post_process.rnnt_decoder._decode`` does, plus NULL biases, a vocabulary size
    of the caller's choosing, a short workspace): outputs are pre-filled with SENTINEL.  Returns (return code, transcripts,
    scores, raw outputs)."""
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    lens = np.asarray(lens)
    steps, n = int(lens.max()), len(lens)
    enc_p = joint.project_encoder(T(enc))
    rnn = pred.rnn.rnn
    L, H, D = pred.num_layers, pred.hidden_size, pred.embedding.weight.shape[1]
    V = pred.vocab_size if V is None else V
    J = joint.out.weight.shape[1]
    keep = []

    def col(name, null=False):
        ts = [None if null else _lib.f32c(getattr(rnn, f"{name}_l{l}").detach()) for l in range(L)]
        arr = (ctypes.c_void_p * L)(*[None if t is None else t.data_ptr() for t in ts])
        keep.extend([ts, arr])
        return ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))

    emb = _lib.f32c(pred.embedding.weight.detach())
    w_pred, w_out = _lib.f32c(joint.pred_proj.weight.detach()), _lib.f32c(joint.out.weight.detach())
    b_out = _lib.f32c(joint.out.bias.detach())
    lens_d = _lib.lens_i32(T(lens).to(torch.int64))
    stride = steps * ms if greedy else steps * max(ms - 1, 0) + 1
    out_idx = torch.full((n, stride), SENTINEL, dtype=torch.int32, device="cuda")
    out_len = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    out_score = torch.full((n,), float(SENTINEL), dtype=torch.float32, device="cuda")
    if ws_bytes is None:
        ws_bytes = lib.ms_rnnt_decode_workspace_bytes(steps, n, V, D, H, L, J, w, ms, int(greedy))
        assert ws_bytes > 0
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    rc = lib.ms_rnnt_decode(_lib.ptr(enc_p), _lib.ptr(lens_d), _lib.ptr(emb), col("weight_ih"), col("weight_hh"),
                            col("bias_ih", null_bias), col("bias_hh", null_bias), _lib.ptr(w_pred), _lib.ptr(w_out),
                            _lib.ptr(b_out), _lib.ptr(out_idx), _lib.ptr(out_len), _lib.ptr(out_score), steps, n, V, D, H, L, J, w,
                            ms, int(greedy), _lib.ptr(ws), ws_bytes - short_by, _lib.stream_ptr())
    torch.cuda.synchronize()
    lens_out, idx = out_len.cpu().tolist(), out_idx.cpu()
    hyps = [idx[i, :max(0, min(lens_out[i], stride))].tolist() for i in range(n)]
    return rc, hyps, out_score.cpu().tolist(), (idx, lens_out)


def decode(c, pred=None, joint=None, enc=None, lens=None):
    """(transcripts, scores or None) of a case on the device, through the decoder modules (NULL biases: the direct call)."""
    from myrtlespeech_amd.post_process.rnnt_decoder import RNNTBeamDecoder, RNNTGreedyDecoder
    if pred is None:
        pred, joint, enc = built(c)
    lens = c.lengths if lens is None else lens
    if c.zero_bias:
        rc, hyps, scores, _ = raw_decode(pred, joint, enc, lens, c.w, c.ms, c.greedy, null_bias=True)
        assert rc == 0
        return hyps, (None if c.greedy else scores)
    if c.greedy:
        return RNNTGreedyDecoder(pred, joint, max_symbols=c.ms)(T(enc), T(lens)), None
    dec = RNNTBeamDecoder(pred, joint, beam_width=c.w, max_symbols=c.ms)
    return dec(T(enc), T(lens)), dec.last_scores


def check(c, hyps, scores, ref=None, rows=None):
    ref = C.reference(c) if ref is None else ref
    rows = range(len(ref)) if rows is None else rows
    want = [ref[n]["hyp"] for n in rows]
    if scores is not None:
        live = [k for k, n in enumerate(rows) if c.lengths[n] > 0]           # (no score is defined for an utterance without frames)
        got_s, want_s = [scores[k] for k in live], [ref[rows[k]]["score"] for k in live]
        print(c.id, "score error", float(np.abs(np.array(got_s) - np.array(want_s)).max()) if live else 0.0)
        assert hyps == want, (c.id, c.gate)
        np.testing.assert_allclose(got_s, want_s, **TOL)
    assert hyps == want, (c.id, c.gate)


@pytest.mark.parametrize("c", C.CASES, ids=[c.id for c in C.CASES])
def test_case_equals_the_float64_reference(c):
    hyps, scores = decode(c)
    check(c, hyps, scores)


@pytest.mark.parametrize("name", ["greedy_zero_mid", "recut_L3_fused_R40", "round4_zero_mid", "recut_w24"])
def test_every_utterance_alone_decodes_as_in_its_batch(name):
    """Not bitwise: R = N w changes the kernel form (32- against 64-row groups, one row block against two)."""
    c = C.BY_ID[name]
    pred, joint, enc = built(c)
    ref = C.reference(c)
    for n in range(c.N):
        ln = int(c.lengths[n])
        hyps, scores = decode(c, pred, joint, enc[:max(ln, 1), n:n + 1], c.lengths[n:n + 1])
        check(c, hyps, scores, ref, rows=[n])


@pytest.mark.parametrize("big,small", [("recut_LH2240", "recut_T1"), ("recut_w32_ms4", "recut_L1"), ("round4_V479_w32", "round4_T1"),
                                       ("greedy_joint_64KB", "greedy_T1")])
def test_a_used_workspace_decodes_like_a_fresh_one(big, small):
    """One decoder object (one workspace) decodes the largest case and then the smallest: nothing stale may be read."""
    from myrtlespeech_amd.post_process.rnnt_decoder import RNNTBeamDecoder, RNNTGreedyDecoder
    cb, cs = C.BY_ID[big], C.BY_ID[small]
    pred, joint, enc = built(cb)
    dec = RNNTGreedyDecoder(pred, joint, max_symbols=cb.ms) if cb.greedy else RNNTBeamDecoder(pred, joint, cb.w, cb.ms)
    check(cb, dec(T(enc), T(cb.lengths)), None if cb.greedy else dec.last_scores)
    used = dec._ws.buf.numel()
    pred, joint, enc = built(cs)
    dec.predictor, dec.joint, dec.max_symbols = pred, joint, cs.ms
    if not cs.greedy:
        dec.beam_width = cs.w
    got = dec(T(enc), T(cs.lengths))
    assert dec._ws.buf.numel() == used                                      # the same, larger, buffer served the small case
    fresh, fresh_scores = decode(cs)
    assert got == fresh
    if not cs.greedy:
        assert dec.last_scores == fresh_scores                                # same kernels, same order of additions: same bits
    check(cs, got, None if cs.greedy else dec.last_scores)


RECUT = [c for c in C.CASES if c.dispatch["sequence"] == "recut" and not c.zero_bias]


@pytest.mark.parametrize("c", RECUT, ids=[c.id for c in RECUT])
def test_three_plane_operands_decode_the_same(c, monkeypatch):
    """MS_RNNT_PLANES=3 (the exact three-bf16 operands; the library reads the variable on every call)."""
    monkeypatch.setenv("MS_RNNT_PLANES", "3")
    hyps, scores = decode(c)
    check(c, hyps, scores)


def _small_parts(V):
    from myrtlespeech_amd.model.rnnt import RNNTJoint, RNNTPredictor
    torch.manual_seed(0)
    pred, joint = RNNTPredictor(V, 8, 64, num_layers=2).eval(), RNNTJoint(C.E, 64, 48, V).eval()
    enc = np.random.default_rng(0).normal(size=(4, 2, C.E)).astype(np.float32)
    return pred, joint, enc, np.array([4, 3])


@pytest.mark.parametrize("what,V,w,ms,short_by,message", [
    ("w * max_symbols = 129", 6, 3, 43, 0, "128"),
    ("w = 33", 6, 33, 2, 0, "beam_width"),
    ("V = 480 at w = 32", 480, 32, 2, 0, "LDS"),
    ("a workspace one byte short", 6, 4, 3, 1, "workspace")])
def test_refused_calls_say_why_and_touch_nothing(what, V, w, ms, short_by, message):
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    pred, joint, enc, lens = _small_parts(V)
    ok_bytes = lib.ms_rnnt_decode_workspace_bytes(4, 2, V, 8, 64, 2, 48, min(w, 32), min(ms, 128 // min(w, 32)), 0)
    assert ok_bytes > 0
    if w > 32:
        assert lib.ms_rnnt_decode_workspace_bytes(4, 2, V, 8, 64, 2, 48, w, ms, 0) == 0
    rc, _, scores, (idx, lens_out) = raw_decode(pred, joint, enc, lens, w, ms, False, ws_bytes=2 * ok_bytes if not short_by else None,
                                                short_by=short_by)
    assert rc != 0, what
    assert message in lib.ms_last_error().decode(), (what, lib.ms_last_error().decode())
    assert lens_out == [SENTINEL] * 2 and scores == [float(SENTINEL)] * 2 and bool((idx == SENTINEL).all())
    assert lib.ms_rnnt_decode_last_iterations() == 0
    # ... and the same arguments on the legal side decode
    if what.startswith("a workspace"):
        rc, hyps, _, _ = raw_decode(pred, joint, enc, lens, w, ms, False)
        assert rc == 0 and all(isinstance(h, list) for h in hyps)


@pytest.mark.parametrize("name", ["greedy_exit_len0", "greedy_exit_len1"])
def test_greedy_decode_stops_when_every_utterance_has_finished(name):
    """The event-driven exit.  An utterance is finished when its frame reaches its length -- an empty one from the start -- and
    the host looks at the device's count of finished utterances after every second iteration (CHECK_EVERY = 2), reading the copy
    it requested two looks earlier: look k (after iteration 2 k, k >= 3) sees the count as of iteration 2 (k - 2) and stops if
    that is N.  With `needed` iterations of work the first such look is k = ceil(needed / 2) + 2, at least the third, so
    launched = 2 k <= max(needed + 5, 6) <= needed + 6; the assertion allows needed + 8 (2 CHECK_EVERY + the ring of 4).
    Before the fix greedy_init_kernel did not count the empty utterance, greedy_scan_kernel never does (it leaves at
    `t0 >= len`), the count stayed below N and all T max_symbols + T / 32 + 1 = 1291 iterations were launched."""
    from myrtlespeech_amd import _lib
    from myrtlespeech_amd.post_process.rnnt_decoder import RNNTBeamDecoder, RNNTGreedyDecoder
    lib = _lib.load()
    c = C.BY_ID[name]
    pred, joint, enc = built(c)
    ref = C.reference(c)
    needed = max(u["iterations"] for u in ref)
    assert needed == 10
    got = RNNTGreedyDecoder(pred, joint, max_symbols=c.ms)(T(enc), T(c.lengths))
    launched = lib.ms_rnnt_decode_last_iterations()
    print(name, "needed", needed, "launched", launched, "bound", c.T * c.ms + (c.T + 31) // 32 + 1)
    assert got == [u["hyp"] for u in ref] == [[]] * c.N
    assert 0 < launched <= needed + 8
    RNNTBeamDecoder(pred, joint, beam_width=2, max_symbols=2)(T(enc[:4]), T(np.array([4, 3, 0, 2])))
    assert lib.ms_rnnt_decode_last_iterations() == 0                        # a beam call enqueues no greedy iteration
