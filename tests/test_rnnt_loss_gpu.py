"""Transducer loss on the device (``ms_rnnt_loss_forward`` / ``ms_rnnt_loss_backward``, ``RNNTLoss``, ``RNNT.joint_lattice``)
against the float64 numpy restatement of its specification (tests/rnnt_loss_ref.py), per utterance:

  B_n = 8 (T_n + U_n) 2^-24 max(1, |nll_n|)   for nll, and for alpha / beta on the existing cells -- the depth of the recursion
                                              times one rounding of the running sum, a factor 8 for the hardware exp / log
                                              forms (the argument of tests/test_ctc_align_gpu.py)
  4 B_n |grad_nll[n]|                          absolute, for the gradient

Z is not part of the recursion's budget; it is held to 16 * 2^-24 max(1, |Z|): the rounding of max + log(sum), the precise
logf, and a sum of V1 hardware exps whose relative errors are weighted by the softmax itself.
The float32 restatement sits at 0.051 / 0.131 / 0.137 / 0.012 of these bounds at worst (tests/test_rnnt_loss_cpu.py); the
device's worst ratios are printed by every test here and recorded by tools/rnnt_loss_time.py in profiles/rnnt_loss_time.json
-- not measured yet.
"""
import numpy as np
import pytest
import torch

import rnnt_loss_ref as R
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
CASES = R.gpu_cases()
_ref64 = {}
worst = {"nll": 0.0, "alpha": 0.0, "beta": 0.0, "grad": 0.0, "Z": 0.0}


def ref64(name):
    """The float64 restatement of a case with grad_nll = 1 (the gradient is linear in grad_nll): computed once, never edited."""
    if name not in _ref64:
        c = CASES[name]
        _ref64[name] = R.rnnt_loss(c["logits"], c["in_lens"], c["targets"], c["tgt_lens"], c["blank"])
    return _ref64[name]


def i32(a):
    return torch.as_tensor(np.ascontiguousarray(a).reshape(-1), dtype=torch.int32).cuda()


def run_abi(logits, in_lens, targets, tgt_lens, blank, grad_nll=None, backward=True):
    """One forward (and one backward) call on the current stream; nll, the lattice and grad are pre-filled with a sentinel.
    Returns numpy arrays exactly as the device wrote them: nll [N], lattice [3, N, T, U1], grad [N, T, U1, V1] (or None)."""
    lib = _lib.load()
    x = logits if torch.is_tensor(logits) else torch.as_tensor(np.asarray(logits), dtype=torch.float32).cuda().contiguous()
    N, T, U1, V1 = x.shape
    xl, yl = i32(in_lens), i32(tgt_lens)
    y = i32(targets) if U1 > 1 else None
    nll = torch.full((N,), SENTINEL, dtype=torch.float32, device="cuda")
    assert lib.ms_rnnt_loss_lattice_bytes(N, T, U1) == 12 * N * T * U1
    lattice = torch.full((3, N, T, U1), SENTINEL, dtype=torch.float32, device="cuda")
    nbytes = lib.ms_rnnt_loss_workspace_bytes(N, T, U1, V1)
    ws = torch.full((max(nbytes, 256),), 0xFF, dtype=torch.uint8, device="cuda")       # NaN bit patterns: nothing relies on it
    _lib.check(lib.ms_rnnt_loss_forward(_lib.ptr(x), _lib.ptr(xl), _lib.ptr(y), _lib.ptr(yl), _lib.ptr(nll), _lib.ptr(lattice),
                                        N, T, U1, V1, blank, _lib.ptr(ws), nbytes, _lib.stream_ptr()), "ms_rnnt_loss_forward")
    grad = None
    if backward:
        del ws                                                    # the workspace is transient: the backward has no use for it
        g = torch.ones(N, device="cuda") if grad_nll is None else torch.as_tensor(np.asarray(grad_nll), dtype=torch.float32).cuda()
        grad = torch.full((N, T, U1, V1), SENTINEL, dtype=torch.float32, device="cuda")
        _lib.check(lib.ms_rnnt_loss_backward(_lib.ptr(x), _lib.ptr(xl), _lib.ptr(y), _lib.ptr(yl), _lib.ptr(nll),
                                             _lib.ptr(lattice), _lib.ptr(g), _lib.ptr(grad), N, T, U1, V1, blank,
                                             _lib.stream_ptr()), "ms_rnnt_loss_backward")
    torch.cuda.synchronize()
    return nll.cpu().numpy(), lattice.cpu().numpy(), (None if grad is None else grad.cpu().numpy())


def run_case(c, **kw):
    return run_abi(c["logits"], c["in_lens"], c["targets"], c["tgt_lens"], c["blank"], **kw)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_against(ref, out, in_lens, tgt_lens, grad_nll, name):
    """Every output of the utterances with a finite reference nll inside its bound; prints and records the ratios."""
    nll, lattice, grad = out
    g = np.ones(len(ref.nll)) if grad_nll is None else np.asarray(grad_nll, dtype=np.float64)
    scaled = ref._replace(grad=ref.grad * g[:, None, None, None])
    w = R.worst_ratios(nll, lattice[1], lattice[2], grad, scaled, in_lens, tgt_lens, grad_nll=g)
    fin = np.isfinite(ref.nll)
    ex = ref.exists & fin[:, None, None]
    w["Z"] = float(np.max(np.abs(lattice[0][ex] - ref.Z[ex]) / (16 * 2.0 ** -24 * np.maximum(1.0, np.abs(ref.Z[ex])))))
    for k, v in w.items():
        worst[k] = max(worst[k], v)
    print(f"{name}: ratios to the bounds {({k: round(v, 4) for k, v in w.items()})}  nll {np.round(nll, 4).tolist()}")
    print("worst ratios so far", {k: round(v, 4) for k, v in worst.items()})
    assert w["nll"] <= 1.0 and w["alpha"] <= 1.0 and w["beta"] <= 1.0 and w["grad"] <= 1.0 and w["Z"] <= 1.0, (name, w)
    # (l) grad is fully written, and exactly 0 in every cell that does not exist
    assert not (grad == SENTINEL).any()
    assert (grad[~ref.exists] == 0).all()
    return w


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_within_the_bounds(name):
    """(a) ragged with U = 0 and T = 1, (b) U1 = 70 crosses a wave, (c) several waves and barriers, (d) U1 = 1024, the supported
    edge, (e) an odd, long row, (f) small nll and a tight bound, (g) a -inf symbol column off the target.  A non-unit grad_nll."""
    c, ref = CASES[name], ref64(name)
    N = len(c["in_lens"])
    grad_nll = np.random.default_rng(17).uniform(0.5, 2.0, size=N).astype(np.float32) * np.where(np.arange(N) % 2, -1, 1)
    out = run_case(c, grad_nll=grad_nll)
    check_against(ref, out, c["in_lens"], c["tgt_lens"], grad_nll, name)
    if name == "g_inf_column":
        assert np.isfinite(out[0]).all() and np.isfinite(out[2]).all()
        assert (out[2][..., 2] == 0).all()                       # the impossible symbol's gradient is exactly 0
    if name == "f_peaked":
        assert (out[0] < 20).all()


def test_a_target_padding_and_lattice_padding_change_no_bit():
    """(a) second run: out-of-range values in the target padding; (j): NaN, +inf and garbage in every cell that does not exist,
    for (a) and (b).  (k): two runs give the same bits."""
    for name in ("a_ragged", "b_cross_wave"):
        c = CASES[name]
        clean = run_case(c)
        again = run_case(c)
        assert all(same_bits(p, q) for p, q in zip(clean, again)), name                       # (k)
        pad = dict(c, targets=R.pad_targets(c["targets"], c["tgt_lens"], 0))
        for n, un in enumerate(c["tgt_lens"]):
            pad["targets"][n, un:] = [(-7, 1 << 30, c["blank"], 10 ** 6)[(n + k) % 4] for k in range(c["targets"].shape[1] - un)]
        out = run_case(pad)
        assert all(same_bits(p, q) for p, q in zip(clean, out)), name
        exists = ref64(name).exists
        dirty = c["logits"].copy()
        fill = np.resize(np.array([np.nan, np.inf, -np.inf, 3e38, -1e30, 7.0], dtype=np.float32), dirty[~exists].shape)
        dirty[~exists] = fill
        assert np.isnan(dirty).any() and (~exists).any()
        out = run_case(dict(pad, logits=dirty))
        assert all(same_bits(p, q) for p, q in zip(clean, out)), name                         # (j)


def test_h_impossible_transcript_gives_inf_and_a_zero_gradient():
    c = CASES["g_inf_column"]
    x = c["logits"].copy()
    needed = int(c["targets"][0, 1])
    x[0, :, :, needed] = -np.inf                                 # a label utterance 0 needs, impossible everywhere
    nll, lattice, grad = run_abi(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"], grad_nll=[1.5, -0.5])
    assert nll[0] == np.inf and (grad[0] == 0).all() and not (grad == SENTINEL).any()
    ref = R.rnnt_loss(x, c["in_lens"], c["targets"], c["tgt_lens"], c["blank"])
    assert ref.nll[0] == np.inf
    if np.isfinite(ref.nll[1]):                                  # utterance 1 does not need that label: untouched, in bound
        check_against(ref, (nll, lattice, grad), c["in_lens"], c["tgt_lens"], [1.5, -0.5], "h (utterance 1)")


def test_i_nan_poisons_its_own_utterance_only():
    c, ref = CASES["b_cross_wave"], ref64("b_cross_wave")
    for bad in (np.nan, np.inf):
        x = c["logits"].copy()
        x[0, 17, 33, 5] = bad                                    # an existing cell of utterance 0, a symbol off the recursion
        nll, lattice, grad = run_case(dict(c, logits=x), grad_nll=[2.0, 0.75])
        assert np.isnan(nll[0])
        assert np.isnan(grad[0][ref.exists[0]]).all() and (grad[0][~ref.exists[0]] == 0).all()
        only1 = ref._replace(nll=np.array([np.nan, ref.nll[1]]))
        check_against(only1, (nll, lattice, grad), c["in_lens"], c["tgt_lens"], [2.0, 0.75], f"i ({bad})")
    x = c["logits"].copy()
    x[0, 17, 33, :] = -np.inf                                    # a row of -inf only: Z is not finite
    assert np.isnan(run_case(dict(c, logits=x), backward=False)[0][0])


def test_the_callers_errors_give_inf_and_read_nothing_out_of_bounds():
    c = CASES["a_ragged"]
    clean = run_case(c)
    y = c["targets"].copy()
    y[0, 1], y[3, 0] = 10 ** 6, c["blank"]                        # a label past V1; a label equal to the blank
    nll, _, grad = run_abi(c["logits"], [7, 0, 8, 3], y, [4, 0, 5, 2], c["blank"])
    assert (nll == np.inf).all() and (grad == 0).all()
    nll, _, grad = run_abi(c["logits"], [7, 5, 1, 3], c["targets"], [4, -1, 3, 2], c["blank"])
    assert nll[1] == np.inf and (grad[1] == 0).all()
    assert all(same_bits(nll[[n]], clean[0][[n]]) and same_bits(grad[n], clean[2][n]) for n in (0, 2, 3))
    # past the supported shapes: MS_ERR_UNSUPPORTED, nothing launched (the outputs keep what they held)
    lib = _lib.load()
    x = torch.zeros((1, 1, 1025, 2), device="cuda")
    out = torch.full((1,), SENTINEL, device="cuda")
    lat = torch.full((3 * 1025,), SENTINEL, device="cuda")
    ws = torch.empty(lib.ms_rnnt_loss_workspace_bytes(1, 1, 1025, 2), dtype=torch.uint8, device="cuda")
    one, yy = i32([1]), i32(np.zeros(1024))
    rc = lib.ms_rnnt_loss_forward(_lib.ptr(x), _lib.ptr(one), _lib.ptr(yy), _lib.ptr(one), _lib.ptr(out), _lib.ptr(lat), 1, 1, 1025,
                                  2, 1, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert _lib.ERR_NAMES[rc] == "MS_ERR_UNSUPPORTED"
    rc = lib.ms_rnnt_loss_backward(_lib.ptr(x), _lib.ptr(one), _lib.ptr(yy), _lib.ptr(one), _lib.ptr(out), _lib.ptr(lat),
                                   _lib.ptr(out), _lib.ptr(x), 1, 1, 1025, 2, 1, _lib.stream_ptr())
    assert _lib.ERR_NAMES[rc] == "MS_ERR_UNSUPPORTED"
    torch.cuda.synchronize()
    assert float(out[0]) == SENTINEL and bool((lat == SENTINEL).all()) and bool((x == 0).all())


def test_u1_equal_1_takes_null_targets_and_blank_need_not_be_last():
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((3, 5, 1, 6)) * 3).astype(np.float32)
    y = np.zeros((3, 0), dtype=np.int32)
    out = run_abi(x, [5, 1, 3], y, [0, 0, 0], 2, grad_nll=[1.0, 2.0, -1.0])
    check_against(R.rnnt_loss(x, [5, 1, 3], y, [0, 0, 0], 2), out, [5, 1, 3], [0, 0, 0], [1.0, 2.0, -1.0], "U1 = 1")
    x = (rng.standard_normal((2, 6, 4, 8)) * 3).astype(np.float32)            # V1 = 8: float4 rows, eight lanes per row
    y = R.random_targets(rng, 2, 3, 8, 0)
    out = run_abi(x, [6, 4], y, [3, 2], 0)
    check_against(R.rnnt_loss(x, [6, 4], y, [3, 2], 0), out, [6, 4], [3, 2], None, "blank = 0, V1 = 8")
    # the same rows at an address that is not 16-byte aligned: the scalar path gives the same values within the bounds
    flat = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.as_tensor(x).reshape(-1).cuda()
    out = run_abi(flat[1:].reshape(x.shape), [6, 4], y, [3, 2], 0)
    check_against(R.rnnt_loss(x, [6, 4], y, [3, 2], 0), out, [6, 4], [3, 2], None, "unaligned rows")


def test_m_autograd_node_matches_the_abi_backward(monkeypatch):
    from myrtlespeech_amd.loss.rnnt_loss import RNNTLoss
    c = CASES["a_ragged"]
    N = len(c["in_lens"])
    xl, yl = torch.as_tensor(c["in_lens"]), torch.as_tensor(c["tgt_lens"])
    y = torch.as_tensor(c["targets"]).to(torch.int64)
    nll_abi = run_case(c, backward=False)[0]
    up = torch.tensor([0.5, -2.0, 3.0, 1.5])
    for reduction, grad_nll in (("none", up), ("sum", torch.full((N,), 1.75)), ("mean", torch.full((N,), 1.75) / N)):
        x = torch.as_tensor(c["logits"]).cuda().requires_grad_()
        loss = RNNTLoss(c["blank"], reduction)((x, xl), (y.cuda() if reduction == "sum" else y, yl))
        want = {"none": nll_abi, "sum": nll_abi.sum(dtype=np.float32), "mean": nll_abi.sum(dtype=np.float32) / N}[reduction]
        np.testing.assert_allclose(loss.detach().cpu().numpy(), want, rtol=1e-6)
        if reduction == "none":
            assert same_bits(loss.detach().cpu().numpy(), nll_abi)
            loss.backward(up.cuda())
        else:
            (loss * 1.75).backward()
        want_grad = run_case(c, grad_nll=grad_nll.numpy())[2]
        assert same_bits(x.grad.cpu().numpy(), want_grad), reduction
    # no gradient work when the logits do not require grad (or grad mode is off)
    lib = _lib.load()
    calls = []
    real = lib.ms_rnnt_loss_backward
    monkeypatch.setattr(lib, "ms_rnnt_loss_backward", lambda *a: calls.append(1) or real(*a))
    x = torch.as_tensor(c["logits"]).cuda()
    out = RNNTLoss(c["blank"], "mean")((x, xl), (y, yl))
    assert out.grad_fn is None and not out.requires_grad
    with torch.no_grad():
        out = RNNTLoss(c["blank"], "sum")((x.clone().requires_grad_(), xl), (y, yl))
    assert out.grad_fn is None and calls == []
    x.requires_grad_()
    RNNTLoss(c["blank"], "sum")((x, xl), (y, yl)).backward()
    assert calls == [1]                                           # (the counter does see a backward)


def test_n_end_to_end_beam_score_is_below_the_loss_of_its_hypothesis():
    """The beam sums a subset of its hypothesis's alignments, the loss all of them (premise: tests/test_rnnt_loss_cpu.py)."""
    import test_rnnt_loss_cpu as C
    from myrtlespeech_amd.loss.rnnt_loss import RNNTLoss
    from myrtlespeech_amd.model.rnnt import RNNT
    from myrtlespeech_amd.post_process.rnnt_decoder import RNNTBeamDecoder
    pred, joint, enc, lens = C.tiny_transducer()
    model = RNNT(torch.nn.Identity(), pred, joint)
    dec = RNNTBeamDecoder(pred, joint)
    hyps = dec(enc.cuda(), lens)
    scores = dec.last_scores
    assert any(len(h) > 0 for h in hyps)
    u_max = max(len(h) for h in hyps)
    y = torch.full((len(hyps), u_max), -3, dtype=torch.int64)     # the padding is never a label
    for n, h in enumerate(hyps):
        y[n, :len(h)] = torch.tensor(h, dtype=torch.int64)
    y_lens = torch.tensor([len(h) for h in hyps])
    lattice = model.joint_lattice(enc.cuda(), lens, y, y_lens)
    assert lattice.shape == (3, 12, u_max + 1, 9) and not lattice.requires_grad
    nll = RNNTLoss(blank=8, reduction="none")((lattice, lens), (y, y_lens)).cpu().numpy()
    lat = lattice.cpu().numpy()
    ref = R.rnnt_loss(lat, lens.numpy(), y.numpy(), y_lens.numpy(), 8)
    psd = {k: v.detach().cpu().numpy() for k, v in pred.state_dict().items()}
    jsd = {k: v.detach().cpu().numpy() for k, v in joint.state_dict().items()}
    for n, h in enumerate(hyps):
        Tn = int(lens[n])
        print(f"utterance {n}: hypothesis {h} beam score {scores[n]:.5f} -nll {-nll[n]:.5f} restatement {-ref.nll[n]:.5f}")
        assert -nll[n] >= scores[n] - 1e-4
        assert abs(nll[n] - ref.nll[n]) <= R.bound(Tn, len(h), ref.nll[n])
        want = C.oracle_joint_lattice(psd, jsd, enc.numpy()[:Tn, n], h, 32, 1, 8)
        np.testing.assert_allclose(lat[n, :Tn, :len(h) + 1], want, rtol=1e-3, atol=1e-3)
