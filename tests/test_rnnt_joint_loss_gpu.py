"""The fused transducer loss with gradient on the device (``ms_rnnt_joint_loss_forward`` / ``_backward``, ``rnnt_joint_loss``,
``RNNTJointLoss``) against the float64 numpy yardstick tests/rnnt_joint_loss_ref.py, whose docstring derives the gradients'
bounds (stated for |w_out| within [2^-10, 2^10] and |grad_nll| within [2^-10, 8]) -- the full ones against the float64
yardstick, and the backward's own share against the float64 gradients that follow from the device's own lattice
(``gradients_given_lattice``: the share a one-plane product misses, tests/test_rnnt_joint_loss_cpu.py).  The forward is held
to the scorer's bounds (tests/test_rnnt_score_gpu.py); Z to max_v eps_v + 16 * 2^-24 max(1, |Z|), its share of the scorer's delta.

The float32 emulation of the device's arithmetic sits at 0.0005 of the gradients' full bounds and 0.16 of the own share at
worst (tests/test_rnnt_joint_loss_cpu.py).  The device's worst ratios are printed by every test here and recorded by
tools/rnnt_joint_loss_time.py in profiles/rnnt_joint_loss_time.json; measured on one MI355X over every test of this file:
nll 0.0049, alpha 0.0022, beta 0.0049, Z 0.049; full bounds d_enc_p 0.00072, d_pred_p 0.0011, d_w_out 0.00092, d_b_out
0.00041; own share d_enc_p 0.11, d_pred_p 0.14, d_w_out 0.075, d_b_out 0.067.
"""
import numpy as np
import pytest
import torch

import rnnt_joint_loss_ref as G
import rnnt_loss_ref as R
import rnnt_score_ref as S
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
CASES = S.cases()
worst = {k: 0.0 for k in ("nll", "alpha", "beta", "Z") + G.TENSORS + tuple(k + " (own share)" for k in G.TENSORS)}


def f32(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda().contiguous()


def i32(a):
    return torch.as_tensor(np.ascontiguousarray(a).reshape(-1), dtype=torch.int32).cuda()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Device:
    """A case's tensors on the device and the two C-ABI calls on them."""

    def __init__(self, c):
        self.c = c
        self.T, self.N, self.J = c["enc_p"].shape
        self.U1, self.V1 = c["pred_p"].shape[0], c["w_out"].shape[0]
        self.e, self.p, self.w = f32(c["enc_p"]), f32(c["pred_p"]), f32(c["w_out"])
        self.b = None if c["b_out"] is None else f32(c["b_out"])
        self.xl, self.yl = i32(c["in_lens"]), i32(c["tgt_lens"])
        self.y = i32(c["targets"]) if self.U1 > 1 else None
        self.dims = (self.N, self.T, self.U1, self.J, self.V1)

    def forward(self, entry="ms_rnnt_joint_loss_forward"):
        lib = _lib.load()
        N, T, U1, J, V1 = self.dims
        planes = 3 if entry == "ms_rnnt_joint_loss_forward" else 2
        assert lib.ms_rnnt_joint_loss_lattice_bytes(N, T, U1) == 12 * N * T * U1
        self.nll = torch.full((N,), SENTINEL, dtype=torch.float32, device="cuda")
        self.lattice = torch.full((planes, N, T, U1), SENTINEL, dtype=torch.float32, device="cuda")
        nbytes = lib.ms_rnnt_score_workspace_bytes(N, T, U1, J, V1)
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
        _lib.check(getattr(lib, entry)(_lib.ptr(self.e), _lib.ptr(self.p), _lib.ptr(self.w), _lib.ptr(self.b), _lib.ptr(self.xl),
                                       _lib.ptr(self.y), _lib.ptr(self.yl), _lib.ptr(self.nll), _lib.ptr(self.lattice), N, T, U1,
                                       J, V1, self.c["blank"], _lib.ptr(ws), nbytes, _lib.stream_ptr()), entry)
        torch.cuda.synchronize()
        return self.nll.cpu().numpy(), self.lattice.cpu().numpy()

    def backward(self, grad_nll, workspace="preferred", want_db=True, expect=None):
        """After ``forward()``.  The gradients pre-filled with a sentinel, the workspace with NaN bytes."""
        lib = _lib.load()
        N, T, U1, J, V1 = self.dims
        lo, hi = (lib.ms_rnnt_joint_loss_backward_workspace_min_bytes(*self.dims),
                  lib.ms_rnnt_joint_loss_backward_workspace_bytes(*self.dims))
        assert 0 < lo <= hi
        nbytes = {"min": lo, "preferred": hi}.get(workspace, workspace)
        ws = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device="cuda")
        gn = f32(grad_nll)
        d = [torch.full_like(x, SENTINEL) for x in (self.e, self.p, self.w)]
        d.append(torch.full((V1,), SENTINEL, dtype=torch.float32, device="cuda") if want_db else None)
        rc = lib.ms_rnnt_joint_loss_backward(
            _lib.ptr(self.e), _lib.ptr(self.p), _lib.ptr(self.w), _lib.ptr(self.b), _lib.ptr(self.xl), _lib.ptr(self.y),
            _lib.ptr(self.yl), _lib.ptr(self.nll), _lib.ptr(self.lattice), _lib.ptr(gn), _lib.ptr(d[0]), _lib.ptr(d[1]),
            _lib.ptr(d[2]), _lib.ptr(d[3]), N, T, U1, J, V1, self.c["blank"], _lib.ptr(ws), nbytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        out = G.Grads(*[None if x is None else x.cpu().numpy() for x in d])
        if expect is not None:
            assert _lib.ERR_NAMES[rc] == expect
            return out
        _lib.check(rc, "ms_rnnt_joint_loss_backward")
        return out


def run(c, grad_nll, workspace="preferred", **change):
    dev = Device(dict(c, **change))
    nll, lattice = dev.forward()
    return nll, lattice, dev.backward(grad_nll, workspace)


def grads_bits(g):
    return b"".join(getattr(g, k).tobytes() for k in G.TENSORS if getattr(g, k) is not None)


def note(w, name):
    for k, v in w.items():
        worst[k] = max(worst[k], v)
    print(f"{name}: ratios to the bounds {({k: round(float(v), 5) for k, v in w.items()})}")
    print("worst ratios so far", {k: round(float(v), 5) for k, v in worst.items()})


def check_forward(name, ref, nll, lattice):
    w = S.worst_ratios(nll, lattice[1], lattice[2], ref.loss, ref.score_bounds)
    ex = ref.exists
    zb = float(np.max(ref.eps)) + 16 * S.U24 * np.maximum(1.0, np.abs(ref.loss.Z[ex]))
    w["Z"] = float(np.max(np.abs(lattice[0][ex].astype(np.float64) - ref.loss.Z[ex]) / zb))
    note(w, name + " forward")
    assert max(w.values()) <= 1.0, (name, w)


def check_grads(name, got, ref, bnd):
    w = G.worst_ratios(got, ref, bnd)
    note(w, name)
    assert max(w.values()) <= 1.0, (name, w)
    return w


RUNS = [(n, "preferred") for n in G.CASE_NAMES] + [("b_tiles", "min"), ("e_vocabulary", "min")]


@pytest.mark.parametrize("name,workspace", RUNS)
def test_case_within_the_bounds(name, workspace):
    """The scorer's cases (a) ragged tiles, U_n = 0, T_n = 1; (b) several cell tiles and units; (c) three column tiles, the
    last ragged; (d) a model that knows the transcript; (e) 4096 symbols.  With the minimum workspace a band is one unit
    (b: 3 + 3 bands, e: 5 + 5), so the sums across bands are exercised; the forward is ms_rnnt_score's bit for bit."""
    c = CASES[name]
    gn, ref, bnd = G.reference(name)
    assert GN_OK(gn)
    dev = Device(c)
    nll, lattice = dev.forward()
    check_forward(name, ref, nll, lattice)
    s_nll, s_lattice = Device(c).forward("ms_rnnt_score")
    ex = ref.exists
    assert same_bits(nll, s_nll)
    assert same_bits(lattice[1][ex], s_lattice[0][ex]) and same_bits(lattice[2][ex], s_lattice[1][ex])
    got = dev.backward(gn, workspace)
    for k in G.TENSORS:
        assert not (getattr(got, k) == SENTINEL).any(), k        # fully written
    check_grads(f"{name} ({workspace} workspace)", got, ref, bnd)
    # ... and to the backward's own share of them, against what follows from the device's own lattice
    given = R.Result(nll, None, np.where(ex, lattice[0], 0), np.where(ex, lattice[1], 0), np.where(ex, lattice[2], 0), ex)
    own, x = G.gradients_given_lattice(c, gn, given)
    w = G.worst_ratios(got, own, G.bounds(own, x, lattice_share=False))
    note({k + " (own share)": v for k, v in w.items()}, name)
    assert max(w.values()) <= 1.0, (name, w)
    for n in range(dev.N):                                       # rows past the lengths: written as 0
        assert not got.d_enc_p[c["in_lens"][n]:, n].any() and not got.d_pred_p[c["tgt_lens"][n] + 1:, n].any()


def GN_OK(gn):
    return bool((np.abs(gn) >= G.GN_MIN).all() and (np.abs(gn) <= G.GN_MAX).all())


@pytest.mark.parametrize("name", ["a_ragged", "b_tiles"])
def test_runs_repeat_and_padding_changes_no_bit(name):
    c = CASES[name]
    gn, ref, _ = G.reference(name)
    ex = ref.exists
    workspace = "min" if name == "b_tiles" else "preferred"
    nll, lattice, clean = run(c, gn, workspace)
    nll2, lattice2, again = run(c, gn, workspace)
    assert same_bits(nll, nll2) and same_bits(lattice[:, ex], lattice2[:, ex]) and grads_bits(clean) == grads_bits(again)
    enc, pred, y = c["enc_p"].copy(), c["pred_p"].copy(), c["targets"].copy()
    junk = np.array([np.nan, np.inf, 3e38, -np.inf, -3e38], dtype=np.float32)
    for n, (Tn, Un) in enumerate(zip(c["in_lens"], c["tgt_lens"])):
        enc[Tn:, n] = np.resize(junk, enc[Tn:, n].shape)
        pred[Un + 1:, n] = np.resize(junk[::-1], pred[Un + 1:, n].shape)
        y[n, Un:] = [(-7, 1 << 30, c["blank"], 10 ** 6)[(n + k) % 4] for k in range(y.shape[1] - Un)]
    assert np.isnan(enc).any() and np.isnan(pred).any()
    nll3, lattice3, dirty = run(c, gn, workspace, enc_p=enc, pred_p=pred, targets=y)
    assert same_bits(nll, nll3) and same_bits(lattice[:, ex], lattice3[:, ex]) and grads_bits(clean) == grads_bits(dirty)


def _subcase(c, keep):
    return dict(c, enc_p=c["enc_p"][:, keep], pred_p=c["pred_p"][:, keep], in_lens=c["in_lens"][keep],
                targets=c["targets"][keep], tgt_lens=c["tgt_lens"][keep])


def test_impossible_transcript_contributes_nothing():
    c = CASES["a_ragged"]
    gn = G.draw_grad_nll("a_ragged", 3)
    # -inf on a label utterance 0 needs and the others do not
    needed = next(int(v) for v in c["targets"][0, :c["tgt_lens"][0]]
                  if not any((c["targets"][n, :c["tgt_lens"][n]] == v).any() for n in (1, 2)))
    b = c["b_out"].copy()
    b[needed] = -np.inf
    nll, _, got = run(c, gn, b_out=b)
    assert nll[0] == np.inf and np.isfinite(nll[1:]).all()
    assert not got.d_enc_p[:, 0].any() and not got.d_pred_p[:, 0].any()
    others = _subcase(dict(c, b_out=b), [1, 2])
    ref, x = G.gradients(others, gn[1:])
    bnd = G.bounds(ref, x)
    _, _, alone = run(others, gn[1:])
    check_grads("the other utterances alone", alone, ref, bnd)
    full = G.Grads(got.d_enc_p[:, 1:], got.d_pred_p[:, 1:], got.d_w_out, got.d_b_out)
    check_grads("the other utterances beside an impossible one", full, ref, bnd)
    assert got.d_b_out[needed] == 0 and not got.d_w_out[needed].any()


def test_nan_poisons_what_the_contract_says_and_nothing_else():
    name = "b_tiles"
    c = CASES[name]
    gn, _, _ = G.reference(name)
    _, _, clean = run(c, gn, "min")
    enc = c["enc_p"].copy()
    enc[11, 0, 40] = np.nan                                       # an existing frame of utterance 0
    nll, _, got = run(c, gn, "min", enc_p=enc)
    T0, U0 = int(c["in_lens"][0]), int(c["tgt_lens"][0])
    assert np.isnan(nll[0]) and np.isfinite(nll[1])
    assert np.isnan(got.d_enc_p[:T0, 0]).all() and np.isnan(got.d_pred_p[:U0 + 1, 0]).all()
    assert not got.d_enc_p[T0:, 0].any() and not got.d_pred_p[U0 + 1:, 0].any()
    assert np.isnan(got.d_w_out).all() and np.isnan(got.d_b_out).all()
    assert same_bits(got.d_enc_p[:, 1], clean.d_enc_p[:, 1]) and same_bits(got.d_pred_p[:, 1], clean.d_pred_p[:, 1])


def test_without_bias_and_without_its_gradient():
    c = dict(CASES["a_ragged"], b_out=None)
    gn = G.draw_grad_nll("a_ragged", 3)
    ref, x = G.gradients(c, gn)
    dev = Device(c)
    dev.forward()
    got = dev.backward(gn)
    check_grads("no bias", got, ref, G.bounds(ref, x))
    without = dev.backward(gn, want_db=False)
    assert without.d_b_out is None and grads_bits(without) == grads_bits(got._replace(d_b_out=None))


def _materialised(c, gn):
    """torch float32 joint, ``RNNTLoss``, autograd."""
    from myrtlespeech_amd.loss.rnnt_loss import RNNTLoss
    leaves = [f32(c[k]).requires_grad_() for k in ("enc_p", "pred_p", "w_out", "b_out")]
    e, p, w, b = leaves
    logits = torch.tanh(e.transpose(0, 1)[:, :, None, :] + p.transpose(0, 1)[:, None, :, :]) @ w.t() + b
    nll = RNNTLoss(c["blank"], "none")((logits, torch.as_tensor(c["in_lens"])),
                                       (torch.as_tensor(c["targets"]), torch.as_tensor(c["tgt_lens"])))
    (nll * f32(gn)).sum().backward()
    return G.Grads(*[x.grad.cpu().numpy() for x in leaves])


def _fused_autograd(c, gn, reduction="none", requires=(True, True, True, True), module=False):
    from myrtlespeech_amd.loss import RNNTJointLoss, rnnt_joint_loss
    leaves = [f32(c[k]).requires_grad_(r) for k, r in zip(("enc_p", "pred_p", "w_out", "b_out"), requires)]
    e, p, w, b = leaves
    xl, y, yl = torch.as_tensor(c["in_lens"]), torch.as_tensor(c["targets"]), torch.as_tensor(c["tgt_lens"])
    if module:
        out = RNNTJointLoss(c["blank"], reduction)((e, xl), p, w, b, (y, yl))
    else:
        out = rnnt_joint_loss(e, p, w, b, xl, y, yl, c["blank"], reduction)
    if reduction == "none":
        (out * f32(gn)).sum().backward()
    else:
        out.backward()
    return out.detach().cpu().numpy(), G.Grads(*[None if x.grad is None else x.grad.cpu().numpy() for x in leaves])


@pytest.mark.parametrize("name", ["a_ragged", "b_tiles", "c_columns_blank150"])
def test_agrees_with_the_materialised_route(name):
    """The materialised route's logits are inside the same eps_v and its float32 products inside the same K-extent terms:
    it is held to the same bounds, the two routes to their sum."""
    c = CASES[name]
    gn, ref, bnd = G.reference(name)
    dense = _materialised(c, gn)
    _, fused = _fused_autograd(c, gn)
    w = {}
    for k in G.TENSORS:
        d = np.abs(getattr(fused, k).astype(np.float64) - getattr(dense, k))
        with np.errstate(all="ignore"):
            w[k] = float(np.max(np.where(d == 0, 0.0, d / (2 * getattr(bnd, k)))))
    print(f"{name}: |fused - materialised| / (sum of the two bounds) {w}")
    assert max(w.values()) <= 1.0
    check_grads(name + " through autograd", fused, ref, bnd)


def test_autograd_node():
    from myrtlespeech_amd.loss.rnnt_loss import rnnt_score
    name = "a_ragged"
    c = CASES[name]
    gn, ref, bnd = G.reference(name)
    nll, everything = _fused_autograd(c, gn)
    # a subset of the inputs: None for the others, the same bits for the rest
    _, some = _fused_autograd(c, gn, requires=(False, True, False, True))
    assert some.d_enc_p is None and some.d_w_out is None
    assert same_bits(some.d_pred_p, everything.d_pred_p) and same_bits(some.d_b_out, everything.d_b_out)
    _, only_w = _fused_autograd(c, gn, requires=(False, False, True, False), module=True)
    assert only_w.d_b_out is None and only_w.d_enc_p is None and same_bits(only_w.d_w_out, everything.d_w_out)
    # the reductions: sum is grad_nll = 1, mean 1 / N
    for reduction, scale in (("sum", 1.0), ("mean", 1.0 / 3)):
        r_ref, r_x = G.gradients(c, np.full(3, scale))
        out, got = _fused_autograd(c, None, reduction, module=True)
        np.testing.assert_allclose(out, nll.astype(np.float64).sum() * scale, rtol=1e-6)
        check_grads(reduction, got, r_ref, G.bounds(r_ref, r_x))
    # grad disabled, or nothing requires grad: the scorer's bits
    args = [f32(c[k]) for k in ("enc_p", "pred_p", "w_out", "b_out")] + [torch.as_tensor(c[k]) for k in
                                                                         ("in_lens", "targets", "tgt_lens")]
    from myrtlespeech_amd.loss import rnnt_joint_loss
    score = rnnt_score(*args, c["blank"]).cpu().numpy()
    plain = rnnt_joint_loss(*args, c["blank"], "none")
    assert not plain.requires_grad and same_bits(plain.cpu().numpy(), score) and same_bits(nll, score)
    with torch.no_grad():
        args[0].requires_grad_()
        off = rnnt_joint_loss(*args, c["blank"], "none")
    assert not off.requires_grad and same_bits(off.cpu().numpy(), score)


def test_the_callers_errors_and_the_limits():
    c = CASES["a_ragged"]
    gn = G.draw_grad_nll("a_ragged", 3)
    nll, _, clean = run(c, gn)
    # the caller's errors: nll = +inf, nothing from that utterance, the others' rows keep their bits
    y = c["targets"].copy()
    y[0, 1] = 10 ** 6                                             # a label past V1
    nll2, _, got = run(c, gn, targets=y, tgt_lens=np.array([3, -1, 0], dtype=np.int32))
    assert nll2[0] == np.inf and nll2[1] == np.inf and nll2[2] == nll[2]
    assert not got.d_enc_p[:, :2].any() and not got.d_pred_p[:, :2].any()
    assert same_bits(got.d_enc_p[:, 2], clean.d_enc_p[:, 2]) and same_bits(got.d_pred_p[:, 2], clean.d_pred_p[:, 2])
    nll3, _, got = run(c, gn, in_lens=np.array([0, 6, 3], dtype=np.int32))
    assert (nll3[:2] == np.inf).all() and not got.d_enc_p[:, :2].any()
    # return codes, with nothing launched
    dev = Device(c)
    dev.forward()
    lo = _lib.load().ms_rnnt_joint_loss_backward_workspace_min_bytes(*dev.dims)
    got = dev.backward(gn, workspace=lo - 16, expect="MS_ERR_WORKSPACE")
    assert all((getattr(got, k) == SENTINEL).all() for k in G.TENSORS)
    lib = _lib.load()
    z = torch.zeros((1025, 2), device="cuda")
    out = torch.full((2 * 1025,), SENTINEL, device="cuda")
    lat = torch.full((3 * 1025,), SENTINEL, device="cuda")
    one, yy = i32([1]), i32(np.zeros(1024))
    nbytes = lib.ms_rnnt_joint_loss_backward_workspace_bytes(1, 1, 1025, 2, 2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.ms_rnnt_joint_loss_forward(_lib.ptr(z), _lib.ptr(z), _lib.ptr(z), None, _lib.ptr(one), _lib.ptr(yy), _lib.ptr(one),
                                        _lib.ptr(out), _lib.ptr(lat), 1, 1, 1025, 2, 2, 1, _lib.ptr(ws), nbytes, _lib.stream_ptr())
    assert _lib.ERR_NAMES[rc] == "MS_ERR_UNSUPPORTED"
    rc = lib.ms_rnnt_joint_loss_backward(_lib.ptr(z), _lib.ptr(z), _lib.ptr(z), None, _lib.ptr(one), _lib.ptr(yy), _lib.ptr(one),
                                         _lib.ptr(z), _lib.ptr(lat), _lib.ptr(z), _lib.ptr(out), _lib.ptr(out), _lib.ptr(out), None,
                                         1, 1, 1025, 2, 2, 1, _lib.ptr(ws), nbytes, _lib.stream_ptr())
    assert _lib.ERR_NAMES[rc] == "MS_ERR_UNSUPPORTED"
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((lat == SENTINEL).all())
