"""The CTC loss and its gradient through the C ABI (``ms_ctc_loss_forward``, ``ms_ctc_loss_backward``, ``ms_ctc_status``) at every
kernel gate of csrc/ctc.hip, against the float64 reference, the three input families and the ONE derived bound of
tests/ctc_loss_cases.py (tests/test_ctc_loss_cpu.py proves those): the lane / wave edges of each states-per-lane form, the
register ring's residues, the alphabets around every normaliser path, both sides of the mailbox gate and of the gradient-row
gate, the refusals, the LDS-row kernels under MS_CTC_WAVE=0, phase 1 inside the pipeline kernel under MS_CTC_WIDE_PHASE1=0,
independence of everything a call must not read, non-finite input on every route, the reductions and two runs through the
``CTCLoss`` module.  nll, reduced and grad_logits lie between sentinel guards that must survive; grad_logits is prefilled with
the sentinel and must be fully written; the workspace behind its status region is prefilled with 0xFF bytes.  The kernels are
never compared with each other except where the issue is bit equality of two calls.

The three defects read from the code beforehand were all real.  On the parent commit, on the device,
``test_a_non_finite_normaliser_poisons_its_utterance_and_only_that`` failed on six of its ten routes and passes on all since the fix
that came with this file: [lds_row_V29], [lds_row_V100] and [lds_row_reached_by_S_max] (``ctc_alpha_kernel`` lost the NaN
normaliser in lse3 and returned +inf, which zero_infinity turns into 0; ``ctc_grad_kernel`` wrote finite rows),
[log_probs_V100] and [log_probs_V100_phase1_inside] (``ctc_normalise_wide_frame`` read a NaN among given log-probabilities as
"impossible": finite losses) and [log_probs_lds_row_V100] (one finite loss, two +inf).  The pipeline routes at V = 29 and
V = 100 with logits, [log_probs_V29] and the -inf tests passed before and after.  ``test_zz_report`` prints the largest
error / bound per family; on the device that was [loss, gradient] count 0.065 / 0.013, gauss 0.128 / 0.025, path 0.050 / 0.007
(the float32 restatement on the CPU: count 0.058, gauss 0.088, path 0.035 for the loss).
Needs a real MI355X: -m gpu."""
import numpy as np
import pytest
import torch

import ctc_loss_cases as C
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7.25e33
S32 = np.float32(SENTINEL)


def guarded(count):
    buf = torch.full((count + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + count]


def unguard(buf, what, written=True):
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == S32) and np.all(host[-GUARD:] == S32), (what, "guards")
    got = host[GUARD:-GUARD]
    if written:
        assert not np.any(got == S32), (what, "an output was not written")
    return got.copy()


def fresh_workspace(nbytes):
    ws = torch.full((max(int(nbytes), C.STATUS_BYTES),), 0xFF, dtype=torch.uint8, device="cuda")
    ws[:C.STATUS_BYTES] = 0
    return ws


def layout(targets, kind="concat", pad=0):
    """(flat int32 targets, offsets, lengths): ``concat`` in utterance order, ``reversed`` concatenated in reverse utterance
    order (offsets descending), ``padded`` [N, S] with ``pad`` behind every target."""
    lens = [len(t) for t in targets]
    if kind == "padded":
        S = max(1, max(lens))
        flat = [k for t in targets for k in list(t) + [pad] * (S - len(t))]
        offs = [n * S for n in range(len(targets))]
    else:
        order = range(len(targets)) if kind == "concat" else reversed(range(len(targets)))
        flat, offs = [], [0] * len(targets)
        for n in order:
            offs[n] = len(flat)
            flat += list(targets[n])
    return np.asarray(flat or [0], dtype=np.int32), np.asarray(offs, dtype=np.int32), np.asarray(lens, dtype=np.int32)


def call(lib, x, in_lens, targets, blank, S_max, flags=0, reduction=0, grad_nll=None, backward=True, kind="concat", pad=0, ws=None,
         short=0, refused=False, what=None):
    """One forward (and backward) call.  Returns dict(nll [N], reduced, grad [T, N, V] or None, ws_f, ws_b); a refused call
    must return non-zero and leave every output untouched."""
    T, N, V = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    flat, offs, lens = layout(targets, kind, pad)
    dev = [torch.from_numpy(a).cuda() for a in (np.asarray(in_lens, dtype=np.int32), flat, offs, lens)]
    il, tg, of, tl = dev
    nll_buf, nll = guarded(N)
    red_buf, red = guarded(1)
    stream = _lib.stream_ptr()
    ws_f = (ws or {}).get("ws_f")
    if ws_f is None:
        ws_f = fresh_workspace(lib.ms_ctc_loss_workspace_bytes(T, N, V, S_max))
    rc = lib.ms_ctc_loss_forward(_lib.ptr(xd), _lib.ptr(il), _lib.ptr(tg), _lib.ptr(of), _lib.ptr(tl), _lib.ptr(nll), _lib.ptr(red), T, N,
                                 V, S_max, blank, reduction, flags, _lib.ptr(ws_f), ws_f.numel() - short, stream)
    out = dict(ws_f=ws_f, ws_b=None, grad=None, rc_f=rc, rc_b=None)
    if refused:
        assert rc != C.MS_OK, (what, "forward accepted")
        assert np.all(nll_buf.cpu().numpy() == S32) and np.all(red_buf.cpu().numpy() == S32), (what, "a refused call wrote")
    else:
        _lib.check(rc, "ms_ctc_loss_forward")
        assert lib.ms_ctc_status(_lib.ptr(ws_f), stream) == C.MS_OK, (what, "forward status")
        out["nll"] = unguard(nll_buf, what)
        out["reduced"] = unguard(red_buf, what, written=reduction != 0)[0]
    if not backward:
        return out
    go = torch.from_numpy(np.ones(N, dtype=np.float32) if grad_nll is None else np.asarray(grad_nll, dtype=np.float32)).cuda()
    g_buf, g = guarded(T * N * V)
    ws_b = (ws or {}).get("ws_b")
    if ws_b is None:
        ws_b = fresh_workspace(lib.ms_ctc_loss_backward_workspace_bytes(T, N, V, S_max))
    rc = lib.ms_ctc_loss_backward(_lib.ptr(xd), _lib.ptr(il), _lib.ptr(tg), _lib.ptr(of), _lib.ptr(tl), _lib.ptr(go), _lib.ptr(g), T, N, V,
                                  S_max, blank, flags, _lib.ptr(ws_b), ws_b.numel() - short, stream)
    out["ws_b"], out["rc_b"] = ws_b, rc
    if refused:
        assert rc != C.MS_OK, (what, "backward accepted")
        assert np.all(g_buf.cpu().numpy() == S32), (what, "a refused call wrote")
        return out
    _lib.check(rc, "ms_ctc_loss_backward")
    assert lib.ms_ctc_status(_lib.ptr(ws_b), stream) == C.MS_OK, (what, "backward status")
    out["grad"] = unguard(g_buf, what).reshape(T, N, V)
    return out


def run_batch(lib, b, wave=True, **kw):
    flags = C.LOG_PROBS_IN if b.log_probs_in else 0
    fwd, bwd = b.routes(wave)
    outs = []
    for zi in (0, 1):
        what = (b.id, "zero_infinity", zi, fwd, bwd)
        o = call(lib, b.logits(), b.in_lens, b.targets, b.blank, b.S_max, flags | zi, what=what, **kw)
        C.check(b, o["nll"], o["grad"], bool(zi), fwd, bwd, what)
        outs.append(o)
    return outs


def same_bits(a, b, what):
    for k in ("nll", "grad"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k, "differs")


def ids(batches):
    return [b.id for b in batches]


ALL = list(C.toleranced_batches())
NO_WAVE = [b for b in ALL if b.gate in C.WITHOUT_WAVE]
WIDE = [b for b in C.alphabet_batches() if b.V > C.WIDE_V]


# ---- structure, time, alphabet and gate cases ------------------------------------------------------------------------------
@pytest.mark.parametrize("b", ALL, ids=ids(ALL))
def test_loss_and_gradient_against_the_reference(lib, b, monkeypatch):
    monkeypatch.delenv("MS_CTC_WAVE", raising=False)
    monkeypatch.delenv("MS_CTC_WIDE_PHASE1", raising=False)
    run_batch(lib, b)


@pytest.mark.parametrize("b", NO_WAVE, ids=ids(NO_WAVE))
def test_lds_row_kernels_against_the_same_reference(lib, b, monkeypatch):
    monkeypatch.setenv("MS_CTC_WAVE", "0")
    run_batch(lib, b, wave=False)


@pytest.mark.parametrize("b", WIDE, ids=ids(WIDE))
def test_phase_1_inside_the_pipeline_kernel_gives_the_bits_of_the_default(lib, b, monkeypatch):
    monkeypatch.delenv("MS_CTC_WAVE", raising=False)
    monkeypatch.delenv("MS_CTC_WIDE_PHASE1", raising=False)
    want = run_batch(lib, b)
    monkeypatch.setenv("MS_CTC_WIDE_PHASE1", "0")
    got = run_batch(lib, b)
    for w, g in zip(want, got):
        same_bits(w, g, b.id)


def test_refusals_write_nothing(lib):
    x = np.zeros((2, 1, 3), dtype=np.float32)
    ok = call(lib, x, [2], [[0]], 1, 3, what="accepted")
    assert np.isfinite(ok["nll"]).all()
    # the first target length each entry point refuses, and the last one it takes (2 frames: an impossible target)
    L = C.FIRST_REFUSED_FORWARD_L
    call(lib, x, [2], [[0, 2] * (L // 2) + [0]], 1, 2 * L + 1, backward=False, refused=True, what="forward, too long")
    o = call(lib, x, [2], [([0, 2] * L)[:L - 1]], 1, 2 * L - 1, backward=False, what="forward, longest")
    assert np.isposinf(o["nll"]).all()
    L = C.FIRST_REFUSED_BACKWARD_L
    xd = torch.from_numpy(x).cuda()
    flat, offs, lens = layout([([0, 2] * L)[:L]])
    dev = [torch.from_numpy(a).cuda() for a in (np.asarray([2], dtype=np.int32), flat, offs, lens, np.ones(1, dtype=np.float32))]
    for S_max, refused in ((2 * L + 1, True), (2 * L - 1, False)):
        dev[3][0] = (S_max - 1) // 2
        g_buf, g = guarded(x.size)
        ws = fresh_workspace(lib.ms_ctc_loss_backward_workspace_bytes(2, 1, 3, S_max))
        rc = lib.ms_ctc_loss_backward(_lib.ptr(xd), *[_lib.ptr(d) for d in dev], _lib.ptr(g), 2, 1, 3, S_max, 1, 1, _lib.ptr(ws),
                                      ws.numel(), _lib.stream_ptr())
        if refused:
            assert rc != C.MS_OK and np.all(g_buf.cpu().numpy() == S32)
        else:
            _lib.check(rc, "ms_ctc_loss_backward")
            assert lib.ms_ctc_status(_lib.ptr(ws), _lib.stream_ptr()) == C.MS_OK
            assert not unguard(g_buf, "backward, longest").any()         # impossible under zero_infinity: zeros
    # a zero_infinity field above 3, and a workspace one byte short
    call(lib, x, [2], [[0]], 1, 3, flags=4, refused=True, what="flags = 4")
    o = call(lib, x, [2], [[0]], 1, 3, short=1, refused=True, what="workspace one byte short")
    assert o["rc_f"] == C.MS_ERR_WORKSPACE and o["rc_b"] == C.MS_ERR_WORKSPACE


# ---- independence: bit equality of two calls -------------------------------------------------------------------------------
INDEPENDENT = [b for b in C.ring_batches() if b.family == "gauss"][:2] + [b for b in C.alphabet_batches()
                                                                          if b.family == "gauss" and (b.V, b.blank) in ((65, 0), (1025, 512))]


@pytest.mark.parametrize("wave", (True, False), ids=("default", "MS_CTC_WAVE=0"))
@pytest.mark.parametrize("b", INDEPENDENT, ids=ids(INDEPENDENT))
def test_nothing_outside_the_utterances_is_read(lib, b, wave, monkeypatch):
    if not wave:
        monkeypatch.setenv("MS_CTC_WAVE", "0")
    x = b.logits()
    args = (b.in_lens, b.targets, b.blank, b.S_max)
    base = call(lib, x, *args, flags=1, what=b.id)
    # frames at or past in_lens: NaN against zeros
    for fill in (np.nan, 0.0):
        y = x.copy()
        for n, Tn in enumerate(b.in_lens):
            y[Tn:, n, :] = fill
        same_bits(base, call(lib, y, *args, flags=1, what=(b.id, "padding frames", fill)), (b.id, "padding frames", fill))
    # target entries past tgt_lens: other in-range symbols, the blank among them
    for pad in (b.blank, 0, b.V - 1):
        same_bits(base, call(lib, x, *args, flags=1, kind="padded", pad=pad, what=(b.id, "target padding", pad)), (b.id, "padded", pad))
    # concatenated targets with offsets in reverse utterance order
    same_bits(base, call(lib, x, *args, flags=1, kind="reversed", what=(b.id, "reversed offsets")), (b.id, "reversed offsets"))
    # a second call on the workspaces the first one left
    same_bits(base, call(lib, x, *args, flags=1, ws=base, what=(b.id, "used workspace")), (b.id, "used workspace"))
    # an utterance alone against the same utterance first, in the middle and last in the batch (the same S_max argument)
    for n in sorted({0, b.N // 2, b.N - 1}):
        alone = call(lib, np.ascontiguousarray(x[:, n:n + 1]), [b.in_lens[n]], [b.targets[n]], b.blank, b.S_max, flags=1,
                     what=(b.id, "alone", n))
        assert np.array_equal(alone["nll"].view(np.uint32), base["nll"][n:n + 1].view(np.uint32)), (b.id, n)
        assert np.array_equal(alone["grad"][:, 0].view(np.uint32), base["grad"][:, n].view(np.uint32)), (b.id, n)


# ---- non-finite input ------------------------------------------------------------------------------------------------------
NONFINITE_ROUTES = [
    ("pipeline_V29", dict(V=29), {}),
    ("pipeline_V100", dict(V=100), {}),
    ("pipeline_V100_phase1_inside", dict(V=100), {"MS_CTC_WIDE_PHASE1": "0"}),
    ("lds_row_V29", dict(V=29), {"MS_CTC_WAVE": "0"}),
    ("lds_row_V100", dict(V=100), {"MS_CTC_WAVE": "0"}),
    ("lds_row_reached_by_S_max", dict(V=5, S_long=512), {}),
    ("log_probs_V29", dict(V=29, log_probs_in=True), {}),
    ("log_probs_V100", dict(V=100, log_probs_in=True), {}),
    ("log_probs_V100_phase1_inside", dict(V=100, log_probs_in=True), {"MS_CTC_WIDE_PHASE1": "0"}),
    ("log_probs_lds_row_V100", dict(V=100, log_probs_in=True), {"MS_CTC_WAVE": "0"}),
]


@pytest.mark.parametrize("name,kw,env", NONFINITE_ROUTES, ids=[r[0] for r in NONFINITE_ROUTES])
def test_a_non_finite_normaliser_poisons_its_utterance_and_only_that(lib, name, kw, env, monkeypatch):
    """nll NaN for utterances 1 to 3 under either zero_infinity setting, NaN on EVERY existing frame of their gradients, exact
    zeros behind; utterances 0 and 4 (a NaN only in a padding frame) inside the bound; the sum NaN; the status MS_OK."""
    for k in ("MS_CTC_WAVE", "MS_CTC_WIDE_PHASE1"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    b = C.nonfinite_batch(**kw)
    wave = env.get("MS_CTC_WAVE") != "0"
    assert b.routes(wave)[0] == ("lds_row" if "lds_row" in name else "pipeline")
    for o in run_batch(lib, b, wave=wave):                       # C.check: the NaN pattern of the reference, loss and gradient
        assert np.isnan(o["nll"][[1, 2, 3]]).all() and np.isfinite(o["nll"][[0, 4]]).all()
        for n in (1, 2, 3):
            assert np.isnan(o["grad"][:b.in_lens[n], n]).all() and not o["grad"][b.in_lens[n]:, n].any()
    for zi in (0, 1):
        o = call(lib, b.logits(), b.in_lens, b.targets, b.blank, b.S_max, flags=(C.LOG_PROBS_IN if b.log_probs_in else 0) | zi,
                 reduction=2, backward=False, what=(name, "sum"))
        assert np.isnan(o["reduced"])


@pytest.mark.parametrize("wave", (True, False), ids=("default", "MS_CTC_WAVE=0"))
def test_a_single_minus_infinity_is_an_impossible_symbol_not_poison(lib, wave, monkeypatch):
    if not wave:
        monkeypatch.setenv("MS_CTC_WAVE", "0")
    for V in (5, 100):
        blank = V // 2
        sym = [k for k in range(V) if k != blank]
        tg = [[sym[0], sym[1], sym[2]], [sym[1], sym[1]], [sym[2]], []]
        base = C.Batch(f"minus_inf_V{V}", 12, V, blank, [12, 10, 7, 5], tg, "gauss", gate="ring", seed=3)
        x = base.logits().copy()
        x[5, 0, sym[3]] = -np.inf                     # avoidable: a symbol the target does not use
        x[4, 1, blank] = -np.inf                      # avoidable: the blank at one frame
        x[0, 2, [blank, sym[2]]] = -np.inf            # unavoidable: neither start is possible
        x[3, 3, blank] = -np.inf                      # unavoidable: an empty target needs the blank at every frame
        with np.errstate(divide="ignore"):             # the same values as log-probabilities: normalised in float64
            x64 = x.astype(np.float64)
            xlp = (x64 - np.log(np.exp(x64 - x64.max(axis=2, keepdims=True)).sum(axis=2, keepdims=True))
                   - x64.max(axis=2, keepdims=True)).astype(np.float32)
        for lpi in (False, True):
            b = base.replaced(xlp if lpi else x, f"minus_inf_V{V}_lp{int(lpi)}")
            b.log_probs_in = lpi
            assert b.reference(False)["infeasible"].tolist() == [False, False, True, True]
            for o in run_batch(lib, b, wave=wave):
                hit = np.isneginf(x) & (np.arange(12)[:, None, None] < np.asarray(b.in_lens)[None, :, None])
                assert np.all(o["grad"][hit][np.isfinite(o["grad"][hit])] == 0.0)
                assert np.all(o["grad"][:, :2][hit[:, :2]] == 0.0), "the gradient at a -inf symbol is exactly 0"


# ---- reductions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wave", (True, False), ids=("default", "MS_CTC_WAVE=0"))
def test_reductions_and_upstream_gradients(lib, wave, monkeypatch):
    """N = 257 (the reduce kernel's strided loop), T = 2, V = 3: sum and mean against the float64 sum of the kernel's own nll
    within N 2^-24 sum |v|; an empty target and an impossible one; grad_nll of 0, a negative value and 1e3 scale the gradient
    by exactly one multiplication."""
    if not wave:
        monkeypatch.setenv("MS_CTC_WAVE", "0")
    N = 257
    tg = [[0] if n % 3 else [2] for n in range(N)]
    tg[5], tg[256], tg[100] = [], [], [0, 0]          # utterance 100: a, a needs 3 frames
    b = C.Batch("reduce", 2, 3, 1, [2 - (n % 7 == 0) for n in range(N)], tg, "gauss", gate="ring", seed=9)
    lens = np.maximum(np.asarray([len(t) for t in tg], dtype=np.float64), 1.0)
    for zi in (0, 1):
        fwd, bwd = b.routes(wave)
        none = call(lib, b.logits(), b.in_lens, b.targets, b.blank, b.S_max, flags=zi, what=("reduce", zi))
        C.check(b, none["nll"], none["grad"], bool(zi), fwd, bwd, ("reduce", zi))
        assert (none["nll"][100] == 0.0) if zi else np.isposinf(none["nll"][100])
        v = none["nll"].astype(np.float64)
        for red, want, scale in ((2, v.sum(), np.abs(v)), (1, (v / lens).sum() / N, np.abs(v / lens) / N)):
            o = call(lib, b.logits(), b.in_lens, b.targets, b.blank, b.S_max, flags=zi, reduction=red, backward=False, what=("reduce", red))
            assert np.array_equal(o["nll"].view(np.uint32), none["nll"].view(np.uint32))
            if zi:
                # (the kernel adds one or two values per thread and then a tree of eight levels: far inside N roundings)
                assert abs(float(o["reduced"]) - want) <= N * C.U * scale.sum(), (red, float(o["reduced"]), want)
            else:
                assert np.isposinf(o["reduced"])
        if zi:
            for go in (0.0, -0.75, 1e3):
                gn = np.full(N, go, dtype=np.float32)
                gn[1::2] *= np.float32(0.5)
                o = call(lib, b.logits(), b.in_lens, b.targets, b.blank, b.S_max, flags=zi, grad_nll=gn, what=("reduce", "go", go))
                assert np.array_equal(o["grad"], none["grad"] * gn[None, :, None]), go


# ---- through the module -----------------------------------------------------------------------------------------------------
def test_module_mean_with_concatenated_targets_under_autograd():
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    b = [r for r in C.ring_batches() if r.family == "gauss"][1]
    keep = [n for n in range(b.N) if n != 3]                          # (without the impossible utterance: a finite mean)
    x = np.ascontiguousarray(b.logits()[:, keep])
    in_lens, tg = [b.in_lens[n] for n in keep], [b.targets[n] for n in keep]
    N = len(keep)
    lens = np.maximum(np.asarray([len(t) for t in tg], dtype=np.float64), 1.0)
    go = 1.0 / (N * lens)
    ref = C.reference(x, in_lens, tg, b.blank, grad_nll=go)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    flat = torch.tensor([k for t in tg for k in t], dtype=torch.int32)
    loss = CTCLoss(blank=b.blank, reduction="mean")((xt, torch.tensor(in_lens)), (flat, torch.tensor([len(t) for t in tg])))
    loss.backward()
    bn = C.bound_nll(ref, "z_serial")
    assert bn.max() <= C.BOUND_CAP
    want = float((ref["nll"] * go).sum())
    assert abs(float(loss) - want) <= float((bn * go).sum()) + (N + 2) * C.U * float((ref["nll"] * go).sum())
    g = xt.grad.cpu().numpy().astype(np.float64)
    bg = C.bound_grad(ref, "z_serial", go)
    assert np.all(np.abs(g - ref["grad"]) <= bg[None, :, None])


def test_module_with_the_blank_in_the_middle_of_a_wide_alphabet():
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    V, blank = 100, 50
    tg = [C.labels(L, V, blank, seed=L) for L in (9, 4, 0, 6)]
    b = C.Batch("module_V100", 24, V, blank, [24, 20, 9, 13], tg, "gauss", gate="alphabet", seed=4)
    xt = torch.from_numpy(b.logits().copy()).cuda().requires_grad_(True)
    S = max(len(t) for t in tg)
    y = torch.tensor([t + [blank] * (S - len(t)) for t in tg], dtype=torch.int32)
    nll = CTCLoss(blank=blank, reduction="none")((xt, torch.tensor(b.in_lens)), (y, torch.tensor([len(t) for t in tg])))
    nll.sum().backward()
    C.check(b, nll.detach().cpu().numpy(), xt.grad.cpu().numpy(), False, *b.routes(), "module, V = 100")


def test_zz_report():
    print("largest error / bound on the device, per family [loss, gradient]:",
          {k: [round(v, 4) for v in r] for k, r in sorted(C.RATIOS.items())})
    over = {k: r for k, r in C.RATIOS.items() if max(r) > 0.5}
    if over:
        print("FINDING: a ratio above 0.5:", over)
