"""The training step on the device: csrc/optim.hip through ``myrtlespeech_amd.optim`` against the numpy restatement of
tests/optim_ref.py, bit for bit, on a tensor list built to sit on every edge of the kernels (``optim_ref.case_numels``): empty
tensors, tensors below / at / above one quad, exactly a chunk, a chunk + 1, two chunks - 1, a parameter that starts one element
past a 16-byte boundary, 300 one-element tensors (seven argument pages) and a parameter without a gradient.  Every parameter,
gradient and state tensor is a view into a larger buffer filled with a sentinel, the roles of one tensor are aligned
differently from each other (``optim_ref.layout``), and after every run each buffer's sentinels are checked.

Then the version protocol (a forward after ``step()`` runs on the new weights) and ``fit`` on the two tiny DeepSpeech2 models
of tests/ds2_train_ref.py."""
import numpy as np
import pytest
import torch

import ds2_train_ref as M
import optim_ref as R

pytestmark = pytest.mark.gpu


class Lists:
    """``nroles`` flat sentinel buffers and the views of ``optim_ref.layout`` into them; ``params`` are Parameters over role 0
    whose ``.grad`` are the views of role 1 (none for ``NO_GRAD``)."""

    def __init__(self, nroles):
        self.numels = R.case_numels()
        self.bufs, self.views, self.masks = [], [], []
        for role in range(nroles):
            starts, total = R.layout(self.numels, role)
            buf = torch.full((total,), R.SENTINEL, device="cuda")
            assert buf.data_ptr() % 16 == 0
            mask = np.ones(total, dtype=bool)
            for s, n in zip(starts, self.numels):
                mask[s:s + n] = False
            self.bufs.append(buf)
            self.masks.append(mask)
            self.views.append([buf[s:s + n] for s, n in zip(starts, self.numels)])
        assert self.views[0][R.ODD_VIEW].data_ptr() % 16 == 4 and self.views[1][R.ODD_VIEW].data_ptr() % 16 == 0
        self.params = [torch.nn.Parameter(v) for v in self.views[0]]
        assert all(p.data_ptr() == v.data_ptr() for p, v in zip(self.params, self.views[0]))
        for i, p in enumerate(self.params):
            p.grad = None if i == R.NO_GRAD else self.views[1][i]

    def fill(self, role, arrays):
        for v, a in zip(self.views[role], arrays):
            v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))

    def read(self, role):
        return [v.detach().cpu().numpy().copy() for v in self.views[role]]

    def check_sentinels(self):
        for role, (buf, mask) in enumerate(zip(self.bufs, self.masks)):
            got = buf.cpu().numpy()
            assert (got[mask] == np.float32(R.SENTINEL)).all(), f"role {role}: a sentinel was overwritten"


def gaussians(numels, seed, scale=0.5):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * scale).astype(np.float32) for n in numels]


def with_grad(arrays):
    return [a for i, a in enumerate(arrays) if i != R.NO_GRAD]


# ---- 1, 2: the norm ------------------------------------------------------------------------------------------------------------
def test_norm_of_small_integers_is_exact():
    """Squares of integers in [-2, 2] over fewer than 2^15 elements: every partial sum is an integer below 2^24, so whatever the
    order of the additions the device's S is exact and a dropped or doubled element at any head, tail or chunk edge changes it."""
    from myrtlespeech_amd import optim
    li = Lists(2)
    rng = np.random.default_rng(5)
    g = [rng.integers(-2, 3, n).astype(np.float32) for n in li.numels]
    for a in g:
        if a.size:
            a[0], a[-1] = 2.0, 1.0 if a.size > 1 else 2.0      # the edges carry weight
    li.fill(1, g)
    s = sum(int((a.astype(np.int64) ** 2).sum()) for a in with_grad(g))
    assert 0 < s < 2 ** 24
    got = optim.grad_norm(li.params).cpu().numpy()
    assert got.dtype == np.float32 and got[0] == np.sqrt(np.float32(s)) and got[1] == 0.0
    li.check_sentinels()
    assert all(np.array_equal(a, b) for a, b in zip(li.read(1), g))
    # no tensors at all, and only empty ones
    assert optim.grad_norm([]).cpu().tolist() == [0.0, 0.0]
    assert optim.grad_norm([li.params[0]]).cpu().tolist() == [0.0, 0.0]


def test_norm_of_gaussians_is_within_its_chain_bound_and_repeats():
    """``optim_ref.norm_rel_bound`` derives the bound from the longest chain of float32 additions an element passes through
    (3 in its quad, 4 on its thread, 1 for the rest, 6 + 3 in the workgroup, then ceil(P / 256) + 6 + 3 among the P partials)."""
    from myrtlespeech_amd import optim
    li = Lists(2)
    g = gaussians(li.numels, 6)
    li.fill(1, g)
    want, flag = R.grad_norm64(with_grad(g))
    a = optim.grad_norm(li.params).cpu().numpy()
    b = optim.grad_norm(li.params).cpu().numpy()
    bound = R.norm_rel_bound(li.numels)
    print("norm", a[0], "float64", want, "relative error", abs(a[0] - want) / want, "bound", bound)
    assert abs(float(a[0]) - want) <= bound * want and a[1] == flag == 0.0
    assert a.tobytes() == b.tobytes()


# ---- 3: the steps -----------------------------------------------------------------------------------------------------------------
SGD_CASES = {"plain": dict(), "momentum": dict(momentum=0.9), "nesterov+decay": dict(momentum=0.9, nesterov=True, weight_decay=0.01)}
ADAM_CASES = {"plain": dict(), "decay": dict(weight_decay=0.01), "amsgrad": dict(amsgrad=True)}
CLIPS = {"noclip": None, "below": 1.0, "above": 1e4}      # the gaussians' norm is about 74


def _run_steps(kind, kw, max_norm, steps=3):
    from myrtlespeech_amd import optim
    amsgrad = bool(kw.get("amsgrad"))
    nstate = {"sgd": 1 if kw.get("momentum") else 0, "adam": 3 if amsgrad else 2}[kind]
    li = Lists(2 + nstate)
    p = gaussians(li.numels, 1, 1.0)
    li.fill(0, p)
    state = [[np.zeros(n, np.float32) for n in li.numels] for _ in range(nstate)]
    for k in range(nstate):
        li.fill(2 + k, state[k])
    lr = 0.05
    if kind == "sgd":
        opt = optim.SGD(li.params, lr=lr, max_grad_norm=max_norm, **kw)
        if nstate:
            for i, q in enumerate(li.params):
                opt.state[q]["momentum_buffer"] = li.views[2][i]
    else:
        opt = optim.Adam(li.params, lr=lr, max_grad_norm=max_norm, **kw)
        for i, q in enumerate(li.params):
            opt.state[q].update(step=torch.tensor(0.0), exp_avg=li.views[2][i], exp_avg_sq=li.views[3][i])
            if amsgrad:
                opt.state[q]["max_exp_avg_sq"] = li.views[4][i]
    for t in range(1, steps + 1):
        g = gaussians(li.numels, 100 + t)
        li.fill(1, g)
        opt.step()
        norm = opt.last_grad_norm.cpu().numpy() if max_norm is not None else None
        if norm is not None:
            want, _ = R.grad_norm64(with_grad(g))
            assert abs(float(norm[0]) - want) <= R.norm_rel_bound(li.numels) * want and norm[1] == 0.0
            assert (R.clip_coef(norm, max_norm) < 1) == (max_norm < want)
        for i in range(len(p)):
            if i == R.NO_GRAD:
                continue
            if kind == "sgd":
                p[i], b = R.sgd_step(p[i], g[i], state[0][i] if nstate else None, lr, norm=norm, max_norm=max_norm or 0.0, **kw)
                if nstate:
                    state[0][i] = b
            else:
                p[i], state[0][i], state[1][i], x = R.adam_step(
                    p[i], g[i], state[0][i], state[1][i], state[2][i] if amsgrad else None, lr, t,
                    weight_decay=kw.get("weight_decay", 0.0), norm=norm, max_norm=max_norm or 0.0)
                if amsgrad:
                    state[2][i] = x
        assert all(np.array_equal(a, b) for a, b in zip(li.read(1), g)), "the fused clip wrote a gradient"
    for i, (a, b) in enumerate(zip(li.read(0), p)):
        assert np.array_equal(a, b), (f"parameter {i} of {li.numels[i]} elements", int((a != b).sum()))
    for k in range(nstate):
        for i, (a, b) in enumerate(zip(li.read(2 + k), state[k])):
            assert np.array_equal(a, b), (f"state {k} of tensor {i}", int((a != b).sum()))
    li.check_sentinels()
    if kind == "adam":
        assert all(float(opt.state[q]["step"]) == (0 if i == R.NO_GRAD else steps) for i, q in enumerate(li.params))


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("case", SGD_CASES)
def test_sgd_steps_are_the_restatement_bit_for_bit(case, clip):
    _run_steps("sgd", SGD_CASES[case], CLIPS[clip])


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("case", ADAM_CASES)
def test_adam_steps_are_the_restatement_bit_for_bit(case, clip):
    _run_steps("adam", ADAM_CASES[case], CLIPS[clip])


@pytest.mark.parametrize("max_norm", (1.0, 1e4), ids=("below", "above"))
def test_grad_clip_alone_is_g_times_c(max_norm):
    from myrtlespeech_amd import optim
    li = Lists(2)
    g = gaussians(li.numels, 9)
    li.fill(1, g)
    norm = optim.clip_grad_norm_(li.params, max_norm).cpu().numpy()
    assert (R.clip_coef(norm, max_norm) < 1) == (max_norm == 1.0)
    for i, (a, b) in enumerate(zip(li.read(1), g)):
        assert np.array_equal(a, b if i == R.NO_GRAD else R.grad_clip(b, norm, max_norm)), i
    li.check_sentinels()


def test_grad_clip_bumps_each_gradient_version_once():
    """(On tensors of their own: the views of ``Lists`` share their buffer's counter.)"""
    from myrtlespeech_amd import optim
    params = [torch.nn.Parameter(torch.randn(5, 3, device="cuda")), torch.nn.Parameter(torch.randn(7, device="cuda"))]
    for p in params:
        p.grad = torch.randn_like(p)
    versions = [p.grad._version for p in params]
    optim.clip_grad_norm_(params, 0.5)
    assert [p.grad._version for p in params] == [v + 1 for v in versions]


# ---- 4: non-finite gradients (arithmetic on NaN and Inf, nothing else) ---------------------------------------------------------
BAD = (5, 17)      # tensor (the one of exactly a chunk) and element that carries the NaN or the Inf


def _sgd_on(value, max_norm, **kw):
    from myrtlespeech_amd import optim
    li = Lists(2)
    p, g = gaussians(li.numels, 1, 1.0), gaussians(li.numels, 2)
    g[BAD[0]][BAD[1]] = value
    li.fill(0, p)
    li.fill(1, g)
    opt = optim.SGD(li.params, lr=0.05, max_grad_norm=max_norm, **kw)
    opt.step()
    li.check_sentinels()
    return li, p, g, opt


def test_nan_gradient_sets_the_flag_and_poisons_what_torch_would():
    li, p, g, opt = _sgd_on(np.nan, 1.0)
    norm = opt.last_grad_norm.cpu().numpy()
    assert np.isnan(norm[0]) and norm[1] == 1.0 and np.isnan(R.clip_coef(norm, 1.0))
    for i, a in enumerate(li.read(0)):
        assert np.array_equal(a, p[i]) if i == R.NO_GRAD else np.isnan(a).all(), i
    # without clipping only that element's chain
    li, p, g, opt = _sgd_on(np.nan, None)
    assert opt.last_grad_norm is None
    for i, a in enumerate(li.read(0)):
        want = p[i] if i == R.NO_GRAD else R.sgd_step(p[i], g[i], None, 0.05)[0]
        assert np.array_equal(a, want, equal_nan=True), i
        assert int(np.isnan(a).sum()) == (1 if i == BAD[0] else 0)


def test_infinite_gradient_clips_to_zero():
    li, p, g, opt = _sgd_on(np.inf, 1.0)
    norm = opt.last_grad_norm.cpu().numpy()
    assert np.isinf(norm[0]) and norm[1] == 1.0 and R.clip_coef(norm, 1.0) == 0.0
    for i, a in enumerate(li.read(0)):
        want = p[i].copy()      # c == 0: g * 0 is 0 and the parameter stays, except Inf * 0 = NaN
        if i == BAD[0]:
            want[BAD[1]] = np.nan
        assert np.array_equal(a, want, equal_nan=True), i


def test_skip_nonfinite_writes_nothing_and_does_not_count_the_step():
    from myrtlespeech_amd import optim
    li = Lists(5)
    li.fill(0, gaussians(li.numels, 1, 1.0))
    for k in (2, 3, 4):
        li.fill(k, [np.zeros(n, np.float32) for n in li.numels])
    opt = optim.Adam(li.params, lr=0.05, amsgrad=True, max_grad_norm=1.0, skip_nonfinite=True)
    for i, q in enumerate(li.params):
        opt.state[q].update(step=torch.tensor(0.0), exp_avg=li.views[2][i], exp_avg_sq=li.views[3][i],
                            max_exp_avg_sq=li.views[4][i])
    li.fill(1, gaussians(li.numels, 2))
    opt.step()
    assert opt.skipped_steps == 0 and float(opt.state[li.params[1]]["step"]) == 1.0
    before = [buf.clone() for buf in li.bufs]
    versions = [q._version for q in li.params]
    g = gaussians(li.numels, 3)
    g[BAD[0]][BAD[1]] = np.nan
    li.fill(1, g)
    g_buf = li.bufs[1].clone()
    opt.step()
    assert opt.skipped_steps == 1 and opt.last_grad_norm.cpu().numpy()[1] == 1.0
    assert all(float(opt.state[q]["step"]) == (0.0 if i == R.NO_GRAD else 1.0) for i, q in enumerate(li.params))
    for role in (0, 2, 3, 4):
        assert li.bufs[role].cpu().numpy().tobytes() == before[role].cpu().numpy().tobytes(), role
    assert li.bufs[1].cpu().numpy().tobytes() == g_buf.cpu().numpy().tobytes()
    assert [q._version for q in li.params] == versions
    # ... and the next finite step is step 2
    li.fill(1, gaussians(li.numels, 4))
    opt.step()
    assert opt.skipped_steps == 1 and float(opt.state[li.params[1]]["step"]) == 2.0


def test_c_abi_refuses_skip_without_norm():
    import ctypes
    from myrtlespeech_amd import _lib
    lib = _lib.load()
    t = torch.zeros(3, 8, device="cuda")
    ptrs = [(ctypes.c_void_p * 1)(t[k].data_ptr()) for k in range(3)]
    numels = (ctypes.c_int64 * 1)(8)
    rc = lib.ms_sgd_step(ptrs[0], ptrs[1], None, numels, 1, 0.1, 0.0, 0.0, 0, None, 0.0, 1, _lib.stream_ptr())
    assert rc == 1      # MS_ERR_INVALID
    rc = lib.ms_adam_step(ptrs[0], ptrs[1], ptrs[2], ptrs[2], None, numels, 1, 0.9, 0.999, 1e-8, 0.0, 0.1, 1.0, None, 0.0, 1,
                          _lib.stream_ptr())
    assert rc == 1
    assert float(t.abs().max()) == 0.0


# ---- 5: the version protocol -------------------------------------------------------------------------------------------------------
def _modules(which):
    from myrtlespeech_amd.model.fully_connected import FullyConnected
    from myrtlespeech_amd.model.rnn import RNN, RNNType
    torch.manual_seed(4)
    if which == "fully_connected":
        make = lambda: FullyConnected(16, 6, 1, 8, torch.nn.Hardtanh(0.0, 20.0)).cuda().eval()      # noqa: E731
        x = torch.randn(3, 7, 16, device="cuda")
    else:
        make = lambda: RNN(RNNType.LSTM, 12, 8).cuda().eval()      # noqa: E731
        x = torch.randn(7, 3, 12, device="cuda")
    return make, x, torch.tensor([7, 5, 2])


@pytest.mark.parametrize("which", ("fully_connected", "rnn"))
@pytest.mark.parametrize("opt_name", ("SGD", "Adam"))
def test_a_forward_after_step_runs_on_the_new_weights(which, opt_name):
    from myrtlespeech_amd import optim
    make, x, lens = _modules(which)
    module = make()

    def run(m):
        out = m((x.clone(), lens))
        out = out[0] if which == "rnn" else out      # ((y, lens), hid) or (y, lens)
        return out[0].clone()

    first = run(module)
    params = list(module.parameters())
    for p in params:
        p.grad = torch.randn_like(p)
    versions = [p._version for p in params]
    before = [p.detach().clone() for p in params]
    opt = getattr(optim, opt_name)(params, lr=0.5)
    opt.step()
    assert all(not torch.equal(p.detach(), b) for p, b in zip(params, before))
    assert [p._version for p in params] == [v + 1 for v in versions]
    second = run(module)
    assert not torch.equal(second, first)
    fresh = make()
    fresh.load_state_dict(module.state_dict())
    assert torch.equal(second, run(fresh))
    if opt_name == "Adam":
        state_versions = [opt.state[p]["exp_avg"]._version for p in params]
        opt.step()
        assert [opt.state[p]["exp_avg"]._version for p in params] == [v + 1 for v in state_versions]


# ---- 6: fit() on the device ------------------------------------------------------------------------------------------------------
def _fit_setup(model):
    from test_ds2_train_gpu import batch, build_model
    from myrtlespeech_amd.loss.ctc_loss import CTCLoss
    from myrtlespeech_amd.model.seq_to_seq import SeqToSeq
    w, d = M.make(model)
    net, params = build_model(model, w)
    inputs, targets = batch(d)
    return SeqToSeq(net, CTCLoss(), []), list(params.values()), [(inputs, targets)] * 2


def _train_losses():
    from myrtlespeech_amd.run.callbacks import Callback
    losses = []

    class Losses(Callback):
        def on_backward_begin(self, **kw):
            if self.training:
                losses.append(float(kw["last_loss"].detach()))

    return Losses(), losses


_SGD_LOSSES = {}


def _want_losses(model):
    if model not in _SGD_LOSSES:
        w, d = M.make(model)
        _SGD_LOSSES[model] = M.sgd_losses(model, w, d, steps=4)[:4]
    return _SGD_LOSSES[model]


@pytest.mark.parametrize("model", M.MODELS)
def test_fit_with_project_sgd_follows_the_float64_losses(model):
    from myrtlespeech_amd import optim
    from myrtlespeech_amd.run.callbacks import ClipGradNorm
    from myrtlespeech_amd.run.train import fit
    finals = []
    for clip in (False, True):
        s, params, loader = _fit_setup(model)
        s.optim = optim.SGD(params, lr=M.LR)
        cb, losses = _train_losses()
        fit(s, 2, loader, callbacks=[cb] + ([ClipGradNorm(s, max_norm=1e9)] if clip else []))
        want = _want_losses(model)
        print("fit losses", losses, "float64", want)
        assert len(losses) == 4 and all(b < a for a, b in zip(losses, losses[1:])), losses
        assert all(abs(a - b) <= 1e-3 * abs(b) for a, b in zip(losses, want)), (losses, want)
        assert all(p.grad is None for p in params) and s.training
        finals.append([p.detach().clone() for p in params])
    # a clip that does not bite multiplies by exactly 1
    assert all(torch.equal(a, b) for a, b in zip(*finals))


@pytest.mark.parametrize("model", M.MODELS)
def test_fit_with_built_adam_and_fused_clip_lowers_the_loss(model):
    from myrtlespeech_amd import optim, protos
    from myrtlespeech_amd.builders import optimizer as B
    from myrtlespeech_amd.run.train import fit
    s, params, loader = _fit_setup(model)
    cfg = protos.parse("adam { learning_rate: 0.01 } exponential_lr { gamma: 0.9 }", protos.TrainConfig)
    s.optim, s.lr_scheduler = B.build(cfg, params, max_grad_norm=1.0)
    assert type(s.optim) is optim.Adam
    cb, losses = _train_losses()
    fit(s, 3, loader, callbacks=[cb])
    print("fit losses under Adam", losses, "last norm", s.optim.last_grad_norm.cpu().tolist())
    assert len(losses) == 6 and losses[4] < losses[0], losses
    assert s.optim.param_groups[0]["lr"] == pytest.approx(0.01 * 0.9 ** 3)
    assert all(float(s.optim.state[p]["step"]) == 6.0 for p in params)
