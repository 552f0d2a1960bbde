"""tests/train_width_cases.py without a device: the lattice is what it says it is, its torch yardstick is the project's own
specification at these widths, torch float32 stays three orders below the criterion of tests/test_train_widths_gpu.py, the
whole list of assertions (``check``) passes on a correct float32 implementation -- torch float32's forward and gradients
standing in for the device's -- and fails on each of four planted faults of the kind the stack nodes could have."""
import numpy as np
import pytest

import bilstm_backward_ref as B
import gru_backward_ref as G
import lstm_backward_ref as L
import train_width_cases as W

IDS = [c.id for c in W.CASES]


def test_lattice():
    assert len(set(IDS)) == len(IDS) == 12
    for i, c in enumerate(W.CASES):
        assert list(c.lens) == sorted(c.lens, reverse=True) and len(c.lens) == c.N, c.id
        assert c.lens[-1] == 1 and c.lens[0] == c.M and c.T == c.M + 3 > c.M, c.id
        assert c.hx == (i % 2 == 0), c.id
        assert not c.in32 or c.In % 32 == 0, c.id
        assert c.M <= (45 if c.id == "L1024p" else 6), c.id      # (45: the shortest batch of 64 that packs its rows)
    assert [c.id for c in W.SINGLE_LAYER] == ["L1024", "L1024g", "L1024p", "L1280", "G1280", "T2600"]
    assert [c.id for c in W.F32_CHILD] == ["L256", "L1024", "G512"]
    assert any(c.hx and c.bidir for c in W.SINGLE_LAYER) and any(not c.hx for c in W.SINGLE_LAYER)


def own_restatement(case):
    """The project's float64 restatement of a single-layer case with its OWN forward, keyed like the yardstick."""
    inp, sd = W.make_inputs(case), W.make_params(case)
    hx, lstm = inp["hx"], case.kind == "LSTM"
    ndir = W.ndir_of(case)
    ps = tuple(W._dir_params(case, sd, d) for d in range(ndir))
    pick = lambda a: a if case.bidir else a[0]      # noqa: E731
    if lstm:
        k = dict(p=pick(ps), T=case.T, N=case.N, H=case.H, In=case.In, lens=inp["lens"], x=inp["x"],
                 h0=None if hx is None else pick(hx[0]), c0=None if hx is None else pick(hx[1]), d_out=inp["d_out"],
                 d_hn=pick(inp["d_hn"]), d_cn=pick(inp["d_cn"]))
        r = B.layer_backward(k) if case.bidir else L.layer_backward(k["p"], k["x"], k["h0"], k["c0"], k["lens"], k["d_out"], k["d_hn"],
                                                                     k["d_cn"])
        if not case.bidir:
            r = {key: (v if key in ("out", "dx") else v[None]) for key, v in r.items()}
        r["d_b_ih"] = r["d_b_hh"] = r.pop("d_b")
    else:
        with np.errstate(over="ignore"):
            r = G.layer_backward(dict(p=ps, T=case.T, N=case.N, H=case.H, In=case.In, lens=inp["lens"], x=inp["x"], h0=hx,
                                      d_out=inp["d_out"], d_hn=inp["d_hn"]), ndir)
    rows = slice(2 * case.H, 3 * case.H) if case.kind == "TANH" else slice(None)
    res = dict(out=r["out"], h_n=r["h_n"], x=r["dx"])
    if lstm:
        res["c_n"] = r["c_n"]
    if hx is not None:
        res["hx"] = r["d_h0"]
        if lstm:
            res["cx"] = r["d_c0"]
    for d in range(ndir):
        sfx = "_l0" + ("_reverse" if d else "")
        for name, key in (("weight_ih", "d_w_ih"), ("weight_hh", "d_w_hh"), ("bias_ih", "d_b_ih"), ("bias_hh", "d_b_hh")):
            res[name + sfx] = r[key][d][rows]
    return res


@pytest.mark.parametrize("cid", [c.id for c in W.SINGLE_LAYER])
def test_yardstick_is_the_specification(cid):
    case = W.BY_ID[cid]
    want, own = W.yardstick(case, np.float64), own_restatement(case)
    assert sorted(want) == sorted(own)
    for key, w in want.items():
        assert own[key].shape == w.shape, key
        assert W.rel_err(own[key], w) <= 1e-10, (cid, key, W.rel_err(own[key], w))


@pytest.mark.parametrize("cid", IDS)
def test_torch_float32_is_far_below_the_criterion(cid):
    """The condition for criterion c: the reference's float32 counterpart sits three orders below 1e-3 (measured worst: 6.8e-7, T200)."""
    case = W.BY_ID[cid]
    want, t32 = W.yardstick(case, np.float64), W.yardstick(case, np.float32)
    worst = max(W.rel_err(t32[key], want[key]) for key in want)
    print(cid, "torch float32 worst error", worst)
    assert worst <= 1e-5, (cid, worst)


_stand_ins = {}


def stand_in(case):
    """torch float32 in place of the device: the five runs of ``check``, computed once per case and never edited."""
    if case.id not in _stand_ins:
        inp = W.make_inputs(case)
        main = W.yardstick(case, np.float32)
        got = {"status": np.zeros((), np.int32)}
        runs = dict(main=main, again=W.yardstick(case, np.float32, inp=inp), short=W.yardstick(case, np.float32, inp=W.cut(inp, case.M)),
                    nan_x=W.yardstick(case, np.float32, inp=dict(inp, x=W.poisoned(inp["x"], case))),
                    nan_dout=W.yardstick(case, np.float32, inp=dict(inp, d_out=W.poisoned(inp["d_out"], case))))
        for run, res in runs.items():
            for key, v in res.items():
                if run == "main" or key not in W.FORWARD_KEYS:
                    got[f"{run}/{key}"] = v
        for key in W.FORWARD_KEYS:
            if key in main:
                got["before/" + key] = got["after/" + key] = main[key]
        _stand_ins[case.id] = got
    return dict(_stand_ins[case.id])


@pytest.mark.parametrize("cid", IDS)
def test_check_passes_on_a_correct_float32_implementation(cid):
    """... criteria b, c, e for every case and d for the single-layer ones: the cap of d is reachable."""
    case = W.BY_ID[cid]
    res = W.check(case, stand_in(case), "torch-float32")
    assert (case.nl == 1) == all(v[2] is not None for v in res.values())


def faulty(case, fault):
    """``stand_in(case)`` with one planted fault."""
    got = stand_in(case)
    inp, sd = W.make_inputs(case), W.make_params(case)
    H, lens = case.H, inp["lens"]
    edit = lambda key, fn, runs=W.RUNS: got.update({f"{r}/{key}": fn(got[f"{r}/{key}"].astype(np.float64)).astype(np.float32) for r in runs})      # noqa: E731
    if fault == "h_prev_late":          # sequence 0's h_prev taken one row too late in direction 0's d_w_hh
        r = W.given_h_parts(case, got["main/out"])[0]
        h = got["main/out"][..., :H].astype(np.float64)
        delta = sum(np.outer(r["dGh"][t, 0], h[t, 0] - r["h_prev"][t, 0]) for t in range(lens[0]))
        edit("weight_hh_l0", lambda a: a + delta)
    elif fault == "d_out_past_length":  # the row of d_out just past the shortest sequence let into the top layer
        n, t = case.N - 1, 1
        assert lens[n] == 1
        leak = 0.1 * np.tile(inp["d_out"][t, n, :H].astype(np.float64), W.gates_of(case.kind))

        def row(a, v):
            a = a.copy()
            a[t, n] += v
            return a
        edit("bias_ih_l0", lambda a: a + leak, ("main", "again", "short", "nan_x"))
        edit("x", lambda a: row(a, leak @ sd["weight_ih_l0"].astype(np.float64)), ("main", "again", "short", "nan_x"))
        edit("bias_ih_l0", lambda a: a + np.nan, ("nan_dout",))
        edit("x", lambda a: row(a, np.nan), ("nan_dout",))
    elif fault == "reverse_h0_at_T":    # the reverse direction's h0 product taken at row T - 1 where len_n - 1 is meant
        assert case.bidir and case.hx
        r = W.given_h_parts(case, got["main/out"])[1]
        h0 = (inp["hx"][0] if case.kind == "LSTM" else inp["hx"])[1].astype(np.float64)
        delta = -sum(np.outer(r["dGh"][lens[n] - 1, n], h0[n]) for n in range(case.N))
        edit("weight_hh_l0_reverse", lambda a: a + delta)
    elif fault == "padded_column_in_dx":  # a padded-width slice taken one unit off: a padded unit's (zero) column left in dx
        edit("x", lambda a: np.concatenate([a[..., 1:], np.zeros_like(a[..., :1])], -1))
    return got


@pytest.mark.parametrize("cid,fault,trips", [
    ("L1280", "h_prev_late", "'weight_hh_l0', 0."), ("G1280", "h_prev_late", "'weight_hh_l0', 0."),
    ("L1280", "d_out_past_length", "dx is not zero in a row past a length"),
    ("L1280", "reverse_h0_at_T", "'weight_hh_l0_reverse'"), ("G1280", "reverse_h0_at_T", "'weight_hh_l0_reverse'"),
    ("L200", "padded_column_in_dx", "padded_column_in_dx', 'x'")])
def test_check_fails_on_a_planted_fault(cid, fault, trips):
    """... on the assertion that is there for it: the tensor's own criterion c (a whole tensor off by a third or more of its
    largest magnitude), or the exact zero of dx past a length."""
    case = W.BY_ID[cid]
    W.check(case, stand_in(case), "torch-float32")
    with pytest.raises(AssertionError) as info:
        W.check(case, faulty(case, fault), "torch-float32 with " + fault)
    assert trips in str(info.value), str(info.value)[:300]
