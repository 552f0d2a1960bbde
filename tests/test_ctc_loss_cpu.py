"""tests/ctc_loss_cases.py proved without a GPU: its float64 reference against exact integer path counts (loss and gradient)
and against torch's float64 CPU loss under autograd, a float32 restatement of the pipeline's log2-domain recursion inside
HALF of the derived bound on every toleranced batch, the <= 1e-2 condition, every batch on its intended side of its gate,
and the trap alignments really invalid."""
import math

import numpy as np
import pytest
import torch

import ctc_loss_cases as C


def ids(batches):
    return [b.id for b in batches]


COUNT = [b for b in C.toleranced_batches() if b.family == "count"]


@pytest.mark.parametrize("b", COUNT, ids=ids(COUNT))
def test_reference_equals_the_integer_path_counts(b):
    ref = b.reference(False)
    for n in range(b.N):
        Tn = int(ref["Tn"][n])
        nll, grad = C.count_exact(Tn, b.targets[n], b.blank, b.V)
        if math.isinf(nll):
            assert ref["nll"][n] == np.inf and ref["infeasible"][n] and (Tn == 0 or not ref["grad_defined"][n]), (b.id, n)
            assert b.reference(True)["nll_out"][n] == 0.0 and not b.reference(True)["grad"][:, n].any()
            continue
        assert abs(ref["nll"][n] - nll) <= 1e-11 * max(1.0, nll), (b.id, n, ref["nll"][n], nll)
        if Tn:
            assert np.abs(ref["grad"][:Tn, n] - grad).max() <= 1e-11, (b.id, n)
        assert not ref["grad"][Tn:, n].any()


def test_reference_equals_the_integer_path_counts_on_a_large_lattice():
    """T = 300, 128 labels (S = 257), V = 70: where the float32 oracle of the sweeps is off by 2.6e-3."""
    V, blank, T = 70, 69, 300
    tg = C.labels(128, V, blank, seed=3)
    x = np.repeat((3.0 * np.random.default_rng(5).standard_normal((T, 1, 1))).astype(np.float32), V, axis=2)
    ref = C.reference(x, [T], [tg], blank)
    nll, grad = C.count_exact(T, tg, blank, V)
    assert abs(ref["nll"][0] - nll) <= 1e-11 * nll, (ref["nll"][0], nll)
    assert np.abs(ref["grad"][:, 0] - grad).max() <= 1e-11


def test_exactly_one_alignment_at_the_feasibility_edge():
    for b in C.feasibility_batches():
        for n in (0, 2, 4):
            need = C.min_frames(b.targets[n])
            assert b.in_lens[n] == need and b.in_lens[n + 1] == need - 1
            assert C.count_paths(need, b.targets[n], b.blank)[2] == 1
            assert C.count_paths(need - 1, b.targets[n], b.blank)[2] == 0


def torch_loss(b, zero_infinity):
    """(nll, gradient) of torch's CPU loss in float64: through log_softmax, or with respect to given log-probabilities."""
    x = torch.from_numpy(b.logits().astype(np.float64)).requires_grad_(True)
    lp = x if b.log_probs_in else torch.log_softmax(x, -1)
    S = max(1, max(len(t) for t in b.targets))
    y = torch.tensor([t + [0] * (S - len(t)) for t in b.targets], dtype=torch.long)
    nll = torch.nn.functional.ctc_loss(lp, y, torch.tensor(b.in_lens), torch.tensor([len(t) for t in b.targets]), blank=b.blank,
                                       reduction="none", zero_infinity=zero_infinity)
    nll.sum().backward()
    return nll.detach().numpy(), x.grad.numpy()


SMALL = [b for b in C.ring_batches() + C.feasibility_batches() + C.trap_batches() + C.alphabet_batches()[:27]]
SMALL += [C.Batch("ring_lp", b.T, b.V, b.blank, b.in_lens, b.targets, "gauss", log_probs_in=True) for b in C.ring_batches()[:1]]


@pytest.mark.parametrize("zero_infinity", (False, True))
@pytest.mark.parametrize("b", SMALL, ids=ids(SMALL))
def test_reference_equals_torch_float64(b, zero_infinity):
    """Repeats, empty targets, in_lens of 0, impossible targets, zero_infinity and given log-probabilities."""
    ref = b.reference(zero_infinity)
    nll, grad = torch_loss(b, zero_infinity)
    assert np.array_equal(np.isinf(nll), np.isinf(ref["nll_out"]))
    fin = np.isfinite(nll)
    assert np.abs(nll[fin] - ref["nll_out"][fin]).max() <= 1e-10
    for n in range(b.N):
        if ref["grad_defined"][n]:
            assert np.abs(grad[:, n] - ref["grad"][:, n]).max() <= 1e-11, (b.id, n)


def test_minus_infinity_entries_and_poison_in_the_reference():
    """A -inf logit is a legal "impossible" (the gradient there is exactly 0, torch agrees); a non-finite normaliser or a NaN
    log-probability poisons that utterance only."""
    b = [r for r in C.ring_batches() if r.family == "gauss"][0]
    x = b.logits().copy()
    free = [k for k in range(b.V) if k != b.blank and k not in b.targets[8]][0]
    x[5, 8, free] = -np.inf           # avoidable
    x[4, 5, b.blank] = -np.inf        # c, c, c in 16 frames: the blank is avoidable at one frame
    x[0, 4, [b.blank, b.targets[4][0]]] = -np.inf      # neither start of a, b, c is possible: +inf, 0 under zero_infinity
    ref = C.reference(x, b.in_lens, b.targets, b.blank, zero_infinity=True)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    y = torch.tensor([t + [0] * (3 - len(t)) for t in b.targets], dtype=torch.long)
    nll = torch.nn.functional.ctc_loss(torch.log_softmax(xt, -1), y, torch.tensor(b.in_lens),
                                       torch.tensor([len(t) for t in b.targets]), blank=b.blank, reduction="none", zero_infinity=True)
    nll.sum().backward()
    assert np.abs(nll.detach().numpy() - ref["nll_out"]).max() <= 1e-10
    tg = xt.grad.numpy()
    # (torch's own gradient is NaN on the frames that hold a -inf logit -- 0 times inf, spread by log_softmax's backward)
    assert np.all(np.isfinite(tg) | np.isneginf(x).any(axis=2, keepdims=True))
    assert np.abs(np.where(np.isfinite(tg), tg - ref["grad"], 0.0)).max() <= 1e-11
    assert not ref["grad"][np.isneginf(x)].any()
    assert ref["grad"][5, 8, free] == 0.0 and ref["grad"][4, 5, b.blank] == 0.0
    assert ref["infeasible"][4] and ref["nll_out"][4] == 0.0 and not ref["grad"][:, 4].any()
    for V, lpi in ((29, False), (29, True), (100, True)):
        nb = C.nonfinite_batch(V, log_probs_in=lpi)
        r = nb.reference(True)
        assert r["poisoned"].tolist() == [False, True, True, True, False]
        for n in (1, 2, 3):
            assert np.isnan(r["nll_out"][n]) and np.isnan(r["grad"][:nb.in_lens[n], n]).all() and not r["grad"][nb.in_lens[n]:, n].any()
        assert np.isfinite(r["grad"][:, [0, 4]]).all()


TOLERANCED = list(C.toleranced_batches()) + [C.nonfinite_batch(29), C.nonfinite_batch(100), C.nonfinite_batch(5, S_long=512),
                                              C.nonfinite_batch(29, log_probs_in=True), C.nonfinite_batch(100, log_probs_in=True)]
RESTATED = {}


@pytest.mark.parametrize("b", TOLERANCED, ids=ids(TOLERANCED))
def test_float32_restatement_stays_inside_half_of_the_bound_and_the_bound_inside_its_cap(b):
    ref = b.reference(False)
    fwd, bwd = b.routes()
    bn, _ = C.bounds(b, ref, fwd, bwd)                                   # asserts bound_nll <= 1e-2
    if b.gate in C.WITHOUT_WAVE:
        C.bounds(b, ref, *b.routes(wave=False))
    ok = ~(ref["poisoned"] | ref["infeasible"])
    x = np.where(np.isfinite(b.logits()), b.logits(), np.float32(0.0))    # (the poisoned utterances are not compared)
    got = C.restate_f32(x, b.in_lens, b.targets, b.blank, b.log_probs_in)
    assert np.array_equal(np.isposinf(got[~ref["poisoned"]]), ref["infeasible"][~ref["poisoned"]]), b.id
    err = np.abs(got[ok].astype(np.float64) - ref["nll"][ok])
    assert np.all(err <= 0.5 * bn[ok]), (b.id, err.tolist(), bn[ok].tolist())
    pos = bn[ok] > 0
    if pos.any():
        RESTATED[b.family] = max(RESTATED.get(b.family, 0.0), float((err[pos] / bn[ok][pos]).max()))


def test_restatement_ratio_report():
    print("float32 restatement, largest loss error / bound per family:", {k: round(v, 4) for k, v in sorted(RESTATED.items())})
    assert all(v <= 0.5 for v in RESTATED.values())


def test_every_batch_is_on_its_intended_side_of_its_gate():
    seen = set()
    for b in C.toleranced_batches():
        fwd, bwd, k = C.INTENDED.get(b.name, ("pipeline", "pipeline", 1))
        assert b.routes() == (fwd, bwd), (b.id, b.routes())
        assert b.routes(wave=False) == ("lds_row", "lds_row")
        if k is not None:
            assert C.states_per_lane(b.S_max) == k, (b.id, b.S_max)
        assert not C.forward_refuses(b.S_max) and not C.backward_refuses(b.T, b.V, b.S_max) and not C.backward_refuses(b.T, b.V, b.S_max, False)
        seen.add(b.name)
    assert set(C.INTENDED) <= seen
    assert [b.S_max for b in C.lane_batches()[::3]] == [255, 511, 1023, 1025]
    # the gates themselves
    assert C.mailbox_bytes(C.LAST_MAILBOX_T) == C.LDS_BYTES and C.mailbox_bytes(C.LAST_MAILBOX_T + 1) > C.LDS_BYTES
    assert (5 * 75 + 16001) * 4 <= C.GRAD_ROWS_LDS_BYTES < (5 * 77 + 16001) * 4
    L = C.FIRST_REFUSED_FORWARD_L
    assert C.forward_refuses(2 * L + 1) and not C.forward_refuses(2 * L - 1)
    L = C.FIRST_REFUSED_BACKWARD_L
    assert C.backward_refuses(2, 3, 2 * L + 1) and not C.backward_refuses(2, 3, 2 * L - 1)
    assert C.forward_route(2, 3, 2 * L + 1) == "lds_row"
    # lattice positions the tables promise
    k1 = C.lane_batches()[0]
    assert {2 * len(t) + 1 for t in k1.targets} >= {65, 129, 193}
    k4 = C.lane_batches()[6]
    assert {v % 8 for v in k4.in_lens} == set(range(8)) and min(k4.in_lens) == 522 and max(k4.in_lens) == 530
    assert {v % 16 for b in (k1, C.ring_batches()[0]) for v in b.in_lens} == set(range(16))
    for b in C.lane_batches() + C.gate_batches():
        assert all(C.min_frames(t) <= n for t, n in zip(b.targets, b.in_lens)), b.id
    for b in C.alphabet_batches():
        sym = [k for k in range(b.V) if k != b.blank]
        if sym:
            used = {k for t in b.targets for k in t}
            assert sym[0] in used and sym[-1] in used


def test_valid_alignments_spell_the_target_and_traps_do_not():
    for b in C.lane_batches() + C.gate_batches() + C.ring_batches():
        if b.family != "path":
            continue
        ref = b.reference(False)
        for n in range(b.N):
            sym = C.alignment(b.variant, b.in_lens[n], b.targets[n], b.blank)
            if ref["infeasible"][n]:
                continue
            assert len(sym) == b.in_lens[n] and C.collapse(sym, b.blank) == b.targets[n], (b.id, n)
            assert ref["nll"][n] <= 1e-3, (b.id, n, ref["nll"][n])       # (V - 1) e^-24 per frame, and little else
    for b in C.trap_batches():
        ref = b.reference(False)
        for n in range(b.N):
            sym = C.alignment(b.variant, b.in_lens[n], b.targets[n], b.blank)
            assert len(sym) == b.in_lens[n] and C.collapse(sym, b.blank) != b.targets[n], (b.id, n)
            assert 10.0 < ref["nll"][n] < np.inf, (b.id, n, ref["nll"][n])
