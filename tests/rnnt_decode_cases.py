"""The RNN-T decode (``csrc/rnnt_decode.hip``) at every kernel gate: the case table of ``test_rnnt_decode_cpu.py`` /
``test_rnnt_decode_gpu.py`` (TEST INFRASTRUCTURE ONLY).

Each case is the smallest shape that crosses the gate it names.  ``dispatch`` restates, from the code of ``ms_rnnt_decode``,
which launch sequence, predictor form, kernel template and branch a shape takes; the CPU test holds the table to it (every
value of every dimension is hit).  Weights come from ``RNNTPredictor`` / ``RNNTJoint`` under the case's seed with
``joint.out.weight`` scaled by 6 (peaked distributions, transcripts of several labels; by 20 where a beam would otherwise
return nothing but empty transcripts: one frame, or 480 symbols); encoder frames are N(0, 1) * 2.

THE MARGIN RULE.  The device tests hold the beam's scores to rtol = atol = 1e-4, so two competing scores may each move by
1e-4 and any decision with a float64 gap above 2e-4 has one right answer.  Every seed below was chosen on the CPU so that
every utterance's smallest decision gap (``rnnt_decode_ref``) is at least MARGIN = 1e-3, which leaves a factor of five; with
that, "transcripts are EQUAL" is asserted on the device with no escape clause.  A case is never skipped for its margin: run
this file (``python tests/rnnt_decode_cases.py [id ...]``) and take another seed.
"""
import functools
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

import rnnt_decode_ref as R64

MARGIN = 1e-3
OUT_SCALE = 6.0
E = 16          # encoder features


def dispatch(V, D, H, L, J, N, w, ms, greedy):
    """What ``ms_rnnt_decode`` launches for a shape, restated from its code (None = the dimension does not exist there)."""
    V1 = V + 1
    w = 1 if greedy else w
    R = N * w
    d = dict(sequence=None, predictor=None, rgj=None, fused_form=None, move=None, joint_slots=None,
             gate_row_blocks=None, top_g=None, init_blocks=min((N + 63) // 64, 2))
    recut = (not greedy and H % 64 == 0 and J % 32 == 0 and (8 * 32 * 33 + 64 * 33) * 4 + V1 * 32 * 4 <= 64 * 1024
             and w * V1 * 4 <= 48 * 1024)
    if recut:
        LH = L * H
        d.update(sequence="recut", rgj=1 if H % 128 == 0 else 2, gate_row_blocks=min((R + 63) // 64, 2),
                 move="fast" if LH % 4 == 0 and J % 4 == 0 and LH // 4 <= 512 and J // 4 <= 256 else "slow",
                 top_g="with_joint_only" if L == 1 else "cell_g_launches")
        return d
    fused = H % 16 == 0 and all(((D if l == 0 else H) + H) % 128 == 0 for l in range(L))
    logits = "tile" if J <= 512 and V1 <= 32 else ("v64" if V1 <= 64 else "vloop")
    d.update(sequence="greedy" if greedy else "round4", predictor="fused" if fused else "exact",
             fused_form=(2 if R > 32 else 1) if fused else None, joint_slots=logits + ("/regs" if J <= 1024 else "/loop"))
    return d


DIMENSIONS = dict(sequence={"greedy", "recut", "round4"}, predictor={"fused", "exact"}, rgj={1, 2}, fused_form={1, 2},
                  move={"fast", "slow"}, joint_slots={"tile/regs", "v64/regs", "v64/loop", "vloop/regs", "vloop/loop"},
                  gate_row_blocks={1, 2}, top_g={"with_joint_only", "cell_g_launches"}, init_blocks={1, 2})


@dataclass(frozen=True)
class Case:
    id: str
    gate: str
    greedy: bool
    V: int = 6
    D: int = 8
    H: int = 64
    L: int = 2
    J: int = 32
    N: int = 4
    T: int = 8
    w: int = 4
    ms: int = 3
    lens: Optional[Tuple[int, ...]] = None
    blank_shift: float = 0.0
    out_scale: float = OUT_SCALE
    zero_bias: bool = False         # b_ih[l] = b_hh[l] = NULL through a direct call of ms_rnnt_decode
    claims: Tuple[str, ...] = ("labels3",)

    @property
    def seed(self):
        return SEEDS.get(self.id, 0)

    @property
    def lengths(self):
        if self.lens is not None:
            return np.array(self.lens)
        return np.array([max(1, self.T - (2 * i) % max(self.T - 1, 1)) for i in range(self.N)])

    @property
    def dispatch(self):
        return dispatch(self.V, self.D, self.H, self.L, self.J, self.N, self.w, self.ms, self.greedy)


def parts(c: Case, seed=None):
    """(predictor, joint, their float32 state dicts as numpy, encoder frames [T, N, E] float32) of a case."""
    from myrtlespeech_amd.model.rnnt import RNNTJoint, RNNTPredictor
    seed = c.seed if seed is None else seed
    torch.manual_seed(seed)
    pred = RNNTPredictor(c.V, c.D, c.H, num_layers=c.L).eval()
    joint = RNNTJoint(E, c.H, c.J, c.V).eval()
    with torch.no_grad():
        joint.out.weight *= c.out_scale
        joint.out.bias[c.V] += c.blank_shift
    psd = {k: v.detach().cpu().numpy() for k, v in pred.state_dict().items()}
    jsd = {k: v.detach().cpu().numpy() for k, v in joint.state_dict().items()}
    enc = (np.random.default_rng(seed).normal(size=(c.T, c.N, E)) * 2.0).astype(np.float32)
    return pred, joint, psd, jsd, enc


def compute_reference(c: Case, seed=None):
    _, _, psd, jsd, enc = parts(c, seed)
    net = R64.Net(psd, jsd, c.L, zero_bias=c.zero_bias)
    if c.greedy:
        return R64.greedy_decode(net, enc, c.lengths, c.ms)
    return R64.beam_decode(net, enc, c.lengths, c.w, c.ms)


@functools.lru_cache(maxsize=None)
def reference(c: Case):
    """The float64 reference of a case, computed once per process and shared (do not modify)."""
    return compute_reference(c)


def failed_claims(c: Case, ref):
    """The statistics a case claims (its reason for being in the table) that the reference does not bear out."""
    bad = []
    if min(u["margin"] for u in ref) < MARGIN:
        bad.append("margin")
    nonempty = sum(1 for u in ref if u["hyp"])
    checks = dict(
        labels3=lambda: nonempty >= 3,
        no_labels=lambda: nonempty == 0,
        b_over_64=lambda: max(u["max_b"] for u in ref) > 64,
        b_full=lambda: max(u["max_b"] for u in ref) == c.w * c.ms,
        best_from_past_64=lambda: max(u["best_last_selected"] for u in ref) >= 64,
        merges=lambda: sum(u["merges"] for u in ref) >= 1,
        full_live=lambda: max(u["max_live"] for u in ref) == c.w,
        moved=lambda: sum(u["moved"] for u in ref) >= 1,
        blank_sum=lambda: all(abs(u["score"] - u["blank_sum"]) <= 1e-9 * max(1.0, abs(u["score"])) for u in ref),
        quota_0_31=lambda: {0, 31} <= set().union(*[set(u["quota_frames_mod32"]) for u in ref]),
        quota_rows_0_31=lambda: {0, 31} <= set().union(*[set(u["quota_rows"]) for u in ref]),
        every_frame_quota=lambda: all(k == c.ms for u in ref for k in u["labels_per_frame"]),
        chunk_boundary=lambda: max(u["iterations"] for u in ref) >= 2)
    return bad + [name for name in c.claims if not checks[name]()]


def G(id, gate, **kw):
    kw = dict(kw, w=1, claims=tuple(c for c in kw.get("claims", ("labels3",)) if c != "moved"))    # (a beam statistic)
    return Case(id=id, gate=gate, greedy=True, **kw)


def B2(id, gate, **kw):      # the re-cut beam sequence: H % 64 == 0, J % 32 == 0
    kw.setdefault("J", 32)
    return Case(id=id, gate=gate, greedy=False, **kw)


def B4(id, gate, **kw):      # the round-4 beam sequence through J % 32 != 0
    kw.setdefault("J", 48)
    return Case(id=id, gate=gate, greedy=False, **kw)


def trio(name, gate, recut=True, gkw=None, **kw):
    """A predictor shape under greedy and under the beam on both sequences."""
    out = [G("greedy_" + name, gate, **dict(kw, **(gkw or {})))]
    if recut:
        out.append(B2("recut_" + name, gate, **kw))
    out.append(B4("round4_" + name, gate, **kw))
    return out


CASES = (
    # ---- predictor depth and shape
    trio("L1", "L = 1: no pred_gemm3_cell_g_kernel launch, the top layer's G rides with the joint at layer 0", L=1)
    + trio("L3_fused_R16", "L = 3, D = H = 64: xrow / xrow2 ping-pong, wih + (l - 1) wplane3, bcat_off / wcat_off walk; R <= 32",
           L=3, D=64, claims=("labels3", "moved"))
    + trio("L3_fused_R40", "L = 3 on the 64-row forms (R = 40)", L=3, D=64, N=5, w=8, gkw=dict(N=40, T=6))
    + trio("L3_exact", "L = 3 on the exact-f32 predictor (D = 8: K = 72)", L=3)
    + trio("D192", "D > H on the fused form: xplane stride max(D, H) + H", D=192, T=10)
    + trio("H40", "H % 16 != 0: exact-f32 predictor, round-4 only", recut=False, H=40)
    + trio("H128_L1", "H % 128 == 0 with L = 1: RGJ = 1", H=128, L=1)
    + [
        # ---- wide beams
        # (best_from_past_64: the RETURNED hypothesis descends from an entry beyond B's 64th -- only the best one is an output,
        # so a survivor taken from there that later drops out would show nothing)
        B2("recut_w32", "w = 32, R = 96: lane + 64 half of beam_select, second row block of the gate GEMMs", w=32, N=3, T=6,
           lens=(6, 5, 4), claims=("labels3", "b_over_64", "best_from_past_64", "merges", "full_live")),
        B4("round4_w32", "w = 32, R = 96 on the round-4 sequence", w=32, N=3, T=6, lens=(6, 5, 4),
           claims=("labels3", "b_over_64", "best_from_past_64", "merges", "full_live")),
        B2("recut_w32_ms4", "w = 32, max_symbols = 4: bcap = 128, the documented maximum, and B fills it", w=32, ms=4, N=3, T=5,
           lens=(5, 4, 3), claims=("labels3", "b_over_64", "b_full", "best_from_past_64", "merges", "full_live")),
        B4("round4_w24_fused", "w = 24, R = 72 (above 64, no multiple of 32) on pred_layer_fused_kernel<2>'s second row block",
           w=24, D=64, N=3, T=6, lens=(6, 4, 5), claims=("labels3", "b_over_64", "full_live")),
        B2("recut_w24", "w = 24, R = 72 on the re-cut sequence", w=24, N=3, T=6, lens=(6, 4, 5), claims=("labels3", "full_live")),
        # ---- the frame end's state move (re-cut)
        B2("recut_J1056", "J > 1024: slow state move", J=1056, N=3, T=6, lens=(6, 4, 5)),
        B2("recut_LH2240", "L H > 2048 (L = 5, H = 448): slow state move", L=5, H=448, w=2, N=3, T=4, lens=(4, 3, 4)),
        # ---- joint_slots_kernel (greedy, and the round-4 beam through J % 32 != 0)
        G("greedy_V40", "V1 in (32, 64]", V=40, J=48), B4("round4_V40", "V1 in (32, 64]", V=40),
        G("greedy_J528", "J in (512, 1024] off the register tile", V=9, J=528), B4("round4_J528", "J in (512, 1024]", V=9, J=528),
        G("greedy_J1040", "J > 1024: encoder row not in registers", J=1040), B4("round4_J1040", "J > 1024", J=1040),
        # ---- limits, on their legal side
        B4("round4_V479_w32", "w (V + 1) 4 = 60 KB of candidates exactly", V=479, w=32, ms=2, N=3, T=3, lens=(3, 2, 3),
           out_scale=20.0),
        G("greedy_joint_64KB", "(J + V + 1) 4 = 64 KB exactly", V=383, J=16000, N=3, T=4, lens=(4, 3, 4)),
        # ---- batch and rounds
        G("greedy_N70", "N > 64: the init kernel's second block", N=70, T=6),
        G("greedy_N70_fused", "N > 64 on pred_layer_fused_kernel<2>: its second row block", N=70, D=64, T=6),
        B2("recut_N70_w2", "N > 64 (R = 140)", N=70, w=2, T=6),
        G("greedy_zero_mid", "a zero length in the middle of an unsorted batch", N=5, lens=(5, 0, 8, 3, 7)),
        B2("recut_zero_mid", "a zero length in the middle of an unsorted batch", N=5, lens=(5, 0, 8, 3, 7)),
        B4("round4_zero_mid", "a zero length in the middle of an unsorted batch", N=5, lens=(5, 0, 8, 3, 7)),
        G("greedy_T1", "T = 1", T=1, lens=(1, 1, 0, 1)),
        B2("recut_T1", "T = 1", T=1, N=5, lens=(1, 1, 0, 1, 1), out_scale=20.0),
        B4("round4_T1", "T = 1", T=1, N=5, lens=(1, 1, 0, 1, 1), out_scale=20.0),
        B2("recut_null_bias", "b_ih[l] = b_hh[l] = NULL (unit_major_add_kernel)", zero_bias=True),
        B4("round4_null_bias", "b_ih[l] = b_hh[l] = NULL (pack_cat_kernel)", zero_bias=True),
        G("greedy_null_bias_fused", "b_ih[l] = b_hh[l] = NULL (pack_cat3_kernel)", D=64, zero_bias=True),
        B2("recut_ms1", "max_symbols = 1: blank transitions only, the score is the sum of blank log-probabilities", ms=1,
           claims=("no_labels", "blank_sum")),
        B4("round4_ms1", "max_symbols = 1", ms=1, claims=("no_labels", "blank_sum")),
        G("greedy_quota", "blank logit - 30: every frame uses its quota, at every frame index mod 32", ms=2, T=33,
          lens=(33, 32, 20, 1), blank_shift=-30.0, claims=("labels3", "quota_0_31", "every_frame_quota")),
        # (an iteration ends at its first label, so with every frame at its quota the quota is always met in row 0 of the chunk;
        # max_symbols = 1 makes every label a quota, and sparse labels put one in the chunk's last row)
        G("greedy_ms1_row31", "max_symbols = 1, blank + 7: a frame's quota met in row 31 of an iteration's chunk", ms=1, N=5, T=96,
          lens=(96, 64, 33, 80, 90), blank_shift=7.0, claims=("labels3", "quota_rows_0_31")),
        G("greedy_len_32_33_64", "lengths at and around the 32-frame chunk", N=3, T=64, lens=(32, 33, 64),
          claims=("labels3", "chunk_boundary")),
        # ---- the event-driven exit (blank + 30: no labels, about ten iterations of 32 blank frames)
        G("greedy_exit_len0", "an empty utterance is finished from the start", ms=4, T=320, lens=(320, 200, 0, 64), blank_shift=30.0,
          claims=("no_labels",)),
        G("greedy_exit_len1", "the same batch with the 0 replaced by 1", ms=4, T=320, lens=(320, 200, 1, 64), blank_shift=30.0,
          claims=("no_labels",)),
    ])

# seed of every case  # the smallest decision margin over its utterances (float64), measured on the CPU
SEEDS = {
    "greedy_L1": 0,  # 4.0e-02
    "recut_L1": 1,  # 1.7e-03
    "round4_L1": 1,  # 1.3e-03
    "greedy_L3_fused_R16": 0,  # 2.2e-02
    "recut_L3_fused_R16": 0,  # 4.0e-03
    "round4_L3_fused_R16": 0,  # 2.0e-03
    "greedy_L3_fused_R40": 0,  # 7.0e-03
    "recut_L3_fused_R40": 0,  # 2.2e-03
    "round4_L3_fused_R40": 2,  # 3.8e-03
    "greedy_L3_exact": 0,  # 1.6e-02
    "recut_L3_exact": 2,  # 2.8e-03
    "round4_L3_exact": 0,  # 3.0e-03
    "greedy_D192": 0,  # 4.5e-02
    "recut_D192": 0,  # 1.8e-03
    "round4_D192": 0,  # 1.4e-03
    "greedy_H40": 0,  # 1.2e-02
    "round4_H40": 12,  # 5.4e-03
    "greedy_H128_L1": 0,  # 1.0e-02
    "recut_H128_L1": 0,  # 5.5e-03
    "round4_H128_L1": 0,  # 6.2e-03
    "recut_w32": 138,  # 1.2e-03
    "round4_w32": 40,  # 1.2e-03
    "recut_w32_ms4": 64,  # 1.3e-03 (B reaches all 128 entries)
    "round4_w24_fused": 5,  # 3.3e-03
    "recut_w24": 4,  # 1.5e-03
    "recut_J1056": 0,  # 5.3e-03
    "recut_LH2240": 21,  # 1.3e-03
    "greedy_V40": 0,  # 1.2e-03
    "round4_V40": 65,  # 1.6e-03
    "greedy_J528": 0,  # 9.6e-03
    "round4_J528": 2,  # 6.4e-03
    "greedy_J1040": 0,  # 4.3e-02
    "round4_J1040": 4,  # 9.4e-03
    "round4_V479_w32": 12,  # 1.2e-03
    "greedy_joint_64KB": 0,  # 2.1e-02
    "greedy_N70": 1,  # 1.2e-03
    "greedy_N70_fused": 0,  # 8.0e-03
    "recut_N70_w2": 104,  # 1.2e-03
    "greedy_zero_mid": 0,  # 7.2e-02
    "recut_zero_mid": 0,  # 5.8e-03
    "round4_zero_mid": 0,  # 2.2e-03
    "greedy_T1": 0,  # 2.5e-01
    "recut_T1": 32,  # 1.3e-02
    "round4_T1": 8,  # 1.3e-02
    "recut_null_bias": 1,  # 3.7e-03
    "round4_null_bias": 4,  # 2.6e-03
    "greedy_null_bias_fused": 0,  # 7.5e-02
    "recut_ms1": 0,  # inf (one hypothesis, no decision)
    "round4_ms1": 0,  # inf
    "greedy_quota": 0,  # 5.8e-02
    "greedy_ms1_row31": 10,  # 2.3e-03
    "greedy_len_32_33_64": 0,  # 6.3e-03
    "greedy_exit_len0": 0,  # 1.8e+01
    "greedy_exit_len1": 0,  # 1.8e+01
}
assert all(isinstance(s, int) for s in SEEDS.values())

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def search(ids):
    """Print, for each case, the first seed whose reference clears MARGIN and bears out the case's claims."""
    for c in CASES:
        if ids and c.id not in ids:
            continue
        for seed in range(200):
            ref = compute_reference(c, seed)
            if not failed_claims(c, ref):
                print(f'    "{c.id}": {seed},  # {min(u["margin"] for u in ref):.1e}', flush=True)
                break
        else:
            print(f"    # {c.id}: no seed below 200", flush=True)


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    search(set(sys.argv[1:]))
