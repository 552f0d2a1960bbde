"""CTC beam-search inputs on which candidates have BIT-EQUAL scores, so that the order in which the reference inserts keys
into Pb[t] / Pnb[t] (the stable sort's tie-break, ``Counter.__add__``'s key order) decides the beam.  numpy only.

Two constructions:

* ``twins``: the non-blank symbols come in pairs (one triple when their number is odd) whose probability columns are copies
  of one column, so bit-identical in every frame, at permuted positions; the blank has a column of its own.  Two prefixes
  that differ by swapping twins go through the same operations on the same numbers: equal scores at any length.
* ``dyadic``: every probability is k/16, k in 0 .. 4 -- many equal entries per row, exact zeros, products and sums exact.
  The rows are not normalised (the search does not need it; 16 frames stay far inside float32).

``CASES`` names one case per kernel route and construction; ``case(name)`` builds it once.  Shared by
tests/test_beam_ties_cpu.py, tests/test_beam_ties_gpu.py and tests/golden/gen_golden.py (``gen_beam_ties``)."""
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np


def _zero_blank(x, blank, every):
    if every:
        x[every - 1::every, blank] = 0.0      # frames every-1, 2*every-1, ...: the first frames build a beam first


def twins(T, V, blank, seed, scale=1.0, zero_blank_every=0):
    """[T, V] float32 rows that sum to 1 (up to rounding): softmax(scale * randn) over the groups, a group's column COPIED
    to its members."""
    rng = np.random.default_rng(seed)
    others = rng.permutation([v for v in range(V) if v != blank])
    groups = [list(others[2 * k:2 * k + 2]) for k in range(len(others) // 2)]
    if len(others) % 2:
        groups[0].append(others[-1])          # the odd symbol out shares a pair
    z = np.exp(scale * rng.standard_normal((T, len(groups) + 1)))
    mult = np.asarray([len(g) for g in groups] + [1], dtype=np.float64)
    cols = (z / (z * mult).sum(axis=1, keepdims=True)).astype(np.float32)
    x = np.empty((T, V), dtype=np.float32)
    for g, members in enumerate(groups):
        for v in members:
            x[:, v] = cols[:, g]
    x[:, blank] = cols[:, -1]
    _zero_blank(x, blank, zero_blank_every)
    return x


def dyadic(T, V, blank, seed, zero_blank_every=0):
    """[T, V] float32, every entry k/16 with k in 0 .. 4."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 5, size=(T, V)) / 16.0).astype(np.float32)
    _zero_blank(x, blank, zero_blank_every)
    return x


class Case(NamedTuple):
    name: str
    x: np.ndarray                 # [T, 3, V] float32
    lens: Tuple[int, int, int]    # full length, shorter (another seed), 0 or 1
    blank: int
    width: int
    prune: float
    sep: Optional[int]
    word_weight: float
    range_safe: bool
    route: str                    # the kernel instantiation the shape is meant to reach
    kind: str                     # "twins" | "twins0" (blank zeroed every third frame, threshold 0) | "dyadic"


# route, V, W of the plain search
SHAPES = [("generic", 9, 5), ("generic", 40, 16),
          ("const", 29, 4), ("const", 29, 8), ("const", 29, 16), ("const", 29, 32),
          ("last_lds", 29, 76), ("last_lds", 29, 77),      # (77 is the last width whose working arrays fit the LDS limit)
          ("big", 29, 100), ("big", 8, 256),
          ("wide_lds", 257, 4), ("wide_big", 300, 16)]
# ... and of the range-safe twins (200 frames, flat posteriors: the rescaling rule fires while scores tie)
RS_SHAPES = [("rs_const", 29, 8, 0.5), ("rs_generic", 9, 5, 0.4), ("rs_big", 29, 100, 0.3)]
KINDS = ("twins", "twins0", "dyadic")
# seeds: 1000 + 100 * (the case's number) + 3 * SEED_PICK (three utterances per case).  The picks are the first seeds for which
# the restatement alone (tests/test_beam_ties_cpu.py) finds the zero-blank clip sensitive to WHERE the keys of Pnb[t] alone
# are merged in: with them in front of Pb[t]'s keys instead of behind, the final beam of the full-length utterance differs
SEED_PICK = {"twins0_9x5": 15, "twins0_40x16": 4, "twins0_29x4": 4, "twins0_29x8": 1, "twins0_29x16": 1, "twins0_29x32": 11,
             "twins0_29x76": 4, "twins0_29x77": 14, "twins0_29x100": 4, "twins0_8x256": 4, "twins0_257x4": 11,
             "twins0_300x16": 39, "rs_twins0_29x100": 1}


def _specs():
    """name -> (route, V, W, kind, T, blank, prune, sep, word_weight, range_safe, scale, zero_blank_every, seed, short, tiny).
    The blank walks last / 0 / middle, the separator (a member of a twin pair whenever the clip is a twins clip; word weight
    1.7) comes with every third case, so every route has one; dyadic cases alternate the thresholds 0 (exact zeros are
    pruned) and 1/16 (``p <= threshold`` on exact equality) and zero the blank every fourth frame in every other case."""
    specs = {}
    k = 0
    for route, V, W in SHAPES:
        for kind in KINDS:
            blank = (V - 1, 0, V // 2)[(k // 3 + 2 * k) % 3]
            sep = None
            if (k + k // 3) % 3 == 0:
                sep = (blank + 1 + k % 5) % V
            T = 16 if kind == "dyadic" else 24
            if kind == "twins":
                prune, zero_every = 1e-3, 0
            elif kind == "twins0":
                prune, zero_every = 0.0, 3
            else:
                prune, zero_every = (0.0, 0.0625)[(k // 3) % 2], (0, 4)[(k // 3 + 1) % 2]
            specs[f"{kind}_{V}x{W}"] = (route, V, W, kind, T, blank, prune, sep, 1.7 if sep is not None else 1.0, False, 1.0,
                                        zero_every, 1000 + 100 * k + 3 * SEED_PICK.get(f"{kind}_{V}x{W}", 0), T - 5 - k % 4, k % 2)
            k += 1
    for route, V, W, scale in RS_SHAPES:
        for kind in ("twins", "twins0"):
            blank = (V - 1, 0, V // 2)[k % 3]
            sep = (blank + 3) % V if kind == "twins0" else None
            prune, zero_every = (1e-3, 0) if kind == "twins" else (0.0, 3)
            specs[f"rs_{kind}_{V}x{W}"] = (route, V, W, kind, 200, blank, prune, sep, 1.7 if sep is not None else 1.0, True,
                                           scale, zero_every, 1000 + 100 * k + 3 * SEED_PICK.get(f"rs_{kind}_{V}x{W}", 0), 61 + k, k % 2)
            k += 1
    return specs


class TieStats:
    """A ``hook`` of ``beam_range_ref.search``: the frames in which the sorted score at rank W-1 equals the one at rank W (a
    tie exactly at the beam cut), those in which two entries inside the beam tie, those with a key that exists in Pnb[t]
    only.  ``reverse=True`` also hands back the order that breaks ties in REVERSED insertion order, ``pnb_first=True`` the
    order in which, among equal scores, the keys of Pnb[t] alone come BEFORE the keys of Pb[t] (``Counter.__add__`` puts them
    behind) and nothing else changes."""

    def __init__(self, width, reverse=False, pnb_first=False):
        self.width, self.reverse, self.pnb_first = width, reverse, pnb_first
        self.cut, self.in_beam, self.pnb_only = [], [], []

    def __call__(self, t, scores, keys, pnb_only, order):
        W = self.width
        top = [scores[j] for j in order[:W + 1]]
        if len(top) > W and top[W - 1] == top[W]:
            self.cut.append(t)
        if any(top[i] == top[i + 1] for i in range(min(W, len(top)) - 1)):
            self.in_beam.append(t)
        if pnb_only:
            self.pnb_only.append(t)
        if self.reverse:
            return sorted(range(len(scores)), key=lambda j: (-float(scores[j]), -j))
        if self.pnb_first:
            first_pnb = len(scores) - pnb_only      # (A_next lists the keys of Pb[t], then those of Pnb[t] alone)
            return sorted(range(len(scores)), key=lambda j: (-float(scores[j]), j < first_pnb, j))
        return None


# the device language model's clip: the 29-symbol alphabet of tests/ngram_lm_cases.py (separator 0, blank 28), a width per
# kernel family -- constant shape, generic, working arrays in the workspace
LM_BLANK, LM_SEP, LM_WIDTHS, LM_WEIGHT, LM_WORD_WEIGHT = 28, 0, (8, 5, 96), 1.3, 1.2


LM_KINDS = {"twins": (1e-3, 0, 7700), "twins0": (0.0, 3, 7883)}      # kind -> prune threshold, zero_blank_every, seed
# (7883: the first seed from 7703 in steps of 3 whose zero-blank clip is, at all three widths, sensitive to where the keys of
# Pnb[t] alone are merged in -- see SEED_PICK)


@functools.lru_cache(maxsize=None)
def lm_clip(kind="twins"):
    """(x [24, 3, 29], lens, prune threshold)."""
    prune, zero_every, seed = LM_KINDS[kind]
    x = np.ascontiguousarray(np.stack([twins(24, 29, LM_BLANK, seed + n, 1.0, zero_every) for n in range(3)], axis=1))
    x.setflags(write=False)
    return x, (24, 17, 1), prune


SPECS = _specs()
CASES = tuple(SPECS)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    route, V, W, kind, T, blank, prune, sep, ww, rs, scale, zero_every, seed, short, tiny = SPECS[name]
    if kind == "dyadic":
        utts = [dyadic(T, V, blank, seed + n, zero_every) for n in range(3)]
    else:
        utts = [twins(T, V, blank, seed + n, scale, zero_every) for n in range(3)]
    x = np.ascontiguousarray(np.stack(utts, axis=1))
    x.setflags(write=False)
    return Case(name, x, (T, short, tiny), blank, W, prune, sep, ww, rs, route, kind)
