"""The case table of the edit-distance tests (CPU and GPU): each case is a batch of (hypothesis, reference) label rows at the
smallest shape that reaches its edge.  ``expected(case)`` is the restatement's answer, computed once per process.

Edges of the kernels (myrtlespeech_amd/csrc/edit_distance.hip) beyond the ones the specification names:
  * wave against workgroup path: a side whose row width holds at most 63 units -- widths 63 / 64 / 65 on either side, in both
    modes (a word-mode row of width w holds (w + 1) // 2 words), and the padded variants of ``matrices`` move cases across;
  * the wave path's lane axis: the hypothesis or the reference, whichever is narrower; 63 units use the last lane; the other
    side is fed in chunks of 64 units (lengths 64 / 65 / 128 / 129 / 300);
  * the workgroup path's strided loop: 255 / 256 / 257 hypothesis units (the anti-diagonal is indexed by the hypothesis), the
    same counts on the reference side, about 600 tokens;
  * the word scan's steps of 64 labels: words, separators and dropped labels astride positions 63 / 64 / 127 / 128, and more
    than 256 words in an utterance (the hash and canonical-id loops stride)."""
import functools
from collections import namedtuple

import numpy as np

import edit_distance_ref as R

Case = namedtuple("Case", ["name", "mode", "separator", "n_symbols", "hyp", "ref"])
BLOCK = 256            # ED_THREADS
INT32_MAX = 2 ** 31 - 1


def _tok(name, hyp, ref):
    return Case(name, R.TOKENS, -1, 0, [list(map(int, h)) for h in hyp], [list(map(int, r)) for r in ref])


def _wrd(name, hyp, ref, separator=2, n_symbols=3):
    return Case(name, R.WORDS, separator, n_symbols, [list(map(int, h)) for h in hyp], [list(map(int, r)) for r in ref])


def _rand_tokens(rng, n, symbols=3):
    return rng.integers(0, symbols, size=n).tolist()


def _rand_words(rng, n_words, letters=2, separator=2, max_len=2, noise=None):
    """A row of exactly ``n_words`` words over ``letters`` symbols, words of 1 .. max_len letters (so repeats are the rule),
    one or two separators between them, sometimes one in front or behind; ``noise`` = labels to sprinkle that must be dropped."""
    row = [separator] * int(rng.integers(0, 2))
    for w in range(n_words):
        for _ in range(int(rng.integers(1, max_len + 1))):
            row.append(int(rng.integers(0, letters)))
            if noise and rng.integers(0, 4) == 0:
                row.append(int(noise[int(rng.integers(0, len(noise)))]))
        if w + 1 < n_words:
            row += [separator] * int(rng.integers(1, 3))
    row += [separator] * int(rng.integers(0, 2))
    return row


def _build():
    rng = np.random.default_rng(20240521)
    c = []
    # ---- the specification's small edges
    c.append(_tok("tok_both_empty", [[]], [[]]))
    c.append(_tok("tok_hyp_empty", [[]], [[1, 2, 3]]))
    c.append(_tok("tok_ref_empty", [[1, 2, 3]], [[]]))
    c.append(_tok("tok_identical", [[4, 5, 6, 7]], [[4, 5, 6, 7]]))
    c.append(_tok("tok_disjoint", [[1, 1, 1]], [[2, 2, 2, 2, 2]]))
    c.append(_tok("tok_1_vs_300", [[1]], [_rand_tokens(rng, 300)]))
    c.append(_tok("tok_300_vs_1", [_rand_tokens(rng, 300)], [[1]]))
    c.append(_tok("tok_zero_mid_batch", [[1, 2], [], [3, 1, 2], [0]], [[1, 2, 2], [1], [], [0]]))
    c.append(_tok("tok_negative_and_big_labels", [[-1, INT32_MAX, 0, -5]], [[INT32_MAX, -1, 0, -5, 7]]))
    c.append(_tok("tok_n70", [_rand_tokens(rng, int(rng.integers(0, 12))) for _ in range(70)],
                  [_rand_tokens(rng, int(rng.integers(0, 12))) for _ in range(70)]))
    c.append(_wrd("wrd_both_empty", [[]], [[]]))
    c.append(_wrd("wrd_hyp_empty", [[]], [[0, 2, 1]]))
    c.append(_wrd("wrd_ref_empty", [[0, 2, 1]], [[]]))
    c.append(_wrd("wrd_identical", [[0, 1, 2, 1, 0]], [[0, 1, 2, 1, 0]]))
    c.append(_wrd("wrd_disjoint", [[0, 2, 0, 2, 0]], [[1, 2, 1]]))
    c.append(_wrd("wrd_separators", [[2, 0, 1, 2, 2, 1, 2], [2, 2, 2], [2], [0, 2]], [[0, 1, 2, 1], [0], [2, 2], [2, 2, 0, 2, 2]]))
    c.append(_wrd("wrd_out_of_range", [[0, 3, 1, 2, -1, 1, 7, 2, 3], [3, 3, -2], [0, INT32_MAX, 0]],
                  [[0, 1, 2, 1], [3], [0, 0, 3, -7]]))
    c.append(_wrd("wrd_no_separator", [[0, 1, 2, 1], [], [2, 2]], [[0, 1, 2, 1], [0], [2, 2]], separator=-1))
    c.append(_wrd("wrd_no_separator_differs", [[0, 1, 2, 1]], [[0, 1, 1, 1]], separator=-1))
    c.append(_wrd("wrd_letter_order", [[0, 1, 2, 1, 0]], [[1, 0, 2, 0, 1]]))
    c.append(_wrd("wrd_length_and_last_letter", [[0, 1, 2, 0, 1, 1, 2, 0, 1, 0]], [[0, 1, 1, 2, 0, 1, 2, 0, 1, 1]]))
    c.append(_wrd("wrd_1_vs_300", [[0]], [_rand_words(rng, 300)]))
    c.append(_wrd("wrd_300_vs_1", [_rand_words(rng, 300)], [[0]]))
    c.append(_wrd("wrd_zero_mid_batch", [[0, 2, 1], [], [1], [2]], [[0], [1, 2, 1], [], []]))
    c.append(_wrd("wrd_n70", [_rand_words(rng, int(rng.integers(0, 7)), noise=[3, -1]) for _ in range(70)],
                  [_rand_words(rng, int(rng.integers(0, 7)), noise=[3, 9]) for _ in range(70)]))
    # ---- ties and repeated words: two or three symbols
    c.append(_tok("tok_ties_2sym", [_rand_tokens(rng, int(rng.integers(0, 40)), 2) for _ in range(24)],
                  [_rand_tokens(rng, int(rng.integers(0, 40)), 2) for _ in range(24)]))
    c.append(_tok("tok_ties_3sym_wide", [_rand_tokens(rng, int(rng.integers(60, 140)), 3) for _ in range(9)],
                  [_rand_tokens(rng, int(rng.integers(60, 140)), 3) for _ in range(9)]))
    c.append(_wrd("wrd_ties_repeats", [_rand_words(rng, int(rng.integers(0, 30))) for _ in range(24)],
                  [_rand_words(rng, int(rng.integers(0, 30))) for _ in range(24)]))
    c.append(_wrd("wrd_ties_3letters", [_rand_words(rng, int(rng.integers(40, 90)), letters=3, separator=3, max_len=3)
                                        for _ in range(6)],
                  [_rand_words(rng, int(rng.integers(40, 90)), letters=3, separator=3, max_len=3) for _ in range(6)],
                  separator=3, n_symbols=4))
    # ---- unit counts at the wave gate and at the workgroup, on the shorter and on the longer side, both modes
    for k in (63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1):
        other_long, other_short = (300, 40) if k < 100 else (260, 70)
        c.append(_tok(f"tok_hyp_{k}_shorter", [_rand_tokens(rng, k), _rand_tokens(rng, 5)],
                      [_rand_tokens(rng, other_long), _rand_tokens(rng, 9)]))
        c.append(_tok(f"tok_ref_{k}_shorter", [_rand_tokens(rng, other_long), _rand_tokens(rng, 9)],
                      [_rand_tokens(rng, k), _rand_tokens(rng, 5)]))
        c.append(_tok(f"tok_hyp_{k}_longer", [_rand_tokens(rng, k)], [_rand_tokens(rng, other_short)]))
        c.append(_tok(f"tok_ref_{k}_longer", [_rand_tokens(rng, other_short)], [_rand_tokens(rng, k)]))
        c.append(_wrd(f"wrd_hyp_{k}_shorter", [_rand_words(rng, k)], [_rand_words(rng, other_long)]))
        c.append(_wrd(f"wrd_ref_{k}_shorter", [_rand_words(rng, other_long)], [_rand_words(rng, k)]))
        c.append(_wrd(f"wrd_hyp_{k}_longer", [_rand_words(rng, k)], [_rand_words(rng, other_short)]))
        c.append(_wrd(f"wrd_ref_{k}_longer", [_rand_words(rng, other_short)], [_rand_words(rng, k)]))
    # word mode's wave gate is (row width + 1) // 2 <= 63: k one-letter words packed into 2 k - 1 labels
    for k in (63, 64, 65):
        tight = [v for w in range(k) for v in (int(rng.integers(0, 2)), 2)][:-1]
        c.append(_wrd(f"wrd_hyp_tight_{k}", [tight], [_rand_words(rng, 90)]))
        c.append(_wrd(f"wrd_ref_tight_{k}", [_rand_words(rng, 90)], [tight]))
        c.append(_wrd(f"wrd_both_tight_{k}", [tight], [tight[2:] + [2, 1]]))
    c.append(_tok("tok_63_63",[_rand_tokens(rng, 63)], [_rand_tokens(rng, 63)]))
    c.append(_tok("tok_64_64", [_rand_tokens(rng, 64)], [_rand_tokens(rng, 64)]))
    # the wave path's chunks of 64 units of the longer side
    for k in (64, 65, 128, 129):
        c.append(_tok(f"tok_chunk_{k}", [_rand_tokens(rng, 20), _rand_tokens(rng, k)], [_rand_tokens(rng, k), _rand_tokens(rng, 33)]))
    c.append(_tok("tok_600", [_rand_tokens(rng, 600)], [_rand_tokens(rng, 590)]))
    # ---- the word scan's steps of 64 labels: one-letter and long words, separators and dropped labels astride the steps
    rows = []
    for width in (63, 64, 65, 127, 128, 129):
        rows.append([0] * width)                                            # one word as long as the row
        rows.append([0] * (width - 1) + [2])                                # ... closed by the row's last label
        rows.append(([0] * 62 + [2, 1, 1, 2])[:width] + [0] * max(0, width - 66))
        rows.append([3] * 63 + [1] + [3] * (width - 64) if width >= 64 else [3] * width)   # one letter among dropped labels
        rows.append(([0, 2] * 70)[:width])                                  # a word every other label
        rows.append([2] * 63 + [0, 1][: max(0, width - 63)] + [2] * max(0, width - 65))
    c.append(_wrd("wrd_scan_steps", rows, rows[1:] + rows[:1]))
    c.append(_wrd("wrd_scan_dropped_between_letters", [[0] * 63 + [3, 3, 1] + [2, 0]], [[0] * 63 + [1, 2] + [3] * 70 + [0]]))
    return c


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def expected(name):
    """[N, 6] int64 by the restatement; computed once, never edited (read-only array)."""
    c = BY_NAME[name]
    out = R.edit_distance(c.hyp, c.ref, c.mode, c.separator, c.n_symbols)
    out.setflags(write=False)
    return out


def poison(case, variant):
    """A value for the padding behind a row: the separator, an in-range label, a negative value, INT32_MAX."""
    return [case.separator if case.separator >= 0 else 0, 1, -3, INT32_MAX][variant % 4]


def matrices(case, extra=0, variant=None):
    """(hyp [N, Wh], hyp_lens, ref [N, Wr], ref_lens) int32 arrays; rows are ``extra`` columns wider than the longest (at least
    one column), the padding filled with 0 or, with ``variant``, cycling through the poisons starting at that one."""
    def side(rows):
        lens = np.asarray([len(r) for r in rows], dtype=np.int32)
        width = max(int(lens.max()) + extra, 1)
        mat = np.zeros((len(rows), width), dtype=np.int32)
        if variant is not None:
            fill = np.asarray([poison(case, variant + k) for k in range(4)], dtype=np.int32)
            mat[:] = fill[(np.arange(width)[None, :] + np.arange(len(rows))[:, None]) % 4]
        for n, r in enumerate(rows):
            mat[n, :len(r)] = r
        return mat, lens
    (h, hl), (r, rl) = side(case.hyp), side(case.ref)
    return h, hl, r, rl
