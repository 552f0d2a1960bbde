"""Plain-Python restatement of the specification of ``ms_edit_distance`` (the comment in include/ms_hotpath.h): how a row of
labels becomes units, the ordered three-way minimum, the operation counts that travel with the cost.  Nothing here is shared
with the kernel: units are tuples of labels compared as tuples, the recurrence is the textbook full matrix walked row by row."""
import numpy as np

TOKENS, WORDS = 0, 1


def units(labels, mode, separator=-1, n_symbols=0):
    """The units of one row: its labels (token mode), or its words as tuples of labels (word mode)."""
    labels = [int(v) for v in labels]
    if mode == TOKENS:
        return labels
    kept = [v for v in labels if 0 <= v < n_symbols]          # Alphabet.get_symbols: an index without a symbol is skipped
    words, word = [], []
    for v in kept:                                             # WordSegmentor: cut at the separator, drop empty words
        if v == separator:
            if word:
                words.append(tuple(word))
                word = []
        else:
            word.append(v)
    if word:
        words.append(tuple(word))
    return words


def counts(a, b):
    """(distance, S, D, I, m, n) for hypothesis units ``a`` and reference units ``b``."""
    m, n = len(a), len(b)
    # a cell is (cost, S, D, I); row i of the matrix
    prev = [(j, 0, j, 0) for j in range(n + 1)]                # D[0][j]: j deletions
    for i in range(1, m + 1):
        cur = [(i, 0, 0, i)]                                   # D[i][0]: i insertions
        ai = a[i - 1]
        for j in range(1, n + 1):
            c, s, d, k = prev[j - 1]                           # 1. (i-1, j-1): a match or a substitution
            if ai != b[j - 1]:
                best = (c + 1, s + 1, d, k)
            else:
                best = (c, s, d, k)
            c, s, d, k = cur[j - 1]                            # 2. (i, j-1): a deletion
            if c + 1 < best[0]:
                best = (c + 1, s, d + 1, k)
            c, s, d, k = prev[j]                               # 3. (i-1, j): an insertion
            if c + 1 < best[0]:
                best = (c + 1, s, d, k + 1)
            cur.append(best)
        prev = cur
    c, s, d, k = prev[n]
    return (c, s, d, k, m, n)


def edit_distance(hyp_rows, ref_rows, mode, separator=-1, n_symbols=0):
    """[N, 6] int64: one ``counts`` row per utterance."""
    out = [counts(units(h, mode, separator, n_symbols), units(r, mode, separator, n_symbols))
           for h, r in zip(hyp_rows, ref_rows)]
    return np.asarray(out, dtype=np.int64).reshape(len(out), 6)
