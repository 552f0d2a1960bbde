"""The dropout specification restated in numpy (TEST INFRASTRUCTURE ONLY): the comment on ``ms_dropout_forward`` in
include/ms_hotpath.h, independent of the package's code.

``philox(counter, key)``           Philox4x32-10 on ``uint64`` arrays holding 32-bit words: counter [..., 4], key [..., 2] -> [..., 4].
``threshold(p)`` / ``scale(p)``    ``ceil(p * 2^32)`` in exact integers; ``float32(1 / (1 - p))`` (0 for p == 1).
``words(n, seed, offset)``         the 32-bit word of each of n elements: element e reads word e & 3 of counter
                                   (q_lo, q_hi, offset_lo, offset_hi), q = e >> 2, under key (seed_lo, seed_hi).
``mask(n, p, seed, offset)``       bool [n]: kept iff word >= threshold.
``multiplier(...)``                float32 [n]: scale where kept, +0 elsewhere.
``forward(x, ...)``                float32 ``x * multiplier`` -- one multiply, so NaN and Inf survive a drop.
``clamp_backward(dy, y, lo, hi, ...)``   ``(lo < y < hi) ? dy * multiplier : 0``.
"""
import math
from fractions import Fraction

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox(counter, key):
    c = [np.asarray(counter, dtype=np.uint64)[..., i].copy() for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i].copy() for i in range(2)]
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]          # (32 x 32 bits: the product fits in 64)
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + np.uint64(W0)) & MASK32, (k[1] + np.uint64(W1)) & MASK32]
    return np.stack(c, axis=-1)


def threshold(p):
    assert 0.0 < p <= 1.0
    return math.ceil(Fraction(float(p)) * 2 ** 32)


def scale(p):
    return np.float32(0.0) if p == 1.0 else np.float32(1.0 / (1.0 - float(p)))


def words(n, seed, offset):
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    counter = np.stack([q & MASK32, q >> np.uint64(32), np.full(nq, offset & 0xFFFFFFFF, dtype=np.uint64),
                        np.full(nq, offset >> 32, dtype=np.uint64)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return philox(counter, np.broadcast_to(key, (nq, 2))).reshape(-1)[:n]


def mask(n, p, seed, offset):
    return words(n, seed, offset) >= np.uint64(threshold(p))


def multiplier(n, p, seed, offset):
    return np.where(mask(n, p, seed, offset), scale(p), np.float32(0.0)).astype(np.float32)


def forward(x, p, seed, offset):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x.reshape(-1) * multiplier(x.size, p, seed, offset)).reshape(x.shape)


def clamp_backward(dy, y, lo, hi, p, seed, offset):
    dy, y = np.asarray(dy, dtype=np.float32), np.asarray(y, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        gate = (np.float32(lo) < y) & (y < np.float32(hi))
    return np.where(gate, forward(dy, p, seed, offset), np.float32(0.0)).astype(np.float32)
