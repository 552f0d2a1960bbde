"""Word-level back-off n-gram language model for the CTC prefix beam search, resident on the device.

The reference's ``CTCBeamDecoder`` takes ``language_model: Callable[[Tuple[int, ...]], float]``
(post_process/ctc_beam_decoder.py:79, 220-230) and ships only ``no_lm``.  ``NGramLanguageModel`` is such a callable
(Katz / ARPA back-off over words spelled in the alphabet's symbols) AND a table the search kernel reads in device
memory, so a decode with a model is one launch (``CTCBeamDecoder`` / ``StreamingCTCBeamDecoder`` recognise the class).

Two views of one model:

* ``lm(prefix) -> float``: the probability in double precision from the parsed dictionaries -- the model's meaning.
* ``lm.factor(prefix, lm_weight) -> numpy.float32``: what the device multiplies in: the float32 product, from
  ``float32(1)``, of the stored per-entry factors ``float32(backoff ** lm_weight)`` (longest context first) and then
  ``float32(p ** lm_weight)``, each computed once in Python double arithmetic when the table is packed.  It is evaluated by
  walking the packed bytes that are uploaded (same hash, same probe sequence, same probe bound), so host and device
  cannot disagree.  ``lm.weighted_callable(a)`` wraps it as a reference-style callable; used with ``lm_weight=1.0`` it
  reproduces the device arithmetic exactly.

Tokenisation of a prefix (the reference's ``_n_words``, ctc_beam_decoder.py:106-114): one trailing separator -- the
``+ (separator,)`` of the decoder's question -- is dropped, words are the runs between separators (empty words are
dropped), the scored word is what follows the last separator (nothing: the factor is exactly 1.0), the context the
up-to-(order - 1) complete words before it, preceded by ``<s>`` when fewer exist and the model has ``<s>``.  A spelling
that is not in the vocabulary is ``<unk>``.  ``</s>`` entries are read and ignored: the decoder never ends a sentence.

The blob's layout is documented in include/ms_hotpath.h ("n-gram language model").
"""
import ctypes
import os
from typing import Dict, Mapping, Optional, Sequence, Tuple

import numpy as np

MAX_ORDER = 5                    # MS_NGRAM_MAX_ORDER
MAGIC = 0x4D4C534D
HEADER_BYTES = 64
BOS, UNK, EOS = "<s>", "<unk>", "</s>"
_M64 = (1 << 64) - 1
_FLT_MIN = 2.0 ** -126           # smallest normal float32: a stored factor below it is flushed to 0.0


def _step(h: int, x: int) -> int:
    """csrc/ngram_lm.h step()."""
    return ((h ^ ((x + 1) & 0xFFFFFFFF)) * 0x100000001B3) & _M64


def _fin(h: int) -> int:
    """csrc/ngram_lm.h fin(): the murmur3 64-bit finaliser, 0 (the empty slot's key) mapped to 1."""
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & _M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & _M64
    h ^= h >> 33
    return h or 1


def _seed(kind: int, attempt: int) -> int:
    return _fin((0x9E3779B97F4A7C15 * (2 * attempt + kind + 1)) & _M64)


def _stored_factor(x: float, weight: float) -> np.float32:
    """float32(x ** weight), evaluated as a Python float; a result below the normal float32 range is stored as 0."""
    v = float(x) ** float(weight)
    return np.float32(0.0) if v < _FLT_MIN else np.float32(v)


def _place(keys, slots_log2):
    """Linear probing: slot of every key (insertion in the given order) and the longest probe run."""
    mask = (1 << slots_log2) - 1
    taken = {}
    longest = 1
    for k in keys:
        s, n = k & mask, 1
        while s in taken:
            s, n = (s + 1) & mask, n + 1
        taken[s] = k
        longest = max(longest, n)
    return taken, longest


def _slots_log2(count: int) -> int:
    n = 2                                # at least 4 slots; load <= 0.5
    while (1 << n) < 2 * count:
        n += 1
    return n


class NGramLanguageModel:
    """``ngrams``: ``{(w1, ..., wk): (log10_p, log10_backoff)}`` (back-off may be None = 0.0), words as strings over
    ``alphabet`` (``alphabet[i]`` is the character of symbol ``i``); orders 1 .. 5."""

    def __init__(self, ngrams: Mapping[Tuple[str, ...], Tuple[float, Optional[float]]], alphabet: Sequence[str],
                 separator_index: int, unk_log10_p: Optional[float] = None):
        alphabet = list(alphabet)
        if len(set(alphabet)) != len(alphabet) or any(len(ch) != 1 for ch in alphabet):
            raise ValueError("alphabet must hold distinct single characters")
        if not 0 <= int(separator_index) < len(alphabet):
            raise ValueError(f"separator_index={separator_index} outside the alphabet of {len(alphabet)}")
        self.alphabet = alphabet
        self.separator_index = int(separator_index)
        entries = {tuple(k): v for k, v in ngrams.items() if EOS not in k}
        if not entries or any(len(k) == 0 for k in entries):
            raise ValueError("the model has no n-grams")
        self.order = max(len(k) for k in entries)
        if not 1 <= self.order <= MAX_ORDER:
            raise ValueError(f"n-gram order {self.order} outside 1 .. {MAX_ORDER}")
        if (UNK,) not in entries:
            if unk_log10_p is None:
                raise ValueError("the model has no <unk> unigram: unk_log10_p is required")
            entries[(UNK,)] = (float(unk_log10_p), 0.0)
        # words: ids in sorted order (deterministic), spellings in the alphabet's symbols
        symbol_of = {ch: i for i, ch in enumerate(alphabet)}
        words = sorted({w for k in entries for w in k})
        self._id: Dict[str, int] = {w: i for i, w in enumerate(words)}
        self._spelling: Dict[Tuple[int, ...], int] = {}
        for w in words:
            if w in (BOS, UNK):
                continue
            if len(w) == 0 or any(ch not in symbol_of or symbol_of[ch] == self.separator_index for ch in w):
                raise ValueError(f"word {w!r} has a character outside the alphabet")
            if (w,) not in entries:
                raise ValueError(f"word {w!r} occurs in an n-gram but has no unigram")
            self._spelling[tuple(symbol_of[ch] for ch in w)] = self._id[w]
        self.bos_id = self._id.get(BOS, -1)
        self.unk_id = self._id[UNK]
        # {ids: (p, backoff)} as doubles
        self._prob: Dict[Tuple[int, ...], Tuple[float, float]] = {}
        for k, v in entries.items():
            lp, lb = (v[0], v[1]) if isinstance(v, (tuple, list)) else (v, None)
            self._prob[tuple(self._id[w] for w in k)] = (10.0 ** float(lp), 10.0 ** float(0.0 if lb is None else lb))
        self._packed: Dict[float, np.ndarray] = {}
        self._device: Dict[Tuple[float, int], object] = {}

    # ------------------------------------------------------------------ construction from ARPA text
    @classmethod
    def from_arpa(cls, path_or_file, alphabet: Sequence[str], separator_index: int,
                  unk_log10_p: Optional[float] = None) -> "NGramLanguageModel":
        if isinstance(path_or_file, (str, bytes, os.PathLike)):
            with open(path_or_file) as f:
                lines = f.read().splitlines()
        else:
            lines = path_or_file.read().splitlines()
        ngrams, n, seen_data = {}, 0, False
        for raw in lines:
            line = raw.strip()
            if not line:
                continue
            if line == "\\data\\":
                seen_data = True
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                n = int(line[1:-len("-grams:")])
                if not 1 <= n <= MAX_ORDER:
                    raise ValueError(f"n-gram order {n} outside 1 .. {MAX_ORDER}")
                continue
            if n == 0:
                if seen_data and line.startswith("ngram "):
                    continue
                raise ValueError(f"ARPA text: unexpected line {raw!r}")
            fields = line.split()
            if len(fields) not in (n + 1, n + 2):
                raise ValueError(f"ARPA text: {n}-gram line {raw!r} has {len(fields)} fields")
            backoff = float(fields[n + 1]) if len(fields) == n + 2 else None
            ngrams[tuple(fields[1:n + 1])] = (float(fields[0]), backoff)
        if not seen_data:
            raise ValueError("ARPA text: no \\data\\ section")
        return cls(ngrams, alphabet, separator_index, unk_log10_p)

    # ------------------------------------------------------------------ tokenisation
    def _split(self, prefix):
        """(complete words before the scored word, the scored word) as symbol tuples; the word is None if empty."""
        sep = self.separator_index
        syms = [int(s) for s in prefix]
        if syms and syms[-1] == sep:
            syms.pop()
        words, cur = [], []
        for s in syms:
            if s == sep:
                if cur:
                    words.append(tuple(cur))
                cur = []
            else:
                cur.append(s)
        return words, (tuple(cur) if cur else None)

    # ------------------------------------------------------------------ the meaning: double precision, dictionaries
    def __call__(self, prefix) -> float:
        words, word = self._split(prefix)
        if word is None:
            return 1.0
        w = self._spelling.get(word, self.unk_id)
        ctx = [self._spelling.get(x, self.unk_id) for x in words[len(words) - min(len(words), self.order - 1):]]
        if len(ctx) < self.order - 1 and self.bos_id >= 0:
            ctx = [self.bos_id] + ctx
        prob = 1.0
        for k in range(len(ctx), -1, -1):
            tail = tuple(ctx[len(ctx) - k:])
            hit = self._prob.get(tail + (w,))
            if hit is not None:
                return prob * hit[0]
            if k > 0 and tail in self._prob:
                prob *= self._prob[tail][1]
        return prob

    # ------------------------------------------------------------------ the packed table
    def packed(self, lm_weight: float) -> np.ndarray:
        """The blob for ``lm_weight`` (numpy uint8, cached per weight)."""
        a = float(lm_weight)
        blob = self._packed.get(a)
        if blob is not None:
            return blob
        spellings = list(self._spelling.items())
        grams = list(self._prob.items())
        v_log2, n_log2 = _slots_log2(len(spellings)), _slots_log2(len(grams))
        for attempt in range(64):                       # re-seed until no two stored keys are equal
            v_seed, n_seed = _seed(0, attempt), _seed(1, attempt)
            v_keys = [self._word_key(v_seed, sp) for sp, _ in spellings]
            n_keys = [self._gram_key(n_seed, ids) for ids, _ in grams]
            if len(set(v_keys)) == len(v_keys) and len(set(n_keys)) == len(n_keys):
                break
        else:
            raise RuntimeError("no collision-free hash seed found")
        v_taken, v_probes = _place(v_keys, v_log2)
        n_taken, n_probes = _place(n_keys, n_log2)
        v_off = HEADER_BYTES
        n_off = v_off + 16 * (1 << v_log2)
        total = n_off + 16 * (1 << n_log2)
        blob = np.zeros(total, dtype=np.uint8)
        hdr = blob[:HEADER_BYTES].view(np.uint32)
        hdr[:] = [MAGIC, self.order, v_log2, n_log2, v_seed & 0xFFFFFFFF, v_seed >> 32, n_seed & 0xFFFFFFFF, n_seed >> 32,
                  self.bos_id & 0xFFFFFFFF, self.unk_id, v_probes, n_probes, v_off, n_off, total, len(self._id)]
        id_of_key = dict(zip(v_keys, (i for _, i in spellings)))
        vt64 = blob[v_off:n_off].view(np.uint64).reshape(-1, 2)
        vt32 = blob[v_off:n_off].view(np.int32).reshape(-1, 4)
        for slot, key in v_taken.items():
            vt64[slot, 0] = key
            vt32[slot, 2] = id_of_key[key]
        val_of_key = dict(zip(n_keys, (v for _, v in grams)))
        nt64 = blob[n_off:].view(np.uint64).reshape(-1, 2)
        ntf = blob[n_off:].view(np.float32).reshape(-1, 4)
        for slot, key in n_taken.items():
            p, bo = val_of_key[key]
            nt64[slot, 0] = key
            ntf[slot, 2] = _stored_factor(p, a)
            ntf[slot, 3] = _stored_factor(bo, a)
        blob.setflags(write=False)
        self._packed[a] = blob
        return blob

    @staticmethod
    def _word_key(seed: int, spelling) -> int:
        h = seed
        for s in spelling:
            h = _step(h, s)
        return _fin(h)

    @staticmethod
    def _gram_key(seed: int, ids) -> int:
        h = seed
        for i in ids:
            h = _step(h, i)
        return _fin(_step(h, len(ids)))

    # ------------------------------------------------------------------ the device's arithmetic, on the host
    def _views(self, a: float):
        rec = getattr(self, "_view_cache", None)
        if rec is None or rec[0] != a:
            blob = self.packed(a)
            hdr = [int(x) for x in blob[:HEADER_BYTES].view(np.uint32)]
            v_off, n_off = hdr[12], hdr[13]
            vt = blob[v_off:v_off + 16 * (1 << hdr[2])]
            nt = blob[n_off:n_off + 16 * (1 << hdr[3])]
            rec = (a, hdr, vt.view(np.uint64).reshape(-1, 2)[:, 0].tolist(), vt.view(np.int32).reshape(-1, 4)[:, 2].tolist(),
                   nt.view(np.uint64).reshape(-1, 2)[:, 0].tolist(), nt.view(np.float32).reshape(-1, 4)[:, 2].copy(),
                   nt.view(np.float32).reshape(-1, 4)[:, 3].copy())
            self._view_cache = rec
        return rec

    @staticmethod
    def _probe(keys, log2, probes, key):
        """Slot of ``key`` or -1: csrc/ngram_lm.h's probe loop (bounded by the recorded probe run)."""
        mask = (1 << log2) - 1
        slot = key & mask
        for i in range(probes):
            k = keys[(slot + i) & mask]
            if k == key:
                return (slot + i) & mask
            if k == 0:
                break
        return -1

    def factor(self, prefix, lm_weight: float) -> np.float32:
        """The float32 factor the device multiplies in for ``prefix``, from the packed bytes."""
        _, hdr, v_keys, v_ids, n_keys, n_pf, n_bf = self._views(float(lm_weight))
        order, v_log2, n_log2 = hdr[1], hdr[2], hdr[3]
        v_seed, n_seed = hdr[4] | (hdr[5] << 32), hdr[6] | (hdr[7] << 32)
        bos = hdr[8] - (1 << 32) if hdr[8] >= (1 << 31) else hdr[8]
        unk, v_probes, n_probes = hdr[9], hdr[10], hdr[11]

        def word_id(spelling):
            s = self._probe(v_keys, v_log2, v_probes, self._word_key(v_seed, spelling))
            return v_ids[s] if s >= 0 else unk

        words, word = self._split(prefix)
        if word is None:
            return np.float32(1.0)
        hist = [-1] * (MAX_ORDER - 2) + [bos]            # the search node's history: the last four complete words
        for x in words:
            hist = hist[1:] + [word_id(x)]
        w = word_id(word)
        ctx = []
        for k in range(1, order):
            if hist[-k] < 0:
                break
            ctx.insert(0, hist[-k])
        f = np.float32(1.0)
        for k in range(len(ctx), -1, -1):
            tail = ctx[len(ctx) - k:]
            s = self._probe(n_keys, n_log2, n_probes, self._gram_key(n_seed, tail + [w]))
            if s >= 0:
                return np.float32(f * n_pf[s])
            if k > 0:
                s = self._probe(n_keys, n_log2, n_probes, self._gram_key(n_seed, tail))
                if s >= 0:
                    f = np.float32(f * n_bf[s])
        return f

    def weighted_callable(self, lm_weight: float):
        """A reference-style callable whose value is the device's factor: use it with ``lm_weight=1.0``."""
        return lambda prefix: float(self.factor(prefix, lm_weight))

    # ------------------------------------------------------------------ upload
    def check_packed(self, blob: np.ndarray) -> None:
        """``ms_ngram_lm_table_check`` on a host blob (no GPU needed); raises ValueError if it is refused."""
        from myrtlespeech_amd import _lib
        lib = _lib.load()
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        if lib.ms_ngram_lm_table_check(ctypes.c_void_p(blob.ctypes.data), blob.size) != _lib.MS_OK:
            raise ValueError(lib.ms_last_error().decode())

    def device_table(self, lm_weight: float):
        """(device uint8 tensor of the blob, its host numpy copy) for the current device; checked, then uploaded once."""
        import torch
        a = float(lm_weight)
        key = (a, torch.cuda.current_device())
        rec = self._device.get(key)
        if rec is None:
            blob = self.packed(a)
            self.check_packed(blob)
            rec = (torch.from_numpy(blob.copy()).cuda(), blob)
            self._device[key] = rec
        return rec

    def score_on_device(self, prefixes, lm_weight: float) -> np.ndarray:
        """``ms_ngram_lm_score`` over a list of prefixes: the device's factors as float32 (testing / diagnosis)."""
        import torch
        from myrtlespeech_amd import _lib
        _lib.require_gpu()
        lib = _lib.load()
        table, blob = self.device_table(lm_weight)
        count = len(prefixes)
        if count == 0:
            return np.zeros(0, dtype=np.float32)
        longest = max(1, max(len(p) for p in prefixes))
        padded = np.zeros((count, longest), dtype=np.int32)
        lens = np.zeros(count, dtype=np.int32)
        for i, p in enumerate(prefixes):
            padded[i, :len(p)] = p
            lens[i] = len(p)
        d_pre, d_len = torch.from_numpy(padded).cuda(), torch.from_numpy(lens).cuda()
        out = torch.empty(count, dtype=torch.float32, device="cuda")
        _lib.check(lib.ms_ngram_lm_score(_lib.ptr(table), ctypes.c_void_p(blob.ctypes.data), blob.size, _lib.ptr(d_pre),
                                         _lib.ptr(d_len), _lib.ptr(out), count, longest, self.separator_index,
                                         _lib.stream_ptr()), "ms_ngram_lm_score")
        return out.cpu().numpy()

    def __repr__(self) -> str:
        return (f"NGramLanguageModel(order={self.order}, words={len(self._id)}, ngrams={len(self._prob)}, "
                f"separator_index={self.separator_index})")
