"""Inputs shared by tests/test_ngram_lm_cpu.py and tests/test_beam_lm_gpu.py: the alphabet, a hand-written trigram ARPA
text, the prefix set of the packed-table checks, the small models of the decoder tests and the sentence-shaped posteriors
on which a language model changes the transcript."""
import itertools

import numpy as np

# 29 symbols: separator 0, a-z 1-26, ' 27, blank 28 (the reference's English alphabet with the blank last)
ALPHABET = [" "] + [chr(ord("a") + i) for i in range(26)] + ["'", "_"]
SEP, BLANK = 0, 28
SYM = {ch: i for i, ch in enumerate(ALPHABET)}

ARPA_TRIGRAM = """\\data\\
ngram 1=12
ngram 2=10
ngram 3=6

\\1-grams:
-99\t<s>\t-0.30
-1.20\t<unk>
-0.70\tthe\t-0.40
-1.10\tcat\t-0.35
-1.60\tcap\t-0.20
-1.15\tsat\t-0.30
-1.70\tsap\t-0.25
-1.00\ton\t-0.45
-1.25\tmat\t-0.15
-1.80\tmap\t-0.10
-1.40\ta\t-0.50
-2.00\t</s>

\\2-grams:
-0.25\t<s> the\t-0.20
-0.90\t<s> a\t-0.10
-0.30\tthe cat\t-0.25
-1.30\tthe cap
-0.35\tthe mat\t-0.05
-0.40\tcat sat\t-0.30
-0.45\tsat on\t-0.20
-0.30\ton the\t-0.15
-1.00\ton a
-0.60\tmat </s>

\\3-grams:
-0.10\t<s> the cat
-0.15\tthe cat sat
-0.12\tcat sat on
-0.08\tsat on the
-0.20\ton the mat
-0.50\tthe mat </s>

\\end\\
"""
ARPA_WORDS = ["the", "cat", "cap", "sat", "sap", "on", "mat", "map", "a"]


def spell(text):
    """'the cat' -> symbols (spaces are separators)."""
    return tuple(SYM[ch] for ch in text)


def ask(text):
    """The decoder's question about the prefix `text`: its symbols + (separator,)."""
    return spell(text) + (SEP,)


def prefix_set():
    """Every sentence of 1 .. 4 words over the ARPA text's vocabulary, sentences with out-of-vocabulary spellings mixed
    in, runs of separators and empty words: 8 000+ prefixes, each as the decoder would ask (+ separator)."""
    out = [(), (SEP,), ask("the "), ask(" the"), ask("the  cat"), ask("  the   cat  sat")]
    for n in range(1, 5):
        for words in itertools.product(ARPA_WORDS, repeat=n):
            out.append(ask(" ".join(words)))
    rng = np.random.default_rng(20240)
    letters = ALPHABET[1:28]
    for _ in range(600):
        words = []
        for _ in range(int(rng.integers(1, 6))):
            if rng.random() < 0.5:
                words.append(ARPA_WORDS[int(rng.integers(len(ARPA_WORDS)))])
            else:
                words.append("".join(letters[int(k)] for k in rng.integers(0, 27, size=int(rng.integers(1, 7)))))
        gaps = [" " * int(rng.integers(1, 3)) for _ in words]
        out.append(ask("".join(g + w for g, w in zip(gaps, words)).lstrip(" ") if rng.random() < 0.8
                       else "".join(g + w for g, w in zip(gaps, words))))
    return out


# ---- the decoder tests' models: {the, cat, cap, sat, sap, on, mat, map} + <s>, <unk>, preferring "the cat sat on the mat"
_UNI = {"<s>": (-99.0, -0.25), "<unk>": (-2.4, None), "the": (-0.7, -0.35), "cat": (-1.0, -0.3), "cap": (-2.2, -0.2),
        "sat": (-1.0, -0.3), "sap": (-2.3, -0.2), "on": (-0.9, -0.4), "mat": (-1.1, -0.2), "map": (-2.2, -0.15)}
_BI = {("<s>", "the"): (-0.15, -0.2), ("the", "cat"): (-0.3, -0.25), ("the", "mat"): (-0.35, -0.1),
       ("the", "cap"): (-1.9, None), ("the", "map"): (-1.9, None), ("cat", "sat"): (-0.2, -0.3),
       ("cat", "sap"): (-1.8, None), ("sat", "on"): (-0.15, -0.2), ("on", "the"): (-0.1, -0.15)}
_TRI = {("<s>", "the", "cat"): (-0.2, None), ("the", "cat", "sat"): (-0.1, None), ("cat", "sat", "on"): (-0.1, None),
        ("sat", "on", "the"): (-0.05, None), ("on", "the", "mat"): (-0.15, None), ("on", "the", "map"): (-2.0, None)}


def decoder_model(order, unk_log10_p=None):
    """unk_log10_p: another probability for <unk> (-0.05: a model under which 501 frames of random posteriors, which spell
    some fifty out-of-vocabulary words, do not underflow the reference's linear float32 search to an empty beam)."""
    from myrtlespeech_amd.language_model import NGramLanguageModel
    grams = {(w,): v for w, v in _UNI.items()}
    if unk_log10_p is not None:
        grams[("<unk>",)] = (unk_log10_p, None)
    grams.update(_BI)
    if order == 3:
        grams.update(_TRI)
    return NGramLanguageModel(grams, ALPHABET, SEP)


SENTENCES = ["the cat sat on the mat", "the mat sat on the cat", "the dog sat on the map", "on the mat the cat sat"]


def sentence_posteriors(sentences=SENTENCES, seed=7, tile_to=None):
    """[T, N, 29] float32 rows and lengths: per character 1-2 frames with 0.85 on it -- but every `t` / `p` frame carries
    0.40 on the right letter and 0.46 on the other one, so the acoustics alone prefer cap / map / sap --, a 0.8 blank frame
    after each character (30 % of them with 0.05 on the separator), the remaining mass random in [0.002, 0.006], rows
    normalised.  tile_to: repeat every utterance's rows up to that many frames."""
    rng = np.random.default_rng(seed)
    utts = []
    for text in sentences:
        rows = []
        for ch in text:
            c = SYM[ch]
            for _ in range(int(rng.integers(1, 3))):
                r = rng.uniform(0.002, 0.006, size=29)
                if ch in "tp":
                    r[c], r[SYM["p" if ch == "t" else "t"]] = 0.40, 0.46
                else:
                    r[c] = 0.85
                rows.append(r)
            r = rng.uniform(0.002, 0.006, size=29)
            r[BLANK] = 0.8
            if rng.random() < 0.3:
                r[SEP] = 0.05
            rows.append(r)
        a = np.asarray(rows)
        utts.append(a / a.sum(axis=1, keepdims=True))
    if tile_to is not None:
        utts = [np.concatenate([u] * (tile_to // len(u) + 1))[:tile_to] for u in utts]
    lens = np.asarray([len(u) for u in utts], dtype=np.int64)
    x = np.full((int(lens.max()), len(utts), 29), 1.0 / 29)
    for n, u in enumerate(utts):
        x[:len(u), n] = u
    return x.astype(np.float32), lens
