"""The CTC prefix beam search on the device where candidates have BIT-EQUAL scores (tests/beam_tie_cases.py): there the beam
is decided by the order keys the kernel gives its candidates (csrc/beam.hip: the Pb key, the +1 / +2 offsets, par_rank, the
0x40000000 rule of keys that exist in Pnb[t] only, S4's (score, key) comparison), in every instantiation -- generic,
constant shape, the last widths that fit the LDS, the workspace ("BIG") path, alphabets above 256 symbols, the range-safe and
language-model twins, the one-wave and MS_BEAM_CONST=0 switches -- and after a resume.  tests/test_beam_ties_cpu.py shows
that the clips do tie where the beam is cut and that the expected beam changes when ties are broken the other way round.

Every comparison is an equality with the numpy restatement tests/beam_range_ref.py (transcripts, the whole final beam in
order, float32 score bits, scale_log2) or with the reference's transcripts in tests/golden/beam_ties.npz.
Needs a real MI355X: -m gpu."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import beam_range_ref as R
import beam_tie_cases as C
from test_beam_range_gpu import T, abi_ex, assert_equals_restatement, assert_nbest_equals_restatement
from util import Golden, unragged

pytestmark = pytest.mark.gpu

RESUME_SHAPES = ("29x4", "29x16", "29x32", "29x100", "257x4", "300x16")
CONST_SHAPES = ("29x4", "29x8", "29x16", "29x32")
ONE_WAVE = [f"{kind}_{shape}" for shape in ("9x5",) + CONST_SHAPES for kind in C.KINDS]      # LDS need <= 64 KB


@functools.lru_cache(maxsize=None)
def want(name):
    """(the restatement of every utterance, the TieStats of utterance 0) -- computed once, never modified."""
    c = C.case(name)
    stats = C.TieStats(c.width)
    kw = dict(prune_threshold=c.prune, separator_index=c.sep, word_weight=c.word_weight, range_safe=c.range_safe)
    out = [R.search(c.x[:, n], c.lens[n], c.blank, c.width, hook=stats if n == 0 else None, **kw) for n in range(3)]
    return out, stats


def device(c, x=None, lens=None, pieces=None):
    return abi_ex(c.x.copy() if x is None else x, c.lens if lens is None else lens, c.blank, c.width, c.prune, c.sep, c.word_weight,
                  c.range_safe, pieces=pieces)


def assert_same_device_result(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3]
    for s, r in zip(a[2], b[2]):
        np.testing.assert_array_equal(s.view(np.uint32), r.view(np.uint32))


# ----------------------------------------------------------------------------- every route
@pytest.mark.parametrize("name", C.CASES)
def test_case_equals_restatement(name):
    c = C.case(name)
    ref, stats = want(name)
    assert 4 * len(stats.cut) >= c.lens[0] and len(ref[0].beam) == c.width      # (the premises: test_beam_ties_cpu.py)
    assert_equals_restatement(device(c), ref)


ENTRIES = Golden("beam_ties").cfg["entries"]


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: f"{e['case']}-{e['tag']}")
def test_decoder_returns_the_reference_transcripts(entry):
    from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
    g = Golden("beam_ties")
    c = C.case(entry["case"])
    np.testing.assert_array_equal(c.x[::5, :, ::7], g[f"{c.name}/x_probe"])
    assert float(np.abs(c.x.astype(np.float64)).sum()) == float(g[f"{c.name}/x_abs_sum"])
    kw = dict(separator_index=c.sep, word_weight=c.word_weight) if entry["tag"] == "words" else {}
    got = CTCBeamDecoder(c.blank, c.width, c.prune, **kw)(T(c.x.copy()), T(np.asarray(c.lens)))
    assert got == unragged(g[f"{c.name}/{entry['tag']}_flat"], g[f"{c.name}/{entry['tag']}_lens"])


# ----------------------------------------------------------------------------- persisted state
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("shape", RESUME_SHAPES)
def test_resume_behind_a_tie_frame(shape, kind):
    """Two calls, cut behind (and in front of) a frame whose scores tie where the beam is cut, and behind frame 0: the beam
    ORDER has to survive the workspace, not only its members."""
    c = C.case(f"{kind}_{shape}")
    ref, stats = want(c.name)
    Tn = c.x.shape[0]
    ties = [t for t in stats.cut if 1 < t < Tn - 1]
    t = ties[len(ties) // 2]
    whole = device(c)
    assert_equals_restatement(whole, ref)
    for cut in (t + 1, t, 1):
        assert_same_device_result(device(c, pieces=[(0, cut), (cut, Tn)]), whole)


@pytest.mark.parametrize("rows", [1, 7])
def test_streaming_decoder_pushed_in_chunks(rows):
    from myrtlespeech_amd.post_process.ctc_beam_decoder import CTCBeamDecoder
    from myrtlespeech_amd.post_process.streaming import StreamingCTCBeamDecoder
    c = C.case("twins_29x8")
    ref, _ = want(c.name)
    assert c.sep is not None
    dec = StreamingCTCBeamDecoder(c.blank, c.width, c.prune, separator_index=c.sep, word_weight=c.word_weight)
    dec.begin(T(np.asarray(c.lens)), c.x.shape[0])
    xd = T(c.x.copy()).cuda()
    for t in range(0, c.x.shape[0], rows):
        dec.push(xd[t:t + rows])
    whole = CTCBeamDecoder(c.blank, c.width, c.prune, separator_index=c.sep, word_weight=c.word_weight)
    assert dec.nbest() == whole.decode_nbest(T(c.x.copy()), T(np.asarray(c.lens)))
    assert_nbest_equals_restatement(dec.nbest(), ref)
    assert dec.result() == R.transcripts(ref)


# ----------------------------------------------------------------------------- the device language model
@pytest.mark.parametrize("kind", sorted(C.LM_KINDS))
@pytest.mark.parametrize("width", C.LM_WIDTHS)
def test_device_language_model_on_ties(width, kind):
    """Constant shape (8), generic (5) and the workspace path (96) of the LM instantiations.  The model separates twins only
    at separators, so the ties survive inside words (asserted here on the host side and in test_beam_ties_cpu.py)."""
    from ngram_lm_cases import BLANK, SEP, decoder_model
    x, lens, prune = C.lm_clip(kind)
    lm = decoder_model(3)
    stats = C.TieStats(width)
    kw = dict(prune_threshold=prune, language_model=lm.weighted_callable(C.LM_WEIGHT), lm_weight=1.0, separator_index=SEP,
              word_weight=C.LM_WORD_WEIGHT)
    ref = [R.search(x[:, n], lens[n], BLANK, width, hook=stats if n == 0 else None, **kw) for n in range(3)]
    assert 4 * len(stats.cut) >= lens[0]
    args = (x.copy(), lens, BLANK, width, prune, SEP, C.LM_WORD_WEIGHT, False)
    got = abi_ex(*args, lm=lm, lm_weight=C.LM_WEIGHT)
    assert_equals_restatement(got, ref)
    cut = stats.cut[len(stats.cut) // 2] + 1          # resumed behind a frame whose scores tie where the beam is cut
    assert_same_device_result(abi_ex(*args, pieces=[(0, cut), (cut, x.shape[0])], lm=lm, lm_weight=C.LM_WEIGHT), got)


# ----------------------------------------------------------------------------- the two A/B switches
@pytest.mark.parametrize("name", [f"{kind}_{shape}" for shape in CONST_SHAPES for kind in C.KINDS]
                         + ["rs_twins_29x8", "rs_twins0_29x8"])
def test_generic_kernel_at_29_symbols(name, monkeypatch):
    """MS_BEAM_CONST=0 (read on every call): the generic instantiation at the constant-shape kernels' sizes."""
    c = C.case(name)
    ref, _ = want(name)
    monkeypatch.delenv("MS_BEAM_CONST", raising=False)
    const = device(c)
    monkeypatch.setenv("MS_BEAM_CONST", "0")
    generic = device(c)
    assert_equals_restatement(generic, ref)
    assert_same_device_result(generic, const)


def run_one_wave_child():
    """In the child (MS_BEAM_THREADS=64): every case whose LDS need is at most 64 KB, as JSON on the last line."""
    assert os.environ.get("MS_BEAM_THREADS") == "64"
    out = {}
    for name in ONE_WAVE:
        outs, beams, scores, scales = device(C.case(name))
        out[name] = dict(outs=outs, beams=[[list(p) for p in b] for b in beams],
                         scores=[s.view(np.uint32).tolist() for s in scores], scales=scales)
    print("ONE_WAVE " + json.dumps(out))


def test_one_wave_instantiation_in_subprocess():
    """MS_BEAM_THREADS=64 is read once per process: one fresh child, once, under its own time limit; S4 runs with NW = 1."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_beam_ties_gpu as G; G.run_one_wave_child()\n") % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MS_BEAM_THREADS="64"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("ONE_WAVE ")]
    assert len(lines) == 1, r.stdout[-3000:]
    got = json.loads(lines[0][len("ONE_WAVE "):])
    assert sorted(got) == sorted(ONE_WAVE)
    for name in ONE_WAVE:
        ref, _ = want(name)
        g = got[name]
        assert g["outs"] == R.transcripts(ref), name
        assert [[tuple(p) for p in b] for b in g["beams"]] == [r_.beam for r_ in ref], name
        assert g["scores"] == [r_.scores.astype(np.float32).view(np.uint32).tolist() for r_ in ref], name
        assert g["scales"] == [0, 0, 0], name


# ----------------------------------------------------------------------------- non-finite probabilities, lengths out of range
def poisoned(c, value, frame=9, whole_row=False):
    """Utterance 0 with `value` in frame 9: in the whole row, or in the most probable non-blank symbol (the first of its
    twins), so that the candidates it spoils are ones the clean search keeps."""
    x = c.x.copy()
    if whole_row:
        x[frame, 0, :] = value
    else:
        row = x[frame, 0].copy()
        row[c.blank] = -1.0
        x[frame, 0, int(np.argmax(row))] = value
    return x


def restated(c, x, lens=None):
    with np.errstate(all="ignore"):
        return R.decode(x, c.lens if lens is None else lens, c.blank, c.width, prune_threshold=c.prune, separator_index=c.sep,
                        word_weight=c.word_weight, range_safe=c.range_safe)


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("name", ["twins_29x8", "twins_9x5"])
def test_one_non_finite_probability(name, value):
    """At the ABI (the search itself is under test, not a wrapper's argument check).  The reference's arithmetic stays well
    defined: a NaN sum is not > 0 and is dropped from A_next, an infinity follows IEEE.  Utterance 0 is the restatement on
    the same input, the other utterances are their clean run bit for bit."""
    c = C.case(name)
    x = poisoned(c, value)
    ref = restated(c, x)
    assert ref[0].beam != want(name)[0][0].beam or not np.array_equal(ref[0].scores, want(name)[0][0].scores, equal_nan=True)
    got, clean = device(c, x=x), device(c)
    assert_equals_restatement(got, ref)
    for k in (0, 1):
        assert got[k][1:] == clean[k][1:]
    for n in (1, 2):
        np.testing.assert_array_equal(got[2][n].view(np.uint32), clean[2][n].view(np.uint32))


@pytest.mark.parametrize("name", ["twins_29x8", "twins_9x5"])
def test_a_frame_of_nans_empties_the_beam(name):
    c = C.case(name)
    x = poisoned(c, float("nan"), whole_row=True)
    ref = restated(c, x)
    assert ref[0].beam == []
    got, clean = device(c, x=x), device(c)
    assert_equals_restatement(got, ref)
    assert got[0][0] == [] and got[1][0] == []
    assert got[0][1:] == clean[0][1:] and got[1][1:] == clean[1][1:]


@pytest.mark.parametrize("name", ["twins_9x5", "twins0_29x8", "twins_257x4", "dyadic_300x16", "rs_twins_9x5"])
def test_lengths_are_clamped_at_the_abi(name):
    """lens = T + 5 behaves as T and lens = -3 as 0: min(max(lens, 0), T) in the kernel."""
    c = C.case(name)
    Tn = c.x.shape[0]
    clamped = (Tn, c.lens[1], 0)
    ref = restated(c, c.x, lens=clamped)
    got = device(c, lens=(Tn + 5, c.lens[1], -3))
    assert_equals_restatement(got, ref)
    assert_same_device_result(got, device(c, lens=clamped))
    assert got[1][2] == [()] and got[0][2] == []              # no frame: the empty prefix alone
