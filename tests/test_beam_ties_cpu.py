"""The premises of tests/test_beam_ties_gpu.py, checked without a GPU: the clips of tests/beam_tie_cases.py DO make
bit-equal scores where the beam is cut, keys that exist in Pnb[t] only and rescales, the expected beam DOES depend on the
insertion order (so an equality with the device is a test of the kernel's order keys), and the restatement that states the
expected beam (tests/beam_range_ref.py) is the oracle, which tests/test_oracle_golden.py::test_beam_ties holds to the reference.

Each condition is a condition on the INPUTS (seeds chosen so that the restatement alone satisfies it), not a measurement of
the code under test.  The counts are printed (-s shows them)."""
import functools

import numpy as np
import pytest

import beam_range_ref as R
import beam_tie_cases as C
from oracle import ds_oracle as O

BEAM_LDS_LIMIT = 150 * 1024


def beam_lds_bytes(V, W):
    """csrc/beam.hip's beam_lds_bytes restated: what decides between the LDS and the workspace ("BIG") kernels."""
    M, WV = W * (V + 1), W * V
    return (V + 10 * M + 6 * WV + 17 * W + 2 * ((W + 7) // 8 * 8) + 8) * 4


def kw_of(c, range_safe=None):
    return dict(prune_threshold=c.prune, separator_index=c.sep, word_weight=c.word_weight,
                range_safe=c.range_safe if range_safe is None else range_safe)


@functools.lru_cache(maxsize=None)
def observed(name):
    """(search of the full-length utterance, its TieStats, the same search with ties broken in reversed insertion order,
    and -- zero-blank cases -- with the keys of Pnb[t] alone in front of Pb[t]'s among equal scores)."""
    c = C.case(name)
    stats = C.TieStats(c.width)
    r = R.search(c.x[:, 0], c.lens[0], c.blank, c.width, hook=stats, **kw_of(c))
    rev = R.search(c.x[:, 0], c.lens[0], c.blank, c.width, hook=C.TieStats(c.width, reverse=True), **kw_of(c))
    pnb_first = None
    if c.kind == "twins0":
        pnb_first = R.search(c.x[:, 0], c.lens[0], c.blank, c.width, hook=C.TieStats(c.width, pnb_first=True), **kw_of(c))
    return r, stats, rev, pnb_first


# ----------------------------------------------------------------------------- the generators
@pytest.mark.parametrize("V,blank", [(9, 8), (29, 0), (40, 20), (257, 256)])
def test_twins_columns_are_bit_identical_in_pairs(V, blank):
    x = C.twins(24, V, blank, seed=5, zero_blank_every=3)
    assert x.dtype == np.float32 and x.shape == (24, V)
    np.testing.assert_array_equal(x, C.twins(24, V, blank, seed=5, zero_blank_every=3))      # seeded
    assert not np.array_equal(x, C.twins(24, V, blank, seed=6, zero_blank_every=3))
    bits = x.view(np.uint32)
    groups = {}
    for v in range(V):
        if v != blank:
            groups.setdefault(bits[:, v].tobytes(), []).append(v)
    sizes = sorted(len(g) for g in groups.values())
    assert sizes == [2] * (len(sizes) - 1) + [3 if (V - 1) % 2 else 2]       # pairs; the odd symbol out shares one
    assert any(abs(g[0] - g[1]) > 1 for g in groups.values())                # ... at permuted positions
    assert bits[:, blank].tobytes() not in groups
    zeroed = np.arange(24) % 3 == 2
    assert (x[zeroed, blank] == 0).all() and (x[~zeroed, blank] > 0).all() and (np.delete(x, blank, axis=1) > 0).all()
    full = C.twins(24, V, blank, seed=5)
    np.testing.assert_allclose(full.astype(np.float64).sum(axis=1), 1.0, atol=1e-5)


def test_dyadic_rows_are_sixteenths():
    x = C.dyadic(16, 29, 14, seed=3, zero_blank_every=4)
    assert x.dtype == np.float32
    np.testing.assert_array_equal(x, C.dyadic(16, 29, 14, seed=3, zero_blank_every=4))
    k = x * 16
    assert set(np.unique(k)) == {0.0, 1.0, 2.0, 3.0, 4.0}
    assert (x[3::4, 14] == 0).all()


# ----------------------------------------------------------------------------- the case table
def test_case_table_reaches_every_route():
    cases = [C.case(n) for n in C.CASES]
    by_route = {}
    for c in cases:
        by_route.setdefault(c.route, []).append(c)
        T, N, V = c.x.shape
        assert N == 3 and c.lens[0] == T and 1 < c.lens[1] < T and c.lens[2] in (0, 1)
        assert T == (200 if c.range_safe else 16 if c.kind == "dyadic" else 24)
        assert c.sep is None or (c.sep != c.blank and c.word_weight == 1.7)
        lds = beam_lds_bytes(V, c.width)
        if c.route in ("big", "wide_big", "rs_big"):
            assert lds > BEAM_LDS_LIMIT
        else:
            assert lds <= BEAM_LDS_LIMIT
        if c.route in ("const", "rs_const"):
            assert V == 29 and c.width in (4, 8, 16, 32)
        if c.route in ("generic", "rs_generic"):
            assert V != 29
        if c.route in ("wide_lds", "wide_big"):
            assert V > 256
        if c.route == "wide_lds":
            assert lds > 64 * 1024                    # above the default dynamic-LDS size: the raised attribute
    assert beam_lds_bytes(29, 77) <= BEAM_LDS_LIMIT < beam_lds_bytes(29, 78)
    assert {(c.x.shape[2], c.width) for c in by_route["last_lds"]} == {(29, 76), (29, 77)}
    assert {(c.x.shape[2], c.width) for c in cases if not c.range_safe} == {
        (9, 5), (40, 16), (29, 4), (29, 8), (29, 16), (29, 32), (29, 76), (29, 77), (29, 100), (8, 256), (257, 4), (300, 16)}
    assert {(c.x.shape[2], c.width) for c in cases if c.range_safe} == {(29, 8), (9, 5), (29, 100)}
    for route, members in by_route.items():
        kinds = {c.kind for c in members}
        assert {"twins", "twins0"} <= kinds and (route.startswith("rs_") or "dyadic" in kinds), route
        assert any(c.sep is not None for c in members), route
    assert any(c.sep is not None and c.kind != "dyadic" for c in cases)          # a separator that is a twin
    for c in cases:
        if c.kind == "twins0":
            assert c.prune == 0.0 and (c.x[2::3, :, c.blank] == 0).all()
    V_of = lambda c: c.x.shape[2]
    assert any(c.blank == V_of(c) - 1 for c in cases) and any(c.blank == 0 for c in cases)
    assert any(0 < c.blank < V_of(c) - 1 for c in cases)


# ----------------------------------------------------------------------------- the premises, per case
@pytest.mark.parametrize("name", C.CASES)
def test_scores_tie_where_the_beam_is_cut(name):
    """At least a quarter of the full-length utterance's frames have score[rank W-1] == score[rank W]; every zero-blank case
    has a Pnb-only key in at least 3 frames; every range-safe case rescales at least 5 times.  V = 8, W = 256: the beam takes
    a few frames to fill (1, 8, 57, ... candidates), so there an in-beam tie is required in EVERY frame as well."""
    c = C.case(name)
    r, stats, _, _ = observed(name)
    T = c.lens[0]
    print(f"{name}: route {c.route}, cut-tie frames {len(stats.cut)}/{T}, in-beam-tie frames {len(stats.in_beam)}/{T}, "
          f"Pnb-only frames {len(stats.pnb_only)}, rescales {len(r.rescaled_at)}, final beam {len(r.beam)}")
    assert len(r.beam) == c.width                 # the search is alive and the beam full at the end
    assert 4 * len(stats.cut) >= T
    if (c.x.shape[2], c.width) == (8, 256):
        assert len(stats.in_beam) == T
    if c.kind == "twins0":
        assert len(stats.pnb_only) >= 3
    if c.range_safe:
        assert len(r.rescaled_at) >= 5 and all(t in stats.cut or t in stats.in_beam for t in r.rescaled_at)
    else:
        assert r.rescaled_at == [] and r.scale_log2 == 0


@pytest.mark.parametrize("name", C.CASES)
def test_reversed_tie_break_changes_the_final_beam(name):
    r, _, rev, pnb_first = observed(name)
    assert rev.beam != r.beam
    if C.case(name).kind == "twins0":      # the place of Pnb[t]'s own keys in Counter.__add__ decides as well
        assert pnb_first.beam != r.beam


@pytest.mark.parametrize("name", C.CASES)
def test_restatement_is_the_oracle(name):
    c = C.case(name)
    got = R.decode(c.x, c.lens, c.blank, c.width, **kw_of(c, range_safe=False))
    want = O.ctc_beam_decode(c.x, np.asarray(c.lens), c.blank, c.width, c.prune, separator_index=c.sep,
                             word_weight=c.word_weight)
    assert R.transcripts(got) == want
    if not c.range_safe:
        assert got[0].beam == observed(name)[0].beam      # (the hook changes nothing)


# ----------------------------------------------------------------------------- the device language model's clip
@pytest.mark.parametrize("kind", sorted(C.LM_KINDS))
@pytest.mark.parametrize("width", C.LM_WIDTHS)
def test_ties_survive_the_language_model(width, kind):
    """The model separates twins only at separators: inside words the ties stay."""
    from ngram_lm_cases import BLANK, SEP, decoder_model
    assert (BLANK, SEP) == (C.LM_BLANK, C.LM_SEP)
    x, lens, prune = C.lm_clip(kind)
    kw = dict(prune_threshold=prune, language_model=decoder_model(3).weighted_callable(C.LM_WEIGHT), lm_weight=1.0,
              separator_index=SEP, word_weight=C.LM_WORD_WEIGHT)
    stats = C.TieStats(width)
    r = R.search(x[:, 0], lens[0], BLANK, width, hook=stats, **kw)
    rev = R.search(x[:, 0], lens[0], BLANK, width, hook=C.TieStats(width, reverse=True), **kw)
    print(f"lm clip {kind}, width {width}: Pnb-only frames {len(stats.pnb_only)}, cut-tie frames {len(stats.cut)}/{lens[0]}, in-beam-tie frames {len(stats.in_beam)}")
    assert 4 * len(stats.cut) >= lens[0] and len(r.beam) == width
    assert rev.beam != r.beam
    if kind == "twins0":
        pnb_first = R.search(x[:, 0], lens[0], BLANK, width, hook=C.TieStats(width, pnb_first=True), **kw)
        assert len(stats.pnb_only) >= 3 and pnb_first.beam != r.beam
    assert any(SEP in k for k in r.beam)          # the model has been consulted on prefixes that are still in the beam
