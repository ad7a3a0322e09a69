"""A wave of the scan kernels whose own words and two edge words hold no void bit skips the void terms of its hit masks (one
wave-uniform branch in own_words_and_masks).  Arenas of three tiles with ONE void word, word of N or word of lower-case bases
in the middle tile, at the places where a wave meets it as its left edge word, its right edge word, one lane's first or one
lane's last word, inside a tile and at the seam of two (tests/void_free_cases.py): rows compared bit for bit with the
oracle in both geometries, both scan modes and two guide lengths.  The generator is checked against the oracle, and the
waves that may and do take the short path are counted from the arena layout, without a GPU."""
import numpy as np
import pytest

import void_free_cases as cases

_BUILT, _ORACLE = {}, {}


def built(geometry, place, kind, l):
    key = (geometry, place, kind, l)
    if key not in _BUILT:
        _BUILT[key] = cases.build(*key)
    return _BUILT[key]


def oracle_rows(oracle, geometry, place, kind, l):
    """the oracle's rows of every contig of a case, computed once and shared (read-only)"""
    key = (geometry, place, kind, l)
    if key not in _ORACLE:
        _ORACLE[key] = [oracle.scan_score(c, l) for c in built(*key)[0]]
    return _ORACLE[key]


def kinds_of(place):
    return cases.KINDS if place != "none" else ("void",)  # (nothing marked: one contig, whatever the kind)


PLACES = sorted(cases.places("large"))


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("geometry", sorted(cases.GEOMETRY))
def test_generator_against_oracle(oracle, geometry, place):
    """Every planted site is in the oracle's rows when the generator says the reference keeps it and absent when not; a
    case that marks a word has sites on both strands next to it, kept and -- where the word is void -- dropped."""
    tile, wave = cases.GEOMETRY[geometry]
    for kind in kinds_of(place):
        for l in cases.GUIDE_LENGTHS:
            contigs, offsets, planted, dropped, W = built(geometry, place, kind, l)
            ctx = (geometry, place, kind, l)
            assert 1 + sum((len(c) + 63) // 64 + 1 for c in contigs) == cases.used_words(geometry), ctx
            assert 2 * tile < cases.used_words(geometry) <= 3 * tile, ctx
            rows = oracle_rows(oracle, *ctx)
            for k, strand, s in planted:
                assert s in rows[k]["pos_" + strand], (ctx, "missing", k, strand, s)
            for k, strand, s in dropped:
                assert s not in rows[k]["pos_" + strand], (ctx, "kept", k, strand, s)
            if W is None:
                assert len(contigs) == 1 and not dropped and len(planted) >= 16, ctx
                continue
            assert W in (tile + r for r in (wave - 1, wave, wave + 1, tile - 1, tile, tile + 1)), ctx
            # sites within a word of the marked one, per strand
            near = lambda sites, strand: [s for k, st, s in sites if st == strand and abs(offsets[k] + s - 64 * W - 32) <= 96]
            if kind.startswith("void"):
                assert len(contigs) == 2 and offsets[1] == 64 * (W + 1) and len(contigs[0]) == 64 * (W - 1), ctx
                assert near(planted, "plus") and near(dropped, "plus"), ctx       # the l + 5 look-behind, either side
                assert len(near(dropped, "minus")) >= 2 and len(near(planted, "minus")) >= 2, ctx  # 2 behind, l - 8 ahead
            else:
                assert len(contigs) == 1 and not near(dropped, "plus") and not near(dropped, "minus"), ctx
                assert len(near(planted, "plus")) >= 2 and len(near(planted, "minus")) >= 6, ctx
                word = np.frombuffer(contigs[0], dtype=np.uint8)[64 * W - 64:64 * W]
                assert (word == ord("N")).all() if kind == "N" else (np.char.islower(word.view("S1"))).all(), ctx


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("geometry", sorted(cases.GEOMETRY))
def test_both_paths_are_taken_in_every_arena(geometry, place):
    """From the layout: which waves hold no void bit in their own and edge words (may skip the void terms), and which of
    those the kernels' test -- every character a base or an upper-case letter -- lets skip.  Both kinds of wave are in every
    arena, and a void word sends exactly the waves that reach it down the full path."""
    tile, wave = cases.GEOMETRY[geometry]
    for kind in kinds_of(place):
        contigs, offsets, _, _, W = built(geometry, place, kind, 20)
        w = cases.waves(geometry, contigs, offsets)
        may, do = [a for a, _ in w], [b for _, b in w]
        ctx = (geometry, place, kind)
        assert all(a or not b for a, b in w), ctx              # the kernels' test never lets a wave with void in reach skip
        assert 0 < sum(do) <= sum(may) < len(w), (ctx, sum(do), sum(may), len(w))
        in_reach = lambda word: {v for v in range(len(w)) if v * wave - 1 <= word <= v * wave + wave}
        end = cases.used_words(geometry) - 1                   # the last separator; padding behind it
        full = in_reach(0) | in_reach(end) | set(range(end // wave, len(w)))
        if kind == "void" and W is not None:
            assert in_reach(W) and not in_reach(W) & full, ctx
            full |= in_reach(W)
        if kind in ("void", "lower") or W is None:             # (bare contigs: nothing but void keeps a wave off the short path)
            assert {v for v in range(len(w)) if not may[v]} == full == {v for v in range(len(w)) if not do[v]}, ctx
        elif kind == "N":
            assert {v for v in range(len(w)) if not may[v]} == full, ctx
            assert {v for v in range(len(w)) if not do[v]} == full | in_reach(W), ctx
        # the middle tile, where the marked word is the only thing that is not plain sequence
        middle = range(tile // wave, 2 * tile // wave)
        if W is None or kind == "lower":
            assert all(do[v] for v in middle), ctx
        else:
            assert any(do[v] for v in middle), ctx


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def _engine():
    from cropsr_amd import Engine
    eng = Engine(0)  # raises if libcropsr_hip.so or the GPU is missing: no fallback
    yield eng
    assert eng.query()["chain_timeouts"] == 0
    eng.close()


@pytest.fixture(params=["single_pass-large", "single_pass-small", "two_pass-large", "two_pass-small"])
def engine(_engine, request):
    mode, geometry = request.param.split("-")
    _engine.configure(two_pass=mode == "two_pass", geometry=geometry)
    yield _engine
    _engine.configure(two_pass=False, geometry="auto")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("place", PLACES)
def test_rows_vs_oracle(engine, oracle, place, request):
    """Every row of every contig, positions and scores (l = 20: the variant without the pre-sigmoid column, the one the
    benchmark times; l = 23: the generic-length variant, with it), and the planted sites among them."""
    geometry = request.node.callspec.params["engine"].split("-")[1]
    for kind in kinds_of(place):
        for l in cases.GUIDE_LENGTHS:
            contigs, offsets, planted, dropped, _ = built(geometry, place, kind, l)
            want = oracle_rows(oracle, geometry, place, kind, l)
            ctx = (geometry, place, kind, l)
            arena = engine.arena(contigs)
            try:
                assert arena.stats()["n_words"] == cases.used_words(geometry), ctx
                assert [int(o) for o in arena.offsets] == offsets, ctx
                tiles = arena.tiles()
                assert tiles["geometry"] == geometry and tiles["n_tiles"] == 3, ctx
                want_pre = l != 20
                hits = arena.scan_score(l, want_pre=want_pre)
                total = 0
                for k, w in enumerate(want):
                    got = hits.contig(k)
                    for key, col in w.items():
                        if key.startswith("pre_") and not want_pre:
                            continue
                        assert got[key].shape == col.shape, (ctx, k, key, got[key].shape, col.shape)
                        assert (bits(got[key]) == bits(col)).all(), (ctx, k, key)
                    for kk, strand, s in planted:
                        assert kk != k or s in got["pos_" + strand], (ctx, "missing", k, strand, s)
                    for kk, strand, s in dropped:
                        assert kk != k or s not in got["pos_" + strand], (ctx, "kept", k, strand, s)
                    total += w["pos_plus"].size + w["pos_minus"].size
                assert hits.n_plus + hits.n_minus == total, ctx
            finally:
                arena.close()
