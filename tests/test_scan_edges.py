"""The words just outside a wave and a tile (scalar edge loads, SALU-derived edge masks, halo words in LDS): arenas whose
PAM sites, void tests and contig ends sit on word, wave and tile boundaries (tests/scan_edge_cases.py), compared exactly
with the oracle in both geometries, both scan modes and two guide lengths.  The generator itself is checked against the
oracle without a GPU."""
import numpy as np
import pytest

import scan_edge_cases as cases

_ORACLE = {}


def oracle_rows(oracle, name, l):
    """the oracle's rows of every contig of a case, computed once and shared (read-only)"""
    key = (name, l)
    if key not in _ORACLE:
        contigs = cases.build(name, l)[0]
        _ORACLE[key] = [oracle.scan_score(c, l) for c in contigs]
    return _ORACLE[key]


def assert_planted(rows, planted, dropped, ctx):
    assert len(planted) >= 8, ctx
    for k, strand, s in planted:
        assert s in rows[k]["pos_" + strand], (ctx, "missing", k, strand, s)
    for k, strand, s in dropped:
        assert s not in rows[k]["pos_" + strand], (ctx, "kept", k, strand, s)


@pytest.mark.parametrize("l", cases.GUIDE_LENGTHS)
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_generator_against_oracle(oracle, name, l):
    """Every site the generator plants is in the oracle's rows when the generator says the reference keeps it, and absent
    when it says not; and the case does put sites astride the boundaries it is named for."""
    contigs, offsets, planted, dropped, used = cases.build(name, l)
    assert used == 1 + sum((len(c) + 63) // 64 + 1 for c in contigs)
    assert all(o % 64 == 0 for o in offsets)
    assert_planted(oracle_rows(oracle, name, l), planted, dropped, (name, l))
    kinds = cases.boundary_kinds(name, l)
    assert kinds["word"] >= 8 and kinds["wave_small"] >= 4, (name, kinds)
    if used > 2 * cases.WAVE:
        assert kinds["wave_large"] >= 2, (name, kinds)
    if used > cases.TILE_S + 1:
        assert kinds["tile_small"] >= 2, (name, kinds)
    if used > cases.TILE_L + 1:
        assert kinds["tile_large"] >= 2, (name, kinds)


def test_generator_covers_contig_ends_and_drops(oracle):
    """Across the cases, void tests that fail at a boundary are exercised too (a site next to a contig start or end that
    the reference drops), on both strands."""
    strands = set()
    for name in cases.CASES:
        for l in cases.GUIDE_LENGTHS:
            strands |= {s for _, s, _ in cases.build(name, l)[3]}
    assert strands == {"plus", "minus"}


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
@pytest.mark.parametrize("l", cases.GUIDE_LENGTHS)
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_edges_vs_oracle(engine, oracle, name, l, request):
    contigs, offsets, planted, dropped, used = cases.build(name, l)
    want = oracle_rows(oracle, name, l)
    arena = engine.arena(contigs)
    try:
        assert arena.stats()["n_words"] == used
        assert [int(o) for o in arena.offsets] == offsets
        tiles = arena.tiles()
        assert tiles["geometry"] in request.node.callspec.id
        assert tiles["n_tiles"] == -(-used // tiles["tile_words"])
        hits = arena.scan_score(l, want_pre=True)
        got = [hits.contig(k) for k in range(len(contigs))]
        total = 0
        for k, w in enumerate(want):
            for key, col in w.items():
                g = got[k][key]
                assert g.shape == col.shape, (name, l, k, key, g.shape, col.shape)
                assert (bits(g) == bits(col)).all(), (name, l, k, key)
            total += w["pos_plus"].size + w["pos_minus"].size
        assert hits.n_plus + hits.n_minus == total
        assert_planted(got, planted, dropped, (name, l))
    finally:
        arena.close()
