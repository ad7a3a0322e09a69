"""The look-back's first window with every request in flight (single-launch emit kernel): lane k, slot j of a look
reads tile t - 1 - k - 64 j, and an index before tile 0 reads tile 0's descriptor in place of the empty prefix it stands
for.  That substitution is live exactly in tiles 0 ... 127 -- in slot 0 for tiles below 64 and, where a look has a second
slot (the instantiation with both extra columns; any A/B build with a deeper look), in slot 1 for tiles below 128 -- so one
arena of 200 tiles runs every affected index.  Poly-A filler (no PAM on either strand) with one island of random
mixed-case sequence per populated tile, a few dozen hits each; the tiles around the slot edges -- 0, 1, 62 ... 65,
126 ... 129 -- are hit-free (aggregate 0, early exit) in one variant and the only populated ones in the other.  Arenas of
1, 2, 64, 65, 128 and 129 tiles put the tile that publishes the totals at each of those places, populated or not.  Both
tables against the oracle row for row, three scans in a row (the two descriptor buffers alternate), with and without the
successor prefetch; no time-out, no fall-back to three launches.  The 200-tile arenas also through the kernel with both
extra columns, whose look keeps two slots."""
import numpy as np
import pytest

from test_emit_row_strands import TILE_CHARS, _draw, arena_offsets, assert_rows_equal, tile_rows

EDGE_TILES = (0, 1, 62, 63, 64, 65, 126, 127, 128, 129)
ARENAS = (200, 1, 2, 64, 65, 128, 129)  # tiles
VARIANTS = ("edges_empty", "edges_only")
ISLAND_AT, ISLAND_CHARS = 100 * 64, 1600  # an island lies in words 100 ... 124 of its tile, far from either end of it
LAST_TILE_WORDS = 200                    # used words of the last tile
KEYS = ("pos_plus", "score_plus", "pos_minus", "score_minus")
_CONTIGS, _ORACLE = {}, {}


def populated(n_tiles, variant):
    edge = set(EDGE_TILES)
    return [t for t in range(n_tiles) if (t in edge) == (variant == "edges_only")]


def contigs_of(geometry, n_tiles, variant):
    """one contig that ends LAST_TILE_WORDS words into tile n_tiles - 1 (word 0 and a gap word behind the contig are void)"""
    key = (geometry, n_tiles, variant)
    if key not in _CONTIGS:
        tile_chars = TILE_CHARS[geometry]
        rng = np.random.default_rng([tile_chars, n_tiles, VARIANTS.index(variant)])
        words = (n_tiles - 1) * (tile_chars // 64) + LAST_TILE_WORDS - 2
        text = bytearray(b"A" * (64 * words - 5))
        for t in populated(n_tiles, variant):
            at = t * tile_chars + ISLAND_AT - 64  # (the contig begins at character 64 of the arena)
            text[at:at + ISLAND_CHARS] = _draw(rng, ISLAND_CHARS, "ACGTacgt", [0.125] * 8)
        _CONTIGS[key] = [bytes(text)]
    return _CONTIGS[key]


def oracle_rows(oracle, key):
    """the oracle's rows of a case, computed once and shared (read-only)"""
    if key not in _ORACLE:
        _ORACLE[key] = [oracle.scan_score(c, 20) for c in contigs_of(*key)]
    return _ORACLE[key]


CASES = [(n, v) for n in ARENAS for v in VARIANTS]


@pytest.mark.parametrize("geometry", sorted(TILE_CHARS))
def test_arenas_hold_their_conditions(oracle, geometry):
    """from the oracle's rows, without a GPU: the tiles with hits are the populated ones and no others, each with a few
    dozen rows; the 200-tile arena has the substitution's whole range behind it and both kinds of tile at each slot edge"""
    for n_tiles, variant in CASES:
        key = (geometry, n_tiles, variant)
        cs, rows = contigs_of(*key), oracle_rows(oracle, key)
        assert arena_offsets(cs)[1] == 64 * ((n_tiles - 1) * (TILE_CHARS[geometry] // 64) + LAST_TILE_WORDS), key
        counts = {t: p.size + m.size for t, (p, m) in tile_rows(cs, rows, geometry).items()}
        assert sorted(counts) == populated(n_tiles, variant), (key, sorted(counts))
        assert all(12 <= c <= 120 for c in counts.values()), (key, counts)
    assert ARENAS[0] > 128 + 64 and set(EDGE_TILES) < set(range(ARENAS[0]))
    assert populated(200, "edges_only") == list(EDGE_TILES) and len(populated(200, "edges_empty")) == 190
    # the last tile, which publishes the totals, is hit-free in one variant of every arena and populated in the other
    for n_tiles in ARENAS:
        assert sum(n_tiles - 1 in populated(n_tiles, v) for v in VARIANTS) == 1, n_tiles


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def _engine():
    from cropsr_amd import Engine
    eng = Engine(0)  # raises if libcropsr_hip.so or the GPU is missing: no fallback
    yield eng
    assert eng.query()["chain_timeouts"] == 0
    eng.close()


@pytest.fixture(params=["large", "small"])
def engine(_engine, request):
    _engine.configure(two_pass=False, geometry=request.param)
    yield _engine
    _engine.configure(geometry="auto", prefetch_tiles=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("n_tiles,variant", CASES)
def test_rows_vs_oracle(engine, oracle, n_tiles, variant, request):
    from cropsr_amd.engine import Hits
    geometry = request.node.callspec.params["engine"]
    key = (geometry, n_tiles, variant)
    cs, want = contigs_of(*key), oracle_rows(oracle, key)
    n_want = (sum(w["pos_plus"].size for w in want), sum(w["pos_minus"].size for w in want))
    arena = engine.arena(cs)
    try:
        tiles = arena.tiles()
        assert tiles["geometry"] == geometry and tiles["n_tiles"] == n_tiles
        for distance in (-1, 0):  # the arena's default, and no prefetch
            engine.configure(prefetch_tiles=distance)
            for scan in range(3):
                hits = arena.scan_score(20, want_pre=False)
                assert (hits.n_plus, hits.n_minus) == n_want, (key, distance, scan)
                for k, w in enumerate(want):
                    assert_rows_equal(hits.contig(k), w, (key, distance, scan, k), KEYS)
        if n_tiles == ARENAS[0]:  # the pre-sigmoid column and the seed words: the instantiation with a second slot
            assert arena.scan_score_device(20, want_pre=True, want_seeds=True) == n_want
            hits = Hits(arena.offsets, arena.lengths, 20, arena.fetch(*n_want, want_pre=True))
            for k, w in enumerate(want):
                assert_rows_equal(hits.contig(k), w, (key, "pre + seeds", k))
        q = engine.query()
        assert q["chain_timeouts"] == 0 and q["two_pass_active"] == 0, q
    finally:
        arena.close()
