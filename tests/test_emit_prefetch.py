"""The single-launch emit kernel's successor prefetch: a tile that is done with its rows asks for the four planes of the
tile `prefetch_tiles` tiles after it (Engine.configure(prefetch_tiles=...), CRP_OPT_PREFETCH_TILES).  Nothing reads what
the requests return, so the tables must be the oracle's bit for bit at every distance -- and the requests must stay inside
the grid of tiles whatever the distance is.  Arenas of 1, 2, 3 and 5 tiles in both geometries, distances 0 (off), 1, 2, 3,
8, 2^31 - 1 and the arena's default; the targets these give -- inside the grid, its last tile, one past it, far past the
arena -- are counted from the arithmetic first, without a GPU.  Arenas end 200 words into their last tile, or one word
short of its end, where the grid ends with the planes' allocation.  Through crp_scan_stream: one slice, and slice arenas
that are reset and refilled, the last time with a shorter slice, so that stale tiles lie behind the grid."""
import numpy as np
import pytest

from test_emit_row_strands import TILE_CHARS, _draw, arena_offsets, assert_rows_equal

TILE_WORDS = {g: c // 64 for g, c in TILE_CHARS.items()}
ALIGN_WORDS = 1024  # arena planes are padded to a multiple of this (crp_kernels.h)
TILES = (1, 2, 3, 5)
DISTANCES = (0, 1, 2, 3, 8, 2 ** 31 - 1, -1)  # -1: the arena's default
SLACK = {"loose": 200, "flush": None}  # used words of the last tile; flush: all but one
_CONTIGS, _ORACLE = {}, {}


def used_words(geometry, n_tiles, fit):
    tw = TILE_WORDS[geometry]
    return n_tiles * tw - 1 if fit == "flush" else (n_tiles - 1) * tw + SLACK[fit]


def contigs_of(geometry, n_tiles, fit):
    """one contig of mixed-case bases with a little N, of as many whole words as the case needs (word 0 and a gap word
    behind the contig are void)"""
    key = (geometry, n_tiles, fit)
    if key not in _CONTIGS:
        rng = np.random.default_rng([TILE_WORDS[geometry], n_tiles, len(fit)])
        words = used_words(*key) - 2
        _CONTIGS[key] = [_draw(rng, 64 * words - 5, "ACGTacgtN", [0.22] * 4 + [0.025] * 4 + [0.02])]
    return _CONTIGS[key]


def oracle_rows(oracle, key, l=20):
    if (key, l) not in _ORACLE:
        _ORACLE[key, l] = [oracle.scan_score(c, l) for c in contigs_of(*key)]
    return _ORACLE[key, l]


CASES = [(g, n, fit) for g in sorted(TILE_WORDS) for n in TILES for fit in sorted(SLACK)]


def test_targets_cover_the_four_situations():
    """Tile t asks for tile t + d.  Over the cases below a target is a tile inside the grid, the grid's last tile, the tile
    one past the grid and a tile far past the end of the planes' allocation; and in every geometry one arena's grid ends
    with its allocation while another's leaves allocated words behind the grid."""
    seen = {g: set() for g in TILE_WORDS}
    for g, n, fit in CASES:
        tw = TILE_WORDS[g]
        used = used_words(g, n, fit)
        assert arena_offsets(contigs_of(g, n, fit))[1] == 64 * used
        assert (n - 1) * tw < used <= n * tw  # n tiles
        padded = -(-(used + 1) // ALIGN_WORDS) * ALIGN_WORDS  # crp_arena_create: capacity = used words, + 1, padded
        seen[g].add("grid ends with the allocation" if n * tw == padded else "allocated words behind the grid")
        for d in DISTANCES:
            if d <= 0:
                continue
            for t in range(n):
                target = t + d
                if target < n - 1:
                    seen[g].add("inside")
                elif target == n - 1:
                    seen[g].add("last tile")
                elif target == n:
                    seen[g].add("one past the grid")
                if target * tw >= padded + 4 * tw:
                    seen[g].add("far past the allocation")
    for g, s in seen.items():
        # (the planes are padded to whole LARGE tiles: only a SMALL grid can end short of the allocation)
        behind = {"allocated words behind the grid"} if TILE_WORDS[g] < ALIGN_WORDS else set()
        assert s == {"inside", "last tile", "one past the grid", "far past the allocation", "grid ends with the allocation"} | behind, (g, s)


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


def _seeds_equal(engine, oracle, arena, cs, want, n_plus, n_minus, ctx):
    engine.offtarget_reset()
    arena.offtarget_add(20)
    engine.offtarget_solve()
    sp, sm = arena.offtarget_seeds(n_plus, n_minus)
    assert (sp == np.concatenate([oracle.seed_codes(c, w["pos_plus"], False, 20) for c, w in zip(cs, want)])).all(), ctx
    assert (sm == np.concatenate([oracle.seed_codes(c, w["pos_minus"], True, 20) for c, w in zip(cs, want)])).all(), ctx


@pytest.mark.gpu
@pytest.mark.parametrize("fit", sorted(SLACK))
@pytest.mark.parametrize("n_tiles", TILES)
def test_rows_vs_oracle_at_every_distance(engine, oracle, n_tiles, fit, request):
    """positions and scores of every row and the table totals at every distance; at distance 1 also the pre-sigmoid
    column and the seed words (the kernel's other variants), and the generic-length kernel (l = 23)"""
    from cropsr_amd.engine import Hits
    geometry = request.node.callspec.params["engine"]
    key = (geometry, n_tiles, fit)
    cs, want = contigs_of(*key), oracle_rows(oracle, key)
    n_want = (sum(w["pos_plus"].size for w in want), sum(w["pos_minus"].size for w in want))
    assert min(n_want) > 100 * n_tiles
    arena = engine.arena(cs)
    try:
        tiles = arena.tiles()
        assert tiles["geometry"] == geometry and tiles["n_tiles"] == n_tiles
        assert arena.stats()["n_words"] == used_words(*key)
        for d in DISTANCES:
            engine.configure(prefetch_tiles=d)
            hits = arena.scan_score(20, want_pre=False)
            assert (hits.n_plus, hits.n_minus) == n_want, (key, d)
            for k, w in enumerate(want):
                assert_rows_equal(hits.contig(k), w, (key, d, k), ("pos_plus", "score_plus", "pos_minus", "score_minus"))
        engine.configure(prefetch_tiles=1)
        assert arena.scan_score_device(20, want_pre=True, want_seeds=True) == n_want
        hits = Hits(arena.offsets, arena.lengths, 20, arena.fetch(*n_want, want_pre=True))
        for k, w in enumerate(want):
            assert_rows_equal(hits.contig(k), w, (key, "pre + seeds", k))
        _seeds_equal(engine, oracle, arena, cs, want, *n_want, ctx=key)
        hits = arena.scan_score(23, want_pre=True)
        for k, w in enumerate(oracle_rows(oracle, key, 23)):
            assert_rows_equal(hits.contig(k), w, (key, "l = 23", k))
        assert engine.query()["chain_timeouts"] == 0
    finally:
        arena.close()


def _stream_contigs():
    if "stream" not in _CONTIGS:
        rng = np.random.default_rng(77)
        _CONTIGS["stream"] = [_draw(rng, n, "ACGTacgtN", [0.22] * 4 + [0.025] * 4 + [0.02])
                              for n in (210_000, 95_000, 180_000, 140_000, 33_000)]
    return _CONTIGS["stream"]


@pytest.mark.gpu
@pytest.mark.parametrize("slice_chars,distance", [(0, 1), (0, -1), (150_000, 1), (150_000, 2), (150_000, -1)])
def test_stream_slices_vs_oracle(engine, oracle, slice_chars, distance):
    """crp_scan_stream: the whole genome as one slice, and as more slices than the pipeline has arenas -- each arena is
    reset and refilled, at last with what is left of the genome: fewer tiles than before, stale ones behind them"""
    cs = _stream_contigs()
    if "stream" not in _ORACLE:
        _ORACLE["stream"] = [oracle.scan_score(c, 20) for c in cs]
    engine.configure(prefetch_tiles=distance)
    hits = engine.scan_stream(cs, 20, want_pre=False, slice_chars=slice_chars)
    slices, lanes = hits.stream_stats["slices"], hits.stream_stats["lanes"]
    assert slices == 1 if slice_chars == 0 else slices > lanes >= 2, hits.stream_stats
    for k, w in enumerate(_ORACLE["stream"]):
        assert_rows_equal(hits.contig(k), w, (slice_chars, distance, k), ("pos_plus", "score_plus", "pos_minus", "score_minus"))
    assert engine.query()["chain_timeouts"] == 0
