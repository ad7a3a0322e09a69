"""The single-launch emit kernel reads its hit tables and chain arguments from the kernel-argument segment where it uses
them, derives the rounds' wave-uniform flags in the round and builds its store descriptors in every round.  Small
seeded arenas, each named for the condition it puts into
a tile -- shown first from the oracle's rows, without a GPU -- compared bit for bit with the oracle in both geometries
and both scan modes.  Contigs are prefixes of a seeded random string, cut where the oracle's own rows say the condition
holds."""
import numpy as np
import pytest

from test_emit_row_strands import (LIST, TILE_CHARS, _draw, arena_offsets, assert_condition, assert_rows_equal, contigs_of,
                                   oracle_rows, tile_rows)

ROW_COUNTS = (1, 63, 64, 65, 511, 512, 513)  # the partial chunk's mask, the exact-multiple exits, waves without rows
SEAMS = (0, 1, 63)                           # n_plus % 64
_CONTIGS, _ORACLE = {}, {}


def _count(oracle, text, strand):
    return int(oracle.scan_score(text, 20)["pos_" + strand].size)


def _cut(oracle, text, strand, n):
    """the shortest prefix of text with n rows on `strand` (a strand's row count grows by at most one per character)"""
    lo, hi = 0, len(text)
    assert _count(oracle, text, strand) >= n
    while lo < hi:
        mid = (lo + hi) // 2
        if _count(oracle, text[:mid], strand) >= n:
            hi = mid
        else:
            lo = mid + 1
    return text[:lo]


def _single_strand(oracle, strand, n):
    letters = "ATG" if strand == "plus" else "ATC"
    text = _draw(np.random.default_rng(11 if strand == "plus" else 12), 24000, letters, [0.4, 0.4, 0.2])
    return [_cut(oracle, text, strand, n)]


def _seam(oracle, rem):
    text = _draw(np.random.default_rng(13), 12000, "ACGT", [0.25] * 4)
    return [_cut(oracle, text, "plus", 320 + rem)]  # ~5 000 characters: one tile, about as many '-' rows


def _hit_free_last_tile(oracle):
    rng = np.random.default_rng(14)
    return [_draw(rng, TILE_CHARS["large"] + 500, "ACGT", [0.25] * 4), b"A" * (TILE_CHARS["large"] + 4000)]


def _table_overflow(oracle):
    """G-rich, then C-rich: most characters end a row on one strand, several rounds per tile; then a hit-free last tile"""
    rng, p = np.random.default_rng(15), [0.85, 0.075, 0.075]
    return [_draw(rng, 40000, "GAT", p), _draw(rng, 40000, "CAT", p), b"A" * (TILE_CHARS["large"] + 4000)]


def first_reservation(cs):
    """rows per strand of the device tables that an arena's first single-launch scan runs with (crp_api.cpp, scan_begin): a
    guess from the arena's characters; the launch after it has the exact sizes"""
    return sum(len(c) for c in cs) // 8 + 1024


def contigs(oracle, name):
    if name not in _CONTIGS:
        kind, _, arg = name.partition(":")
        if kind in ("plus", "minus"):
            _CONTIGS[name] = _single_strand(oracle, kind, int(arg))
        elif kind == "seam":
            _CONTIGS[name] = _seam(oracle, int(arg))
        elif kind == "table_overflow":
            _CONTIGS[name] = _table_overflow(oracle)
        else:
            _CONTIGS[name] = _hit_free_last_tile(oracle)
    return _CONTIGS[name]


def rows(oracle, name):
    """the oracle's rows of every contig of a case, computed once and shared (read-only)"""
    if name not in _ORACLE:
        _ORACLE[name] = [oracle.scan_score(c, 20) for c in contigs(oracle, name)]
    return _ORACLE[name]


CASES = (["%s:%d" % (s, n) for s in ("plus", "minus") for n in ROW_COUNTS] + ["seam:%d" % r for r in SEAMS] + ["hit_free_last_tile"])
OVERFLOW = "table_overflow"  # (run by a test of its own: only an arena's FIRST scan has the guessed table sizes)


def assert_case(oracle, name):
    cs, want = contigs(oracle, name), rows(oracle, name)
    kind, _, arg = name.partition(":")
    for geometry in sorted(TILE_CHARS):
        tiles = tile_rows(cs, want, geometry)
        counts = {t: (p.size, m.size) for t, (p, m) in tiles.items()}
        where = (name, geometry, counts)
        n_tiles = -(-arena_offsets(cs)[1] // TILE_CHARS[geometry])  # tiles with characters in them (padding adds void ones)
        if kind in ("plus", "minus"):
            assert arena_offsets(cs)[1] <= TILE_CHARS[geometry], where  # one tile with characters in it
            assert counts == {0: (int(arg), 0) if kind == "plus" else (0, int(arg))}, where
        elif kind == "seam":
            (p, m), = counts.values()  # one tile, one round
            assert arena_offsets(cs)[1] <= TILE_CHARS[geometry] and p % 64 == int(arg) and m > 64 and p + m <= LIST[geometry], where
        else:
            # the last tile that holds characters has no rows (and is more than a few characters away from any), nor has
            # any tile of padding behind it; earlier tiles have rows
            assert max(counts) < n_tiles - 1 and len(counts) >= 2, (where, n_tiles)
            last_row = max(int(w[k].max()) + o for w, o in zip(want, arena_offsets(cs)[0]) for k in ("pos_plus", "pos_minus") if w[k].size)
            assert last_row + 64 < (n_tiles - 1) * TILE_CHARS[geometry], (where, last_row)
            if kind == OVERFLOW:
                # either strand has more rows than the first launch's tables hold, and some tile takes several rounds
                n = [sum(w["pos_" + s].size for w in want) for s in ("plus", "minus")]
                assert min(n) > first_reservation(cs) + LIST[geometry], (where, n, first_reservation(cs))
                assert any(p > LIST[geometry] for p, _ in counts.values()) and any(m > LIST[geometry] for _, m in counts.values()), where


@pytest.mark.parametrize("name", CASES + [OVERFLOW])
def test_cases_hold_their_conditions(oracle, name):
    assert_case(oracle, name)


def test_two_round_cases_hold_their_conditions(oracle):
    for name in ("by_strand", "windowed"):
        assert_condition(name, 20, contigs_of(name), oracle_rows(oracle, name, 20))


# the pipelined scan's `density`: the caller's HOST tables hold density * characters + 1 024 rows per strand (the slice
# arenas' device tables are sized from the slice, not from it)
OVERFLOW_DENSITY = 0.001


def test_density_case_overflows_the_callers_tables(oracle):
    cs, want = contigs_of("by_strand"), oracle_rows(oracle, "by_strand", 20)
    cap = int(sum(len(c) for c in cs) * OVERFLOW_DENSITY) + 1024
    assert sum(w["pos_plus"].size for w in want) > 2 * cap and sum(w["pos_minus"].size for w in want) > 2 * cap


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


def _seeds_equal(engine, oracle, arena, cs, want, n_plus, n_minus, ctx):
    engine.offtarget_reset()
    arena.offtarget_add(20)
    engine.offtarget_solve()
    sp, sm = arena.offtarget_seeds(n_plus, n_minus)
    assert (sp == np.concatenate([oracle.seed_codes(c, w["pos_plus"], False, 20) for c, w in zip(cs, want)])).all(), ctx
    assert (sm == np.concatenate([oracle.seed_codes(c, w["pos_minus"], True, 20) for c, w in zip(cs, want)])).all(), ctx


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_rows_vs_oracle(engine, oracle, name, request):
    """positions, scores and the pre-sigmoid column of every row, the table totals, and the same rows from the kernel
    variant that also writes seed words"""
    geometry = request.node.callspec.params["engine"].split("-")[1]
    cs, want = contigs(oracle, name), rows(oracle, name)
    arena = engine.arena(cs)
    try:
        tiles = arena.tiles()
        assert tiles["geometry"] == geometry and tiles["tile_words"] * 64 == TILE_CHARS[geometry]
        assert [int(o) for o in arena.offsets] == arena_offsets(cs)[0]
        assert tiles["n_tiles"] >= -(-arena_offsets(cs)[1] // TILE_CHARS[geometry])
        n_want = (sum(w["pos_plus"].size for w in want), sum(w["pos_minus"].size for w in want))
        for want_pre in (False, True):
            hits = arena.scan_score(20, want_pre=want_pre)
            keys = None if want_pre else ("pos_plus", "score_plus", "pos_minus", "score_minus")
            for k, w in enumerate(want):
                assert_rows_equal(hits.contig(k), w, (name, k, want_pre), keys)
            assert (hits.n_plus, hits.n_minus) == n_want
        assert arena.scan_score_device(20, want_pre=True, want_seeds=True) == n_want
        _seeds_equal(engine, oracle, arena, cs, want, *n_want, ctx=name)
    finally:
        arena.close()


def test_unscored_case_mixes_scored_and_unscored_rows(oracle):
    """`incomplete` puts unscored rows into the pre-sigmoid column: chunks of 64 rows with both kinds on either strand
    (the condition it is named for), and an unscored row's pre-sigmoid value is its score"""
    want = oracle_rows(oracle, "incomplete", 20)
    assert_condition("incomplete", 20, contigs_of("incomplete"), want)
    for strand in ("plus", "minus"):
        score = np.concatenate([w["score_" + strand] for w in want])
        pre = np.concatenate([w["pre_" + strand] for w in want])
        assert (score == -1.0).any() and (score != -1.0).any(), strand
        assert (pre[score == -1.0] == -1.0).all(), strand


# two rounds: the store descriptors are built twice; unscored rows: their pre-sigmoid value is stored from the score
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["by_strand", "windowed", "incomplete"])
def test_all_columns_of_the_widest_variant(engine, oracle, name):
    """pre-sigmoid column, scores and seed words from the kernel variant that writes all of them"""
    cs, want = contigs_of(name), oracle_rows(oracle, name, 20)
    arena = engine.arena(cs)
    try:
        n_want = (sum(w["pos_plus"].size for w in want), sum(w["pos_minus"].size for w in want))
        assert arena.scan_score_device(20, want_pre=True, want_seeds=True) == n_want
        cols = arena.fetch(*n_want, want_pre=True)
        at = [0, 0]
        for w in want:
            for j, strand in enumerate(("plus", "minus")):
                n = w["pos_" + strand].size
                for col, key in ((1, "pre_"), (2, "score_")):
                    got = cols[3 * j + col][at[j]:at[j] + n]
                    assert (got.view(np.uint64) == w[key + strand].view(np.uint64)).all(), (name, strand, key)
                at[j] += n
        _seeds_equal(engine, oracle, arena, cs, want, *n_want, ctx=name)
    finally:
        arena.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["by_strand", "hit_free_last_tile"])
def test_pipelined_scan_overflows_then_gives_the_oracles_rows(_engine, oracle, name):
    """host tables too small for the genome: the pipelined scan stops copying rows where they end and goes on counting,
    the totals of its single-launch kernels say what is needed, and the repeated scan gives the oracle's rows.  (The
    device tables of its slice arenas fit here; test_device_tables_overflow_... is the case where they do not.)"""
    cs = contigs_of(name) if name == "by_strand" else contigs(oracle, name)
    want = oracle_rows(oracle, name, 20) if name == "by_strand" else rows(oracle, name)
    hits = _engine.scan_stream(cs, 20, want_pre=False, density=OVERFLOW_DENSITY)
    for k, w in enumerate(want):
        assert_rows_equal(hits.contig(k), w, ("stream", name, k), ("pos_plus", "score_plus", "pos_minus", "score_minus"))
    assert (hits.n_plus, hits.n_minus) == (sum(w["pos_plus"].size for w in want), sum(w["pos_minus"].size for w in want))


@pytest.mark.gpu
@pytest.mark.parametrize("want_pre,want_seeds", [(False, False), (True, False), (True, True)])
def test_device_tables_overflow_then_give_the_oracles_rows(engine, oracle, want_pre, want_seeds):
    """device tables too small: a fresh arena's first single-launch scan runs with first_reservation() rows per strand,
    fewer than either strand has (shown above from the oracle's rows), so the rows past the capacity that the kernel
    read late are dropped by its stores' range check; the totals say what is needed and the launch that follows, with
    exact sizes, gives the oracle's rows.  (The three-launch mode sizes its tables before it emits: same rows.)"""
    from cropsr_amd.engine import Hits
    cs, want = contigs(oracle, OVERFLOW), rows(oracle, OVERFLOW)
    n_want = (sum(w["pos_plus"].size for w in want), sum(w["pos_minus"].size for w in want))
    arena = engine.arena(cs)
    try:
        assert arena.stats()["n_chars"] // 8 + 1024 == first_reservation(cs) < min(n_want)
        assert arena.scan_score_device(20, want_pre=want_pre, want_seeds=want_seeds) == n_want
        hits = Hits(arena.offsets, arena.lengths, 20, arena.fetch(*n_want, want_pre=want_pre))
        keys = None if want_pre else ("pos_plus", "score_plus", "pos_minus", "score_minus")
        for k, w in enumerate(want):
            assert_rows_equal(hits.contig(k), w, (OVERFLOW, k, want_pre, want_seeds), keys)
        if want_seeds:
            _seeds_equal(engine, oracle, arena, cs, want, *n_want, ctx=OVERFLOW)
    finally:
        arena.close()
