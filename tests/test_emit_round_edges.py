"""The emit kernel's round plan decides on exact equalities with the capacity C of its per-round hit list (G::LIST): more
than C rows in a tile, each strand within C, windows of C ranks, a round that begins exactly at the first '-' row, a last
round of one row.  Every case here is one tile whose kept '+' and '-' row counts (p, m) sit exactly on such a boundary
(tests/emit_round_edge_cases.py builds them, in context, from the oracle's own positions).  Without a GPU: the counts,
the placement and the property each group is named for, from a plain restatement of the plan.  On the GPU, bit for bit
against the oracle: every case alone in both scan modes over three scans, through the kernel with both extra columns,
between neighbouring tiles, through the pipelined scan, and arenas whose rows are one below, on and one above what a
first scan's guessed tables hold.  A tile's last round also asks for the planes of the tile `prefetch_tiles` behind it,
into the register that holds every round's first list offset -- but only when that tile is one of the grid, and the
default distance lies far past these arenas: so every case also runs with a populated tile behind it at distance 1,
where the CPU tests show from the kernel's own arithmetic that the request is issued."""
import re

import numpy as np
import pytest

import emit_round_edge_cases as ec
from emit_round_edge_cases import R, SEAMS, case_id, rounds
from test_emit_row_strands import LIST, TILE_CHARS, arena_offsets, assert_rows_equal, tile_rows

GEOMETRIES = sorted(TILE_CHARS)
KEYS = ("pos_plus", "score_plus", "pos_minus", "score_minus")


def test_list_and_tile_sizes_are_the_headers():
    """a changed geometry fails here; it does not silently move the cases off the boundary"""
    header = ec.emit_geometries()  # (tests/sparse_genome_cases.py reads the TileGeo lines)
    assert sorted(header) == GEOMETRIES
    for geometry, geo in header.items():
        assert geo["list"] == LIST[geometry] and geo["words"] * 64 == TILE_CHARS[geometry], (geometry, geo)
        assert geo["block"] == 512, (geometry, geo)  # R is stated on eight chunks of 64 rows per trip
        assert max(SEAMS) + 200 <= geo["list"] and max(R) < geo["list"] // 2, (geometry, geo)


@pytest.mark.parametrize("C", [5, 64, 3072, 5016])
def test_round_plan_covers_every_rank_once(C):
    for p in (0, 1, C - 1, C, C + 1, 2 * C, 2 * C + 1):
        for m in (0, 1, C - 1, C, C + 1, 2 * C, 2 * C + 1):
            plan = rounds(p, m, C)
            assert [lo for lo, _, _ in plan] == [0] * bool(plan) + [hi for _, hi, _ in plan[:-1]], (p, m, plan)
            assert (plan[-1][1] if plan else 0) == p + m and all(0 < hi - lo <= C for lo, hi, _ in plan), (p, m, plan)
            assert len({kind for _, _, kind in plan}) <= 1, (p, m, plan)
            assert (len(plan) > 1) == (p + m > C), (p, m, plan)
            if plan and plan[0][2] == "by_strand":
                assert plan == [(0, p, "by_strand"), (p, p + m, "by_strand")] and 0 < p <= C and 0 < m <= C, (p, m, plan)
            elif len(plan) > 1:
                assert p > C or m > C, (p, m, plan)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_cases_have_their_counts_and_lie_in_one_tile(oracle, geometry):
    """the oracle's rows of every built contig are exactly (p, m), and its arena ends inside tile 0"""
    assert len(ec.cases(geometry)) >= 70
    for p, m, l in ec.runs(geometry):
        text, want = ec.text_of(oracle, p, m), ec.rows_of(oracle, p, m, l)
        where = (geometry, p, m, l)
        assert (want["pos_plus"].size, want["pos_minus"].size) == (p, m), where
        assert text.startswith(ec.SEP) and text.endswith(ec.SEP) and arena_offsets([text])[1] <= TILE_CHARS[geometry], where
        counts = {t: (a.size, b.size) for t, (a, b) in tile_rows([text], [want], geometry).items()}
        assert counts == {0: (p, m)}, (where, counts)
        # l = 20: every row is scored, both tables hold real scores to compare (l = 23: a window of 33 characters is not scored)
        unscored = np.concatenate([want["score_plus"], want["score_minus"]]) == -1.0
        assert unscored.all() if l == 23 else not unscored.any(), where


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_groups_hold_their_properties(geometry):
    """each group's named property, from the round plan"""
    C = LIST[geometry]
    groups = ec.groups(C)
    assert sorted(groups) == list(ec.GROUPS) and all(ec.pick(C)[g] in groups[g] for g in groups)
    plan = lambda pm: rounds(pm[0], pm[1], C)
    sizes = lambda pm: [hi - lo for lo, hi, _ in plan(pm)]
    kinds = lambda pm: {kind for _, _, kind in plan(pm)}
    # A: one round, exactly full
    assert all(plan(pm) == [(0, C, "single")] for pm in groups["A"]), groups["A"]
    assert {(C, 0), (0, C), (C - 1, 1), (1, C - 1)} <= set(groups["A"])
    assert sorted(p % 64 for p, m in groups["A"] if min(p, m) > 64) == [0, 1, 63]
    # B: one row over
    assert all(p + m == C + 1 for p, m in groups["B"])
    assert [pm for pm in groups["B"] if plan(pm) == [(0, C, "window"), (C, C + 1, "window")]] == [(C + 1, 0), (0, C + 1)]
    assert [pm for pm in groups["B"] if plan(pm) == [(0, pm[0], "by_strand"), (pm[0], C + 1, "by_strand")]] == groups["B"][2:]
    assert len(groups["B"]) == 5 and any(min(pm) > 64 for pm in groups["B"])
    # C: by strand with a full strand, the other strand's round of every size in R (and C)
    assert all(kinds(pm) == {"by_strand"} and sizes(pm) == list(pm) and C in pm for pm in groups["C"]), groups["C"]
    assert sorted(m for p, m in groups["C"] if p == C) == sorted(R + (C,))
    assert sorted(p for p, m in groups["C"] if m == C) == sorted(R + (C,))
    # D: one strand over by one, windowed, both strands present
    assert all(kinds(pm) == {"window"} and min(pm) > 0 and max(pm) == C + 1 for pm in groups["D"]), groups["D"]
    assert len(groups["D"]) == 5
    # E: rows from a LATER window's first rank to the seam -- 0: the window begins exactly at n_plus
    into = {}
    for p, m in groups["E"]:
        assert kinds((p, m)) == {"window"} and p > 0 and m > 0, (p, m)
        into[p, m] = [p - lo for lo, hi, _ in plan((p, m)) if 0 < lo <= p < hi]
    assert into[C, C + 1] == [0] and into[2 * C, 1] == [0] and sizes((2 * C, 1))[-1] == 1, into
    assert [into[C + s, 200] for s in SEAMS] == [[s] for s in SEAMS], into
    assert sorted(x for v in into.values() for x in v) == [0, 0, 1, 63, 64, 65], into
    assert into[C - 1, C + 1] == [] and [lo for lo, _, _ in plan((C - 1, C + 1))] == [0, C], into  # a window begins one past the seam
    # F: exact multiples, and one row past them
    assert all(sum(pm) % C == 0 and sizes(pm) == [C, C] and kinds(pm) == {"window"} for pm in groups["F"][:3]), groups["F"]
    assert [p - lo for p, m in groups["F"][2:3] for lo, hi, _ in plan((p, m)) if 0 < lo <= p < hi] == [64]
    assert all(sizes(pm) == [C, C, 1] and kinds(pm) == {"window"} for pm in groups["F"][3:]) and len(groups["F"]) == 5
    # G: windowed, every last-round size, on either strand
    assert all(kinds(pm) == {"window"} and len(plan(pm)) == 2 and min(pm) == 0 for pm in groups["G"]), groups["G"]
    assert [sizes(pm)[-1] for pm in groups["G"]] == list(R) * 2
    assert [p > 0 for p, m in groups["G"]] == [True] * len(R) + [False] * len(R)
    # H: three rounds or more on both strands
    (p, m), = groups["H"]
    assert p > 2 * C and m > 2 * C and len(plan((p, m))) == 5 and sizes((p, m))[-1] == 2
    # at l = 20 nothing of R is trimmed
    at20 = [pm for pm, l in ((x[:2], x[2]) for x in ec.runs(geometry)) if l == 20]
    assert all(pm in at20 for g in groups.values() for pm in g) and len(at20) == len(set(at20))


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_neighbour_arenas_hold_their_tiles(oracle, geometry):
    """per tile, from the oracle's rows: the exact tiles hold exactly their (p, m) -- more than one round each --, the random
    ones a few dozen rows, the hit-free one none; every island is 64 words or more from its tile's ends"""
    C = LIST[geometry]
    assert [g for g in "BCDEFGH" if len(rounds(*ec.pick(C)[g], C)) > 1] == list("BCDEFGH")
    for layout, pm in ec.neighbour_cases(geometry):
        cs, plan = ec.neighbour_contig(oracle, geometry, layout, pm)
        want = ec.neighbour_rows(oracle, geometry, layout, pm)
        where = (geometry, layout, pm)
        assert len(cs) == 1 and -(-arena_offsets(cs)[1] // TILE_CHARS[geometry]) == len(plan), where
        counts = {t: (a.size, b.size) for t, (a, b) in tile_rows(cs, want, geometry).items()}
        assert sorted(counts) == [t for t, what in enumerate(plan) if what is not None], (where, counts)
        for t, what in enumerate(plan):
            if what == "random":
                assert 12 <= sum(counts[t]) <= 120, (where, counts)
            elif what is not None:
                assert counts[t] == what, (where, counts)
        edge = 64 * ec.EDGE_WORDS
        for strand in ("plus", "minus"):
            at = (want[0]["pos_" + strand].astype(np.int64) + 64) % TILE_CHARS[geometry]
            assert at.size == 0 or (edge <= at.min() and at.max() < TILE_CHARS[geometry] - edge), (where, strand)
        # the exact tile's last round asks for the tile behind it exactly where it has one: not at the default distance
        # (3/8 of the GPU's tiles) nor at 0, at distance 1 in `between` and `adjacent`, where the target is a grid tile
        n_tiles = ec.grid_tiles(geometry, cs)
        issued = [ec.prefetch_issued(t, 1, n_tiles) for t, what in enumerate(plan) if isinstance(what, tuple)]
        assert n_tiles == len(plan) and issued == {"between": [True], "last": [False], "adjacent": [True, True]}[layout], where
    assert ec.PREFETCH_DISTANCES == (-1, 0, 1) and not ec.prefetch_issued(0, 0, 3)
    layouts = {layout: ec._layout(geometry, layout, ec.pick(C)["D"]) for layout in ec.LAYOUTS}
    assert layouts["between"][0] == layouts["between"][2] == "random" and layouts["last"][0] is None
    assert all(isinstance(what, tuple) for what in layouts["adjacent"][:2]) and layouts["adjacent"][0] != layouts["adjacent"][1]


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_followed_arenas_hold_their_tiles_and_ask_for_the_successor(oracle, geometry):
    """every run with a populated tile behind it: tile 0 holds exactly (p, m), tile 1 a few dozen rows, and at distance 1
    tile 0's request is inside the grid (0 < d < n_tiles - t, as prefetch_successor_plane decides it) -- while alone in
    its arena, as in the one-tile tests, no case asks for anything"""
    for p, m, l in ec.runs(geometry):
        cs, plan = ec.neighbour_contig(oracle, geometry, ec.FOLLOWED, (p, m))
        want = ec.neighbour_rows(oracle, geometry, ec.FOLLOWED, (p, m), l)
        where = (geometry, p, m, l)
        counts = {t: (a.size, b.size) for t, (a, b) in tile_rows(cs, want, geometry).items()}
        assert plan == [(p, m), "random"] and counts[0] == (p, m) and 12 <= sum(counts[1]) <= 120 and len(counts) == 2, (where, counts)
        n_tiles = ec.grid_tiles(geometry, cs)
        assert n_tiles == 2 and ec.prefetch_issued(0, 1, n_tiles) and not ec.prefetch_issued(1, 1, n_tiles), where
        alone = ec.grid_tiles(geometry, [ec.text_of(oracle, p, m)])
        assert alone == 1 and not ec.prefetch_issued(0, 1, alone), where


def test_table_edge_arenas_hold_their_rows(oracle):
    """the capacity of a first single-launch scan's tables, restated from the two expressions of crp_api.cpp -- which still
    stand there --, and arenas with one row less, as many and one more on either strand"""
    source = ec.api_source()
    begin = source[source.index("int scan_begin("):source.index("int scan_finish(")]
    assert len(re.findall(ec.FIRST_ROWS, begin)) == 2, "scan_begin sizes a first scan's tables otherwise"
    grow = source[source.index("int grow("):]
    assert re.search(ec.GROW_ROWS, grow[:grow.index("\n}\n")]), "grow allocates otherwise"
    cap0 = ec.first_capacity(ec.TABLE_CHARS)
    assert cap0 == 3744 and ec.first_capacity(0) == 1088
    seen = []
    for kind, d in ec.TABLE_EDGE_CASES:
        cs, want = ec.table_edge_contig(oracle, kind, d), ec.table_edge_rows(oracle, kind, d)
        n = (want[0]["pos_plus"].size, want[0]["pos_minus"].size)
        assert len(cs[0]) == ec.TABLE_CHARS and n == ec.table_edge_counts(kind, d), (kind, d, n)
        seen.append((n[0] - cap0, n[1] - cap0))
    assert seen == [(-1, -cap0), (0, -cap0), (1, -cap0), (-cap0, -1), (-cap0, 0), (-cap0, 1), (1, 500 - cap0)], seen
    assert LIST["small"] < cap0 < LIST["large"]  # several rounds in one geometry, one round in the other


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def _engine():
    from cropsr_amd import Engine
    eng = Engine(0)  # raises if libcropsr_hip.so or the GPU is missing: no fallback
    yield eng
    assert eng.query()["chain_timeouts"] == 0
    eng.close()


@pytest.fixture
def configured(_engine):
    """configured(mode, geometry) -> the engine in that setting; the defaults come back afterwards"""
    def go(mode, geometry):
        _engine.configure(two_pass=mode == "two_pass", geometry=geometry)
        return _engine
    yield go
    _engine.configure(two_pass=False, geometry="auto", prefetch_tiles=-1)


SETTINGS = [(mode, geometry) for mode in ("single_pass", "two_pass") for geometry in ("large", "small")]


def _params(cases_of, settings=SETTINGS):
    name = lambda case: "%s-%s" % (case[0], case_id(case[1])) if isinstance(case[0], str) else case_id(case)
    return [pytest.param(mode, geometry, *case, id="%s-%s-%s" % (mode, geometry, name(case)))
            for mode, geometry in settings for case in cases_of(geometry)]


def _totals(want):
    return (sum(w["pos_plus"].size for w in want), sum(w["pos_minus"].size for w in want))


def _assert_single_launch_held(engine, mode, ctx):
    if mode == "single_pass":
        q = engine.query()
        assert q["chain_timeouts"] == 0 and q["two_pass_active"] == 0, (ctx, q)


def _seeds_equal(engine, oracle, arena, cs, want, ctx):
    """the seed words of the last scan (written by the kernel) against oracle.seed_codes"""
    engine.offtarget_reset()
    arena.offtarget_add(20)
    engine.offtarget_solve()
    sp, sm = arena.offtarget_seeds(*_totals(want))
    assert (sp == np.concatenate([oracle.seed_codes(c, w["pos_plus"], False, 20) for c, w in zip(cs, want)])).all(), ctx
    assert (sm == np.concatenate([oracle.seed_codes(c, w["pos_minus"], True, 20) for c, w in zip(cs, want)])).all(), ctx


@pytest.mark.gpu
@pytest.mark.parametrize("mode,geometry,p,m,l", _params(ec.runs))
def test_rows_vs_oracle(configured, oracle, mode, geometry, p, m, l):
    """every case alone in a one-tile arena, three scans in a row: the two chain buffers alternate; the first scan runs
    with the guessed table sizes, the later ones with tables sized from it (the second also writes the pre-sigmoid column)"""
    engine = configured(mode, geometry)
    cs, want = [ec.text_of(oracle, p, m)], [ec.rows_of(oracle, p, m, l)]
    arena = engine.arena(cs)
    try:
        tiles = arena.tiles()
        assert tiles["geometry"] == geometry and tiles["tile_words"] * 64 == TILE_CHARS[geometry]
        assert [int(o) for o in arena.offsets] == arena_offsets(cs)[0]
        for scan, want_pre in enumerate((False, True, False)):
            hits = arena.scan_score(l, want_pre=want_pre)
            assert (hits.n_plus, hits.n_minus) == (p, m), (scan, hits.n_plus, hits.n_minus)
            assert_rows_equal(hits.contig(0), want[0], (geometry, p, m, l, scan), None if want_pre else KEYS)
        _assert_single_launch_held(engine, mode, (geometry, p, m, l))
    finally:
        arena.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,geometry,p,m", _params(ec.both_columns_cases))
def test_both_extra_columns_vs_oracle(configured, oracle, mode, geometry, p, m):
    """the instantiation that writes the pre-sigmoid column and the seed words (its look-back keeps two slots)"""
    from cropsr_amd.engine import Hits
    engine = configured(mode, geometry)
    cs, want = [ec.text_of(oracle, p, m)], [ec.rows_of(oracle, p, m, 20)]
    arena = engine.arena(cs)
    try:
        assert arena.tiles()["geometry"] == geometry
        assert arena.scan_score_device(20, want_pre=True, want_seeds=True) == (p, m)
        hits = Hits(arena.offsets, arena.lengths, 20, arena.fetch(p, m, want_pre=True))
        assert_rows_equal(hits.contig(0), want[0], (geometry, p, m, "pre + seeds"))
        _seeds_equal(engine, oracle, arena, cs, want, (geometry, p, m))
        _assert_single_launch_held(engine, mode, (geometry, p, m))
    finally:
        arena.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,geometry,layout,pm", _params(ec.neighbour_cases, [s for s in SETTINGS if s[0] == "single_pass"]))
def test_rows_with_neighbours_vs_oracle(configured, oracle, mode, geometry, layout, pm):
    """the exact tile between populated tiles, last behind a hit-free tile, and next to another multi-round tile; the rows
    of the tiles behind it depend on the totals it published.  prefetch_tiles at the arena's default and at 0 (neither
    issues a request in a grid this small) and at 1, where the exact tile of `between` and `adjacent` asks for the tile
    behind it (shown without a GPU above)"""
    engine = configured(mode, geometry)
    cs, plan = ec.neighbour_contig(oracle, geometry, layout, pm)
    want = ec.neighbour_rows(oracle, geometry, layout, pm)
    arena = engine.arena(cs)
    try:
        tiles = arena.tiles()
        assert tiles["geometry"] == geometry and tiles["n_tiles"] == ec.grid_tiles(geometry, cs) == len(plan)
        for distance in ec.PREFETCH_DISTANCES:
            engine.configure(prefetch_tiles=distance)
            hits = arena.scan_score(20, want_pre=False)
            assert (hits.n_plus, hits.n_minus) == _totals(want), (distance, hits.n_plus, hits.n_minus)
            assert_rows_equal(hits.contig(0), want[0], (geometry, layout, pm, distance), KEYS)
        _assert_single_launch_held(engine, mode, (geometry, layout, pm))
    finally:
        engine.configure(prefetch_tiles=-1)
        arena.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,geometry,p,m,l", _params(ec.runs, [s for s in SETTINGS if s[0] == "single_pass"]))
def test_rows_with_a_successor_vs_oracle(configured, oracle, mode, geometry, p, m, l):
    """every run with a populated tile behind it and prefetch_tiles = 1: waves 1 ... 4 of the exact tile load a word of the
    successor's planes into the register of their first list offset, in the last round and in no earlier one.  Two scans;
    at l = 20 a third through the instantiation with both extra columns, seed words included."""
    from cropsr_amd.engine import Hits
    engine = configured(mode, geometry)
    cs, _ = ec.neighbour_contig(oracle, geometry, ec.FOLLOWED, (p, m))
    want = ec.neighbour_rows(oracle, geometry, ec.FOLLOWED, (p, m), l)
    arena = engine.arena(cs)
    try:
        tiles = arena.tiles()
        assert tiles["geometry"] == geometry and tiles["n_tiles"] == ec.grid_tiles(geometry, cs) == 2
        engine.configure(prefetch_tiles=1)
        for scan, want_pre in enumerate((False, True)):
            hits = arena.scan_score(l, want_pre=want_pre)
            assert (hits.n_plus, hits.n_minus) == _totals(want), (scan, hits.n_plus, hits.n_minus)
            assert_rows_equal(hits.contig(0), want[0], (geometry, p, m, l, scan), None if want_pre else KEYS)
        if l == 20:
            assert arena.scan_score_device(20, want_pre=True, want_seeds=True) == _totals(want)
            hits = Hits(arena.offsets, arena.lengths, 20, arena.fetch(*_totals(want), want_pre=True))
            assert_rows_equal(hits.contig(0), want[0], (geometry, p, m, "pre + seeds"))
            _seeds_equal(engine, oracle, arena, cs, want, (geometry, p, m))
        _assert_single_launch_held(engine, mode, (geometry, p, m, l))
    finally:
        engine.configure(prefetch_tiles=-1)
        arena.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,geometry,p,m,l", _params(ec.runs, [s for s in SETTINGS if s[0] == "single_pass"]))
def test_pipelined_scan_vs_oracle(configured, oracle, mode, geometry, p, m, l):
    """every case alone through the pipelined scan: one contig, one slice (host tables sized for a row per character).
    The slice arenas are sealed by the engine's context, so the configured geometry should hold for them, but nothing the
    pipelined scan reports names the geometry it ran with: that is NOT checked here (a slice this small is SMALL by
    default, so it is the LARGE cases that rest on the setting)."""
    engine = configured(mode, geometry)
    want = ec.rows_of(oracle, p, m, l)
    hits = engine.scan_stream([ec.text_of(oracle, p, m)], l, want_pre=False, density=1.0)
    assert hits.stream_stats["slices"] == 1, hits.stream_stats
    assert (hits.n_plus, hits.n_minus) == (p, m)
    assert_rows_equal(hits.contig(0), want, ("stream", geometry, p, m, l), KEYS)
    _assert_single_launch_held(engine, mode, ("stream", geometry, p, m, l))


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", ["large", "small"])
@pytest.mark.parametrize("kind,d", ec.TABLE_EDGE_CASES)
def test_first_scans_tables_exactly_full(configured, oracle, geometry, kind, d):
    """ONE scan of a fresh arena whose rows are one fewer than, as many as and one more than the tables of a first
    single-launch scan hold (first_capacity(): shown above to restate crp_api.cpp), on either strand, and '+' one over
    while '-' fits.  One over, the kernel drops the row past the capacity and the scan is launched again with the exact
    sizes; no statistic reports whether that relaunch ran, so this test sees only that the rows are the oracle's either way."""
    engine = configured("single_pass", geometry)
    cs, want = ec.table_edge_contig(oracle, kind, d), ec.table_edge_rows(oracle, kind, d)
    arena = engine.arena(cs)
    try:
        assert arena.tiles()["geometry"] == geometry
        assert ec.first_capacity(arena.stats()["n_chars"]) == ec.first_capacity(ec.TABLE_CHARS)
        hits = arena.scan_score(20, want_pre=True)
        assert (hits.n_plus, hits.n_minus) == ec.table_edge_counts(kind, d)
        assert_rows_equal(hits.contig(0), want[0], (geometry, kind, d))
        _assert_single_launch_held(engine, "single_pass", (geometry, kind, d))
    finally:
        arena.close()
