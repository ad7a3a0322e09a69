"""The row loop of the emit kernel carries a row's strand as one flag, orients '+' windows and sets the -1.0 of an
unscored row in regions that whole waves skip, and tells the strands apart by the row's place in the round's hit list.
Small seeded arenas, each named for the condition it puts into a tile -- shown first from the oracle's rows, without a
GPU -- compared bit for bit with the oracle in both geometries and both scan modes, through the seed-word variant and
through the pipelined scan."""
import numpy as np
import pytest

# tile geometries of the emit kernel (cropsr_amd/csrc/crp_kernels.h): characters per tile and hit-list entries per round
TILE_CHARS = {"large": 1024 * 64, "small": 512 * 64}
LIST = {"large": 5016, "small": 3072}
BLOCK = 512  # threads per tile: eight chunks of 64 rows per trip


def _draw(rng, n, letters, p):
    return np.frombuffer(letters.encode(), dtype=np.uint8)[rng.choice(len(letters), size=n, p=p)].tobytes()


def _plus_only(rng):
    return [_draw(rng, 2 * TILE_CHARS["large"], "ATG", [0.4, 0.4, 0.2])]


def _minus_only(rng):
    return [_draw(rng, 2 * TILE_CHARS["large"], "ATC", [0.4, 0.4, 0.2])]


def _mixed_seam(rng):
    return [_draw(rng, 12000, "ACGT", [0.25] * 4)]


def _by_strand(rng):
    return [_draw(rng, 2 * TILE_CHARS["large"], "ACGT", [0.25] * 4)]


def _windowed(rng):
    return [_draw(rng, 30000, "GAT", [0.85, 0.075, 0.075]) + _draw(rng, 30000, "CAT", [0.85, 0.075, 0.075])]


def _incomplete(rng):
    return [_draw(rng, int(rng.integers(26, 41)), "ACGT", [0.1, 0.4, 0.4, 0.1]) for _ in range(200)]


def _mixed_chars(rng):
    letters = "ACGTacgtNRYUZ"
    return [_draw(rng, 20000, letters, [0.14, 0.22, 0.22, 0.14] + [0.02] * 4 + [0.04] * 5)]


BUILDERS = {"plus_only": _plus_only, "minus_only": _minus_only, "mixed_seam": _mixed_seam, "by_strand": _by_strand,
            "windowed": _windowed, "incomplete": _incomplete, "mixed_chars": _mixed_chars}
# every case on the l = 20 scorer; the seam, the windowed rounds and the contig ends also on the generic path (whose
# windows are cut to 30 by the contig end), the contig ends also where no row is scored
RUNS = [(name, 20) for name in BUILDERS] + [("mixed_seam", 23), ("windowed", 23), ("incomplete", 23), ("incomplete", 18)]
_CONTIGS, _ORACLE = {}, {}


def contigs_of(name):
    if name not in _CONTIGS:
        _CONTIGS[name] = BUILDERS[name](np.random.default_rng(1 + sorted(BUILDERS).index(name)))
    return _CONTIGS[name]


def oracle_rows(oracle, name, l):
    """the oracle's rows of every contig of a case, computed once and shared (read-only)"""
    if (name, l) not in _ORACLE:
        _ORACLE[name, l] = [oracle.scan_score(c, l) for c in contigs_of(name)]
    return _ORACLE[name, l]


def arena_offsets(contigs, first=64):
    """character offset of every contig in an arena that holds them in this order (a gap word after each)"""
    offs, off = [], first
    for c in contigs:
        offs.append(off)
        off += ((len(c) + 63) // 64 + 1) * 64
    return offs, off


def tile_rows(contigs, rows, geometry, first=64):
    """{tile: (scores of its '+' rows, scores of its '-' rows)} in table order.  A row is counted in the tile its
    position falls in; the kernel's own attribution differs by a few characters at most, so the conditions below keep a
    margin of 16 rows wherever they are stated on a tile that has neighbours."""
    offs, _ = arena_offsets(contigs, first)
    out = {}
    for strand, j in (("plus", 0), ("minus", 1)):
        pos = np.concatenate([r["pos_" + strand].astype(np.int64) + o for r, o in zip(rows, offs)])
        score = np.concatenate([r["score_" + strand] for r in rows])
        tile = pos // TILE_CHARS[geometry]
        for t in np.unique(tile):
            out.setdefault(int(t), [np.empty(0), np.empty(0)])[j] = score[tile == t]
    return out


MARGIN = 16


def assert_condition(name, l, contigs, rows, first=64, ctx=None):
    """the condition a case is named for, in both geometries, from the oracle's rows"""
    for geometry in sorted(TILE_CHARS):
        tiles = tile_rows(contigs, rows, geometry, first)
        cap = LIST[geometry]
        counts = {t: (p.size, m.size) for t, (p, m) in tiles.items()}
        where = (name, l, geometry, ctx, counts)
        if name == "plus_only":
            assert all(m == 0 for _, m in counts.values()), where
            assert any(BLOCK < p <= cap - MARGIN for p, _ in counts.values()), where
        elif name == "minus_only":
            assert all(p == 0 for p, _ in counts.values()), where
            assert any(BLOCK < m <= cap - MARGIN for _, m in counts.values()), where
        elif name == "mixed_seam":
            (p, m), = counts.values()  # one tile
            assert p % 64 not in (0, 1, 63) and m > 64 and p + m <= cap, where
        elif name == "by_strand":
            assert any(p + m >= cap + MARGIN and p <= cap - MARGIN and m <= cap - MARGIN for p, m in counts.values()), where
        elif name == "windowed":
            # some round of `cap` ranks begins below n_plus and ends above it, and a later round begins above n_plus
            def straddles(p, m):
                first_above = -(-p // cap) * cap
                return (p > cap and m > 0 and MARGIN <= p % cap <= cap - MARGIN and first_above + MARGIN <= p + m)
            assert any(straddles(p, m) for p, m in counts.values()), where
            assert any(m > cap + MARGIN for _, m in counts.values()), where
        elif name == "incomplete":
            assert len(counts) == 1, where
            for sp, sm in tiles.values():
                for strand, s, rank0 in (("plus", sp, 0), ("minus", sm, sp.size)):
                    chunk = (rank0 + np.arange(s.size)) // 64
                    unscored = s == -1.0
                    if l < 20:
                        assert s.size > 64 and unscored.all(), (where, strand)
                    elif l > 20 and strand == "plus":
                        # (a window can be cut to 30 only by the contig's END, which lies past a '+' row's PAM)
                        assert s.size > 64, (where, strand)
                    else:
                        both = [c for c in np.unique(chunk) if unscored[chunk == c].any() and not unscored[chunk == c].all()]
                        assert both, (where, strand)
        elif name == "mixed_chars":
            for strand, lo, hi in (("plus", -l - 5, 5), ("minus", -2, l + 8)):
                seen = set()
                for c, r in zip(contigs, rows):
                    for p in r["pos_" + strand][r["score_" + strand] != -1.0][:400].astype(np.int64):
                        seen |= set(c[p + lo:p + hi])
                assert seen >= set(b"acgtNRYUZ"), (where, strand, bytes(sorted(seen)))
                assert any((r["score_" + strand] != -1.0).sum() > 64 for r in rows), (where, strand)


@pytest.mark.parametrize("name,l", RUNS)
def test_cases_hold_their_conditions(oracle, name, l):
    assert_condition(name, l, contigs_of(name), oracle_rows(oracle, name, l))


# one genome for the pipelined scan: the tile-filling cases first, each long enough to fill a tile wherever it starts
STREAM_ORDER = ("windowed", "by_strand", "plus_only", "minus_only", "mixed_seam", "incomplete", "mixed_chars")


def test_stream_genome_holds_the_conditions(oracle):
    first = 64
    for name in STREAM_ORDER:
        contigs = contigs_of(name)
        if name not in ("mixed_seam", "incomplete"):  # (stated on a tile of their own: the case tests)
            assert_condition(name, 20, contigs, oracle_rows(oracle, name, 20), first, ctx="stream")
        first = arena_offsets(contigs, first)[1]


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


def assert_rows_equal(got, want, ctx, keys=None):
    for key in keys or sorted(want):
        g, w = got[key], want[key]
        assert g.shape == w.shape, (ctx, key, g.shape, w.shape)
        assert (bits(g) == bits(w)).all(), (ctx, key, int(np.flatnonzero(g != w)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,l", RUNS)
def test_rows_vs_oracle(engine, oracle, name, l, request):
    """positions, scores and the pre-sigmoid column of every row, and the table totals"""
    geometry = request.node.callspec.params["engine"].split("-")[1]
    contigs, want = contigs_of(name), oracle_rows(oracle, name, l)
    arena = engine.arena(contigs)
    try:
        tiles = arena.tiles()
        assert tiles["geometry"] == geometry and tiles["tile_words"] * 64 == TILE_CHARS[geometry]
        assert [int(o) for o in arena.offsets] == arena_offsets(contigs)[0]
        hits = arena.scan_score(l, want_pre=True)
        for k, w in enumerate(want):
            assert_rows_equal(hits.contig(k), w, (name, l, k))
        assert hits.n_plus == sum(w["pos_plus"].size for w in want)
        assert hits.n_minus == sum(w["pos_minus"].size for w in want)
    finally:
        arena.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed_chars", "incomplete", "windowed"])
def test_seed_words_vs_oracle(engine, oracle, name):
    """the seed-word variant of the kernel: a row's seed does not depend on whether its window is complete"""
    contigs, want = contigs_of(name), oracle_rows(oracle, name, 20)
    arena = engine.arena(contigs)
    try:
        n_plus, n_minus = arena.scan_score_device(20, want_pre=True, want_seeds=True)
        assert n_plus == sum(w["pos_plus"].size for w in want) and n_minus == sum(w["pos_minus"].size for w in want)
        engine.offtarget_reset()
        arena.offtarget_add(20)
        engine.offtarget_solve()
        sp, sm = arena.offtarget_seeds(n_plus, n_minus)
        assert (sp == np.concatenate([oracle.seed_codes(c, w["pos_plus"], False, 20) for c, w in zip(contigs, want)])).all()
        assert (sm == np.concatenate([oracle.seed_codes(c, w["pos_minus"], True, 20) for c, w in zip(contigs, want)])).all()
    finally:
        arena.close()


@pytest.mark.gpu
@pytest.mark.parametrize("l", [20, 23])
def test_pipelined_scan_vs_oracle(_engine, oracle, l):
    """the same kernel behind the pipelined scan: every case in one genome, one slice"""
    contigs, want = [], []
    for name in STREAM_ORDER:
        contigs += contigs_of(name)
        want += oracle_rows(oracle, name, l)
    hits = _engine.scan_stream(contigs, l, want_pre=False, density=0.5)
    assert hits.stream_stats["slices"] == 1, hits.stream_stats
    for k, w in enumerate(want):
        assert_rows_equal(hits.contig(k), w, ("stream", l, k), ("pos_plus", "score_plus", "pos_minus", "score_minus"))
    assert hits.n_plus + hits.n_minus == sum(w["pos_plus"].size + w["pos_minus"].size for w in want)
