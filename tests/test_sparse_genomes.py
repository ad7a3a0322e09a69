"""Sparse genomes: N runs and AT-only stretches of many tiles, one-strand stretches and tiles with a handful of rows
(tests/sparse_genome_cases.py) through the scan, the pipelined scan, the node handle's exchange, the annotation join, the
off-target seed scan and the guide search.  These are the inputs on which a tile publishes an aggregate and no prefix,
a look-back has to sum over hundreds of tiles, a bucket of the 16-bit position exchange has no row, a device's share no
hit and a chunk of the search no candidate.  Every comparison is exact, against the CPU oracle, the search references
or the numpy join; every condition a case is named for is asserted from the oracle's rows first.  The generator itself
is checked against the oracle without a GPU."""
import numpy as np
import pytest

import sparse_genome_cases as cases

_ROWS = {}
GEOMETRIES = {"large": cases.TILE_L, "small": cases.TILE_S}


def oracle_rows(oracle, case, l):
    """the oracle's rows of every contig of a case, computed once and shared (read-only)"""
    key = (case.name, case.tile_words, l)
    if key not in _ROWS:
        _ROWS[key] = [oracle.scan_score(c, l) for c in case.contigs]
    return _ROWS[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_named_condition(case, rows, block):
    """what the case is named for, from the oracle's rows and the arena layout alone"""
    name = case.name
    plus, minus = case.tile_counts(rows)
    both = plus + minus
    runs = cases.empty_runs(plus, minus)
    between = [(t, n) for t, n in runs if t > 0 and t + n < case.n_tiles]  # a populated tile on either side
    for seg in case.gap_segments():
        assert case.rows_inside(rows, seg) == 0, (name, seg)
    if name.startswith("gap_mid_"):
        assert between and max(n for _, n in between) >= 2, (name, runs)
        assert both[0] > 0 and both[-1] > 0
    elif name.startswith("gap_first_"):
        assert runs and runs[0][0] == 0 and runs[0][1] >= 2 and both[runs[0][1]] > 0, (name, runs)
    elif name.startswith("gap_last_"):
        t, n = runs[-1]
        assert t + n == case.n_tiles and n >= 3 and both[t - 1] > 0, (name, runs)
    elif name.startswith("lookback_"):
        want = int(name.split("_")[1])
        assert len(between) == 1 and between[0][1] >= want and between[0][1] <= want + 1, (name, runs)
    elif name == "one_strand":
        assert ((plus > 0) & (minus == 0)).sum() >= 2 and ((plus == 0) & (minus > 0)).sum() >= 2, (name, plus, minus)
        if case.tile_words == cases.TILE_S:
            # the alternating contig: five whole SMALL tiles, '-' only and '+' only by turns
            k, _, a, _ = [s for s in case.segments if s[0] == 2][1]
            assert (case.offsets[2] + a) % (64 * cases.TILE_S) == 0
            t = (case.offsets[2] + a) // (64 * cases.TILE_S)
            for j in range(5):
                own, other = (minus, plus) if j % 2 == 0 else (plus, minus)
                assert own[t + j] > 1000 and other[t + j] == 0, (name, j, plus[t + j], minus[t + j])
    elif name == "few_rows":
        assert (plus[0], minus[0]) == (1, 0) and (plus[1], minus[1]) == (0, 1) and both[2] == 0 and (plus[3], minus[3]) == (1, 0)
        # the single row of tile 3 lies in the tile's last owner wave: the last eighth of its words
        tc = 64 * case.tile_words
        p = int(rows[0]["pos_plus"][1]) + case.offsets[0]  # ('+' rows in position order: tile 0's, then tile 3's)
        assert p // tc == 3 and (p % tc) // 64 >= case.tile_words - case.tile_words // 8
        targets = cases.few_rows_targets(block)
        assert block % 64 == 0 and targets == [63, 64, 65, block - 64, block - 63, block, block + 1]
        assert [int(v) for v in both[4:4 + len(targets)]] == targets, (name, both[:12])
        assert all(plus[4 + j] > 0 and minus[4 + j] > 0 for j in range(len(targets)))
    else:
        raise AssertionError("no condition stated for " + name)


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
@pytest.mark.parametrize("name", cases.CASES)
def test_generator_against_oracle(oracle, name, geometry):
    """Every case shows, in the oracle's rows, what it is named for: no row inside an N run or an AT-only stretch, the
    run of empty tiles of the promised length with populated tiles around it, one-strand tiles, the exact row counts."""
    tw = GEOMETRIES[geometry]
    block = cases.emit_block_sizes()[tw]
    case = cases.build(name, tw)
    assert case.used == 1 + sum((len(c) + 63) // 64 + 1 for c in case.contigs)
    assert all(o % 64 == 0 for o in case.offsets)
    for l in cases.GUIDE_LENGTHS:
        assert_named_condition(case, oracle_rows(oracle, case, l), block)


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


def assert_rows_equal(got, want, ctx, keys=None):
    for key in keys or sorted(want):
        g, w = got[key], want[key]
        assert g.shape == w.shape, (ctx, key, g.shape, w.shape)
        assert (bits(g) == bits(w)).all(), (ctx, key, int(np.flatnonzero(g != w)[0]) if g.size else None)


@pytest.mark.gpu
@pytest.mark.parametrize("l", cases.GUIDE_LENGTHS)
@pytest.mark.parametrize("name", cases.CASES)
def test_scan_vs_oracle(engine, oracle, name, l, request):
    """A. every case in both scan modes and both geometries: all columns, the table totals, the tile count -- and for
    l = 20 the seed words the scan hands to the off-target step.  (The look-back cases are laid out for the geometry
    they run in, like all others: the run of empty tiles is 70, 130 or 260 tiles of THAT geometry.)"""
    geometry = request.node.callspec.params["engine"].split("-")[1]
    tw = GEOMETRIES[geometry]
    case = cases.build(name, tw)
    want = oracle_rows(oracle, case, l)
    assert_named_condition(case, want, cases.emit_block_sizes()[tw])
    arena = engine.arena(case.contigs)
    try:
        tiles = arena.tiles()
        assert tiles["geometry"] == geometry and tiles["tile_words"] == tw
        assert arena.stats()["n_words"] == case.used and tiles["n_tiles"] == case.n_tiles
        assert [int(o) for o in arena.offsets] == case.offsets
        hits = arena.scan_score(l, want_pre=True)
        for k, w in enumerate(want):
            assert_rows_equal(hits.contig(k), w, (name, l, k))
        assert hits.n_plus == sum(w["pos_plus"].size for w in want)
        assert hits.n_minus == sum(w["pos_minus"].size for w in want)
        if l == 20:
            n_plus, n_minus = arena.scan_score_device(l, want_pre=True, want_seeds=True)
            assert (n_plus, n_minus) == (hits.n_plus, hits.n_minus)
            engine.offtarget_reset()
            arena.offtarget_add(l)
            engine.offtarget_solve()
            sp, sm = arena.offtarget_seeds(n_plus, n_minus)
            assert (sp == np.concatenate([oracle.seed_codes(c, w["pos_plus"], False, l) for c, w in zip(case.contigs, want)])).all()
            assert (sm == np.concatenate([oracle.seed_codes(c, w["pos_minus"], True, l) for c, w in zip(case.contigs, want)])).all()
    finally:
        arena.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,tile_words", [("gap_mid_nrun", cases.TILE_L), ("gap_mid_at", cases.TILE_L), ("lookback_130", cases.TILE_S)])
def test_stream_slices_inside_a_gap(_engine, oracle, name, tile_words):
    """B. the pipelined scan with slices a third of the gap long.  A slice owns fewer characters than slice_chars (the
    cut leaves room for the halo), so a stretch of 2 * slice_chars characters holds a whole slice and two slice
    boundaries: at least one slice has no hit at all."""
    case = cases.build(name, tile_words)
    (gap,) = case.gap_segments()
    slice_chars = (gap[3] - gap[2]) // 3 // 64 * 64
    total = len(case.contigs[0])
    for l in cases.GUIDE_LENGTHS:
        hits = _engine.scan_stream(case.contigs, l, want_pre=False, slice_chars=slice_chars)
        assert hits.stream_stats["slices"] >= -(-total // slice_chars) and gap[3] - gap[2] >= 2 * slice_chars + 64, hits.stream_stats
        want = oracle_rows(oracle, case, l)
        for k, w in enumerate(want):
            assert_rows_equal(hits.contig(k), w, (name, l, k), ("pos_plus", "score_plus", "pos_minus", "score_minus"))
        assert hits.n_plus + hits.n_minus == sum(w["pos_plus"].size + w["pos_minus"].size for w in want)


# ---- C. the node handle: shares without a hit, buckets of the 16-bit position exchange without a row
NODE_OPTIONS = ((20, {}), (20, {"pos16": False}), (20, {"root": -1}), (20, {"root": -1, "pos16": False}), (20, {"to_host": True}), (23, {}))


def check_node_genome(node, world, oracle, transport=None):
    """the node genome over `world` logical devices, every option of the exchange: the oracle's rows, bit for bit -- after
    the cut that was made and the oracle's rows have shown each condition of the exchange on some device"""
    import test_node as tn
    case = cases.node_genome()
    node.load(case.contigs)
    plan = node.plan()
    cond = cases.share_conditions(plan, oracle_rows(oracle, case, 20), world)
    assert all(cond[k] for k in ("no_hit", "empty_middle", "starts_in_gap", "ends_in_gap")), (world, cond, plan)
    assert len(cond["no_hit"]) >= world // 2  # (the genome's second half is one gap)
    total = 0
    for l, kw in NODE_OPTIONS:
        kw = dict(kw, root=world - 1) if "root" in kw else kw
        hits = node.scan(l, **kw)
        total += tn._check_against_oracle(hits, case.contigs, oracle, l, (world, l, kw))
        if transport is not None and not kw.get("to_host"):
            assert node.gather_stats()["transport"] == transport, node.gather_stats()
    return total, cond


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4, 7])
def test_node_shares_without_hits_and_empty_buckets(oracle, world):
    from cropsr_amd import node as nd
    with nd.Node([0] * world) as node:
        total, _ = check_node_genome(node, world, oracle)
    assert total > 5000


# ---- D. the annotation join: cut points inside buckets without a hit, features that begin and end in gaps
def _cut_sites(rows, l, text_len):
    """genome coordinates (dec = 1) of the rows that have a cut site, ascending"""
    out = []
    for strand, back in (("plus", 3), ("minus", 0)):
        p = rows["pos_" + strand].astype(np.int64)
        out.append((p - back)[rows["score_" + strand] != -1])
    return np.sort(np.concatenate(out))


def _gap_gff(name, case, rows, l):
    """hand-written features of one contig around its first gap: (type, first, last, id), coordinates 1-based as in a GFF
    (dec = 1: coordinate x is string index x, arena position offset + x)"""
    off = case.offsets[0]
    gap = case.gap_segments()[0] if case.gap_segments() else [s for s in case.segments if s[1] == "isolated"][2]
    g0, g1 = gap[2], gap[3]
    cuts = _cut_sites(rows[0], l, len(case.contigs[0]))
    before, after = int(cuts[cuts < g0][-1]), int(cuts[cuts >= g1][0])
    # (reaching the nearest cut site on either side, however far: few_rows has one row per tile there)
    feats = [("gene", min(g0 - 2000, before - 5), g0 + 1000, "ends_inside"), ("gene", g1 - 1000, max(g1 + 700, after + 5), "starts_inside"),
             ("gene", min(g0 - 5000, before - 9), max(g1 + 5000, after + 9), "spans"), ("CDS", g0 + 10, g1 - 10, "inside"),
             ("CDS", after, after + 100, "starts_on_first_cut"), ("CDS", after + 1, after + 50, "starts_after_first_cut"),
             ("CDS", before - 100, before, "ends_on_last_cut"), ("CDS", before - 50, before - 1, "ends_before_last_cut")]
    # >= 40 cut points inside one 2 048-position bucket that lies wholly inside the gap
    kb = (off + g0) // 2048 + 2
    assert off + g0 <= 2048 * kb and 2048 * (kb + 1) <= off + g1
    for j in range(25):
        feats.append(("CDS", 2048 * kb - off + 8 + 80 * j, 2048 * kb - off + 8 + 80 * j + 30, "in_bucket_%d" % j))
    # points at arena positions 2048 k - 1, 2048 k, 2048 k + 1: a feature that begins at x puts a point at offset + x,
    # one that ends at x a point at offset + x + 1 -- in the dense part before the gap, at the gap's own bucket and after it
    for k in (3, (off + g0) // 2048 + 1, (off + g1) // 2048 + 2):
        for d in (-1, 0, 1):
            feats.append(("gene", 2048 * k + d - off, 2048 * k + d - off + 700, "b%d_%d" % (k, d + 1)))
            feats.append(("CDS", 2048 * k + d - off - 300, 2048 * k + d - off - 1, "e%d_%d" % (k, d + 1)))
    return [(name, t, a, b, "ID=" + i) for t, a, b, i in feats], (before, after)


@pytest.mark.gpu
def test_annotation_join_around_gaps(_engine, oracle, tmp_path):
    """gap_mid and few_rows (SMALL layout) and a contig the GFF does not know, in one arena: ids == the oracle's numpy
    join, strings == the brute-force rows; then the same tables against an empty track.  (l = 20: with any other guide
    length no row has a 30-character window, hence no cut site.)"""
    l = 20
    from cropsr_amd import annotate
    from oracle import annotate_oracle
    from test_annotate import _brute_rows, _strings_of
    parts = [cases.build("gap_mid_nrun", cases.TILE_S), cases.build("few_rows", cases.TILE_S), cases.build("gap_first_at", cases.TILE_S)]
    names = ["c0", "c1", "unknown"]
    texts = [p.contigs[0] for p in parts]
    feats = []
    for name, part in zip(names[:2], parts[:2]):
        rows = oracle_rows(oracle, part, l)
        f, (before, after) = _gap_gff(name, part, rows, l)
        feats += f
    path = str(tmp_path / "gaps.gff")
    with open(path, "w") as f:
        f.write("##gff-version 3\n")
        for row in feats:
            f.write("%s\tsrc\t%s\t%d\t%d\t.\t+\t.\t%s\n" % row)
        f.write("elsewhere\tsrc\tgene\t1\t100000\t.\t+\t.\tID=elsewhere\n")
    ann = annotate.Annotation(path)
    genome = _engine.genome(texts)
    try:
        hits = genome.scan_score(l, annotation=annotate.Request(ann, names, 1))
        n_labelled = 0
        for k, t in enumerate(texts):
            h = hits.contig(k)
            assert_rows_equal(h, oracle.scan_score(t, l), (l, k), ("pos_plus", "score_plus", "pos_minus", "score_minus"))
            want = annotate_oracle.host_join(ann, names[k], 0, 1, h, l, len(t))
            assert (h["feat_plus"] == want[0]).all() and (h["feat_minus"] == want[1]).all(), (l, k)
            got = _strings_of(ann, np.concatenate([h["feat_plus"], h["feat_minus"]]))
            assert got == _brute_rows([x for x in feats if x[0] == names[k]], None, h, l, len(t), 1), (l, k)
            n_labelled += sum(1 for s in got if s)
            if k == 2:
                assert not any(got)
            else:  # the rows on the features' ends carry them: the boundary cases are not vacuous
                joined = " ".join(got)
                for label in ("starts_on_first_cut", "ends_on_last_cut", "spans", "ends_inside", "starts_inside"):
                    assert label in joined, (l, k, label)
        assert n_labelled > 100
        # hits, but a track without a feature: every id is NO_FEATURE
        hits = genome.scan_score(l, annotation=annotate.Request(ann, ["x0", "x1", "x2"], 1))
        for k in range(3):
            h = hits.contig(k)
            assert h["feat_plus"].size + h["feat_minus"].size > 0
            assert (h["feat_plus"] == annotate.NO_FEATURE).all() and (h["feat_minus"] == annotate.NO_FEATURE).all()
    finally:
        genome.close()
        ann.close()


# ---- E. the off-target seed scan
def _offtarget(engine, contigs, l, seeds_from_scan):
    arena = engine.arena(contigs)
    try:
        n = arena.scan_score_device(l, want_seeds=seeds_from_scan)
        engine.offtarget_reset()
        sites = arena.offtarget_add(l)
        engine.offtarget_solve()
        cp, cm = arena.offtarget_counts(*n)
        sp, sm = arena.offtarget_seeds(*n)
        return n, sites, (cp, cm), (sp, sm), engine.offtarget_hist()
    finally:
        arena.close()


def _no_site_genome():
    """isolated sites whose 12 seed characters all hold an N: hits, but not one site"""
    rng = np.random.default_rng(77)
    out = []
    for k in range(2):
        a = rng.choice(np.frombuffer(b"ATat", dtype=np.uint8), 70_000 + 1000 * k)
        for j, p in enumerate(range(100, a.size - 100, 97)):
            if j % 2 == 0:
                a[p:p + 4] = np.frombuffer(b"AGGA", dtype=np.uint8)   # '+' row at p: its seed is p - 12 .. p - 1
                a[p - 1 - j % 12] = ord("N")
            else:
                a[p:p + 4] = np.frombuffer(b"TCCT", dtype=np.uint8)   # '-' row at p + 1: its seed is p + 4 .. p + 15
                a[p + 4 + j % 12] = ord("N")
        a[0] = ord("'")
        a[-3:] = np.frombuffer(b"')," if k == 0 else b"')]", dtype=np.uint8)
        out.append(a.tobytes())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("seeds", ["seeds_from_scan", "seeds_from_planes"])
def test_offtarget_on_sparse_genomes(_engine, oracle, seeds):
    from_scan = seeds == "seeds_from_scan"
    NOT = oracle.NOT_A_SITE
    for part in (cases.build("gap_mid_nrun", cases.TILE_S), cases.build("gap_mid_at", cases.TILE_L), cases.build("few_rows", cases.TILE_S),
                 cases.build("few_rows", cases.TILE_L)):
        want = oracle.offtarget_genome(part.contigs, 20)
        n, sites, counts, got_seeds, hist = _offtarget(_engine, part.contigs, 20, from_scan)
        for j, strand in enumerate(("plus", "minus")):
            ws = np.concatenate([w["seed_" + strand] for w in want])
            assert got_seeds[j].shape == ws.shape and (got_seeds[j] == ws).all(), (part.name, strand)
            wc = np.concatenate([w["ot_" + strand] for w in want])
            assert counts[j].shape == wc.shape and (counts[j] == wc).all(), (part.name, strand)
        codes = np.concatenate([np.concatenate([w["seed_plus"], w["seed_minus"]]) for w in want])
        assert sites == int((codes != NOT).sum()) and (hist == oracle.offtarget_hist([codes])).all(), part.name
    # hits, but every one has an N among its 12 seed characters
    contigs = _no_site_genome()
    want = oracle.offtarget_genome(contigs, 20)
    codes = np.concatenate([np.concatenate([w["seed_plus"], w["seed_minus"]]) for w in want])
    assert codes.size > 1000 and (codes == NOT).all()
    n, sites, counts, got_seeds, hist = _offtarget(_engine, contigs, 20, from_scan)
    assert n[0] + n[1] == codes.size and n[0] > 300 and n[1] > 300 and sites == 0
    assert (counts[0] == 0xFFFFFFFF).all() and (counts[1] == 0xFFFFFFFF).all() and counts[0].shape == (n[0], 4)
    assert (got_seeds[0] == NOT).all() and (got_seeds[1] == NOT).all() and not hist.any()
    # no hit at all
    empty = cases.Case("no_hit", cases.TILE_S, [[("at", 50_000), ("nrun", 90_000)], [("nrun", 40_000), ("at", 3_000)]], 5).contigs
    assert all(w["pos_plus"].size + w["pos_minus"].size == 0 for w in (oracle.scan_score(c, 20) for c in empty))
    n, sites, counts, got_seeds, hist = _offtarget(_engine, empty, 20, from_scan)
    assert n == (0, 0) and sites == 0 and counts[0].shape == (0, 4) and counts[1].shape == (0, 4) and not hist.any()


# ---- F. the search of given guides: workgroups, chunks and whole arenas without a candidate
SPCAS9 = "N" * 21 + "GG"
SEARCH_WORDS = 256  # arena words per workgroup of the extraction kernels (crp_search.h)


def _as_tuples(sites):
    return list(zip(sites["query"].tolist(), sites["contig"].tolist(), sites["position"].tolist(),
                    (sites["strand"] == b"-").astype(int).tolist(), sites["mismatches"].tolist()))


def _guides_from(case, rows, n, width):
    """n guides of `width` letters cut from the dense parts: the letters in front of '+' rows (soft-masked ones in upper
    case), where they hold no N"""
    text = case.contigs[0]
    out = []
    for p in rows[0]["pos_plus"].astype(np.int64).tolist()[::7]:
        g = text[p - 20:p - 20 + width].decode().upper()
        if p >= 40 and len(g) == width and set(g) <= set("ACGT") and g not in out:
            out.append(g)
        if len(out) == n:
            return out
    raise AssertionError("too few guides")


@pytest.mark.gpu
@pytest.mark.parametrize("gap", cases.GAP_KINDS)
def test_search_over_a_gap(_engine, oracle, gap):
    """N x 21 + GG, eight guides, up to three mismatches over gap_mid: the gap is longer than two extraction workgroups,
    so some have no candidate; counts and sites == the reference's, with the default budget and the smallest one."""
    import search_reference as ref
    from cropsr_amd import search as srch
    case = cases.build("gap_mid_" + gap, cases.TILE_S)
    (seg,) = case.gap_segments()
    assert seg[3] - seg[2] >= 3 * 64 * SEARCH_WORDS
    queries = [srch.check_query(SPCAS9, g, 3) for g in _guides_from(case, oracle_rows(oracle, case, 20), 8, 20)]
    want_counts, s = ref.search(case.contigs, SPCAS9, queries, 3)
    want = sorted(zip(*[s[f].tolist() for f in ref.SITE_FIELDS]))
    assert len(want) >= 8
    g = _engine.genome(case.contigs)
    try:
        for budget in (None, 1):
            res = g.search(SPCAS9, queries, 3, budget=budget)
            assert (res.counts == want_counts).all() and _as_tuples(res.sites) == want, budget
        assert sum(res.candidates) > 0
    finally:
        g.close()


@pytest.mark.gpu
def test_search_all_n_pattern_over_an_n_run(_engine, oracle):
    """N x 23: every window without a void is a candidate, those inside the N run too (every nb bit set).  Counts and sites
    == the reference's in chunks of one workgroup; no site of an ACGT guide lies inside the run at three mismatches."""
    import search_reference as ref
    from cropsr_amd import search as srch
    case = cases.build("gap_mid_nrun", cases.TILE_S)
    (seg,) = case.gap_segments()
    pattern = "N" * 23
    queries = _guides_from(case, oracle_rows(oracle, case, 20), 8, 23)
    want_counts, s = ref.search(case.contigs, pattern, queries, 3)
    want = sorted(zip(*[s[f].tolist() for f in ref.SITE_FIELDS]))
    assert len(want) >= 8 and not [w for w in want if seg[2] <= w[2] and w[2] + 23 <= seg[3]]
    g = _engine.genome(case.contigs)
    try:
        for budget in (None, 1):
            res = g.search(pattern, queries, 3, budget=budget)
            assert (res.counts == want_counts).all() and _as_tuples(res.sites) == want, budget
            assert tuple(res.candidates) == (len(case.contigs[0]) - 22,) * 2  # the windows of the run are candidates
        h = srch.ArenaSearch(g.arenas[0], pattern, budget=1)
        try:
            h.run(queries[:1], 3, 1 << 30)
            assert h.stats()["chunks"] >= (seg[3] - seg[2]) // (64 * SEARCH_WORDS)  # whole chunks inside the run
        finally:
            h.close()
    finally:
        g.close()


@pytest.mark.gpu
def test_search_genome_without_a_candidate(_engine):
    """AT-only sequence and N runs under N x 21 + GG: no candidate in the arena (its one chunk is empty).  All counts zero,
    no site, no error -- plain, scheme-scored, pair-table, with a bulge, and the self search."""
    import search_reference as ref
    from cropsr_amd import search as srch
    contigs = cases.Case("no_candidate", cases.TILE_S, [[("at", 40_000), ("nrun", 70_000), ("at", 9_000)], [("nrun", 30_000)]], 6).contigs
    queries = ["ACGTTGCAACGTTGCAACGT", "GATTACAGATTACAGATTAC", "A" * 20, "T" * 20]
    checked = [srch.check_query(SPCAS9, q, 3) for q in queries]
    want_counts, s = ref.search(contigs, SPCAS9, checked, 3)
    assert not want_counts.any() and s["query"].size == 0
    pair = np.full((20, 4, 4), 0.5)
    pair[:, np.arange(4), np.arange(4)] = 1.0
    g = _engine.genome(contigs)
    try:
        for budget in (None, 1):
            for score in (None, "hsu2013", srch.PairTable(pair)):
                res = g.search(SPCAS9, queries, 3, budget=budget, pam_len=3, score=score)
                assert res.counts.shape == (4, 4) and not res.counts.any() and res.sites.size == 0 and tuple(res.candidates) == (0, 0)
                if score is not None:
                    assert not res.hit_sum.any()
        res = g.search_bulges(SPCAS9, queries, 3, 3, 1, 0)
        assert not res.counts.any() and res.sites.size == 0
        res = g.search_self(SPCAS9, 3, 3)
        assert len(res.sites) == 0 and res.counts.shape[0] == 0 and tuple(res.candidates) == (0, 0)
    finally:
        g.close()
