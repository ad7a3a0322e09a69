"""The off-target seed scan (crp_offtarget.hip) on planted genomes (tests/offtarget_partition_cases.py): strand tables
exactly on, below and above the partition's units (OT_STAGE, OT_CHUNK), site counts on those edges below larger row
counts and over scratch that holds older codes, one-seed / two-seed / ladder histograms, Hamming families with prime
multiplicities, an arbitrary histogram through Engine.offtarget_hist(new), and the half-open edges of own_ranges.

  A  row counts on the edges, every row a site       D  Hamming families around two centres
  B  site counts on the edges, fewer sites than rows E  an arbitrary histogram through the setter
  C  skewed seed distributions                       F  ownership ranges

The CPU tests state, from the oracle alone, that every case holds the numbers it was built for.  The GPU tests compare,
exactly: both seed columns with the oracle's, `sites` with the number of codes that are neither 0xFFFFFFFF nor
0xFFFFFFFE, the whole 4^12 histogram with oracle.offtarget_hist, and the four counts of every row with
oracle.offtarget_enum -- and, up to 40 000 codes, with the definition, oracle.offtarget_pairs (cases.reference).
Every GPU case runs with both seed sources: the scan's seed words (want_seeds) and the planes.
"""
import numpy as np
import pytest

import offtarget_partition_cases as cases
from offtarget_partition_cases import C, NOT_A_SITE, NOT_OWNED, S

gpu = pytest.mark.gpu
SOURCES = ["seeds_from_scan", "seeds_from_planes"]
ALL_ONES = 0xFFFFFFFF


def _is_site(codes):
    return (codes != NOT_A_SITE) & (codes != NOT_OWNED)


def _planted_as_the_oracle_reads_it(case, oracle, l=None):
    """the oracle's rows are the plants, one row each, with the planted seeds; returns them"""
    r = case.rows(oracle, l)
    for strand, at in (("plus", case.at_plus), ("minus", case.at_minus)):
        plan = getattr(case, "plan_" + strand)
        assert r["seed_" + strand].shape == plan.shape and (r["seed_" + strand] == plan).all(), (case.name, strand)
        for k, pos in enumerate(r["pos_" + strand]):
            assert (pos == at[at[:, 0] == k, 1]).all(), (case.name, strand, k)
    return r


# ------------------------------------------------------------------------------- CPU: the cases hold their numbers
def test_letters_and_plantable_codes(oracle):
    assert cases.letters_for(cases.code_of([3, 2, 1, 0] * 3), "-") == b"GCTA" * 3
    assert cases.letters_for(cases.code_of([3, 2, 1, 0] * 3), "+") == b"TAGC" * 3  # reversed and complemented
    assert cases.plantable(cases.LOWEST) and cases.plantable(cases.HIGHEST) and cases.LOWEST == 0
    assert not cases.plantable(cases.code_of([0] * 5 + [3, 3] + [0] * 5)) and not cases.plantable(cases.code_of([2, 2] + [1] * 10))
    for lo in range(cases.HIGHEST + 1, cases.N_SEEDS, 1 << 18):  # no plantable code above HIGHEST
        assert not cases.plantable_mask(np.arange(lo, min(lo + (1 << 18), cases.N_SEEDS))).any()
    # one plant of each strand, read by the oracle: the letters give the code, on its own row
    code = cases.code_of([3, 0, 2, 1, 1, 3, 0, 2, 0, 1, 2, 3])
    for strand, minus in (("+", False), ("-", True)):
        text = b"'" + b"AT" * 20 + (cases.letters_for(code, "+") + b"AGGA" if not minus else b"TCCT" + cases.letters_for(code, "-")) + b"TA" * 20 + b"')]"
        plus, minus_rows = oracle.scan(text, 20)
        rows = minus_rows if minus else plus
        assert plus.size + minus_rows.size == 1 and rows.size == 1
        assert oracle.seed_codes(text, rows, minus, 20)[0] == code


@pytest.mark.parametrize("n_plus,n_minus", cases.EDGE_ROWS)
def test_case_a_row_counts(oracle, n_plus, n_minus):
    case = cases.edge_rows(n_plus, n_minus)
    r = _planted_as_the_oracle_reads_it(case, oracle)
    assert (r["seed_plus"].size, r["seed_minus"].size) == (n_plus, n_minus)
    assert _is_site(r["seed_plus"]).all() and _is_site(r["seed_minus"]).all()
    if (n_plus, n_minus) == cases.LARGEST:  # the same rows at l = 23
        r = _planted_as_the_oracle_reads_it(case, oracle, 23)
        assert (r["seed_plus"].size, r["seed_minus"].size) == (n_plus, n_minus)


def test_case_a_covers_the_edges():
    rows = cases.EDGE_ROWS
    assert rows == [(8191, 8193), (8192, 16384), (16383, 16385), (16386, 3), (40963, 1), (0, 16385), (5, 0), (3, 16386)]
    for s in (0, 1):
        assert {r[s] % 4 for r in rows if r[s]} == {0, 1, 2, 3}
    assert {S - 1, S, S + 1, C - 1, C, C + 1} <= {r[0] for r in rows} | {r[1] for r in rows}
    assert any(a > b > 0 for a, b in rows) and any(0 < a < b for a, b in rows) and any(a == 0 for a, _ in rows) and any(b == 0 for _, b in rows)
    assert cases.LARGEST == max(rows) and cases.PROBE in rows and max(cases.LARGEST) > cases.SITE_ROWS  # B's scratch is older and longer


@pytest.mark.parametrize("m", cases.SITE_COUNTS)
def test_case_b_site_counts(oracle, m):
    case = cases.edge_sites(m)
    r = _planted_as_the_oracle_reads_it(case, oracle)
    for strand in ("plus", "minus"):
        codes = r["seed_" + strand]
        site = _is_site(codes)
        assert codes.size == cases.SITE_ROWS == 2 * C + 5 and int(site.sum()) == m and (codes[~site] == NOT_A_SITE).all()
        # the non-sites are scattered through the table: some in every third of it, and sites behind them
        third = codes.size // 3
        assert all((~site[k * third:(k + 1) * third]).any() for k in range(3)) and (~site[:np.flatnonzero(site)[-1]]).any()


@pytest.mark.parametrize("m", cases.OWNED_SITE_COUNTS)
def test_case_b_owned_site_counts(oracle, m):
    case, ranges = cases.edge_sites_owned(m)
    r = _planted_as_the_oracle_reads_it(case, oracle)
    assert ranges.shape == (5, 2) and (ranges[1:, 0] > ranges[:-1, 1]).all()
    for strand in ("plus", "minus"):
        assert r["seed_" + strand].size == cases.SITE_ROWS and _is_site(r["seed_" + strand]).all()
        own = cases.owned_mask(r["pos_" + strand][0], ranges)
        assert int(own.sum()) == m and own[0] and own[-1] and not own[cases.SITE_ROWS // 2]


def test_case_c_one_seed_and_two_seeds(oracle):
    case = cases.one_seed()
    r = _planted_as_the_oracle_reads_it(case, oracle)
    assert (r["seed_plus"].size, r["seed_minus"].size) == cases.ONE_SEED_ROWS == (C + S + 5, S + 1)
    for strand in ("plus", "minus"):  # one bucket, more than one trip of the histogram's 8 x 1024 loop, on each strand
        assert (r["seed_" + strand] == cases.ONE_SEED).all() and r["seed_" + strand].size > 8 * 1024
    case = cases.two_seeds()
    r = _planted_as_the_oracle_reads_it(case, oracle)
    assert (r["seed_plus"].size, r["seed_minus"].size) == cases.TWO_SEED_ROWS
    for strand in ("plus", "minus"):
        assert set(np.unique(r["seed_" + strand]).tolist()) == {cases.LOWEST, cases.HIGHEST}
    assert cases.LOWEST >> 12 == 0 and cases.HIGHEST >> 18 == 59 and cases.HIGHEST == 0xEEEEEE


def test_case_c_ladder(oracle):
    case = cases.ladder()
    r = _planted_as_the_oracle_reads_it(case, oracle)
    buckets, cp, cm = cases.ladder_plan()
    assert buckets.size >= 300 and (np.diff(buckets.astype(np.int64)) > 0).all()
    for strand, plan in (("plus", cp), ("minus", cm)):
        codes = r["seed_" + strand]
        assert _is_site(codes).all()
        per_bucket = np.bincount(codes >> 12, minlength=cases.BUCKETS)
        assert (per_bucket[buckets] == plan).all() and per_bucket.sum() == plan.sum()  # nothing outside the ladder
        assert sorted(set(plan.tolist())) == list(range(18)) and int((plan > 0).sum()) >= 300
        occupied = np.flatnonzero(per_bucket)
        assert (np.diff(occupied) > 1).any()  # empty buckets between occupied ones
        start = np.concatenate([[0], np.cumsum(per_bucket)])[:-1]
        for length in (1, 7, 8, 9, 15, 16, 17):  # each length begins at every residue of the 16-byte body
            assert {int(x) % 8 for x in start[per_bucket == length]} == set(range(8)), (strand, length)
        # inside a bucket: several low-12-bit values, some of them more than once
        for b in buckets[plan >= 6][:40].tolist():
            values, copies = np.unique(codes[codes >> 12 == b] & 0xFFF, return_counts=True)
            assert values.size >= 3 and copies.max() >= 2
        order = (codes >> 12).astype(np.int64)
        assert (np.diff(order) < 0).sum() > order.size // 3  # table order is not bucket order
    # case C4: the contigs fall into three arenas of case.max_words words
    assert len(case.contigs) == 6 and cases.ladder() is case
    groups, used = 1, 1
    for c in case.contigs:
        need = (len(c) + 63) // 64 + 1
        if used + need > case.max_words:
            groups, used = groups + 1, 1
        used += need
    assert groups == 3


def test_case_d_families(oracle):
    case = cases.families()
    r = _planted_as_the_oracle_reads_it(case, oracle)
    codes = np.concatenate([r["seed_plus"], r["seed_minus"]])
    assert codes.size <= cases.PAIRS_LIMIT and r["seed_plus"].size > 1000 and r["seed_minus"].size > 1000
    plan = cases.family_plan()
    mult = cases.family_multiplicity()
    assert len(mult) == 2 * (1 + len(cases.CHANGED)) and dict(zip(*[x.tolist() for x in np.unique(codes, return_counts=True)])) == mult
    assert plan[0][0] >> 12 == 0 and cases.seed_distance(plan[0][0], plan[1][0]) == 12  # bucket 0; the families do not meet
    want = cases.family_counts(mult)
    for centre, members in plan:
        copies = [c for _, _, c in members]
        assert len(set(copies)) == len(copies) and set(copies) <= set(cases.PRIMES) and min(copies) >= 7 and max(copies) <= 97
        by_distance = [0, 0, 0, 0, 0]
        for x, where, c in members:
            assert cases.seed_distance(centre, x) == len(where) and all(((centre ^ x) >> (2 * k)) & 3 for k in where)
            by_distance[len(where)] += c
        assert by_distance[4] > 0  # there, and never counted:
        assert want[centre] == [cases.CENTRE_COPIES - 1] + by_distance[1:4]
    assert {w for w in cases.CHANGED if len(w) > 1 and len({k // 4 for k in w}) > 1} >= {(3, 4), (7, 8), (0, 11), (3, 4, 8), (0, 5, 11)}
    assert all(any(len(w) == d and {k // 4 for k in w} == {p} for w in cases.CHANGED) for d in (1, 2, 3, 4) for p in (0, 1, 2))
    # the definition, on all codes, gives what plain Python gives from the multiplicities
    pairs = oracle.offtarget_pairs(codes)
    assert (pairs == np.array([want[c] for c in codes.tolist()], dtype=np.uint32)).all()
    assert (pairs == np.concatenate([case.expected(oracle)["ot_plus"], case.expected(oracle)["ot_minus"]])).all()


def test_case_e_histogram(oracle):
    case, r, h, ref = cases.probe_reference(oracle)
    probes = np.concatenate([r["seed_plus"], r["seed_minus"]])
    assert case is cases.edge_rows(C - 1, C + 1)
    assert h.dtype == np.uint32 and h.shape == (cases.N_SEEDS,) and (h[probes] >= 1).all()
    assert int((h == 600_000).sum()) == 10 and int(h[h != 600_000].max()) == 255 and int(h.min()) == 0
    assert abs(float(h[h != 600_000].mean()) - 127.5) < 0.1 and (np.bincount(h[h != 600_000], minlength=256) > 60000).all()
    assert 6571 * 255 + 10 * 600_000 < 2 ** 32  # no ball sum can reach 2^32
    counts = np.concatenate([ref["ot_plus"], ref["ot_minus"]])
    assert int(counts.max()) < 6571 * 255 + 10 * 600_000 and int(counts[:, 1:].max()) >= 600_000  # a hot entry inside a probe's ball
    assert cases.arbitrary_hist(probes) is h


def test_case_f_ownership_edges(oracle):
    case = cases.owned_genome()
    r = _planted_as_the_oracle_reads_it(case, oracle)
    assert (r["seed_plus"].size, r["seed_minus"].size) == (cases.OWN_PLANTS, cases.OWN_PLANTS) == (3000, 3000)
    assert 50 < int((r["seed_plus"] == NOT_A_SITE).sum()) < 200  # a few non-sites: they stay 0xFFFFFFFF, owned or not
    rows = np.sort(np.concatenate([r["pos_plus"][0], r["pos_minus"][0]])).astype(np.int64)
    assert np.unique(rows).size == 6000
    sets = cases.ownership_sets(rows)
    assert list(sets) == cases.OWNERSHIP_SETS and sorted(len(v) for v in sets.values()) == [1, 1, 2, 3, 4, 5, 2000]
    total = dict.fromkeys(cases.EDGE_KINDS, 0)
    for name, ranges in sets.items():
        assert (ranges[:, 0] <= ranges[:, 1]).all() and (ranges[1:, 0] >= ranges[:-1, 1]).all(), name  # what offtarget_add takes
        for kind, n in cases.edge_kinds(rows, ranges).items():
            total[kind] += n
    assert all(total[kind] >= 1 for kind in cases.EDGE_KINDS), total
    kinds = {name: cases.edge_kinds(rows, sets[name]) for name in sets}
    owned = {name: int(cases.owned_mask(rows, sets[name]).sum()) for name in sets}
    assert owned == {"tight_1": 1, "end_begin_2": 1100, "adjacent_3": 2400, "empty_4": 110, "mixed_5": 1010, "many_2000": 4400, "empty_alone": 0}
    assert kinds["tight_1"]["tight"] == 1 and kinds["end_begin_2"]["at_end"] == 1 and kinds["end_begin_2"]["at_begin"] == 1
    assert kinds["adjacent_3"]["at_joint"] == 2 and kinds["empty_4"]["at_empty"] == 2 and kinds["empty_alone"]["at_empty"] == 1
    assert kinds["mixed_5"]["before_first"] == 10 and kinds["mixed_5"]["after_last"] == 10
    assert kinds["many_2000"]["at_end"] == 1600 and kinds["many_2000"]["at_joint"] == 400
    # the seeds repeat, so the counts depend on who is owned
    e = case.expected(oracle)
    assert int(e["ot_plus"][_is_site(r["seed_plus"]), 0].min()) >= 5 and int(e["ot_plus"][_is_site(r["seed_plus"]), 1].max()) >= 20


# ------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def _run(engine, contigs, l, from_scan, own=None, max_words=None, new_hist=None, n_arenas=1):
    """reset, scan + offtarget_add of every arena, [the histogram replaced,] solve, look-up.  own: ranges in positions of
    the (single) contig.  Returns dict(sites, hist, seed_plus, seed_minus, ot_plus, ot_minus), tables arena after arena."""
    genome = engine.genome(contigs, max_words=max_words)
    try:
        assert len(genome.arenas) == n_arenas
        engine.offtarget_reset()
        sites, n = 0, []
        for a in genome.arenas:
            n.append(a.scan_score_device(l, want_seeds=from_scan))
            sites += a.offtarget_add(l, None if own is None else own + int(a.offsets[0]))
        if new_hist is not None:
            engine.offtarget_hist(new_hist)
        hist = engine.offtarget_hist()
        engine.offtarget_solve()
        seeds = [a.offtarget_seeds(*k) for a, k in zip(genome.arenas, n)]
        counts = [a.offtarget_counts(*k) for a, k in zip(genome.arenas, n)]
        return dict(sites=sites, hist=hist, seed_plus=np.concatenate([s[0] for s in seeds]), seed_minus=np.concatenate([s[1] for s in seeds]),
                    ot_plus=np.concatenate([c[0] for c in counts]), ot_minus=np.concatenate([c[1] for c in counts]))
    finally:
        genome.close()


def _check(got, seed_plus, seed_minus, ref, what):
    """the comparisons of every case, all exact"""
    for strand, want in (("plus", seed_plus), ("minus", seed_minus)):
        g = got["seed_" + strand]
        assert g.shape == want.shape and (g == want).all(), (what, strand, "seeds")
    n_sites = int(_is_site(seed_plus).sum() + _is_site(seed_minus).sum())
    assert got["sites"] == n_sites == ref["sites"], (what, got["sites"], n_sites)
    assert (got["hist"] == ref["hist"]).all(), (what, "histogram", np.flatnonzero(got["hist"] != ref["hist"])[:8])
    for strand, seeds in (("plus", seed_plus), ("minus", seed_minus)):
        g, want = got["ot_" + strand], ref["ot_" + strand]
        assert g.shape == want.shape == (seeds.size, 4) and (g == want).all(), (what, strand, "counts", np.flatnonzero((g != want).any(axis=1))[:8])
        assert (g[~_is_site(seeds)] == ALL_ONES).all(), (what, strand)


def _run_case(engine, oracle, case, source, l=None, **kw):
    l = case.l if l is None else l
    r, ref = case.rows(oracle, l), case.expected(oracle, l)
    got = _run(engine, case.contigs, l, source == "seeds_from_scan", **kw)
    _check(got, r["seed_plus"], r["seed_minus"], ref, (case.name, source, l))
    return got


@gpu
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("n_plus,n_minus", cases.EDGE_ROWS)
def test_gpu_row_counts_on_the_edges(engine, oracle, n_plus, n_minus, source):
    _run_case(engine, oracle, cases.edge_rows(n_plus, n_minus), source)


@gpu
def test_gpu_largest_table_at_guide_length_23(engine, oracle):
    """l != 20: the seeds come from the planes whatever the scan wrote"""
    _run_case(engine, oracle, cases.edge_rows(*cases.LARGEST), "seeds_from_planes", l=23)


@gpu
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("m", cases.SITE_COUNTS)
def test_gpu_site_counts_on_the_edges(engine, oracle, m, source):
    """m sites in tables of 2C + 5 rows, after a run that left 2C + S + 3 valid codes in the partition's scratch"""
    _run(engine, cases.edge_rows(*cases.LARGEST).contigs, 20, source == "seeds_from_scan")
    _run_case(engine, oracle, cases.edge_sites(m), source)


@gpu
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("m", cases.OWNED_SITE_COUNTS)
def test_gpu_owned_site_counts_on_the_edges(engine, oracle, m, source):
    """the same with own_ranges making the non-sites: every row has a seed, m of each strand are owned"""
    case, ranges = cases.edge_sites_owned(m)
    r = case.rows(oracle)
    sp, sm = (cases.owned_columns(r["seed_" + s], cases.owned_mask(r["pos_" + s][0], ranges)) for s in ("plus", "minus"))
    assert int((sp == NOT_OWNED).sum()) == int((sm == NOT_OWNED).sum()) == cases.SITE_ROWS - m
    _run(engine, cases.edge_rows(*cases.LARGEST).contigs, 20, source == "seeds_from_scan")
    got = _run(engine, case.contigs, 20, source == "seeds_from_scan", own=ranges)
    _check(got, sp, sm, cases.reference(oracle, sp, sm), (case.name, source))


@gpu
@pytest.mark.parametrize("source", SOURCES)
def test_gpu_one_seed(engine, oracle, source):
    case = cases.one_seed()
    got = _run_case(engine, oracle, case, source)
    m = sum(cases.ONE_SEED_ROWS)
    assert got["sites"] == m and got["hist"][cases.ONE_SEED] == m and int(got["hist"].astype(np.int64).sum()) == m
    for strand in ("plus", "minus"):
        assert (got["ot_" + strand] == np.array([m - 1, 0, 0, 0], dtype=np.uint32)).all()


@gpu
@pytest.mark.parametrize("source", SOURCES)
def test_gpu_two_seeds(engine, oracle, source):
    got = _run_case(engine, oracle, cases.two_seeds(), source)
    assert np.flatnonzero(got["hist"]).tolist() == [cases.LOWEST, cases.HIGHEST]


@gpu
@pytest.mark.parametrize("source", SOURCES)
def test_gpu_ladder_in_one_arena_and_in_three(engine, oracle, source):
    case = cases.ladder()
    one = _run_case(engine, oracle, case, source)
    three = _run_case(engine, oracle, case, source, max_words=case.max_words, n_arenas=3)
    for key in ("sites", "hist", "seed_plus", "seed_minus", "ot_plus", "ot_minus"):
        assert np.array_equal(one[key], three[key]), key


@gpu
@pytest.mark.parametrize("source", SOURCES)
def test_gpu_hamming_families(engine, oracle, source):
    """the reference is the definition (all pairs) on every code: cases.reference compares it with the enumeration"""
    case = cases.families()
    got = _run_case(engine, oracle, case, source)
    want = cases.family_counts(cases.family_multiplicity())
    for centre, _ in cases.family_plan():
        rows = np.flatnonzero(got["seed_plus"] == centre)
        assert rows.size > 100 and (got["ot_plus"][rows] == np.array(want[centre], dtype=np.uint32)).all()


@gpu
@pytest.mark.parametrize("source", SOURCES)
def test_gpu_arbitrary_histogram_through_the_setter(engine, oracle, source):
    from cropsr_amd import CropsrHipError
    case, r, h, ref = cases.probe_reference(oracle)
    got = _run(engine, case.contigs, 20, source == "seeds_from_scan", new_hist=h)
    assert got["hist"].dtype == h.dtype and got["hist"].tobytes() == h.tobytes()  # bit for bit
    _check(got, r["seed_plus"], r["seed_minus"], ref, ("arbitrary histogram", source))
    with pytest.raises(CropsrHipError):
        engine.offtarget_hist(h)  # solved: the histogram can no longer be replaced
    assert engine.offtarget_hist().tobytes() == h.tobytes()  # reading still works


@gpu
@pytest.mark.parametrize("source", SOURCES)
def test_gpu_ownership_ranges(engine, oracle, source):
    case = cases.owned_genome()
    r = case.rows(oracle)
    pos = {s: r["pos_" + s][0].astype(np.int64) for s in ("plus", "minus")}
    sets = dict(cases.ownership_sets(np.sort(np.concatenate([pos["plus"], pos["minus"]]))))
    sets["none"], sets["zero_length"] = None, np.zeros((0, 2), dtype=np.uint64)
    arena = engine.arena(case.contigs)
    try:
        n = arena.scan_score_device(20, want_seeds=source == "seeds_from_scan")
        off = int(arena.offsets[0])
        cols = arena.fetch(*n)
        assert n == (pos["plus"].size, pos["minus"].size)
        assert (cols[0].astype(np.int64) == pos["plus"] + off).all() and (cols[3].astype(np.int64) == pos["minus"] + off).all()
        for name, ranges in sets.items():
            everything = ranges is None or len(ranges) == 0
            own = {s: np.ones(pos[s].size, dtype=bool) if everything else cases.owned_mask(pos[s], ranges) for s in pos}
            sp, sm = (cases.owned_columns(r["seed_" + s], own[s]) for s in ("plus", "minus"))
            engine.offtarget_reset()
            sites = arena.offtarget_add(20, ranges if everything else ranges + off)
            hist = engine.offtarget_hist()
            engine.offtarget_solve()
            seeds, counts = arena.offtarget_seeds(*n), arena.offtarget_counts(*n)
            got = dict(sites=sites, hist=hist, seed_plus=seeds[0], seed_minus=seeds[1], ot_plus=counts[0], ot_minus=counts[1])
            _check(got, sp, sm, cases.reference(oracle, sp, sm), ("ownership", name, source))
            assert sites == int((own["plus"] & (r["seed_plus"] != NOT_A_SITE)).sum() + (own["minus"] & (r["seed_minus"] != NOT_A_SITE)).sum())
            if name == "empty_alone":
                assert sites == 0 and not hist.any()
    finally:
        arena.close()
