"""The off-target search at the limits of its pattern geometry: T = 32 with the PAM on either
side, T = 31, guide regions of 31 down to 1 letters, patterns without a PAM, bulge windows of 32 letters.  The case table
and the planted genomes are in search_geometry_cases.py; the PAM's length is passed everywhere.

Without a GPU: the references themselves at these shapes (each against its plain statement), the host's value functions,
the refusals.  On the GPU: given guides (plain, scheme-scored, pair-table-scored, bulges), the self search and the
command line, every row and every sum against the reference, exact integers throughout."""
import functools
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import search_bulge_reference as bref
import search_geometry_cases as geo
import search_pair_reference as pref
import search_reference as ref
import search_score_reference as sref
import search_self_reference as selfref
from cropsr_amd import search as srch
from test_search_pair import _table_text

ONE = 1 << 30
BY_ID = {c.id: c for c in geo.ALL}
SELF_M = {"L3": 4, "L5": 4, "W3": 4, "W5": 4, "S5": 2, "S5'": 2, "S3": 0, "S2": 0}  # the largest M of a case's self search


def _m_values(case):
    return sorted({0, min(1, case.G), min(8, case.G)})


def _seed(case, salt):
    return [salt, sum(ord(ch) * (k + 1) for k, ch in enumerate(case.id))]


@functools.lru_cache(maxsize=None)
def _guides_case(cid, tiny=False):
    """(queries, contigs, plants) of a case's given-guides runs; tiny: the inputs of the CPU tests."""
    case = BY_ID[cid]
    rng = np.random.default_rng(_seed(case, 2 if tiny else 1))
    queries = geo.make_queries(case, rng, 2 if tiny else 3)
    contigs, plants = geo.build_genome(case, queries, 0 if tiny else geo.CHARS[cid], rng)
    return queries, contigs, plants


@functools.lru_cache(maxsize=None)
def _self_genome(cid, tiny=False):
    case = BY_ID[cid]
    rng = np.random.default_rng(_seed(case, 4 if tiny else 3))
    queries = geo.make_queries(case, rng, 1 if tiny else 2)
    return queries, geo.build_genome(case, queries, 0 if tiny else geo.SELF_CHARS[cid], rng)[0]


def _assert_plants_are_hit(case, contigs, plants, rows):
    """What keeps a given-guides comparison from passing on nothing: the reference's own rows hold a hit on each strand,
    at position 0, at the last possible start, astride a word boundary and (a long contig 0) astride both planted
    workgroup boundaries."""
    hit = {(q, k, pos, strand) for q, k, pos, strand, _ in rows}
    assert {r[3] for r in rows} == {0, 1}
    for q, tag, k, at, strand in plants:
        if tag.startswith("at-") or tag in ("word", "group", "exact"):
            assert (q, k, at, strand) in hit, (case, tag, q, at)
    tags = {tag: (k, at) for q, tag, k, at, strand in plants}
    assert tags["at-0"][1] == 0 and tags["at-end"][1] == len(contigs[tags["at-end"][0]]) - case.T
    if case.T >= 2:
        assert geo.straddles(tags["word"][1], case.T, 0, geo.WORD)
        if len(contigs[0]) > geo.GROUP + case.T:
            ats = [at for q, tag, k, at, strand in plants if tag == "group"]
            assert any(geo.straddles(at, case.T, 0, geo.GROUP) for at in ats)
            assert any(geo.straddles(at, case.T, geo.WORD, geo.GROUP) for at in ats)


def _assert_masks_reach_the_ends(case, masks):
    masks = [int(m) for m in masks]
    assert any(m & 1 for m in masks) and any(m >> (case.G - 1) & 1 for m in masks), case
    if case.G >= 2:
        assert any(m & 1 and m >> (case.G - 1) & 1 for m in masks), case  # d = G - 1


# ------------------------------------------------------------------ the references at these shapes (CPU)
@pytest.mark.parametrize("cid", [c.id for c in geo.ALL])
def test_reference_agrees_with_plain_statement(cid):
    case = BY_ID[cid]
    queries, contigs, plants = _guides_case(cid, True)
    M = min(8, case.G)
    counts, s = ref.search(contigs, case.pattern, queries, M)
    got = geo.rows_of(s)
    assert got == ref.search_slow(contigs, case.pattern, queries, M)
    _assert_plants_are_hit(case, contigs, plants, got)
    for q in range(len(queries)):
        assert counts[q].tolist() == [sum(1 for r in got if r[0] == q and r[4] == k) for k in range(M + 1)]
    if case.T >= 28:  # nothing but the copies at these lengths: every variant is found with the mismatches it was given
        want = {"exact": 0, "first": 1, "last": 1, "n-first": 1, "n-last": 1, "ends": 2, "ends+1": 3, "ends+2": 4, "ends+6": 8}
        mm_at = {r[:4]: r[4] for r in got}
        for q, tag, k, at, strand in plants:
            if tag in want:
                assert mm_at[(q, k, at, strand)] == want[tag], (cid, tag)


def test_score_values_agree_with_the_loop_at_wide_regions():
    rng = np.random.default_rng(31)
    for G in (31, 30, 29, 28):
        weights = np.round(rng.random(G), 3)
        weights[[0, G // 2]] = 0.0, 1.0
        weights = weights.tolist()
        factor, shape = sref.tables(weights)
        top = 1 << (G - 1)
        masks = [0, 1, top, 1 | top, 3, 3 << (G - 2), 0xFF, 0xFF << (G - 8), 0x7F | top, 1 | 0x7F << (G - 7)]
        for n in range(1, 9):
            for _ in range(40):
                masks.append(sum(1 << int(g) for g in rng.choice(G, n, replace=False)))
            for _ in range(10):  # n = 8 and fewer with both ends set
                masks.append(1 | top | sum(1 << int(g) for g in rng.choice(np.arange(1, G - 1), max(0, n - 2), replace=False)))
        v = sref.values(masks, factor, shape)
        for m, got in zip(masks, v.tolist()):
            assert sref.value_loop(m, weights, factor, shape)[0] == got, (G, bin(m))
        assert sum(1 for m in masks if bin(m).count("1") == 8 and m & 1 and m & top) >= 10 and int((v > 0).sum()) > 100
        for pattern, P in (("N" * G + "G" * (32 - G), 32 - G), ("T" * (32 - G) + "N" * G, 32 - G)):
            sc = srch.make_scheme(pattern, P, weights)
            assert (sc.factor == factor).all() and (sc.shape == shape).all()
            assert (srch.mask_values(masks, sc) == v).all()


@pytest.mark.parametrize("cid", [c.id for c in geo.SCORED])
def test_scored_references_and_host_values_on_the_planted_sites(cid):
    """search_score_reference.search and search_pair_reference.search on the tiny planted genome: the planted sites'
    values against a direct call of the loops on their letters, and the host functions of search.py (site_masks,
    mask_values, site_codes, pair_values through hit_values) against both."""
    case = BY_ID[cid]
    queries, contigs, plants = _guides_case(cid, True)
    rng = np.random.default_rng(_seed(case, 5))
    M = min(8, case.G)
    weights = geo.weights_for(case, rng)
    factor, shape = sref.tables(weights)
    counts, s, hit_sum = sref.search(contigs, case.pattern, queries, M, case.P, factor, shape)
    assert sref.guide_positions(case.pattern, case.P) == case.gpos
    _assert_masks_reach_the_ends(case, s["mask"])
    sites = np.empty(s["query"].size, srch.SITE_DTYPE)
    for f in ref.SITE_FIELDS:
        sites[f] = s[f] if f != "strand" else np.where(s[f] == 0, b"+", b"-")
    sc = srch.make_scheme(case.pattern, case.P, weights)
    assert sc.g_positions().tolist() == case.gpos
    assert srch.site_masks(sites, queries, contigs, sc).tolist() == s["mask"].tolist()
    assert srch.hit_values(sites, queries, contigs, sc).tolist() == s["value"].tolist()
    assert [sref.value_loop(int(m), weights, factor, shape)[0] for m in s["mask"].tolist()] == s["value"].tolist()
    pair, offsets, pam = geo.table_for(case, rng)
    pcounts, ps, phit_sum = pref.search(contigs, case.pattern, queries, M, case.P, pair, offsets, pam)
    assert (pcounts == counts).all() and geo.rows_of(ps) == geo.rows_of(s)
    psc = srch.make_scheme(case.pattern, case.P, srch.PairTable(pair, offsets, pam))
    assert srch.hit_values(sites, queries, contigs, psc).tolist() == ps["value"].tolist()
    value_at = {r[:4]: v for r, v in zip(zip(*[ps[f].tolist() for f in ref.SITE_FIELDS]), ps["value"].tolist())}
    n_zero = n_pos = 0
    for q, tag, k, at, strand in plants:
        window = contigs[k][at:at + case.T].decode().upper()
        site = geo.rc(window) if strand else window  # (N stays N: a non-base)
        want = pref.value_loop(queries[q], site, case.pattern, case.P, pair, offsets, pam)
        assert value_at[(q, k, at, strand)] == want, (cid, tag)
        n_zero += tag.startswith("n-") and want == 0
        n_pos += want > 0
    assert n_zero >= 2 and n_pos >= 2
    for q in range(len(queries)):
        assert phit_sum[q] == sum(v for r, v in value_at.items() if r[0] == q)


@pytest.mark.parametrize("cid", list(SELF_M))
def test_self_reference_statements_agree(cid):
    case = BY_ID[cid]
    queries, contigs = _self_genome(cid, True)
    rng = np.random.default_rng(_seed(case, 6))
    weights = geo.weights_for(case, rng)
    for M in range(SELF_M[cid] + 1):
        a = selfref.search_self(contigs, case.pattern, M, case.P, None, weights)
        b = selfref.search_self_pairs(contigs, case.pattern, M, case.P, None, weights)
        assert a[0] == b[0] and a[1] == b[1] and len(a[0]) >= 8
        assert (a[2] == b[2]).all() and a[3] == b[3]
        c = geo.self_reference(contigs, case, M, weights)
        assert c[0] == a[0] and c[1] == a[1] and (c[2] == a[2]).all() and c[3] == a[3]
        plain = geo.self_reference(contigs, case, M)
        assert plain[:2] == a[:2] and (plain[2] == a[2]).all() and plain[3] is None
        if case.G >= 3:  # the pair-table form: the grouped sum against the given-guides loop reference, row by row
            pair, offsets, pam = geo.table_for(case, rng)
            sites, guides, counts, hit_sum = geo.self_pair_reference(contigs, case, M, pair, offsets, pam)
            assert sites == a[0] and guides == a[1] and (counts == a[2]).all()
            rows = list(range(0, len(sites), max(1, len(sites) // 12)))
            qs = [srch.check_query(case.pattern, guides[r], case.P) for r in rows]
            assert [hit_sum[r] for r in rows] == pref.search(contigs, case.pattern, qs, M, case.P, pair, offsets, pam)[2]
    if SELF_M[cid] >= 2:
        assert int(a[2][:, 1:].sum()) > 0 and sum(a[3]) > 0


def _distinct_guide(rng, n):
    """n letters, none equal to either of the two before it: a bulge then has one placement that pairs without a mismatch."""
    out = []
    for _ in range(n):
        out.append(str(rng.choice([b for b in "ACGT" if b not in out[-2:]])))
    return "".join(out)


def _bulge_sites(case, D, R, rng):
    """sites_of for build_genome: per kind the window that pairs with the query for a bulge at the first placement and
    at the last, each exact and with two substitutions; the unbulged variants as everywhere."""
    def sites_of(query):
        out = geo.variants(case, query, rng, counts=(4,))
        first, last = bref.span(case.pattern, case.P, query)
        for bulge, size in bref.kinds(D, R)[1:]:
            ss = bref.placements(first, last, bulge, size)
            for where, s in (("first", ss[0]), ("last", ss[-1])):
                for subs in (0, 2):
                    kp = bref.kind_pattern(case.pattern, case.P, bulge, size)
                    win = [str(rng.choice(list(geo.letters_of(c)))) for c in kp]
                    pairs = [(i, w) for i, w in bref.pairing(case.T, bulge, size, s) if query[i] in "ACGT"]
                    for i, w in pairs:
                        win[w] = query[i]
                    if bulge == "DNA":  # the unpaired letters: the last one differs from the query's letter before the bulge
                        win[s + size - 1] = str(rng.choice([b for b in "ACGT" if b != query[s - 1]]))
                    for j in rng.choice(len(pairs), subs, replace=False):
                        i, w = pairs[int(j)]
                        win[w] = str(rng.choice([b for b in "ACGT" if b != query[i]]))
                    out.append(("%s%d-%s-%d" % (bulge, size, where, subs), "".join(win)))
        return out
    return sites_of


@functools.lru_cache(maxsize=None)
def _bulge_case(index, tiny=False):
    case, D, R = geo.BULGES[index]
    rng = np.random.default_rng([7 + tiny, index])
    queries = []
    for k in range(1 if tiny else 2):
        q = ["N"] * case.T
        for p, ch in zip(sorted(case.gpos), _distinct_guide(rng, case.G)):
            q[p] = ch
        queries.append("".join(q))
    contigs, plants = geo.build_genome(case, queries, 0 if tiny else 20_000, rng, _bulge_sites(case, D, R, rng))
    return case, D, R, queries, contigs, plants


def _assert_bulge_rows_are_not_vacuous(case, D, R, queries, rows):
    kinds = bref.kinds(D, R)
    for q, query in enumerate(queries):
        first, last = bref.span(case.pattern, case.P, query)
        assert (first, last) == (min(case.gpos), max(case.gpos))  # the span reaches the region's last position
        for k, (bulge, size) in enumerate(kinds):
            at = {r[6] for r in rows if r[0] == q and r[1] == k}
            assert at, (case, bulge, size)
            if size:
                ss = bref.placements(first, last, bulge, size)
                assert ss[0] - first in at and ss[-1] - first in at, (case, bulge, size, sorted(at))


@pytest.mark.parametrize("index", range(len(geo.BULGES)))
def test_bulge_reference_agrees_with_plain_statement(index):
    case, D, R, queries, contigs, plants = _bulge_case(index, True)
    for M in (0, 2, 4):
        counts, s = bref.search(contigs, case.pattern, queries, M, case.P, D, R)
        got = geo.rows_of(s, bref.FIELDS)
        assert got == bref.search_slow(contigs, case.pattern, queries, M, case.P, D, R), (case, M)
        for k in range(1 + D + R):
            assert counts[0, k].tolist() == [sum(1 for r in got if r[1] == k and r[5] == m) for m in range(M + 1)]
    _assert_bulge_rows_are_not_vacuous(case, D, R, queries, got)
    assert srch.check_bulges(case.pattern, case.P, D, R) == (D, R)
    assert [srch.kind_pattern(case.pattern, case.P, *kd) for kd in srch.bulge_kinds(D, R)[1:]] == \
        [bref.kind_pattern(case.pattern, case.P, *kd) for kd in bref.kinds(D, R)[1:]]
    assert srch.query_spans(case.pattern, case.P, queries, D, R).tolist() == [list(bref.span(case.pattern, case.P, q)) for q in queries]


def test_refusals_at_the_limits():
    E = srch.SearchInputError
    for case, M in ((geo.S3, 1), (geo.S5, 3), (geo.S5P, 3), (geo.S2, 1)):  # G < M + 1
        with pytest.raises(E):
            srch.check_self(case.pattern, M, case.P)
        with pytest.raises(E):  # before the genome is touched (None has no arenas)
            srch.search_self(None, case.pattern, M, case.P)
    for cid, M in SELF_M.items():
        assert srch.check_self(BY_ID[cid].pattern, M, BY_ID[cid].P)[2:4] == (M, BY_ID[cid].P)
    for case in (geo.L3, geo.L5):  # T + D > 32
        query = geo.make_queries(case, np.random.default_rng(1), 1)
        for D in (1, 2):
            with pytest.raises(E):
                srch.check_bulges(case.pattern, case.P, D, 2)
            with pytest.raises(E):
                srch.search_bulges(None, case.pattern, query, 2, case.P, D, 2)
        assert srch.check_bulges(case.pattern, case.P, 0, 2) == (0, 2)
    with pytest.raises(E):
        srch.check_bulges(geo.B28.pattern, 3, 2, 0)  # 31 + 2
    assert srch.check_bulges(geo.B28.pattern, 3, 1, 2) == (1, 2)
    for pattern in ("N" * 30 + "NGG", "TTTV" + "N" * 29):  # T = 33
        with pytest.raises(E):
            srch.check_pattern(pattern)
        with pytest.raises(E):
            srch.check_self(pattern, 2, 3)
        with pytest.raises(E):
            srch.search(None, pattern, ["N" * 33], 2)
        with pytest.raises(E):
            srch.search_bulges(None, pattern, ["N" * 33], 2, 3, 0, 1)
    for case in geo.ALL:
        assert srch.check_pattern(case.pattern) == case.pattern
        if case.P is not None:
            lo, hi, pam3 = srch.guide_region(case.pattern, case.P)
            assert (hi - lo, pam3) == (case.G, case.pam3)
            guide = "ACGT" * 8
            assert srch.check_query(case.pattern, guide[:case.G], case.P)[lo:hi] == guide[:case.G]


# ------------------------------------------------------------------ the library (GPU)
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def _site_tuples(sites):
    return list(zip(sites["query"].tolist(), sites["contig"].tolist(), sites["position"].tolist(),
                    (sites["strand"] == b"-").astype(int).tolist(), sites["mismatches"].tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in geo.ALL])
def test_gpu_given_guides_plain(engine, cid):
    case = BY_ID[cid]
    queries, contigs, plants = _guides_case(cid)
    Ms = _m_values(case)
    want_counts, s = ref.search(contigs, case.pattern, queries, Ms[-1])
    want = geo.rows_of(s)
    _assert_plants_are_hit(case, contigs, plants, want)
    g = engine.genome(contigs)
    try:
        assert len(g.arenas) == 1
        if case.T >= 2 and len(contigs[0]) > geo.GROUP:  # on the arena's own positions: a hit astride a workgroup boundary
            off = int(g.arenas[0].offsets[0])
            assert any(r[0] == 0 and r[1] == 0 and geo.straddles(r[2], case.T, off, geo.GROUP) for r in want), off
        for M in Ms:
            res = g.search(case.pattern, queries, M, pam_len=case.P)
            print(cid, "M", M, "sites", res.sites.size, "candidates", res.candidates)
            assert (res.counts == want_counts[:, :M + 1]).all(), (cid, M)
            assert _site_tuples(res.sites) == [w for w in want if w[4] <= M], (cid, M)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in geo.SCORED])
def test_gpu_given_guides_scheme_scored(engine, cid):
    case = BY_ID[cid]
    queries, contigs, plants = _guides_case(cid)
    weights = geo.weights_for(case, np.random.default_rng(_seed(case, 8)))
    assert 0.0 in weights and 1.0 in weights
    factor, shape = sref.tables(weights)
    scheme = srch.make_scheme(case.pattern, case.P, weights)
    g = engine.genome(contigs)
    try:
        for M in _m_values(case):
            want_counts, s, want_sum = sref.search(contigs, case.pattern, queries, M, case.P, factor, shape)
            res = g.search(case.pattern, queries, M, pam_len=case.P, score=weights)
            print(cid, "M", M, "hit_sum", [int(x) for x in res.hit_sum], "want", want_sum)
            assert res.hit_sum.dtype == np.uint64 and [int(x) for x in res.hit_sum] == want_sum, (cid, M)
            assert (res.counts == want_counts).all() and _site_tuples(res.sites) == geo.rows_of(s)
            assert srch.hit_values(res.sites, queries, contigs, scheme).tolist() == s["value"].tolist()
            assert res.specificity.tolist() == sref.specificity(want_sum)
            if M >= min(2, case.G):
                _assert_masks_reach_the_ends(case, s["mask"][s["mismatches"] > 0])
                assert sum(want_sum) > 0
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in geo.SCORED])
def test_gpu_given_guides_pair_table(engine, cid):
    case = BY_ID[cid]
    queries, contigs, plants = _guides_case(cid)
    pair, offsets, pam = geo.table_for(case, np.random.default_rng(_seed(case, 9)))
    assert all(case.pattern[(case.T - case.P if case.pam3 else 0) + o] != "N" for o in offsets) and len(offsets) >= 1
    table = srch.PairTable(pair, offsets, pam)
    scheme = srch.make_scheme(case.pattern, case.P, table)
    g = engine.genome(contigs)
    try:
        for M in _m_values(case):
            want_counts, s, want_sum = pref.search(contigs, case.pattern, queries, M, case.P, pair, offsets, pam)
            res = g.search(case.pattern, queries, M, pam_len=case.P, score=table)
            print(cid, "M", M, "hit_sum", [int(x) for x in res.hit_sum], "want", want_sum)
            assert res.hit_sum.dtype == np.uint64 and [int(x) for x in res.hit_sum] == want_sum, (cid, M)
            assert (res.counts == want_counts).all() and _site_tuples(res.sites) == geo.rows_of(s)
            assert srch.hit_values(res.sites, queries, contigs, scheme).tolist() == s["value"].tolist()
            if M >= 1:
                hits = {r[:4]: v for r, v in zip(zip(*[s[f].tolist() for f in ref.SITE_FIELDS]), s["value"].tolist())}
                dead = [hits[(q, k, at, st)] for q, tag, k, at, st in plants if tag.startswith("n-")]
                assert len(dead) >= 4 and not any(dead)              # counted, and worth nothing because of a non-base
                assert any(v > 0 for v in s["value"].tolist())
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(geo.BULGES)))
def test_gpu_bulges(engine, index):
    case, D, R, queries, contigs, plants = _bulge_case(index)
    g = engine.genome(contigs)
    try:
        for M in (0, 2, 4):
            want_counts, s = bref.search(contigs, case.pattern, queries, M, case.P, D, R)
            want = geo.rows_of(s, bref.FIELDS)
            if M == 4:
                _assert_bulge_rows_are_not_vacuous(case, D, R, queries, want)
            res = g.search_bulges(case.pattern, queries, M, case.P, D, R)
            print(case, D, R, "M", M, "counts per kind", res.counts.sum(axis=(0, 2)).tolist())
            assert res.counts.shape == (len(queries), 1 + D + R, M + 1) and (res.counts == want_counts).all(), (case, M)
            got = list(zip(res.sites["query"].tolist(), res.sites["kind"].tolist(), res.sites["contig"].tolist(),
                           res.sites["position"].tolist(), (res.sites["strand"] == b"-").astype(int).tolist(),
                           res.sites["mismatches"].tolist(), res.sites["bulge_at"].tolist()))
            assert got == want, (case, M)
            sizes = np.array([size for _, size in res.kinds])[res.sites["kind"]]
            assert (res.sites["bulge_size"] == sizes).all()
        if case.T == 32:  # a DNA bulge has no window to sit in: refused before anything reaches the GPU
            for D_bad in (1, 2):
                with pytest.raises(srch.SearchInputError):
                    g.search_bulges(case.pattern, queries, 2, case.P, D_bad, 2)
    finally:
        g.close()


def _assert_self_equals(res, want, scored):
    sites, guides, counts, hit_sum = want
    rows = list(zip(res.sites["contig"].tolist(), res.sites["position"].tolist(), (res.sites["strand"] == b"-").astype(int).tolist()))
    assert rows == sites
    assert [gd.decode() for gd in res.guides.tolist()] == guides
    assert res.counts.dtype == np.uint32 and (res.counts.astype(np.int64) == counts).all()
    if scored:
        assert res.hit_sum.dtype == np.uint64 and [int(x) for x in res.hit_sum] == [int(x) for x in hit_sum]
    else:
        assert res.hit_sum is None and res.specificity is None


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(SELF_M))
def test_gpu_self_search(engine, cid):
    case = BY_ID[cid]
    queries, contigs = _self_genome(cid)
    rng = np.random.default_rng(_seed(case, 10))
    weights = geo.weights_for(case, rng)
    table = geo.table_for(case, rng) if case.G >= 3 else None
    if SELF_M[cid] >= 2:  # the planted family's pairs: mismatches at g = 0, at g = G - 1, and both (d = G - 1)
        factor, shape = sref.tables(weights)
        _assert_masks_reach_the_ends(case, sref.search(contigs, case.pattern, queries, 2, case.P, factor, shape)[1]["mask"])
    g = engine.genome(contigs)
    try:
        for M in range(SELF_M[cid] + 1):
            want = geo.self_reference(contigs, case, M, weights)
            assert len(want[0]) >= 16
            res = g.search_self(case.pattern, M, case.P, score=weights)
            print(cid, "M", M, "guide sites", len(want[0]), "candidates", res.candidates, "counted", int(want[2].sum()))
            _assert_self_equals(res, want, True)
            assert res.specificity.tolist() == sref.specificity(want[3])
            _assert_self_equals(g.search_self(case.pattern, M, case.P), want[:3] + (None,), False)
            if table is not None:
                pwant = geo.self_pair_reference(contigs, case, M, *table)
                assert pwant[0] == want[0] and (pwant[2] == want[2]).all()
                _assert_self_equals(g.search_self(case.pattern, M, case.P, score=srch.PairTable(table[0], table[1], table[2])), pwant, True)
                if M >= 1:
                    assert sum(pwant[3]) > 0
            if M >= 1:
                assert int(want[2][:, 1:].sum()) > 0 and sum(want[3]) > 0
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["L5", "S2"])
def test_gpu_self_search_rows_equal_the_given_guides_search(engine, cid):
    case, M = BY_ID[cid], SELF_M[cid]
    queries, contigs = _self_genome(cid)
    weights = geo.weights_for(case, np.random.default_rng(_seed(case, 11)))
    g = engine.genome(contigs)
    try:
        res = g.search_self(case.pattern, M, case.P, score=weights)
        qs = [srch.check_query(case.pattern, gd.decode(), case.P) for gd in res.guides.tolist()]
        assert len(qs) >= 16
        given = g.search(case.pattern, qs, M, pam_len=case.P, score=weights, sites=False)
        want = given.counts.astype(np.int64)
        want[:, 0] -= 1
        assert (res.counts.astype(np.int64) == want).all() and (res.hit_sum == given.hit_sum).all()
        assert int(want.sum()) > 0
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_self_search_one_letter_segments_launches_and_cut(engine):
    """S5 at M = 2: three segments of one letter, so four buckets per segment, each a quarter of the genome's candidates.
    The result must not depend on how many launches cover a bucket nor on the arenas the genome is cut into."""
    case = geo.S5
    queries, contigs = _self_genome("S5")
    contigs = [contigs[0][i:i + 10_000] for i in range(0, len(contigs[0]), 10_000)] + contigs[1:]  # (contigs an arena of 160 words holds)
    sizes = geo.buckets(contigs, case)
    # (this genome: 11 271 candidates, 9 563 guide sites; the largest bucket holds 4 493 candidates and 4 002 guide sites)
    print("S5 buckets (candidates, guide sites):", sizes)
    assert max(c for c, _ in sizes) > 2048 and any(c > 2048 and n > 256 for c, n in sizes)
    weights = geo.weights_for(case, np.random.default_rng(_seed(case, 12)))
    want = geo.self_reference(contigs, case, 2, weights)
    one = engine.genome(contigs)
    many = engine.genome(contigs, max_words=160)
    try:
        assert len(one.arenas) == 1 and len(many.arenas) >= 3
        uncut = one.search_self(case.pattern, 2, case.P, score=weights)
        _assert_self_equals(uncut, want, True)
        low = one.search_self(case.pattern, 2, case.P, score=weights, pairs_per_launch=1 << 20)
        assert low.stats["compare_launches"] > 3 * uncut.stats["compare_launches"] and low.pairs == uncut.pairs
        cut = many.search_self(case.pattern, 2, case.P, score=weights)
        both = many.search_self(case.pattern, 2, case.P, score=weights, pairs_per_launch=1 << 20)
        for res in (low, cut, both):
            _assert_self_equals(res, want, True)
            assert res.candidates == uncut.candidates
    finally:
        one.close()
        many.close()


@pytest.mark.gpu
def test_gpu_cli_end_to_end(tmp_path):
    # L5, --self --score-table
    case = geo.L5
    queries, contigs = _self_genome("L5")
    contigs = [c for c in contigs if c]
    names = ["c%d" % k for k in range(len(contigs))]
    fa = tmp_path / "l5.fa"
    geo.write_fasta(fa, names, contigs)
    pair, offsets, pam = geo.table_for(case, np.random.default_rng(_seed(case, 13)))
    tf = tmp_path / "table.txt"
    tf.write_text(_table_text(pair, offsets, pam))
    out = tmp_path / "self.tsv"
    r = subprocess.run([sys.executable, "-m", "cropsr_amd.search", "-f", str(fa), "--pattern", case.pattern, "--pam-length", "4", "--self",
                        "-m", "3", "--score-table", str(tf), "-o", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sites, guides, counts, hit_sum = geo.self_pair_reference(contigs, case, 3, pair, offsets, pam)
    assert len(sites) >= 16 and sum(hit_sum) > 0
    assert out.read_text() == selfref.format_rows(names, sites, guides, counts, hit_sum)
    # L3, --guides --weights
    case = geo.L3
    queries, contigs, plants = _guides_case("L3")
    keep = [k for k, c in enumerate(contigs) if c]
    assert keep == list(range(len(keep)))  # (the empty contigs, if any, come last: contig numbers stay)
    contigs = [contigs[k] for k in keep]
    names = ["c%d" % k for k in keep]
    fa = tmp_path / "l3.fa"
    geo.write_fasta(fa, names, contigs)
    weights = geo.weights_for(case, np.random.default_rng(_seed(case, 14)))
    wf = tmp_path / "w.txt"
    wf.write_text(" ".join(repr(w) for w in weights) + "\n")
    gd = tmp_path / "guides.txt"
    lo, hi, _ = srch.guide_region(case.pattern, case.P)
    gd.write_text("".join("%s g%d\n" % (q[lo:hi].lstrip("N"), k) for k, q in enumerate(queries)))
    gnames = ["g%d" % k for k in range(len(queries))]
    out, cnt = tmp_path / "sites.tsv", tmp_path / "counts.tsv"
    r = subprocess.run([sys.executable, "-m", "cropsr_amd.search", "-f", str(fa), "--pattern", case.pattern, "--pam-length", "3", "--guides",
                        str(gd), "-m", "4", "--weights", str(wf), "-o", str(out), "--counts", str(cnt)], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    factor, shape = sref.tables(weights)
    counts, s, hit_sum = sref.search(contigs, case.pattern, queries, 4, case.P, factor, shape)
    rows = list(zip(*[s[f].tolist() for f in ref.SITE_FIELDS]))
    strings = [srch.site_string(contigs[k], pos, "+-"[st], queries[q]) for q, k, pos, st, _ in rows]
    assert sum(hit_sum) > 0 and len(rows) > 20
    assert out.read_text() == sref.format_sites(gnames, queries, names, rows, strings, s["value"].tolist())
    assert cnt.read_text() == sref.format_counts(gnames, queries, counts, hit_sum)
