"""The off-target search with DNA and RNA bulges (search.search_bulges, crp_search_run_bulge): the CPU reference against a
plain statement of the definition, hand-made answers, refusals and TSV bytes without a GPU; on the GPU the library
against the reference, through chunks, arenas, launches and the capacity protocol, and against an expansion of every
query per bulge placement through the existing no-bulge search."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import search_bulge_reference as bref
import search_reference as ref
from cropsr_amd import _native as nat
from cropsr_amd import search as srch

SPCAS9 = "N" * 21 + "GG"
SPCAS9_NAG = "N" * 21 + "RG"
SACAS9 = "N" * 21 + "NNGRRT"
CAS12A = "TTTV" + "N" * 23
PAM_LEN = {SPCAS9: 3, SPCAS9_NAG: 3, SACAS9: 6, CAS12A: 4}
NOISE = np.frombuffer(b"ACGTACGTACGTACGTacgtacgtNNNNRYKMUuZ.-", dtype=np.uint8)
_RC = str.maketrans("ACGTacgt", "TGCAtgca")


def rc(s):
    return s.translate(_RC)[::-1]


def _bulged_window(rng, pattern, pam_len, query, bulge, size, subs):
    """An oriented window of the kind's pattern that pairs with `query` for a bulge at a random placement, with
    `subs` substitutions at paired query bases."""
    T = len(pattern)
    kp = bref.kind_pattern(pattern, pam_len, bulge, size)
    win = [str(rng.choice(list(ref.IUPAC_SETS.get(c, "ACGT")))) for c in kp]
    if size:
        first, last = bref.span(pattern, pam_len, query)
        s = int(rng.choice(bref.placements(first, last, bulge, size)))
    else:
        s = 0
    pairs = [(i, w) for i, w in bref.pairing(T, bulge, size, s) if query[i] in "ACGT"]
    for i, w in pairs:
        win[w] = query[i]
    for k in rng.choice(len(pairs), min(subs, len(pairs)), replace=False):
        i, w = pairs[int(k)]
        win[w] = str(rng.choice([b for b in "ACGT" if b != query[i]]))
    return "".join(win)


def _planted(rng, pattern, queries, n_chars, n_contigs, D, R, max_subs, alpha=NOISE):
    """Random contigs plus, per query and kind, copies on both strands with 0..max_subs substitutions."""
    P = PAM_LEN[pattern]
    lens = rng.multinomial(n_chars, [1 / n_contigs] * n_contigs)
    contigs = [bytearray(rng.choice(alpha, int(n)).tobytes()) for n in lens]
    big = [k for k, c in enumerate(contigs) if len(c) > 4 * len(pattern)]
    for q in queries:
        for bulge, size in bref.kinds(D, R):
            for rep in range(2):
                w = _bulged_window(rng, pattern, P, q, bulge, size, int(rng.integers(0, max_subs + 1)))
                if rep:
                    w = rc(w)
                if rng.random() < 0.3:
                    w = w.lower()
                k = int(rng.choice(big))
                at = int(rng.integers(0, len(contigs[k]) - len(w) + 1))
                contigs[k][at:at + len(w)] = w.encode()
    return [bytes(c) for c in contigs]


def _queries(rng, pattern, n, short=0):
    """n random guides next to the PAM, the last `short` of them truncated by 2."""
    P = PAM_LEN[pattern]
    L = len(pattern) - P
    return [srch.check_query(pattern, "".join(rng.choice(list("ACGT"), L - (2 if k >= n - short else 0))), P) for k in range(n)]


def _ref_rows(contigs, pattern, queries, M, D, R):
    counts, s = bref.search(contigs, pattern, queries, M, PAM_LEN[pattern], D, R)
    return counts, sorted(zip(*[s[f].tolist() for f in bref.FIELDS]))


# ------------------------------------------------------------------ the reference itself (CPU)
@pytest.mark.parametrize("pattern,seed", [(SPCAS9, 1), (SPCAS9_NAG, 2), (SACAS9, 3), (CAS12A, 4)])
def test_bulge_reference_agrees_with_plain_statement(pattern, seed):
    rng = np.random.default_rng(seed)
    for D, R in ((1, 0), (0, 1), (2, 2), (1, 2)):
        queries = _queries(rng, pattern, 3, short=1)
        contigs = _planted(rng, pattern, queries, 1500, 3, D, R, 2)
        M = int(rng.integers(2, 4))
        counts, got = _ref_rows(contigs, pattern, queries, M, D, R)
        want = bref.search_slow(contigs, pattern, queries, M, PAM_LEN[pattern], D, R)
        assert got == want, (pattern, D, R)
        assert len({r[:2] for r in want}) >= len(queries) * (1 + D + R) // 2
        for q in range(len(queries)):
            for k in range(1 + D + R):
                assert counts[q, k].tolist() == [sum(1 for s in want if s[:2] == (q, k) and s[5] == m) for m in range(M + 1)]


# ------------------------------------------------------------------ hand-made answers (CPU)
G = "GATCCAGTTACGGATCAAGC"  # no base equals its neighbours at 9..11


def _zero(contigs, query, D, R, pattern=SPCAS9):
    return [r for r in _ref_rows(contigs, pattern, [query], 0, D, R)[1] if r[1] > 0]


def test_planted_insertion_and_deletion():
    q = G + "NNN"
    assert G[9] != G[10] != G[11]
    dna = G[:10] + "T" + G[10:] + "AGG"   # one extra genomic base after guide position 9
    rna = G[:10] + G[11:] + "AGG"         # guide position 10 has no genomic partner
    for strand, f in ((0, lambda w: w), (1, rc)):
        # kind 1 = DNA 1 and kind 2 = RNA 1: position = forward start of that kind's window, bulge_at = s - span_first
        assert _zero(["CCCCC" + f(dna) + "CCCCC"], q, 1, 1) == [(0, 1, 0, 5, strand, 0, 10)]
        assert _zero(["CCCCC" + f(rna) + "CCCCC"], q, 1, 1) == [(0, 2, 0, 5, strand, 0, 10)]
    # the 18-nt truncated guide finds the same insertion: its span starts at query position 2
    q18 = srch.check_query(SPCAS9, G[2:], 3)
    assert _zero(["CCCCC" + dna + "CCCCC"], q18, 1, 0) == [(0, 1, 0, 5, 0, 0, 8)]
    # Cas12a: the PAM on the 5' side, the window grows at its 3' end
    p23 = "GATCCAGTTACGGATCAAGCTTG"
    qa = "NNNN" + p23
    assert _zero(["TTTA" + p23[:12] + "T" + p23[12:]], qa, 1, 0, CAS12A) == [(0, 1, 0, 0, 0, 0, 12)]
    # inside the GG run at 11..12 the smallest placement wins
    assert _zero(["TTTA" + p23[:12] + "G" + p23[12:]], qa, 1, 0, CAS12A) == [(0, 1, 0, 0, 0, 0, 11)]


def test_homopolymer_takes_the_smallest_placement():
    g = "ACGTACGT" + "AAAA" + "CGTACGTA"
    q = g + "NNN"
    # any s in 8..12 pairs an extra A with nothing; the smallest is reported: bulge_at 8
    assert _zero([g[:8] + "AAAAA" + g[12:] + "TGG"], q, 1, 0) == [(0, 1, 0, 0, 0, 0, 8)]
    assert _zero([g[:8] + "AAA" + g[12:] + "TGG"], q, 0, 1) == [(0, 1, 0, 0, 0, 0, 8)]
    assert bref.search_slow([g[:8] + "AAAAA" + g[12:] + "TGG"], SPCAS9, [q], 0, 3, 1, 0)[-1] == (0, 1, 0, 0, 0, 0, 8)


def test_kind_patterns_and_spans():
    assert srch.kind_pattern(SPCAS9, 3, "DNA", 2) == "N" * 22 + "NGG" and len(srch.kind_pattern(SPCAS9, 3, "DNA", 2)) == 25
    assert srch.kind_pattern(SACAS9, 6, "RNA", 1) == "N" * 20 + "NNGRRT"
    assert srch.kind_pattern(CAS12A, 4, "DNA", 1) == "TTTV" + "N" * 24
    assert srch.kind_pattern(CAS12A, 4, "-", 0) == CAS12A
    assert srch.bulge_kinds(2, 1) == [("-", 0), ("DNA", 1), ("DNA", 2), ("RNA", 1)]
    qs = [srch.check_query(SPCAS9, "NNACGTACGTACGTACGTAN", 3), srch.check_query(CAS12A, "ACGT", 4)]
    assert srch.query_spans(SPCAS9, 3, qs[:1], 1, 2).tolist() == [[2, 18]]
    assert srch.query_spans(CAS12A, 4, qs[1:], 1, 2).tolist() == [[4, 7]]


# ------------------------------------------------------------------ refusals (CPU)
def test_bulge_refusals():
    q = ["ACGTACGTACGTACGTACGTNNN"]
    for D, R, P in ((1, 0, None), (0, 1, None), (3, 0, 3), (0, 3, 3), (-1, 0, 3), (1.0, 0, 3)):
        with pytest.raises(srch.SearchInputError):
            srch.check_bulges(SPCAS9, P, D, R)
    with pytest.raises(srch.SearchInputError):  # T + D > 32
        srch.check_bulges("N" * 28 + "NGG", 3, 2, 0)
    assert srch.check_bulges("N" * 27 + "NGG", 3, 2, 2) == (2, 2)
    with pytest.raises(srch.SearchInputError):  # letters other than N outside the PAM
        srch.check_bulges("NNNNANNNNNNNNNNNNNNNNGG", 3, 1, 0)
    # a span too short: DNA needs 2 letters, RNA r + 2
    one = [srch.check_query(SPCAS9, "N" * 19 + "A", 3)]
    three = [srch.check_query(SPCAS9, "N" * 17 + "ACG", 3)]
    with pytest.raises(srch.SearchInputError):
        srch.query_spans(SPCAS9, 3, one, 1, 0)
    srch.query_spans(SPCAS9, 3, three, 1, 1)
    with pytest.raises(srch.SearchInputError):
        srch.query_spans(SPCAS9, 3, three, 0, 2)
    with pytest.raises(srch.SearchInputError):
        srch.query_spans(SPCAS9, 3, [srch.check_query(SPCAS9, "N" * 20, 3)], 1, 0)
    # search_bulges refuses before it touches a genome
    for args in ((q, 4, None, 1, 0), (q, 4, 3, 3, 0), (one, 4, 3, 1, 0), (q, 9, 3, 1, 0)):
        with pytest.raises(srch.SearchInputError):
            srch.search_bulges(None, SPCAS9, *args)


def test_cli_refuses_bad_bulges_before_the_gpu(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">c1\nACGT\n")
    gd = tmp_path / "g.txt"
    gd.write_text("ACGTACGTACGTACGTACGT\n")
    short = tmp_path / "s.txt"
    short.write_text("NNNNNNNNNNNNNNNNNNAC\n")
    cases = [["--pam-length", "3", "--dna-bulge", "3"], ["--pam-length", "3", "--rna-bulge", "-1"],
             ["--guides", str(tmp_path / "full.txt"), "--dna-bulge", "1"],  # no --pam-length
             ["--pam-length", "3", "--rna-bulge", "1", "--guides", str(short)],
             ["--pattern", "N" * 29 + "GG", "--pam-length", "3", "--dna-bulge", "2"]]
    (tmp_path / "full.txt").write_text("ACGTACGTACGTACGTACGTNNN\n")
    for args in cases:
        cmd = [sys.executable, "-m", "cropsr_amd.search", "-f", str(fa), "--pattern", SPCAS9, "--guides", str(gd), "-m", "2",
               "-o", str(tmp_path / "o.tsv")] + args
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 2 and "error:" in r.stderr, (args, r.stderr)
        assert not (tmp_path / "o.tsv").exists()


def test_library_declares_bulge_abi():
    L = nat.lib()
    with open(os.path.join(ROOT, "include", "cropsr_hip.h")) as f:
        header = f.read()
    for name in ("crp_search_run_bulge", "crp_search_fetch_bulge"):
        assert hasattr(L, name) and name in nat.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header)
    for name, v in (("CRP_SEARCH_BULGE_DNA", nat.SEARCH_BULGE_DNA), ("CRP_SEARCH_BULGE_RNA", nat.SEARCH_BULGE_RNA),
                    ("CRP_SEARCH_MAX_BULGE", srch.MAX_BULGE)):
        assert re.search(r"#define %s %d\b" % (name, v), header)
    assert L.crp_abi_version() == 6


# ------------------------------------------------------------------ TSV bytes (CPU)
# c1: GATCCAGTTAC + an extra T + GGATaAAGC + AGG (a DNA bulge and a mismatch); c2 at 2 on '-': GAT(C)CAGTTACGGATCAAGC + TGG
# with one C of the guide's CC missing (an RNA bulge in a run of two: the smaller placement, bulge_at 3)
TSV_GENOME = [b"TTGATCCAGTTACTGGATAAAGCAGGTT", b"CC" + rc("GATCAGTTACGGATCAAGCTGG").encode() + b"AA"]
TSV_GUIDE = "GATCCAGTTACGGATCAAGC"


def _result_of(contigs, pattern, queries, M, D, R):
    counts, s = bref.search(contigs, pattern, queries, M, PAM_LEN[pattern], D, R)
    sites = np.empty(s["query"].size, srch.BULGE_SITE_DTYPE)
    kinds = srch.bulge_kinds(D, R)
    for f in bref.FIELDS:
        sites[f] = s[f] if f != "strand" else np.where(s[f] == 0, b"+", b"-")
    sites["bulge_size"] = [kinds[k][1] for k in s["kind"]]
    spans = srch.query_spans(pattern, PAM_LEN[pattern], queries, D, R)
    return srch.BulgeSearchResult(counts, sites, kinds, spans, None)


def test_bulge_tsv_bytes():
    queries = [srch.check_query(SPCAS9, TSV_GUIDE, 3)]
    res = _result_of(TSV_GENOME, SPCAS9, queries, 1, 1, 1)
    text = srch.format_bulge_sites(["g1"], queries, ["c1", "c2"], TSV_GENOME, res)
    q = "GATCCAGTTACGGATCAAGCNNN"
    assert text == ("name\tquery\tcontig\tposition\tstrand\tmismatches\tbulge\tbulge_size\tbulge_at\tsite\tquery_aligned\n"
                    "g1\t%s\tc1\t2\t+\t1\tDNA\t1\t11\tGATCCAGTTACTGGATaAAGCAGG\tGATCCAGTTAC-GGATCAAGCNNN\n"
                    "g1\t%s\tc2\t2\t-\t0\tRNA\t1\t3\tGAT-CAGTTACGGATCAAGCTGG\t%s\n" % (q, q, q))
    assert srch.format_bulge_counts(["g1"], queries, res.kinds, res.counts) == (
        "name\tquery\tbulge\tbulge_size\tmm0\tmm1\n"
        "g1\t%s\t-\t0\t0\t0\ng1\t%s\tDNA\t1\t0\t1\ng1\t%s\tRNA\t1\t1\t0\n" % (q, q, q))


def test_bulge_alignment_strings():
    q = "ACGTNACGTA" + "NNN"
    # DNA 2 at s = 3: window positions 3, 4 unpaired (upper case, N if no base); a mismatch at query 5 (window 7)
    site, qa = srch.bulge_alignment(b"ACGntTTGCGTAAGG", 0, "+", q, "DNA", 2, 3)
    assert (site, qa) == ("ACGNTTTgCGTAAGG", "ACG--TNACGTANNN")
    # RNA 1 at s = 2, '-' strand: the window is the reverse complement
    site, qa = srch.bulge_alignment(rc("ACTNACGTAAGG").encode(), 0, "-", q, "RNA", 1, 2)
    assert (site, qa) == ("AC-TNACGTAAGG", q)


# ------------------------------------------------------------------ the library (GPU)
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def _tuples(sites):
    return list(zip(sites["query"].tolist(), sites["kind"].tolist(), sites["contig"].tolist(), sites["position"].tolist(),
                    (sites["strand"] == b"-").astype(int).tolist(), sites["mismatches"].tolist(), sites["bulge_at"].tolist()))


def _select(rows, counts, D, R, M, D_all=2):
    """The reference rows (computed with D_all, R_all = 2) for a search with D, R, M: kinds renumbered."""
    keep = {0: 0}
    keep.update({d: d for d in range(1, D + 1)})
    keep.update({D_all + r: D + r for r in range(1, R + 1)})
    out = [(r[0], keep[r[1]]) + r[2:] for r in rows if r[1] in keep and r[5] <= M]
    c = counts[:, sorted(keep), :M + 1]
    return sorted(out), c


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,seed", [(SPCAS9, 1), (SPCAS9_NAG, 2), (CAS12A, 3), (SACAS9, 4)])
def test_gpu_bulges_match_reference(engine, pattern, seed):
    rng = np.random.default_rng(seed)
    queries = _queries(rng, pattern, 10, short=2)
    contigs = _planted(rng, pattern, queries, 150_000, 9, 2, 2, 4)
    counts, rows = _ref_rows(contigs, pattern, queries, 4, 2, 2)
    g = engine.genome(contigs)
    try:
        for D, R in ((0, 0), (1, 1), (2, 2), (2, 0), (0, 2), (1, 2)):
            for M in (0, 2, 4):
                res = g.search_bulges(pattern, queries, M, PAM_LEN[pattern], D, R)
                want, wc = _select(rows, counts, D, R, M)
                assert res.counts.shape == (len(queries), 1 + D + R, M + 1)
                assert (res.counts == wc).all(), (D, R, M)
                assert _tuples(res.sites) == want, (D, R, M)
                sizes = np.array([s for _, s in res.kinds])[res.sites["kind"]] if res.sites.size else []
                assert (res.sites["bulge_size"] == sizes).all()
        assert len(rows) > len(queries) * 5
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_bulges_arenas_chunks_launches(engine):
    rng = np.random.default_rng(11)
    queries = _queries(rng, SPCAS9, 40, short=5)
    contigs = _planted(rng, SPCAS9, queries[:20], 200_000, 30, 2, 2, 3,
                       alpha=np.frombuffer(b"ACGTACGTACGTacgtNRYU", dtype=np.uint8))
    counts, rows = _ref_rows(contigs, SPCAS9, queries, 3, 2, 2)
    one = engine.genome(contigs)
    many = engine.genome(contigs, max_words=600)
    try:
        assert len(many.arenas) > 3
        for g, budget in ((many, None), (one, 1), (many, 1)):
            res = g.search_bulges(SPCAS9, queries, 3, 3, 2, 2, budget=budget)
            assert (res.counts == counts).all() and _tuples(res.sites) == rows, budget
        # one handle, DNA 2: 40 queries, 3 per launch (14 launches), a first device list of 8 slots that must grow
        kp = srch.kind_pattern(SPCAS9, 3, "DNA", 2)
        h = srch.ArenaSearch(one.arenas[0], kp)
        try:
            h.set_limits(batch_queries=3, first_site_slots=8)
            spans = srch.query_spans(SPCAS9, 3, queries, 2, 0)
            st, c, n = h.run(queries, 3, 1 << 40, ("DNA", 2), spans)
            want = [r for r in rows if r[1] == 2]
            assert st == nat.CRP_OK and n == len(want) > 8 and (c == counts[:, 2]).all()
            assert h.stats()["compare_launches"] == 2 * 14
            qi, pos, strand, mm, at = h.fetch(n, ("DNA", 2))
            offs = np.asarray(one.arenas[0].offsets, dtype=np.int64)
            j = np.searchsorted(offs, pos.astype(np.int64), "right") - 1
            got = list(zip(qi.tolist(), [2] * n, j.tolist(), (pos.astype(np.int64) - offs[j]).tolist(), strand.tolist(),
                           mm.tolist(), at.tolist()))
            assert got == want
        finally:
            h.close()
    finally:
        one.close()
        many.close()


@pytest.mark.gpu
def test_gpu_bulge_capacity_and_misuse(engine):
    rng = np.random.default_rng(8)
    contigs = [rng.choice(np.frombuffer(b"AAAAAAACGTG", dtype=np.uint8), 100_000).tobytes()]
    q = srch.check_query(SPCAS9, "A" * 20, 3)
    counts, rows = _ref_rows(contigs, SPCAS9, [q], 4, 1, 1)
    need = len(rows)
    assert need > 1000
    g = engine.genome(contigs)
    kp = srch.kind_pattern(SPCAS9, 3, "RNA", 1)
    h = srch.ArenaSearch(g.arenas[0], kp)
    L = nat.lib()
    try:
        spans = srch.query_spans(SPCAS9, 3, [q], 0, 1)
        n_rna = sum(1 for r in rows if r[1] == 2)
        st, c, n = h.run([q], 4, 10, ("RNA", 1), spans)
        assert st == nat.CRP_ERR_CAPACITY and n == n_rna and (c == counts[:, 2]).all()
        with pytest.raises(nat.CropsrHipError):
            h.fetch(n, ("RNA", 1))
        st, c, n = h.run([q], 4, n_rna, ("RNA", 1), spans)
        assert st == nat.CRP_OK and n == n_rna
        with pytest.raises(srch.SiteCapacityError) as e:
            g.search_bulges(SPCAS9, [q], 4, 3, 1, 1, site_cap=need - 1)
        assert e.value.n_sites == need and (e.value.counts == counts).all()
        res = g.search_bulges(SPCAS9, [q], 4, 3, 1, 1, site_cap=need)
        assert _tuples(res.sites) == rows
        # the ABI: kind, size, span and query length checked
        n = __import__("ctypes").c_uint64()
        sp = np.array([0, 19], np.uint8)
        spp = sp.ctypes.data_as(nat.u8p)
        blob = q.encode()
        assert L.crp_search_run_bulge(h._h, blob, 1, 3, 1, spp, 4, 10, None, n) == nat.CRP_ERR_INVALID
        assert L.crp_search_run_bulge(h._h, blob, 1, 2, 3, spp, 4, 10, None, n) == nat.CRP_ERR_UNSUPPORTED
        assert L.crp_search_run_bulge(h._h, blob, 1, 2, 1, spp, 9, 10, None, n) == nat.CRP_ERR_UNSUPPORTED
        assert L.crp_search_run_bulge(h._h, blob, 1, 2, 1, None, 4, 10, None, n) == nat.CRP_ERR_INVALID
        bad = np.array([18, 19], np.uint8)  # no RNA placement
        assert L.crp_search_run_bulge(h._h, blob, 1, 2, 1, bad.ctypes.data_as(nat.u8p), 4, 10, None, n) == nat.CRP_ERR_INVALID
        past = np.array([0, 23], np.uint8)
        assert L.crp_search_run_bulge(h._h, blob, 1, 2, 1, past.ctypes.data_as(nat.u8p), 4, 10, None, n) == nat.CRP_ERR_INVALID
    finally:
        h.close()
        g.close()


@pytest.mark.gpu
def test_gpu_kind_none_is_search(engine):
    rng = np.random.default_rng(5)
    queries = _queries(rng, SACAS9, 16, short=4)
    contigs = _planted(rng, SACAS9, queries, 300_000, 5, 1, 1, 4)
    g = engine.genome(contigs, max_words=2000)
    try:
        plain = g.search(SACAS9, queries, 4, pam_len=6)
        res = g.search_bulges(SACAS9, queries, 4, 6, 1, 1)
        none = res.sites[res.sites["kind"] == 0]
        for f in srch.SITE_DTYPE.names:
            assert (none[f] == plain.sites[f]).all(), f
        assert (res.counts[:, 0] == plain.counts).all() and (none["bulge_at"] == 0).all()
    finally:
        g.close()


def _expanded(pattern, pam_len, queries, bulge, size):
    """Every query per placement s, as a plain query of the kind's pattern: d N inserted at s, or r letters deleted."""
    out, owner = [], []
    spans = srch.query_spans(pattern, pam_len, queries, size if bulge == "DNA" else 0, size if bulge == "RNA" else 0)
    for q, query in enumerate(queries):
        first, last = (int(v) for v in spans[q])
        for s in bref.placements(first, last, bulge, size):
            out.append(query[:s] + "N" * size + query[s:] if bulge == "DNA" else query[:s] + query[s + size:])
            owner.append((q, s - first))
    return out, np.array(owner, dtype=np.int64).reshape(-1, 2)


@pytest.mark.gpu
@pytest.mark.slow
def test_gpu_bulges_equal_expansion_through_plain_search(engine):
    """At 24 Mb with 64 guides and planted bulged copies: search_bulges equals the no-bulge search of every query
    expanded per placement, reduced per site to the fewest mismatches at the smallest placement."""
    rng = np.random.default_rng(31)
    pattern, P, M = SPCAS9, 3, 3
    queries = _queries(rng, pattern, 64, short=8)
    contigs = _planted(rng, pattern, queries, 24_000_000, 12, 2, 2, M,
                       alpha=np.frombuffer(b"ACGTACGTACGTACGTacgtN", dtype=np.uint8))
    g = engine.genome(contigs)
    try:
        res = g.search_bulges(pattern, queries, M, P, 2, 2)
        plain = g.search(pattern, queries, M, pam_len=P)
        none = res.sites[res.sites["kind"] == 0]
        assert (none["position"] == plain.sites["position"]).all() and (res.counts[:, 0] == plain.counts).all()
        for k, (bulge, size) in enumerate(res.kinds[1:], 1):
            exp, owner = _expanded(pattern, P, queries, bulge, size)
            e = g.search(srch.kind_pattern(pattern, P, bulge, size), exp, M)
            s = e.sites
            q, at = owner[s["query"], 0], owner[s["query"], 1]
            minus = (s["strand"] == b"-").astype(np.int64)
            # per site: fewest mismatches, then the smallest placement
            o = np.lexsort((at, s["mismatches"], minus, s["position"], s["contig"], q))
            key = np.stack([q[o], s["contig"][o], s["position"][o], minus[o]], axis=1)
            first = np.ones(o.size, bool)
            first[1:] = (key[1:] != key[:-1]).any(axis=1)
            o = o[first]
            got = res.sites[res.sites["kind"] == k]
            assert got.size == o.size > 64, (bulge, size)
            assert (got["query"] == q[o]).all() and (got["contig"] == s["contig"][o]).all()
            assert (got["position"] == s["position"][o]).all() and (got["strand"] == s["strand"][o]).all()
            assert (got["mismatches"] == s["mismatches"][o]).all() and (got["bulge_at"] == at[o]).all(), (bulge, size)
            want_counts = np.zeros((len(queries), M + 1), np.int64)
            np.add.at(want_counts, (q[o], s["mismatches"][o].astype(np.int64)), 1)
            assert (res.counts[:, k] == want_counts).all()
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_bulge_cli_end_to_end(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">c1 first\n" + TSV_GENOME[0][:10] + b"\n" + TSV_GENOME[0][10:] + b"\n>c2\n" + TSV_GENOME[1] + b"\n")
    gd = tmp_path / "guides.txt"
    gd.write_text(TSV_GUIDE + " g1\n")
    out, cnt = tmp_path / "sites.tsv", tmp_path / "counts.tsv"
    r = subprocess.run([sys.executable, "-m", "cropsr_amd.search", "-f", str(fa), "--pattern", SPCAS9, "--guides", str(gd),
                        "--pam-length", "3", "-m", "1", "--dna-bulge", "1", "--rna-bulge", "1", "-o", str(out), "--counts", str(cnt)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    queries = [srch.check_query(SPCAS9, TSV_GUIDE, 3)]
    res = _result_of(TSV_GENOME, SPCAS9, queries, 1, 1, 1)
    assert out.read_text() == srch.format_bulge_sites(["g1"], queries, ["c1", "c2"], TSV_GENOME, res)
    assert cnt.read_text() == srch.format_bulge_counts(["g1"], queries, res.kinds, res.counts)
