"""The off-target search of given guides (cropsr_amd/search.py, crp_search_*): the CPU reference against a plain statement
of the definition, hand-made answers, input handling and TSV bytes without a GPU; the library against the reference on
the GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import search_reference as ref
from cropsr_amd import _native as nat
from cropsr_amd import search as srch

SPCAS9 = "N" * 21 + "GG"
SPCAS9_NAG = "N" * 21 + "RG"
SACAS9 = "N" * 21 + "NNGRRT"
CAS12A = "TTTV" + "N" * 23
PAM_LEN = {SPCAS9: 3, SPCAS9_NAG: 3, SACAS9: 6, CAS12A: 4}
NOISE = np.frombuffer(b"ACGTACGTACGTACGTacgtacgtNNNNRYKMUuZ.-", dtype=np.uint8)


def _ref_sorted(contigs, pattern, queries, max_mm):
    counts, s = ref.search(contigs, pattern, queries, max_mm)
    return counts, sorted(zip(*[s[f].tolist() for f in ref.SITE_FIELDS]))


def _rand_seq(rng, n, alpha=NOISE):
    return rng.choice(alpha, n).tobytes()


# ------------------------------------------------------------------ the reference itself (CPU)
def test_reference_agrees_with_plain_statement():
    rng = np.random.default_rng(2024)
    letters = "ACGTRYSWKMBDHVNNNNNN"
    for trial in range(200):
        T = int(rng.integers(1, 9))
        pattern = "".join(rng.choice(list(letters), T))
        contigs = [_rand_seq(rng, int(rng.integers(0, 30))) for _ in range(int(rng.integers(1, 5)))]
        queries = ["".join(rng.choice(list("ACGTNacgtn"), T)) for _ in range(int(rng.integers(1, 4)))]
        M = int(rng.integers(0, min(T, 8) + 1))
        counts, got = _ref_sorted(contigs, pattern, queries, M)
        want = ref.search_slow(contigs, pattern, queries, M)
        assert got == want, (trial, pattern, contigs, queries, M)
        for q in range(len(queries)):
            assert counts[q].tolist() == [sum(1 for s in want if s[0] == q and s[4] == k) for k in range(M + 1)]


def _sites(contigs, pattern, query, M):
    return _ref_sorted(contigs, pattern, [query], M)[1]


def test_known_answers():
    g = "ACGTACGTACGTACGTACGA"  # a 20-nt guide
    rc = lambda s: s.translate(str.maketrans("ACGTacgt", "TGCAtgca"))[::-1]
    q = g + "NNN"
    # planted exact '+' site and a 1-mismatch '-' site
    c0 = "TTTTT" + g + "AGG" + "CCCCC"
    c1 = "AAAA" + rc("ACGTACGTACGTACGTACGT" + "TGG") + "AAAA"
    assert _sites([c0, c1], SPCAS9, q, 1) == [(0, 0, 5, 0, 0), (0, 1, 4, 1, 1)]
    # broken by the contig boundary: the same characters split over two contigs
    assert _sites([g[:10], g[10:] + "AGG"], SPCAS9, q, 8) == []
    # an N inside the site costs a mismatch; a lower-case PAM and soft-masked sequence are found
    assert _sites([g[:7] + "N" + g[8:] + "AGG"], SPCAS9, q, 2) == [(0, 0, 0, 0, 1)]
    assert _sites([g.lower() + "agg"], SPCAS9, q, 0) == [(0, 0, 0, 0, 0)]
    assert _sites([g + "aGg"], SPCAS9, q, 0) == [(0, 0, 0, 0, 0)]
    # an N in the PAM is no PAM
    assert _sites([g + "ANG"], SPCAS9, q, 8) == []
    # first and last possible start of a contig
    c = g + "TGG" + "A" * 7 + g + "CGG"
    assert _sites([c], SPCAS9, q, 0) == [(0, 0, 0, 0, 0), (0, 0, len(c) - 23, 0, 0)]
    # a palindrome is found on both strands
    pal = "CCAGTACGTACGTACGTACTGG"  # its reverse complement is itself
    assert rc(pal) == pal
    assert _sites([pal], "N" * 22, pal, 0) == [(0, 0, 0, 0, 0), (0, 0, 0, 1, 0)]
    # NAG only with ...NRG
    assert _sites([g + "TAG"], SPCAS9, q, 0) == []
    assert _sites([g + "TAG"], SPCAS9_NAG, q, 0) == [(0, 0, 0, 0, 0)]
    # Cas12a: TTTV on the 5' side; TTTT is no PAM
    p23 = "ACGTTGCAACGTTGCAACGTTGC"
    assert _sites(["TTTA" + p23, "TTTT" + p23, rc("TTTG" + p23)], CAS12A, "NNNN" + p23, 0) == [(0, 0, 0, 0, 0), (0, 2, 0, 1, 0)]
    # SaCas9 NNGRRT 27-mer: NNGAAT and NNGGGT are PAMs, NNGCAT is not
    p21 = "ACGTTGCAACGTTGCAACGTA"
    sq = p21 + "N" * 6
    assert _sites([p21 + "CAGAAT", p21 + "TTGGGT", p21 + "CAGCAT"], SACAS9, sq, 0) == [(0, 0, 0, 0, 0), (0, 1, 0, 0, 0)]
    # U is read as A, u is not a base
    assert _sites([g.replace("A", "U") + "AGG"], SPCAS9, q, 0) == [(0, 0, 0, 0, 0)]
    assert _sites([g.replace("A", "u", 1) + "AGG"], SPCAS9, q, 1) == [(0, 0, 0, 0, 1)]


# ------------------------------------------------------------------ input handling (CPU)
def test_library_declares_search_abi():
    L = nat.lib()
    for name in ("crp_search_create", "crp_search_run", "crp_search_fetch", "crp_search_candidates", "crp_search_destroy",
                 "crp_search_set_budget", "crp_search_stats"):
        assert hasattr(L, name) and name in nat.SIGNATURES


def test_guides_file_and_padding():
    text = "# shortlist\nACGTACGTACGTACGTACGT  first guide\n\nacgtacgtacgtacgtacgaNNN # comment\n  TTTTACGTACGTACGTACGG\n"
    names, queries = srch.parse_guides(text, SPCAS9, pam_len=3)
    assert names == ["first guide", "4", "5"]
    assert queries == ["ACGTACGTACGTACGTACGTNNN", "ACGTACGTACGTACGTACGANNN", "TTTTACGTACGTACGTACGGNNN"]
    # without the PAM's length: only a guide exactly as long as the N run, filling it
    assert srch.check_query(SPCAS9, "A" * 21) == "A" * 21 + "NN"
    assert srch.check_query(SACAS9, "A" * 23) == "A" * 23 + "N" * 4
    assert srch.check_query(CAS12A, "C" * 23) == "NNNN" + "C" * 23
    with pytest.raises(srch.SearchInputError):
        srch.parse_guides(text, SPCAS9)
    # with it: next to the PAM, on its 3' or 5' side, truncated guides included
    assert srch.check_query(SPCAS9, "C" * 18, 3) == "NN" + "C" * 18 + "NNN"
    assert srch.check_query(SACAS9, "A" * 21, 6) == "A" * 21 + "N" * 6
    assert srch.check_query(SACAS9, "A" * 20, 6) == "N" + "A" * 20 + "N" * 6
    assert srch.check_query(CAS12A, "C" * 20, 4) == "NNNN" + "C" * 20 + "NNN"
    for bad in ((SPCAS9, "A" * 21, 3), (SPCAS9, "A" * 20, 1), (SPCAS9, "A" * 10, 0), (SPCAS9, "A" * 10, 23),
                (CAS12A, "A" * 20, 3), ("NNNGGNNN", "ACG", 3)):
        with pytest.raises(srch.SearchInputError):
            srch.check_query(*bad)


def test_short_guides_find_their_on_target():
    """A 20- or truncated 18-nt SpCas9 guide and a 20-nt SaCas9 guide find the site they were taken from, next to the PAM."""
    g = "GATTACAGATTACAGATTAC"
    for guide, pattern, P, pam in ((g, SPCAS9, 3, "TGG"), (g[2:], SPCAS9, 3, "TGG"), (g[:20], SACAS9, 6, "CTGAAT")):
        contig = "CCCCC" + g + pam + "CCCCC"
        q = srch.check_query(pattern, guide, P)
        start = 5 + len(g) + len(pam) - len(pattern)
        assert ref.search_slow([contig], pattern, [q], 0) == [(0, 0, start, 0, 0)], (guide, pattern)


@pytest.mark.parametrize("pattern", ["", "N" * 33, "NNNNX", "NNN GG", "NNU"])
def test_bad_pattern_refused(pattern):
    with pytest.raises(srch.SearchInputError):
        srch.check_pattern(pattern)


def test_bad_guides_and_mismatches_refused():
    for g in ("ACGTU" + "A" * 15, "A" * 22, "A" * 24, "A" * 20, "A" * 18, "ACGTRACGT", ""):
        with pytest.raises(srch.SearchInputError):
            srch.check_query(SPCAS9, g)
    with pytest.raises(srch.SearchInputError):
        srch.check_query("NNNGGNNN", "ACG")  # two N runs: no padding
    for m in (-1, 9, 2.5):
        with pytest.raises(srch.SearchInputError):
            srch.check_max_mm(m)


def test_cli_refuses_bad_input_before_the_gpu(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">c1\nACGT\n")
    gd = tmp_path / "g.txt"
    gd.write_text("ACGTACGTACGTACGTACGTNNN\n")
    cases = [["--pattern", "NNNXGG", "-m", "2"], ["--pattern", SPCAS9, "-m", "9"], ["--pattern", SPCAS9, "--pam-length", "23"]]
    short = tmp_path / "short.txt"
    short.write_text("ACGTACGTACGTACGTACGT\n")  # 20 letters: needs --pam-length
    cases.append(["--pattern", SPCAS9, "-m", "2", "--guides", str(short)])
    bad = tmp_path / "bad.txt"
    bad.write_text("ACGTRACGTACGTACGTACG\n")
    for args in cases + [["--pattern", SPCAS9, "-m", "2", "--guides", str(bad)]]:
        cmd = [sys.executable, "-m", "cropsr_amd.search", "-f", str(fa), "--guides", str(gd), "-o", str(tmp_path / "o.tsv")] + args
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 2 and "error:" in r.stderr, (args, r.stderr)
        assert not (tmp_path / "o.tsv").exists()


def test_fasta_plain_parse():
    names, seqs = srch.parse_fasta(b">chr1 some words\nACGT acgt\r\nNN\n>chr2\n\n>chr3\tx\nA C\tG\n")
    assert names == ["chr1", "chr2", "chr3"] and seqs == [b"ACGTacgtNN", b"", b"ACG"]


TSV_GENOME = [b"TTACGTACGTACGTACGTACGAAGGTT", b"CCTACGTACGTNCGTACGTACGTAA"]


def _tsv_case():
    queries = [srch.check_query(SPCAS9, "ACGTACGTACGTACGTACGA", 3)]
    counts, s = ref.search(TSV_GENOME, SPCAS9, queries, 2)
    sites = np.empty(s["query"].size, srch.SITE_DTYPE)
    for f in ref.SITE_FIELDS:
        sites[f] = s[f] if f != "strand" else np.where(s[f] == 0, b"+", b"-")
    return queries, counts, sites


def test_tsv_bytes():
    queries, counts, sites = _tsv_case()
    text = srch.format_sites(["g1"], queries, ["c1", "c2"], TSV_GENOME, sites)
    assert text == ("name\tquery\tcontig\tposition\tstrand\tmismatches\tsite\n"
                    "g1\tACGTACGTACGTACGTACGANNN\tc1\t2\t+\t0\tACGTACGTACGTACGTACGAAGG\n"
                    "g1\tACGTACGTACGTACGTACGANNN\tc2\t0\t-\t2\tACGTACGTACGnACGTACGtAGG\n")
    assert srch.format_counts(["g1"], queries, counts) == "name\tquery\tmm0\tmm1\tmm2\ng1\tACGTACGTACGTACGTACGANNN\t1\t0\t1\n"


# ------------------------------------------------------------------ the library (GPU)
def _planted_genome(rng, pattern, n_chars, n_contigs, guides, max_mm):
    """Random mixed-case contigs with N runs, IUPAC codes and U, plus copies of every query with 0..max_mm substitutions
    on both strands."""
    cuts = np.sort(rng.choice(np.arange(1, n_chars), n_contigs - 1, replace=False))
    lens = np.diff(np.concatenate([[0], cuts, [n_chars]]))
    lens[: max(1, n_contigs // 10)] = rng.integers(0, 40, max(1, n_contigs // 10))  # some contigs shorter than T
    alpha = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTacgtacgtacgtNRYU", dtype=np.uint8)
    contigs = [bytearray(rng.choice(alpha, int(n)).tobytes()) for n in lens]
    for c in contigs:
        for _ in range(len(c) // 50000):
            s = int(rng.integers(0, len(c)))
            c[s:s + 300] = b"N" * len(c[s:s + 300])
    T = len(pattern)
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    big = [k for k, c in enumerate(contigs) if len(c) > 4 * T]
    for q in guides:
        for rep in range(6):
            site = []
            for p in range(T):
                if q[p] != "N":
                    site.append(q[p])
                else:
                    site.append(str(rng.choice(list(ref.IUPAC_SETS.get(pattern[p], "ACGT")))))
            comp_pos = [p for p in range(T) if q[p] != "N"]
            for p in rng.choice(comp_pos, int(rng.integers(0, max_mm + 1)), replace=False):
                site[p] = str(rng.choice([b for b in "ACGT" if b != site[p]]))
            s = "".join(site).encode()
            if rng.random() < 0.3:
                s = s.lower()
            if rep % 2:
                s = s.translate(comp)[::-1]
            k = int(rng.choice(big))
            at = int(rng.integers(0, len(contigs[k]) - T + 1))
            contigs[k][at:at + T] = s
    return [bytes(c) for c in contigs]


def _queries_for(rng, pattern, n):
    P = PAM_LEN[pattern]
    return [srch.check_query(pattern, "".join(rng.choice(list("ACGT"), len(pattern) - P)), P) for _ in range(n)]


def _as_tuples(sites):
    return list(zip(sites["query"].tolist(), sites["contig"].tolist(), sites["position"].tolist(),
                    (sites["strand"] == b"-").astype(int).tolist(), sites["mismatches"].tolist()))


@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,seed", [(SPCAS9, 1), (SPCAS9_NAG, 2), (CAS12A, 3), (SACAS9, 4)])
def test_gpu_matches_reference(engine, pattern, seed):
    rng = np.random.default_rng(seed)
    queries = _queries_for(rng, pattern, 24)
    contigs = _planted_genome(rng, pattern, 1_500_000 + seed * 500_000, 60, queries[:16], 8)
    want_counts, s = ref.search(contigs, pattern, queries, 8)
    want = sorted(zip(*[s[f].tolist() for f in ref.SITE_FIELDS]))
    g = engine.genome(contigs)
    try:
        for M in (0, 2, 4, 6, 8):
            res = g.search(pattern, queries, M)
            assert (res.counts == want_counts[:, :M + 1]).all(), M
            assert _as_tuples(res.sites) == [w for w in want if w[4] <= M], M
        assert sum(res.candidates) > 0 and res.sites.size > 16 * 6
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_query_counts_and_multi_arena_and_budget(engine):
    rng = np.random.default_rng(11)
    queries = _queries_for(rng, SPCAS9, 3000)
    contigs = _planted_genome(rng, SPCAS9, 1_000_000, 40, queries[:20], 4)
    want_counts, s = ref.search(contigs, SPCAS9, queries, 4)
    want = np.array(sorted(zip(*[s[f].tolist() for f in ref.SITE_FIELDS])), dtype=np.int64).reshape(-1, 5)
    one = engine.genome(contigs)
    many = engine.genome(contigs, max_words=3000)
    try:
        assert len(many.arenas) > 3 and len(one.arenas) == 1
        for n in (1, 1001, 3000):
            sub = want[want[:, 0] < n]
            for g, budget in ((one, None), (many, None), (one, 1)):
                res = g.search(SPCAS9, queries[:n], 4, budget=budget)
                assert (res.counts == want_counts[:n]).all(), (n, budget)
                assert _as_tuples(res.sites) == [tuple(r) for r in sub.tolist()], (n, budget)
        h = srch.ArenaSearch(one.arenas[0], SPCAS9, budget=1)
        st, _, _ = h.run(queries[:3], 4, 1 << 30)
        assert st == nat.CRP_OK and h.stats()["chunks"] >= 3
        h.close()
    finally:
        one.close()
        many.close()


@pytest.mark.gpu
def test_gpu_all_n_pattern_in_chunks(engine):
    rng = np.random.default_rng(5)
    contigs = [_rand_seq(rng, int(n)) for n in (70000, 5, 33, 40000)]
    queries = ["ACGTACGTAC", "NNNNNNNNNN", "AAAAAAAAAN"]
    want_counts, s = ref.search(contigs, "N" * 10, queries, 3)
    want = sorted(zip(*[s[f].tolist() for f in ref.SITE_FIELDS]))
    g = engine.genome(contigs)
    try:
        for budget in (None, 1):
            res = g.search("N" * 10, queries, 3, budget=budget)
            assert (res.counts == want_counts).all() and _as_tuples(res.sites) == want
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_many_launches_and_growing_site_list(engine):
    """Queries split over many compare launches (1 001 queries, 7 per launch: the last launch is short) and a first
    device site list of 16 slots that the run must grow (its second pass) give the reference's answer."""
    rng = np.random.default_rng(21)
    queries = _queries_for(rng, SPCAS9, 1001)
    contigs = _planted_genome(rng, SPCAS9, 600_000, 12, queries[:30], 4)
    want_counts, s = ref.search(contigs, SPCAS9, queries, 4)
    want = sorted(zip(*[s[f].tolist() for f in ref.SITE_FIELDS]))
    assert len(want) > 16 * 4
    g = engine.genome(contigs)
    h = srch.ArenaSearch(g.arenas[0], SPCAS9)
    try:
        h.set_limits(batch_queries=7, first_site_slots=16)
        st, counts, n = h.run(queries, 4, 1 << 40)
        assert st == nat.CRP_OK and n == len(want) and (counts == want_counts).all()
        stats = h.stats()
        assert stats["compare_launches"] == 2 * 143  # ceil(1001 / 7) launches, twice: the site list grew once
        qi, pos, strand, mm = h.fetch(n)
        a = g.arenas[0]
        offs = np.asarray(a.offsets, dtype=np.int64)
        j = np.searchsorted(offs, pos.astype(np.int64), "right") - 1
        got = list(zip(qi.tolist(), j.tolist(), (pos.astype(np.int64) - offs[j]).tolist(), strand.tolist(), mm.tolist()))
        assert got == want
    finally:
        h.close()
        g.close()


@pytest.mark.gpu
def test_gpu_empty_query_list(engine):
    g = engine.genome([b"ACGTACGTACGTACGTACGTAGG" * 10])
    try:
        res = g.search(SPCAS9, [], 4)
        assert res.counts.shape == (0, 5) and res.sites.size == 0
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_capacity_protocol(engine):
    rng = np.random.default_rng(8)
    contigs = [_rand_seq(rng, 200000, np.frombuffer(b"AAAAAAACGTG", dtype=np.uint8))]
    q = "A" * 20 + "NNN"
    want_counts, s = ref.search(contigs, SPCAS9, [q], 6)
    need = int(want_counts.sum())
    assert need > 1000
    g = engine.genome(contigs)
    h = srch.ArenaSearch(g.arenas[0], SPCAS9)
    try:
        st, counts, n = h.run([q], 6, 100)
        assert st == nat.CRP_ERR_CAPACITY and n == need and (counts == want_counts).all()
        with pytest.raises(nat.CropsrHipError):
            h.fetch(n)
        st, counts, n = h.run([q], 6, need)
        assert st == nat.CRP_OK and n == need and (counts == want_counts).all()
        qi, pos, strand, mm = h.fetch(n)
        got = sorted(zip(pos.tolist(), strand.tolist(), mm.tolist()))
        off = int(g.arenas[0].offsets[0])
        assert got == sorted(zip((s["position"] + off).tolist(), s["strand"].tolist(), s["mismatches"].tolist()))
        with pytest.raises(srch.SiteCapacityError) as e:
            g.search(SPCAS9, [q], 6, site_cap=need - 1)
        assert e.value.n_sites == need and (e.value.counts == want_counts).all()
    finally:
        h.close()
        g.close()


@pytest.mark.gpu
def test_gpu_abi_misuse(engine):
    L = nat.lib()
    g = engine.genome([b"ACGTACGTACGTACGTACGTAGG" * 10])
    a = g.arenas[0]
    h = ctypes.c_void_p()
    try:
        assert L.crp_search_create(a._h, b"NNGG", 0, ctypes.byref(h)) == nat.CRP_ERR_UNSUPPORTED
        assert L.crp_search_create(a._h, b"N" * 33, 33, ctypes.byref(h)) == nat.CRP_ERR_UNSUPPORTED
        assert L.crp_search_create(a._h, b"NNXG", 4, ctypes.byref(h)) == nat.CRP_ERR_INVALID
        assert L.crp_search_create(None, b"NNGG", 4, ctypes.byref(h)) == nat.CRP_ERR_INVALID
        assert L.crp_search_create(a._h, b"NNGG", 4, ctypes.byref(h)) == nat.CRP_OK
        n = ctypes.c_uint64()
        assert L.crp_search_fetch(h, None, None, None, None, 0) == nat.CRP_ERR_STATE
        assert L.crp_search_run(h, b"ACNN", 1, 9, 10, None, ctypes.byref(n)) == nat.CRP_ERR_UNSUPPORTED
        assert L.crp_search_run(h, b"ACNN", 1, -1, 10, None, ctypes.byref(n)) == nat.CRP_ERR_UNSUPPORTED
        assert L.crp_search_run(h, b"ACRN", 1, 1, 10, None, ctypes.byref(n)) == nat.CRP_ERR_INVALID
        assert L.crp_search_run(h, b"ACGT", 1, 1, 10, None, None) == nat.CRP_ERR_INVALID
        assert L.crp_search_run(h, b"TAGG", 1, 0, 1000, None, ctypes.byref(n)) == nat.CRP_OK and n.value == 10
        assert L.crp_search_fetch(h, None, None, None, None, 9) == nat.CRP_ERR_CAPACITY
        assert L.crp_search_fetch(h, None, None, None, None, 10) == nat.CRP_OK
        assert L.crp_search_stats(h, None, 7) == nat.CRP_ERR_INVALID
    finally:
        if h:
            L.crp_search_destroy(h)
        g.close()
    assert L.crp_search_destroy(None) == nat.CRP_ERR_INVALID


@pytest.mark.gpu
def test_gpu_cli_end_to_end(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">c1 first\nTTACGTACGTACGT\nACGTACGAAGGTT\n>c2\nCCTACGTACGTNCGTACGTACGTAA\n")
    gd = tmp_path / "guides.txt"
    gd.write_text("ACGTACGTACGTACGTACGA g1\n")
    out, cnt = tmp_path / "sites.tsv", tmp_path / "counts.tsv"
    r = subprocess.run([sys.executable, "-m", "cropsr_amd.search", "-f", str(fa), "--pattern", SPCAS9, "--guides", str(gd),
                        "--pam-length", "3", "-m", "2", "-o", str(out), "--counts", str(cnt)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    queries, counts, sites = _tsv_case()
    assert out.read_text() == srch.format_sites(["g1"], queries, ["c1", "c2"], TSV_GENOME, sites)
    assert cnt.read_text() == "name\tquery\tmm0\tmm1\tmm2\ng1\tACGTACGTACGTACGTACGANNN\t1\t0\t1\n"
