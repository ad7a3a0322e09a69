"""Guide selection for any nuclease (cropsr_amd/select_self.py, csrc/crp_select_self.hip): the K most
specific guide sites of every gene, over the rows of a self search.

Without a GPU: the two statements of the reference against each other, the key packing and its saturation points, the
cut-letter rule, the default cut offset, the percent-to-count rule, every command-line refusal, and the unchanged bytes of a
--self run without --select.  On the GPU: the rows come from the GPU self search (whose own tests pin them); the numpy
reference is applied to those fetched rows and sel, n_in, n_pass and the gathered fields must be exactly equal.  Every case
first proves on the reference what it claims to exercise."""
import numpy as np
import pytest

import select_self_cases as cases
import select_self_reference as ref
from cropsr_amd import _native as nat
from cropsr_amd import search as srch
from cropsr_amd import select as sel_mod
from cropsr_amd import select_self as ss

NONE = ref.NONE
W = {G: [round(0.05 + 0.9 * g / max(1, G - 1), 3) for g in range(G)] for G in (4, 23, 29)}  # weights, PAM-distal first


# ---------------------------------------------------------------- without a GPU

@pytest.mark.parametrize("scored", [False, True])
@pytest.mark.parametrize("M", [0, 2, 4])
def test_reference_statements_agree(M, scored):
    rng = np.random.default_rng([11, M, scored])
    rows = cases.random_rows(rng, 400, M, scored)
    lo = np.array([0, 100, 100, 900, 4990, 2000, 0], np.uint32)
    hi = np.array([5100, 400, 400, 905, 5100, 2000, 0], np.uint32)
    track = (np.arange(0, 5200, 130), np.arange(40) % 4, np.array([0, 1, 0, 1], np.uint8))
    for k in (1, 5, 64):
        for extra in (dict(), dict(max_mm0=1), dict(gc_min=8, gc_max=12), dict(max_t_run=1), dict(track=track),
                      dict(max_hit_sum=1 << 28, max_mm0=0, max_t_run=2, track=track)):
            sp = ref.spec(23, 17, ref.region_mask(23, 3, True), k, **extra)
            a, b = ref.select_numpy(rows, lo, hi, sp), ref.select_loop(rows, lo, hi, sp)
            for x, y in zip(a, b):
                assert np.array_equal(x, y), (k, extra)
            assert a[0][0] == 400 and a[1][0] <= 400 and (a[2][0] != NONE).sum() == min(k, a[1][0])
    # hand-built: three sites in one gene with equal e, decided by the cut letter and then the strand
    rows = dict(pos=np.array([10, 4, 10], np.uint32), strand=np.array([0, 1, 0], np.uint8), hi=np.zeros(3, np.uint32), lo=np.zeros(3, np.uint32),
                counts=np.ones((3, 1), np.uint32), hit_sum=None, cand=np.array([7, 8, 9], np.uint32))
    sp = ref.spec(23, 17, ref.region_mask(23, 3, True), 3)
    assert ref.cut_letters(rows["pos"], rows["strand"], 23, 17).tolist() == [27, 10, 27]
    for f in (ref.select_numpy, ref.select_loop):
        n_in, n_pass, sel = f(rows, [0], [100], sp)
        assert (n_in[0], n_pass[0], sel[0].tolist()) == (3, 3, [8, 7, 9])
    rows["strand"] = np.array([0, 1, 1], np.uint8)
    rows["pos"] = np.array([10, 21, 4], np.uint32)  # cuts 27 '+', 27 '-', 10 '-'
    assert ref.select_loop(rows, [0], [100], sp)[2][0].tolist() == [9, 7, 8]


def test_key_packing():
    assert ref.scored_e(0, 5) == 5 and ref.scored_e(3, 5) == 5 + (3 << 30)
    assert int(ss.scored_e(np.array([0xFFFFFFFF]), np.array([(1 << 62) - 1], np.uint64))[0]) == ref.scored_e(0xFFFFFFFF, (1 << 62) - 1) < 1 << 64
    for M in range(5):
        c = [3] + [j + 1 for j in range(M)]
        want = 3 << 48
        for j in range(1, M + 1):
            want |= j << (48 - 12 * j)
        assert ref.packed_e(c) == want == int(ss.packed_e(np.array([c], np.uint32))[0])
    # saturation exactly at 65 535 / 65 536 and 4 095 / 4 096
    assert ref.packed_e([65534, 0]) < ref.packed_e([65535, 0]) == ref.packed_e([65536, 0]) == ref.packed_e([0xFFFFFFFF, 0])
    assert ref.packed_e([0, 4094]) < ref.packed_e([0, 4095]) == ref.packed_e([0, 4096]) == ref.packed_e([0, 0xFFFFFFFF])
    assert ref.packed_e([0, 4096, 0, 0, 1]) > ref.packed_e([0, 4095, 0, 0, 0]) and ref.packed_e([1, 0, 0, 0, 0]) > ref.packed_e([0, 4095] * 2 + [4095])
    assert ref.packed_e([65535] + [4095] * 4) == (1 << 64) - 1
    big = np.array([[65536, 4096, 4095, 5000, 7], [65535, 4095, 4095, 4095, 7]], np.uint32)
    assert int(ss.packed_e(big)[0]) == int(ss.packed_e(big)[1]) == ref.packed_e(big[0])


@pytest.mark.parametrize("T, P, pam3", [(23, 3, True), (27, 4, False)])
def test_cut_letter_rule(T, P, pam3):
    for c in (1, T - 1):
        assert ss.check_cut(c, T, P, pam3) == c
        got = ss.cut_letter(np.array([100, 100]), np.array([0, 1]), T, c)
        assert got.tolist() == [100 + c, 100 + T - c] == ref.cut_letters([100, 100], [0, 1], T, c).tolist()
        # the mirror: the '-' site's oriented position c is forward letter start + T - 1 - c, and the cut lies behind it
        assert got[1] == 100 + (T - 1 - c) + 1
    for c in (0, T, -1, True, 2.0):
        with pytest.raises(ValueError):
            ss.check_cut(c, T, P, pam3)
    if pam3:  # ...NGG, c = 17: section 16's i - 3 on '+' (i = start + 20), the true mirror j + 6 on '-'
        assert ss.cut_letter(50, 0, 23, 17) == 50 + 20 - 3 and ss.cut_letter(50, 1, 23, 17) == 50 + 6


def test_default_cut():
    assert ss.default_cut(23, 3, True) == 17 == ref.default_cut(23, 3, True)
    assert ss.default_cut(27, 4, False) == 22 == ref.default_cut(27, 4, False)  # Cas12a: 18 letters behind the PAM
    assert ss.default_cut(32, 3, True) == 26 and ss.default_cut(7, 3, True) == 1
    assert ss.default_cut(10, 4, False) == 4 + 5 and ss.default_cut(27, 6, True) == 18
    for T, P, pam3 in ((23, 3, True), (27, 4, False), (32, 3, True), (7, 3, True), (8, 4, False), (5, 1, True), (5, 1, False)):
        if T - P >= 4 or not pam3:
            assert 1 <= ss.check_cut(None, T, P, pam3) <= T - 1


def test_percent_to_count():
    assert ss.gc_bounds(None, None, 23) == (0, ss.NO_LIMIT)
    assert ss.gc_bounds(40, 60, 20) == (8, 12)
    assert ss.gc_bounds(40, 60, 23) == (10, 13)   # ceil(9.2), floor(13.8)
    assert ss.gc_bounds(0, 100, 29) == (0, 29) and ss.gc_bounds(100, None, 4) == (4, ss.NO_LIMIT)
    assert ss.gc_bounds(1, 99, 23) == (1, 22)


BASE = ["-f", "genome.fa", "--pattern", "TTTV" + "N" * 23, "--pam-length", "4", "-m", "3"]
REFUSALS = [
    (BASE + ["--self", "-o", "o", "--select", "5"], "needs -g"),
    (BASE + ["--guides", "g.txt", "-o", "o", "--select", "5", "-g", "x.gff"], "belongs to --self"),
    (BASE + ["--self", "-o", "o", "--cut-offset", "5"], "--cut-offset belongs to --select"),
    (BASE + ["--self", "-o", "o", "-g", "x.gff"], "-g/--gff belongs to --select"),
    (BASE + ["--self", "-o", "o", "--select-output", "s"], "--select-output belongs to --select"),
    (BASE + ["--self", "-o", "o", "--select-max-perfect", "0"], "--select-max-perfect belongs to --select"),
    (BASE + ["--self", "-o", "o", "--select-min-specificity", "0.5"], "--select-min-specificity belongs to --select"),
    (BASE + ["--self", "-o", "o", "--select-cds"], "--select-cds belongs to --select"),
    (BASE + ["--self", "-o", "o", "--select-gc-min", "40"], "--select-gc-min belongs to --select"),
    (BASE + ["--self", "-o", "o", "--select-gc-max", "60"], "--select-gc-max belongs to --select"),
    (BASE + ["--self", "-o", "o", "--select-max-t-run", "3"], "--select-max-t-run belongs to --select"),
    (BASE + ["--self", "-o", "o", "--select-only"], "--select-only belongs to --select"),
    (BASE + ["--guides", "g.txt", "-o", "o", "--select-cds"], "--select-cds belongs to --select"),
    (BASE + ["--self", "-o", "o", "-g", "x.gff", "--select", "0"], "K must be 1..64"),
    (BASE + ["--self", "-o", "o", "-g", "x.gff", "--select", "65"], "K must be 1..64"),
    (BASE + ["--self", "-o", "o", "-g", "x.gff", "--select", "5", "--cut-offset", "0"], "cut offset must be 1..26"),
    (BASE + ["--self", "-o", "o", "-g", "x.gff", "--select", "5", "--cut-offset", "27"], "cut offset must be 1..26"),
    (BASE + ["--self", "-o", "o", "-g", "x.gff", "--select", "5", "--select-min-specificity", "0.5"], "needs a scored search"),
    (BASE + ["--self", "-o", "o", "-g", "x.gff", "--select", "5", "--select-gc-min", "70", "--select-gc-max", "30"], "gc_min"),
    (BASE + ["--self", "-g", "x.gff", "--select", "5"], "needs -o/--output"),
    (BASE + ["--self", "-g", "x.gff", "--select", "5", "--select-only"], "needs -o/--output"),
]


@pytest.mark.parametrize("argv, text", REFUSALS, ids=[str(k) for k in range(len(REFUSALS))])
def test_command_line_refusals(argv, text, capsys, monkeypatch):
    """Refused through ap.error before anything is read or the GPU is opened: none of the named files exists."""
    import cropsr_amd.engine as engine
    monkeypatch.setattr(engine, "Engine", lambda *a, **k: pytest.fail("the GPU was opened"))
    with pytest.raises(SystemExit) as e:
        srch.main(argv)
    assert e.value.code == 2
    assert text in capsys.readouterr().err


def test_self_without_select_writes_unchanged_bytes():
    sites = np.zeros(3, srch.SELF_SITE_DTYPE)
    sites["contig"], sites["position"], sites["strand"] = [0, 0, 1], [5, 9, 0], [b"+", b"-", b"+"]
    for scored in (False, True):
        res = srch.SelfSearchResult(sites, np.array([b"ACGT", b"TTTT", b"GGCA"]), np.array([[0, 1], [2, 0], [0, 0]], np.uint32),
                                    np.array([0, 1 << 30, 3 << 29], np.uint64) if scored else None, (3, 1), (4, 12))
        assert res.selection is None
        text = "".join(srch.format_self(["chrA", "chrB"], res))
        want = ("contig\tposition\tstrand\tguide\tn0\tn1" + ("\thit_sum\tspecificity" if scored else "") + "\n" +
                "chrA\t5\t+\tACGT\t0\t1" + ("\t0.000000\t1.000000" if scored else "") + "\n" +
                "chrA\t9\t-\tTTTT\t2\t0" + ("\t1.000000\t0.500000" if scored else "") + "\n" +
                "chrB\t0\t+\tGGCA\t0\t0" + ("\t1.500000\t0.400000" if scored else "") + "\n")
        assert text == want


def test_format_selection():
    rows = np.zeros(2, ss.ROW_DTYPE)
    rows["gene"], rows["rank"], rows["contig"], rows["position"], rows["strand"], rows["cut"] = [1, 1], [1, 2], [0, 1], [5, 7], [b"+", b"-"], [22, 13]
    s = ss.Selection(["gene:a", "gene:b"], np.array([0, 9]), np.array([0, 4]), rows, np.array([b"ACGT", b"TTGA"]),
                     np.array([[0, 2], [1, 0]], np.uint32), np.array([1 << 30, 0], np.uint64), np.array([1 << 30, 1 << 30], np.uint64))
    assert ss.format_selection(["c0", "c1"], s) == ("gene\trank\tpassing\tcontig\tposition\tstrand\tguide\tcut\tn0\tn1\thit_sum\tspecificity\n"
                                                    "gene:b\t1\t4\tc0\t5\t+\tACGT\t22\t0\t2\t1.000000\t0.500000\n"
                                                    "gene:b\t2\t4\tc1\t7\t-\tTTGA\t13\t1\t0\t0.000000\t1.000000\n")


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


class Session:
    """The self search of one genome under one pattern: the open handles and, per arena, the fetched rows of its guide sites."""

    def __init__(self, engine, pid, M, scored, three, contigs=None):
        pattern, gp, P, pam3, c = cases.PATTERNS[pid]
        self.pattern, self.P, self.pam3, self.M, self.scored = pattern, P, pam3, M, scored
        self.T, self.G = len(pattern), len(pattern) - P
        self.c = ref.default_cut(self.T, P, pam3) if c is None else c
        self.region = ref.region_mask(self.T, P, pam3)
        score = None if not scored else ("hsu2013" if self.G == 20 else W[self.G])
        self.contigs = cases.genome() if contigs is None else contigs
        self.genome = engine.genome(self.contigs, max_words=480) if three else engine.genome(self.contigs)
        assert len(self.genome.arenas) == (3 if three else 1)
        self.handles = []
        try:
            pattern, gpat, M, P, scheme = srch.check_self(pattern, M, P, gp, score)
            srch._self_handles(self.genome, pattern, gpat, P, M, scheme, None, None, self.handles)
            srch._self_compare_all(self.handles, M)
            self.rows = []
            for a, h in enumerate(self.handles):
                pos, strand, hi, lo, counts, hs = h.fetch(scored)
                # every candidate of the arena in extraction order, stated on the letters; the handle counts as many
                arena = self.genome.arenas[a]
                cpos, cstrand = cases.candidates([self.contigs[t] for t in self.genome.groups[a]], arena.offsets, pattern)
                n_plus, n_minus, n_guides = h.sizes()
                assert (n_plus, n_minus, n_guides) == (int((cstrand == 0).sum()), int((cstrand == 1).sum()), pos.size)
                where = {(int(p), int(st)): i for i, (p, st) in enumerate(zip(cpos, cstrand))}
                cand = np.array([where[(int(p), int(st))] for p, st in zip(pos, strand)], np.uint32)
                assert (np.diff(cand.astype(np.int64)) > 0).all()
                self.rows.append(dict(pos=pos, strand=strand, hi=hi, lo=lo, counts=counts, hit_sum=hs, cand=cand))
        except BaseException:
            self.close()
            raise

    def close(self):
        for h in self.handles:
            h.close()
        self.genome.close()

    def spec(self, k, **kw):
        return ref.spec(self.T, self.c, self.region, k, **kw)


@pytest.fixture(scope="module")
def sessions(engine):
    made = {}

    def get(pid, M, scored, three=False):
        key = (pid, M, scored, three)
        if key not in made:
            made[key] = Session(engine, pid, M, scored, three)
        return made[key]

    yield get
    for s in made.values():
        s.close()


def native(sp, require_cds=False):
    return nat.SelectSelfParams(sp["max_hit_sum"], sp["max_mm0"], sp["k"], sp["c"], int(require_cds), sp["gc_min"], sp["gc_max"], sp["max_t_run"], 0)


def run_gpu(s, a, lo, hi, sp, slice_rows=0, items_per_launch=0, sel=None):
    """(fetch_self()'s dict, stats) of one run on arena a of session s (sel: an open ArenaSelect to reuse)."""
    own = sel is None
    if own:
        sel = sel_mod.ArenaSelect(s.genome.arenas[a], lo, hi)
    try:
        sel.set_limits(slice_rows)
        sel.set_self_limits(items_per_launch)
        if sp["track"] is not None:
            points, ids, flags = sp["track"]
            s.genome.arenas[a].annotate_set_track(points, ids)
            sel.set_flags(flags)
        sel.run_self(native(sp, sp["track"] is not None), s.handles[a])
        return sel.fetch_self(), sel.self_stats()
    finally:
        if own:
            sel.close()


def assert_equal(s, a, got, want, sp):
    """sel, n_in, n_pass and the gathered fields of a GPU result against the reference's (n_in, n_pass, sel)."""
    n_in, n_pass, sel = want
    assert np.array_equal(got["n_in"], n_in) and np.array_equal(got["n_pass"], n_pass)
    assert np.array_equal(got["sel"], sel)
    rows = s.rows[a]
    row_of = np.full(int(rows["cand"].max()) + 1 if rows["cand"].size else 1, -1, np.int64)
    row_of[rows["cand"]] = np.arange(rows["cand"].size)
    have = sel != NONE
    r = row_of[sel[have]]
    assert (r >= 0).all()
    assert np.array_equal(got["arena_pos"][have], rows["pos"][r]) and np.array_equal(got["strand"][have], rows["strand"][r])
    assert np.array_equal(got["hi"][have], rows["hi"][r]) and np.array_equal(got["lo"][have], rows["lo"][r])
    assert np.array_equal(got["counts"][have], rows["counts"][r])
    if rows["hit_sum"] is not None:
        assert np.array_equal(got["hit_sum"][have], rows["hit_sum"][r])
    for key in ("arena_pos", "hi", "lo"):
        assert (got[key][~have] == NONE).all()
    assert (got["strand"][~have] == 0xFF).all() and (got["counts"][~have] == NONE).all()


SESSIONS = [("ngg", 3, True, False), ("ngg", 4, False, True), ("ngg", 0, True, True), ("cas12a", 3, True, False), ("cas12a", 0, False, True),
            ("t32", 4, False, False), ("t32", 3, True, True), ("tiny", 0, False, False), ("tiny", 3, True, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [0, 64])
@pytest.mark.parametrize("K", [1, 5, 64])
@pytest.mark.parametrize("key", SESSIONS, ids=["%s-M%d-%s-%s" % (p, m, "scored" if sc else "counts", "3arenas" if t else "1arena")
                                               for p, m, sc, t in SESSIONS])
def test_gene_sizes_and_edges(sessions, key, K, slice_rows):
    """Genes of 0, 1, K - 1, K, K + 1, 63, 64, 65 and 129 guide sites, and the edge, nested, overlapping, duplicate and one-strand
    genes, on every arena of the session."""
    s = sessions(*key)
    sizes = sorted({0, 1, max(K - 1, 0), K, K + 1, 63, 64, 65, 129})
    for a, rows in enumerate(s.rows):
        arena = s.genome.arenas[a]
        few = rows["pos"].size < 400  # (a short arena of a sparse pattern: the sizes it can hold)
        use = [n for n in sizes if not few or n <= 5]
        lo1, hi1 = cases.size_genes(rows, s.T, s.c, use)
        names, lo2, hi2 = cases.edge_genes(rows, s.T, s.c, arena.offsets, arena.lengths)
        lo, hi = np.concatenate([lo1, lo2]), np.concatenate([hi1, hi2])
        sp = s.spec(K)
        want = ref.select_numpy(rows, lo, hi, sp)
        # the claims, on the reference: the sizes; the one-letter genes hold one strand; the clamped bound and the arena's ends
        assert want[0][:len(use)].tolist() == use
        cut = ref.cut_letters(rows["pos"], rows["strand"], s.T, s.c)
        for name, strand in (("plus-in-minus-out", 0), ("minus-in-plus-out", 1), ("plus-only", 0), ("minus-only", 1)):
            if name in names:
                g = len(use) + names[name]
                inside = (cut >= lo[g]) & (cut <= hi[g])
                assert inside.any() and (rows["strand"][inside] == strand).all(), name
        assert {"lo-below-T", "first-candidate", "last-candidate", "whole-contig", "duplicate", "nested"} <= set(names)
        g0 = len(use)
        assert want[0][g0 + names["first-candidate"]] >= 1 and want[0][g0 + names["last-candidate"]] >= 1
        assert want[0][g0 + names["whole-arena"]] == rows["pos"].size
        assert np.array_equal(want[2][g0 + names["nested"]], want[2][g0 + names["duplicate"]])
        assert lo[g0 + names["lo-0-mod-64"]] % 64 == 0 and lo[g0 + names["lo-63-mod-64"]] % 64 == 63
        assert hi[g0 + names["hi-0-mod-64"]] % 64 == 0 and hi[g0 + names["hi-63-mod-64"]] % 64 == 63
        got, stats = run_gpu(s, a, lo, hi, sp, slice_rows)
        assert_equal(s, a, got, want, sp)
        if slice_rows == 64 and not few:
            assert stats["self_items"] > len(lo)  # genes were cut, and merged


@pytest.mark.gpu
def test_non_guide_candidates_are_ignored(sessions):
    """...NRG candidates against ...NGG guides: inside a gene lie candidates that are no guide sites, and sel skips them."""
    s = sessions("ngg", 3, True)
    rows = s.rows[0]
    assert not np.array_equal(rows["cand"], np.arange(rows["cand"].size))
    # a gene around a stretch where candidate indices jump: non-guide candidates lie between its guide sites
    jump = int(np.nonzero(np.diff(rows["cand"].astype(np.int64)) > 1)[0][5])
    cut = ref.cut_letters(rows["pos"], rows["strand"], s.T, s.c)
    lo, hi = np.array([cut[jump - 3:jump + 4].min()], np.uint32), np.array([cut[jump - 3:jump + 4].max()], np.uint32)
    sp = s.spec(64)
    want = ref.select_numpy(rows, lo, hi, sp)
    picked = want[2][0][want[2][0] != NONE]
    assert picked.size >= 7 and picked.max() - picked.min() + 1 > want[0][0]  # more candidates in the span than guide sites
    got, _ = run_gpu(s, 0, lo, hi, sp)
    assert_equal(s, 0, got, want, sp)


@pytest.mark.gpu
@pytest.mark.parametrize("scored", [True, False])
def test_ties_are_decided_by_the_tie_word(sessions, scored):
    """The tandem repeats give at least 65 rows of equal e per strand; a '+' and a '-' site share a cut letter."""
    s = sessions("ngg", 3, True) if scored else sessions("ngg", 4, False, True)
    for a, rows in enumerate(s.rows):
        arena = s.genome.arenas[a]
        cut = ref.cut_letters(rows["pos"], rows["strand"], s.T, s.c)
        e = ref.row_keys(rows)
        genes = []
        for text, at, strand in ((0, 9000, 0), (2, 10000, 1)):
            where = [j for j, grp in enumerate(s.genome.groups) if text in grp]
            if where != [a]:
                continue
            off = int(arena.offsets[list(s.genome.groups[a]).index(text)])
            lo, hi = off + at + 30, off + at + 23 * cases.REPEATS - 30
            inside = (cut >= lo) & (cut <= hi) & (rows["strand"] == strand)
            top = sorted(e[inside].tolist())
            assert inside.sum() >= 65 and top[0] == top[64]  # 65 equal rows of the best e on this strand
            genes.append((lo, hi))
        where = [j for j, grp in enumerate(s.genome.groups) if 1 in grp]
        if where == [a]:
            off = int(arena.offsets[list(s.genome.groups[a]).index(1)])
            shared = off + cases.SHARED_AT + 17
            both = rows["strand"][cut == shared]
            assert sorted(both.tolist()) == [0, 1]  # a '+' and a '-' site cut before the same letter
            genes.append((shared, shared))
        if not genes:
            continue
        lo, hi = np.array([g[0] for g in genes], np.uint32), np.array([g[1] for g in genes], np.uint32)
        for K in (5, 64):
            sp = s.spec(K)
            want = ref.select_numpy(rows, lo, hi, sp)
            for slice_rows in (0, 64):
                got, _ = run_gpu(s, a, lo, hi, sp, slice_rows)
                assert_equal(s, a, got, want, sp)


@pytest.mark.gpu
def test_thresholds_and_filters(sessions):
    """Thresholds that pass nothing and exactly K; each of the CDS, GC and T-run limits changes the result on the reference."""
    s = sessions("ngg", 3, True)
    rows, arena = s.rows[0], s.genome.arenas[0]
    K = 5
    cuts, order = cases.sorted_cuts(rows, s.T, s.c)
    # gene 0: the K sites before text 0's tandem repeat (no perfect copy elsewhere) and 31 sites of the repeat (69 or more each);
    # gene 1: wholly inside the repeat; genes 2, 3: 129 and 64 sites of the random text
    c0 = rows["counts"][order, 0]
    first = int(np.nonzero(c0 >= cases.REPEATS - 1)[0][0])
    assert (c0[first - K:first] == 0).all() and (c0[first:first + 31] >= cases.REPEATS - 1).all() and cuts[first - K - 1] < cuts[first - K]
    lo2, hi2 = cases.size_genes(rows, s.T, s.c, [129, 64])
    lo = np.concatenate([np.array([cuts[first - K], cuts[first + 5]], np.uint32), lo2])
    hi = np.concatenate([np.array([cuts[first + 30], cuts[first + 25]], np.uint32), hi2])
    plain = ref.select_numpy(rows, lo, hi, s.spec(K))
    end = int(arena.offsets[-1] + arena.lengths[-1])
    track = (np.arange(0, end, 97, dtype=np.uint32), (np.arange(len(range(0, end, 97))) % 4).astype(np.uint32), np.array([0, 1, 0, 0], np.uint8))
    nothing_cds = (np.array([0], np.uint32), np.array([2], np.uint32), np.array([0, 1, 0, 0], np.uint8))  # no CDS anywhere
    top = int(rows["hit_sum"].max())
    for name, extra in (("exactly-K", dict(max_mm0=0)), ("exactly-K-sum", dict(max_mm0=0, max_hit_sum=top)), ("nothing", dict(gc_min=21)),
                        ("cds", dict(track=track)), ("cds-free", dict(track=nothing_cds)), ("gc", dict(gc_min=9, gc_max=11)),
                        ("t-run", dict(max_t_run=2)),
                        ("all", dict(track=track, gc_min=6, gc_max=14, max_t_run=3, max_mm0=1, max_hit_sum=top))):
        sp = s.spec(K, **extra)
        want = ref.select_numpy(rows, lo, hi, sp)
        if name.startswith("exactly-K"):
            assert want[1][0] == K < want[0][0] and want[1][1] == 0 < want[0][1]  # gene 0: exactly K pass; gene 1: nothing does
        elif name.startswith("nothing") or name == "cds-free":
            assert (want[1] == 0).all() and (want[0] > 0).all()
        else:
            assert not np.array_equal(want[2], plain[2]) and want[1].sum() > 0, name  # the limit changes the result
        for slice_rows in (0, 64):
            got, _ = run_gpu(s, 0, lo, hi, sp, slice_rows)
            assert_equal(s, 0, got, want, sp)


@pytest.mark.gpu
def test_multi_launch_and_slices(sessions):
    """Slices of 64 and two items a launch: a cut gene's items lie on both sides of a launch boundary."""
    s = sessions("ngg", 3, True)
    rows = s.rows[0]
    lo, hi = cases.size_genes(rows, s.T, s.c, [129, 1, 65, 129, 0])
    for K in (1, 64):
        sp = s.spec(K)
        want = ref.select_numpy(rows, lo, hi, sp)
        got, stats = run_gpu(s, 0, lo, hi, sp, 64, 2)
        assert stats["self_items"] >= 9 and stats["self_launches"] == -(-int(stats["self_items"]) // 2)  # gene 0: 3+ items, launches of 2
        assert_equal(s, 0, got, want, sp)
        one, st1 = run_gpu(s, 0, lo, hi, sp)
        assert st1["self_launches"] == 1 and st1["self_items"] == len(lo)
        for key in got:
            assert np.array_equal(got[key], one[key]), key


@pytest.mark.gpu
def test_handle_reuse_and_refusals(engine, sessions):
    """A smaller K after a larger one, limits set and cleared, section 16's run before and after on an arena that also has scan
    tables, and the refusals: none touches the other results."""
    s = sessions("ngg", 3, True)
    rows, arena = s.rows[0], s.genome.arenas[0]
    arena.scan_score_device(20)
    lo, hi = cases.size_genes(rows, s.T, s.c, [129, 64, 5, 0])
    sel = sel_mod.ArenaSelect(arena, lo, hi)
    other = engine.genome([cases.genome()[3]])
    try:
        sel.run(sel_mod.Params(5))
        before = sel.fetch()
        assert before[1].sum() > 0
        with pytest.raises(nat.CropsrHipError, match="no crp_select_run_self"):
            sel.fetch_self()
        for K, extra in ((64, {}), (5, {}), (5, dict(gc_min=9, gc_max=11, max_t_run=2)), (5, {}), (1, dict(max_mm0=0))):
            sp = s.spec(K, **extra)
            got, _ = run_gpu(s, 0, lo, hi, sp, sel=sel)
            assert_equal(s, 0, got, ref.select_numpy(rows, lo, hi, sp), sp)
        kept = sel.fetch_self()
        for bad, text in ((dict(k=0), "k must be 1..64"), (dict(k=65), "k must be 1..64"), (dict(c=0), "cut offset must be 1..22"),
                          (dict(c=23), "cut offset must be 1..22"), (dict(gc_min=12, gc_max=11), "gc_min")):
            sp = dict(s.spec(5), **bad)
            with pytest.raises(nat.CropsrHipError, match=text):
                sel.run_self(native(sp), s.handles[0])
        with pytest.raises(nat.CropsrHipError, match="require_cds needs"):
            sel.run_self(native(s.spec(5), True), s.handles[0])
        # a handle of another arena, and one that has not been through every segment's compare
        fresh = []
        try:
            pattern, gp, M, P, scheme = srch.check_self(s.pattern, 3, 3, cases.PATTERNS["ngg"][1], None)
            srch._self_handles(other, pattern, gp, P, M, None, None, None, fresh)
            with pytest.raises(nat.CropsrHipError, match="another arena"):
                sel.run_self(native(s.spec(5)), fresh[0])
            osel = sel_mod.ArenaSelect(other.arenas[0], lo[:1] * 0, hi[:1] * 0 + 100)
            try:
                with pytest.raises(nat.CropsrHipError, match="every segment"):
                    osel.run_self(native(s.spec(5)), fresh[0])
                for j in range(M):  # all but the last segment: still refused
                    fresh[0].order(j)
                    fresh[0].compare(fresh[0])
                with pytest.raises(nat.CropsrHipError, match="every segment"):
                    osel.run_self(native(s.spec(5)), fresh[0])
                fresh[0].order(M)
                fresh[0].compare(fresh[0])
                osel.run_self(native(s.spec(5)), fresh[0])  # no scan tables on this arena: none are needed
                assert osel.fetch_self()["n_in"][0] >= 0
            finally:
                osel.close()
        finally:
            for h in fresh:
                h.close()
        # a refusal resets this run's own result and nothing else; section 16's run is what it was, before and after
        with pytest.raises(nat.CropsrHipError, match="no crp_select_run_self"):
            sel.fetch_self()
        after = sel.fetch()
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        got, _ = run_gpu(s, 0, lo, hi, s.spec(1, max_mm0=0), sel=sel)
        for key in kept:
            assert np.array_equal(got[key], kept[key]), key
        sel.run(sel_mod.Params(5))
        for x, y in zip(before, sel.fetch()):
            assert np.array_equal(x, y)
    finally:
        sel.close()
        other.close()


@pytest.mark.gpu
def test_saturated_counts(engine):
    """counts[0] above 65 535 (a poly-G text) and a count of one mismatch above 4 095 (two repeat families), both unscored: the
    saturating comparison, and nothing else, orders the picked rows."""
    s = Session(engine, "ngg", 1, False, False, contigs=cases.saturation_c0())
    try:
        rows = s.rows[0]
        c0 = rows["counts"][:, 0].astype(np.int64)
        # the text holds what it claims: two classes above 65 535 with different raw counts (the repeat family, first in the
        # text, has MORE copies than the poly-G run), and a small family in between
        big = sorted(set(c0[c0 > 65535].tolist()))
        assert (c0 > 65535).sum() > 2 * 65536 and len(big) >= 2 and (rows["strand"] == 0).all()
        assert (c0 == cases.SMALL_COPIES - 1).sum() == cases.SMALL_COPIES
        off = int(s.genome.arenas[0].offsets[0])
        lo, hi = np.array([off, off + 30000], np.uint32), np.array([off + len(s.contigs[0]) - 1, off + 30100], np.uint32)
        sp = s.spec(64)
        want = ref.select_numpy(rows, lo, hi, sp)
        # on the fetched rows: the saturating key, and neither the raw counts nor a 16-bit field that merely truncates, gives
        # this order -- raw counts put the poly-G sites (fewer copies) before the repeat family, a truncated field puts both
        # classes (65 5xx mod 65 536 is small) before the small family
        cut = ref.cut_letters(rows["pos"], rows["strand"], s.T, s.c)
        c1 = np.minimum(rows["counts"][:, 1].astype(np.int64), 4095)
        tie = cut * 2 + rows["strand"]

        def top(field0):
            order = np.lexsort((tie, c1, field0))[:64]
            return rows["cand"][order].tolist()

        saturated, raw, truncated = top(np.minimum(c0, 65535)), top(c0), top(c0 & 0xFFFF)
        assert want[2][0].tolist() == saturated and saturated != raw and saturated != truncated and raw != truncated
        picked_c0 = c0[np.isin(rows["cand"], want[2][0])]
        assert (picked_c0 > 65535).any() and (picked_c0 == cases.SMALL_COPIES - 1).sum() == cases.SMALL_COPIES  # both classes in play
        assert picked_c0[picked_c0 > 65535].max() == big[-1]  # saturated, the family with MORE copies leads: the cut letter decided
        got, _ = run_gpu(s, 0, lo, hi, sp)
        assert_equal(s, 0, got, want, sp)
        got, _ = run_gpu(s, 0, lo, hi, sp, 64)
        assert_equal(s, 0, got, want, sp)
    finally:
        s.close()
    s = Session(engine, "ngg", 1, False, False, contigs=cases.saturation_c1())
    try:
        rows = s.rows[0]
        odd = np.nonzero((rows["counts"][:, 0] == 0) & (rows["counts"][:, 1] > 4095))[0]
        assert odd.size == 2 and rows["counts"][odd[0], 1] > rows["counts"][odd[1], 1]  # 4 200 hits first in the text, then 4 100
        cut = ref.cut_letters(rows["pos"], rows["strand"], s.T, s.c)
        off = int(s.genome.arenas[0].offsets[0])
        lo, hi = np.array([off], np.uint32), np.array([off + len(s.contigs[0]) - 1], np.uint32)
        sp = s.spec(64)
        want = ref.select_numpy(rows, lo, hi, sp)
        # raw counts would put the 4 100 site first; saturated they tie and the smaller cut letter wins
        picked = want[2][0].tolist()
        first, second = int(rows["cand"][odd[0]]), int(rows["cand"][odd[1]])
        assert first in picked and second in picked and picked.index(first) + 1 == picked.index(second) and cut[odd[0]] < cut[odd[1]]
        raw = sorted(range(rows["pos"].size), key=lambda i: (tuple(int(v) for v in rows["counts"][i]), int(cut[i])))
        assert raw.index(int(odd[1])) < raw.index(int(odd[0]))
        for slice_rows in (0, 64):
            got, _ = run_gpu(s, 0, lo, hi, sp, slice_rows)
            assert_equal(s, 0, got, want, sp)
    finally:
        s.close()


GFF = """##gff-version 3
c0\ttest\tgene\t2001\t9000\t.\t+\t.\tID=g1
c0\ttest\tCDS\t2500\t4000\t.\t+\t0\tParent=g1
c0\ttest\tCDS\t6000\t7000\t.\t+\t0\tParent=g1
c1\ttest\tgene\t100\t4000\t.\t-\t.\tID=g2
c1\ttest\tCDS\t200\t3900\t.\t-\t0\tParent=g2
c2\ttest\tgene\t50\t60\t.\t+\t.\tID=g3
ghost\ttest\tgene\t1\t100\t.\t+\t.\tID=g4
c3\ttest\tgene\t1\t5003\t.\t+\t.\tID=g5
c3\ttest\tCDS\t1000\t4000\t.\t+\t0\tParent=g5
"""


def reference_selection_text(engine, contigs, names, gff_path, pattern, P, M, score, sp):
    """(the selection file, the sites TSV) that select_self.format_selection and search.format_self must give for a genome:
    the plain self search of the genome in ONE arena, the numpy reference over its rows per layout row, and the definition's
    rule for a gene met in several texts (summed counts, rows by e, then the texts in order, then the tie word; the first K).
    sp: ref.spec without its track (require_cds: sp["track"] is True)."""
    from cropsr_amd import annotate
    T = len(pattern)
    glo = 0 if set(pattern[:T - P]) <= {"N"} else P
    g = engine.genome(contigs)
    try:
        assert len(g.arenas) == 1
        res = srch.search_self(g, pattern, M, P, score=score)
        arena = g.arenas[0]
        ann = annotate.Annotation(str(gff_path))
        req = annotate.Request(ann, names, 0)
        layout = sel_mod.arena_layout(g, 0)
        lo, hi, gene = req.gene_layout(layout)
        track = (req.track(layout) + (ann.cds_flags(),)) if sp["track"] else None
        labels = ann.genes()[0]
        ann.close()
        offs = np.asarray(arena.offsets, np.int64)
    finally:
        g.close()
    # the rows of the search, in extraction order, from the result (one arena: arena position = offset + position)
    pos = offs[res.sites["contig"]] + res.sites["position"]
    strand = (res.sites["strand"] == b"-").astype(np.uint8)
    order = np.argsort(((pos >> 6) << 7) | (strand.astype(np.int64) << 6) | (pos & 63), kind="stable")
    table = {b"A": 0, b"T": 1, b"C": 2, b"G": 3}
    hi_bits, lo_bits = np.zeros(pos.size, np.uint32), np.zeros(pos.size, np.uint32)
    for i, gd in enumerate(res.guides):
        for k in range(T - P):
            code = table[gd[k:k + 1]]
            hi_bits[i] |= np.uint32((code >> 1) << (glo + k))
            lo_bits[i] |= np.uint32((code & 1) << (glo + k))
    rows = dict(pos=pos[order], strand=strand[order], hi=hi_bits[order], lo=lo_bits[order], counts=res.counts[order],
                hit_sum=None if res.hit_sum is None else res.hit_sum[order], cand=np.arange(pos.size, dtype=np.uint32))
    sp = dict(sp, track=track)
    n_in, n_pass, sel = ref.select_numpy(rows, lo, hi, sp)
    e = ref.row_keys(rows)
    cut = ref.cut_letters(rows["pos"], rows["strand"], T, sp["c"])
    per_gene = {}
    for r in range(len(lo)):
        entry = per_gene.setdefault(int(gene[r]), [0, []])
        entry[0] += int(n_pass[r])
        entry[1] += [(e[c], r, int(cut[c]) * 2 + int(rows["strand"][c]), int(order[c])) for c in sel[r][sel[r] != NONE]]
    head = ["gene", "rank", "passing", "contig", "position", "strand", "guide", "cut"] + ["n%d" % j for j in range(M + 1)]
    lines = ["\t".join(head + (["hit_sum", "specificity"] if score is not None else []))]
    for gi in sorted(per_gene):
        passing, picked = per_gene[gi]
        for rank, (_, _, _, i) in enumerate(sorted(picked)[:sp["k"]]):
            cutl = int(ref.cut_letters(pos[i], strand[i], T, sp["c"])) - int(offs[res.sites["contig"][i]])
            f = [labels[gi], str(rank + 1), str(passing), names[int(res.sites["contig"][i])], str(int(res.sites["position"][i])),
                 res.sites["strand"][i].decode(), res.guides[i].decode(), str(cutl)] + [str(int(v)) for v in res.counts[i]]
            if score is not None:
                f += ["%.6f" % (float(res.hit_sum[i]) / (1 << 30)), "%.6f" % float(res.specificity[i])]
            lines.append("\t".join(f))
    return "\n".join(lines) + "\n", "".join(srch.format_self(names, res)), (n_in, n_pass, gene, len(labels))


@pytest.mark.gpu
def test_command_line_end_to_end(engine, tmp_path):
    """One small FASTA + GFF through python -m cropsr_amd.search --self --select, the selection file line by line against the
    reference's result over the rows of the same search."""
    contigs = cases.genome()
    names = ["c0", "c1", "c2", "c3"]
    fa, gff, wts = tmp_path / "g.fa", tmp_path / "g.gff3", tmp_path / "w23.txt"
    fa.write_bytes(b"".join(b">" + n.encode() + b" x\n" + c + b"\n" for n, c in zip(names, contigs)))
    gff.write_text(GFF)
    wts.write_text(" ".join(str(v) for v in W[23]) + "\n")
    pattern = "TTTV" + "N" * 23
    out, sel_out = tmp_path / "sites.tsv", tmp_path / "sites.tsv.selected.tsv"
    argv = ["-f", str(fa), "--pattern", pattern, "--pam-length", "4", "--self", "-m", "3", "--weights", str(wts), "-g", str(gff), "--select", "5",
            "--select-cds", "--select-max-perfect", "0", "--select-max-t-run", "3", "-o", str(out)]
    assert srch.main(argv) == 0
    sp = ref.spec(27, 22, ref.region_mask(27, 4, False), 5, max_mm0=0, max_t_run=3, track=True)
    want, sites_text, (n_in, n_pass, gene, n_labels) = reference_selection_text(engine, contigs, names, gff, pattern, 4, 3, W[23], sp)
    assert out.read_text() == sites_text  # the sites TSV is what it is without --select
    assert n_pass.sum() > 5 and (n_pass < n_in).any() and n_labels == 5 and len(gene) == 4  # the ghost gene has no row
    assert sel_out.read_text().split("\n") == want.split("\n")
    # --select-only writes the selection alone, and copies no per-site row to the host
    only = tmp_path / "only.tsv"
    assert srch.main(argv[:-2] + ["--select-only", "--select-output", str(only)]) == 0
    assert only.read_text() == sel_out.read_text() and not (tmp_path / "only.tsv.selected.tsv").exists()


GFF_TWO_TEXTS = """##gff-version 3
c0\ttest\tgene\t10031\t10570\t.\t+\t.\tID=rep
c0\ttest\tgene\t2001\t9000\t.\t+\t.\tID=g1
c1\ttest\tgene\t100\t4000\t.\t-\t.\tID=g2
c3\ttest\tgene\t1\t5003\t.\t+\t.\tID=g5
ghost\ttest\tgene\t1\t100\t.\t+\t.\tID=g4
"""


@pytest.mark.gpu
@pytest.mark.parametrize("scored", [True, False])
def test_search_self_select_over_three_arenas(engine, tmp_path, scored):
    """search_self(select=) and the host's assemble over three arenas against the per-row reference.  Texts 0 and 2 carry one
    FASTA name and lie in different arenas; the gene `rep` covers the '+' tandem repeat of the one and the '-' repeat of the other
    -- one guide, so equal e in both arenas -- and its K rows must be the first text's and then the second's, as in one arena."""
    from cropsr_amd import annotate
    contigs = cases.genome()
    names = ["c0", "c1", "c0", "c3"]
    gff = tmp_path / "two.gff3"
    gff.write_text(GFF_TWO_TEXTS)
    pattern, K = "N" * 20 + "NGG", 30
    score = "hsu2013" if scored else None
    sp = ref.spec(23, 17, ref.region_mask(23, 3, True), K, max_t_run=4)
    want, _, (n_in, n_pass, gene, _) = reference_selection_text(engine, contigs, names, gff, pattern, 3, 3, score, sp)
    # the claim, on the reference: the gene `rep` (index 0) has rows in two layout rows, each with 15 to 29 passing sites of one e, more than K together
    rep_rows = np.nonzero(np.asarray(gene) == 0)[0]
    assert rep_rows.size == 2 and (n_pass[rep_rows] >= 15).all() and (n_pass[rep_rows] < K).all() and n_pass[rep_rows].sum() > K
    rep_lines = [ln.split("\t") for ln in want.split("\n")[1:] if ln.startswith("gene:rep\t")]
    first = int(n_pass[rep_rows[0]])  # every row of the first text, then the second text's: equal e, the texts in order
    assert len(rep_lines) == K and [ln[5] for ln in rep_lines] == ["+"] * first + ["-"] * (K - first)
    assert len({tuple(ln[8:]) for ln in rep_lines}) == 1
    ann = annotate.Annotation(str(gff))
    texts = {}
    try:
        for three in (False, True):
            g = engine.genome(contigs, max_words=480) if three else engine.genome(contigs)
            try:
                assert len(g.arenas) == (3 if three else 1)
                req = ss.Request(ss.Params(K, 17, max_t_run=4), annotate.Request(ann, names, 0), slice_rows=64 if three else None)
                res = srch.search_self(g, pattern, 3, 3, score=score, select=req, sites=not three)
                assert res.n_guides > 0 and len(res.sites) == (0 if three else res.n_guides)
                texts[three] = ss.format_selection(names, res.selection)
            finally:
                g.close()
    finally:
        ann.close()
    assert texts[False].split("\n") == want.split("\n")
    assert texts[True].split("\n") == want.split("\n")
