"""Restriction sites: cloning-safe guides and cut-site assays (cropsr_amd/sites.py, csrc/crp_sites.hip).
The definition is restated twice in tests/site_reference.py; the inputs come from tests/site_cases.py, whose own checks say
what every case holds.  The selection's definition comes from tests/select_reference.py and, under every kernel that
includes csrc/crp_select_predicate.inc, from tests/test_select_predicate_matrix.py's Matrix and Device (imported, not edited):
the site term's matrix is written here.

The site term's cells -- kernel x term, every one held by test_gpu_site_cell (K = 5, whole genes and slices of 64; the plain
kernel at K = 1, 5 and 64), exact against the kernel's own reference over the rows the masks keep:

  kernel   forbid  need  both  with properties and variants
  plain    M       M     M     M
  pairs    M       M     M     M
  coding   M       M     M     M
  edit     M       M     M     M
  splice   M       M     M     M
  family   M       M     M     M
  step     M       M     M     M
  spaced   M       M     M     M

The masks of a cell are SITE_TERMS, over the built-in set with its last three enzymes replaced by the six letters around the
cut of a row the splice, the family and the edit kernel pick (SiteMatrix): none of their few rows on this genome has an assay
with a built-in enzyme.  No cell is vacuous (test_no_site_cell_is_vacuous, on the references alone): the term lowers n_pass in
some gene, changes some gene's picks and leaves passing rows -- but for family x `with properties and variants`, where the
property and variant limits leave four rows and each holds a four-cutter: the device must pass nothing there."""
import os

import numpy as np
import pytest

import select_reference as sref
import site_cases as cases
import site_reference as ref
import test_high_positions as thp
import test_select_predicate_matrix as tm
from cropsr_amd import _native as nat
from cropsr_amd import select as sel
from cropsr_amd import sites

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
SMALL = cases.small_cases()
SMALL_NAMES = [c["name"] for c, _ in SMALL]


@pytest.fixture(scope="module")
def small():
    return {c["name"]: (c, check, cases.arena(c)) for c, check in SMALL}


@pytest.fixture(scope="module")
def random_case():
    c = cases.random_case()
    return c, cases.arena(c)


# ---------------------------------------------------------------------------------------------- without a GPU: the definition
@pytest.mark.parametrize("name", SMALL_NAMES)
def test_the_cases_hold_what_they_are_for(small, name):
    case, check, A = small[name]
    check(case, A)


def test_the_random_case_holds_what_it_is_for(random_case):
    cases.check_random(*random_case)


@pytest.mark.parametrize("name", SMALL_NAMES)
def test_loop_equals_numpy(small, name):
    case, _, A = small[name]
    occ = ref.occurrences_loop(A["bytes"], cases.motifs(case))
    for e, m in enumerate(cases.motifs(case)):
        assert np.array_equal(np.array(occ[e], bool), ref.occurrences_numpy(A["bytes"], m)), m
    for flank in case["flanks"]:
        for s in ("plus", "minus"):
            pos = A["pos_" + s][::max(1, A["pos_" + s].size // 80)]
            assert np.array_equal(ref.column_loop(A["bytes"], A["bounds"], pos, s == "minus", case["l"], flank, cases.motifs(case), occ),
                                  ref.column_numpy(A["bytes"], A["bounds"], pos, s == "minus", case["l"], flank, cases.motifs(case))), (flank, s)


def test_loop_equals_numpy_on_the_random_case(random_case):
    case, A = random_case
    occ = ref.occurrences_loop(A["bytes"], cases.motifs(case))
    for e, m in enumerate(cases.motifs(case)):
        assert np.array_equal(np.array(occ[e], bool), ref.occurrences_numpy(A["bytes"], m)), m
    for flank in (8, 64, 300):
        for s in ("plus", "minus"):
            pos = A["pos_" + s][::40]
            assert np.array_equal(ref.column_loop(A["bytes"], A["bounds"], pos, s == "minus", 20, flank, cases.motifs(case), occ),
                                  ref.column_numpy(A["bytes"], A["bounds"], pos, s == "minus", 20, flank, cases.motifs(case))), (flank, s)


def test_reverse_complement_of_every_letter():
    want = dict(A="T", C="G", G="C", T="A", R="Y", Y="R", S="S", W="W", K="M", M="K", B="V", V="B", D="H", H="D", N="N")
    assert len(want) == 15 and set(want) == set(sites.SETS) == set(ref.IUPAC)
    for ch, rc in want.items():
        assert sites.reverse_complement("AAAA" + ch) == rc + "TTTT" and ref.rc_loop("AAAA" + ch) == rc + "TTTT", ch
        assert sites.SETS[ch] == sum(1 << "ACGT".index(b) for b in ref.IUPAC[ch])
        assert sites.complement_set(sites.SETS[ch]) == sites.SETS[rc]
    assert sites.reverse_complement("gantcu") == "AGANTC" and sites.normalize("gaUtc") == "GATTC"


def test_palindromes_count_once():
    text = b"TTTTGAATTCTTTTGGTCTCTTTTGAGACCTTTT"
    assert sites.is_palindrome("GAATTC") and not sites.is_palindrome("GGTCTC") and sites.is_palindrome("GANTC") and not sites.is_palindrome("CCWGGA")
    assert np.flatnonzero(ref.occurrences_numpy(text, "GAATTC")).tolist() == [4]
    assert np.flatnonzero(ref.occurrences_numpy(text, "GGTCTC")).tolist() == [14, 24]
    assert sum(ref.occurrences_loop(text, ["GAATTC"])[0]) == 1
    pal = [n for n, m in sites.BUILTIN if sites.is_palindrome(m)]
    assert len(pal) == 27 and not set(pal) & {"BsaI", "BbsI", "BsmBI", "SapI", "AarI"}


def test_the_builtin_table():
    assert len(sites.BUILTIN) == 32 and list(sites.BUILTIN) == cases.BUILTIN
    assert [n for n, _ in sites.BUILTIN[:5]] == ["BsaI", "BbsI", "BsmBI", "SapI", "AarI"] and sites.N_CLONING == 5
    assert dict(sites.BUILTIN)["NotI"] == "GCGGCCGC" and dict(sites.BUILTIN)["HinfI"] == "GANTC" and dict(sites.BUILTIN)["BstNI"] == "CCWGG"
    s = sites.EnzymeSet()
    assert s.builtin and len(s) == 32 and s.m_max == 8 and s.mask(["cloning"]) == 31 and s.mask(["any"]) == 0xFFFFFFFF
    assert s.mask(["ecori", "NotI"]) == 1 << 5 | 1 << 24 and s.check_flank(None) == 300 and s.check_flank(8) == 8
    for bad in (7, 100001):
        with pytest.raises(ValueError):
            s.check_flank(bad)
    with pytest.raises(ValueError):
        s.mask(["EcoR1"])


def test_the_parser():
    s = sites.parse("# my set\nBsaI\tggtctc\n\nMine\tGANTCU  # comment\n")
    assert s.names == ["BsaI", "Mine"] and s.motifs == ["GGTCTC", "GANTCT"] and not s.builtin and s.m_max == 6
    with pytest.raises(ValueError, match="cloning"):
        s.mask(["cloning"])
    assert s.mask(["mine"]) == 2
    for bad, what in (("BsaI GGTCTC\n", "line 1"), ("a\tGGT\n", "line 1"), ("a\tGGTCTC\nb\tGGTXTC\n", "line 2"), ("", "1..32"), ("a\tGGTCTC\nA\tGGTCTC\n", "twice"),
                      ("a\t" + "A" * 17 + "\n", "line 1"), ("a\tGGTCTC\textra\n", "line 1"), ("any\tGGTCTC\n", "name"),
                      ("".join("e%d\tGGTCTC\n" % k for k in range(33)), "1..32")):
        with pytest.raises(ValueError, match=what):
            sites.parse(bad)


def test_names_and_unpack():
    col = sites.pack([0, 1, 1 << 31 | 1 << 5], [0, 1 << 24, 3])
    assert col.dtype == np.uint64 and col.tolist() == [0, 1 | 1 << 56, (1 << 31 | 1 << 5) | 3 << 32]
    g, a = sites.unpack(col)
    assert g.dtype == a.dtype == np.uint32 and g.tolist() == [0, 1, 1 << 31 | 1 << 5] and a.tolist() == [0, 1 << 24, 3]
    assert sites.names(0) == [] and sites.names(1 << 31 | 1 << 5) == ["EcoRI", "BstNI"] and sites.names(3, ["x", "y", "z"]) == ["x", "y"]
    assert sites.fields(col[2]) == ("EcoRI;BstNI", "BsaI;BbsI") and sites.fields(0) == ("", "") and sites.HEADER == ["guide_sites", "assay_enzymes"]


def test_the_predicate_term_numpy_and_loop():
    rng = np.random.default_rng(2710)
    col = sites.pack(rng.integers(0, 1 << 32, 500, dtype=np.uint64) & rng.integers(0, 1 << 32, 500, dtype=np.uint64),
                     rng.integers(0, 1 << 32, 500, dtype=np.uint64) & rng.integers(0, 1 << 32, 500, dtype=np.uint64) & rng.integers(0, 1 << 32, 500, dtype=np.uint64))
    col[:4] = [0, 1 << 31, 1 << 63, 0xFFFFFFFFFFFFFFFF]
    for forbid, need in ((0, 0), (31, 0), (0, 0xFFFFFFFF), (1 << 31, 1 << 31), (0xFFFFFFFF, 1), (5, 0xF0)):
        a = ref.passes_numpy(col, forbid, need)
        assert np.array_equal(a, ref.passes_loop(col, forbid, need)) and np.array_equal(a, sites.passes(col, forbid, need)), (forbid, need)
    assert ref.passes_numpy(col[:4], 1 << 31, 0).tolist() == [True, False, True, False]
    assert ref.passes_numpy(col[:4], 0, 1 << 31).tolist() == [False, False, True, True]
    assert ref.passes_numpy(col, 0, 0).all()


def test_request_refusals():
    s = sites.EnzymeSet()
    for kw in (dict(assay_flank=300), dict(forbid_sites=["cloning"]), dict(need_assay=["any"])):
        with pytest.raises(ValueError, match="enzymes="):
            sel.Request(sel.Params(5), None, **kw)
    for kw in (dict(assay_flank=7), dict(assay_flank=100001), dict(forbid_sites=["nope"]), dict(need_assay=1 << 32), dict(forbid_sites=-1)):
        with pytest.raises(ValueError):
            sel.Request(sel.Params(5), None, enzymes=s, **kw)
    r = sel.Request(sel.Params(5), None, enzymes=s, forbid_sites=["cloning"], need_assay=["any"])
    assert r.site_limits == (31, 0xFFFFFFFF) and r.assay_flank == 300
    assert sel.Request(sel.Params(5), None, enzymes=s).site_limits is None
    assert not r.site_fields and sel.Request(sel.Params(5), None, enzymes=s).site_fields and not sel.Request(sel.Params(5), None).site_fields
    assert sel.Request(sel.Params(5), None, enzymes=s, forbid_sites=1, site_fields=True).site_fields
    with pytest.raises(ValueError, match="1..32"):
        sites.EnzymeSet([])
    for bad in ("GGT", "G" * 17, "GGTXTC"):
        with pytest.raises(ValueError):
            sites.EnzymeSet([("a", bad)])


def test_the_abi_version_stays():
    assert nat.lib().crp_abi_version() == 6
    with open(os.path.join(ROOT, "include", "cropsr_hip.h")) as f:
        assert "#define CRP_ABI_VERSION 6\n" in f.read()


# ---------------------------------------------------------------------------------------------- on the GPU: the column
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def _status(fn):
    with pytest.raises(nat.CropsrHipError) as e:
        fn()
    return e.value.status, str(e.value)


def _check_columns(arena, case, A):
    """Scan, set the case's enzymes, and compare the device's column with the reference at every flank of the case."""
    assert [int(o) for o in arena.offsets] == A["offsets"]
    n_plus, n_minus = arena.scan_score_device(case["l"])
    cols = arena.fetch(n_plus, n_minus)
    assert np.array_equal(cols[0], A["pos_plus"]) and np.array_equal(cols[3], A["pos_minus"])
    arena.set_enzymes(sites.EnzymeSet(case["enzymes"]))
    for flank in case["flanks"]:
        gp, gm = arena.site_columns(n_plus, n_minus, flank)
        want = cases.reference(case, A, flank)
        for got, s in ((gp, "plus"), (gm, "minus")):
            bad = np.flatnonzero(got != want[s]["value"])
            assert bad.size == 0, (case["name"], flank, s, bad[:5], [hex(int(x)) for x in got[bad[:5]]], [hex(int(x)) for x in want[s]["value"][bad[:5]]])
        st = arena.site_stats()
        assert st["rows"] == n_plus + n_minus and st["enzymes"] == len(case["enzymes"]) and st["flank"] == flank
        assert st["planes_ms"] > 0 and st["rank_ms"] > 0 and (st["kernel_ms"] > 0 or n_plus + n_minus == 0)
        words = A["offsets"][-1] // 64 + (len(case["texts"][-1]) + 63) // 64
        assert 12 * len(case["enzymes"]) * words <= st["bytes"] <= 12 * len(case["enzymes"]) * (words + 2) + 4 * len(case["enzymes"]) * (words // 1024 + 3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL_NAMES)
def test_gpu_columns_equal_the_reference(engine, small, name):
    case, _, A = small[name]
    arena = engine.arena(case["texts"])
    try:
        _check_columns(arena, case, A)
    finally:
        arena.close()


@pytest.mark.gpu
def test_gpu_random_case_every_row(engine, random_case):
    case, A = random_case
    arena = engine.arena(case["texts"])
    try:
        _check_columns(arena, case, A)
    finally:
        arena.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_arenas", [1, 3], ids=["one-arena", "three-arenas"])
def test_gpu_genome_level_columns(engine, random_case, n_arenas):
    """Genome.site_columns passes every arena the bounds of its own texts."""
    case = dict(random_case[0], texts=[random_case[0]["texts"][k] for k in (1, 2, 0, 3)])  # (an order that three arenas of 800 words hold)
    g = engine.genome(case["texts"], max_words=None if n_arenas == 1 else 800)
    try:
        assert len(g.arenas) == n_arenas
        hits = g.scan_score(20)
        es = sites.EnzymeSet()
        got = g.site_columns(es, [(h.n_plus, h.n_minus) for h in hits.per_arena])
        assert g.site_stats["rows"] == hits.n_plus + hits.n_minus and g.site_stats["flank"] == 300 and g.site_stats["enzymes"] == 32
        some = 0
        for a, (arena, group) in enumerate(zip(g.arenas, g.groups)):
            sub = dict(case, texts=[case["texts"][k] for k in group])
            A = cases.arena(sub)
            assert [int(o) for o in arena.offsets] == A["offsets"]
            want = cases.reference(sub, A, 300)
            assert np.array_equal(got[a][0], want["plus"]["value"]) and np.array_equal(got[a][1], want["minus"]["value"]), a
            some += int(np.count_nonzero(got[a][0] >> np.uint64(32))) + int(np.count_nonzero(got[a][1] >> np.uint64(32)))
        assert some > 50
        # the planes are kept while the set is the same: a second call builds nothing
        built = g.site_stats["planes_ms"]
        again = g.site_columns(es, [(h.n_plus, h.n_minus) for h in hits.per_arena], flank=64)
        assert g.site_stats["planes_ms"] == built and not all(np.array_equal(x[0], y[0]) for x, y in zip(got, again))
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_states_and_refusals(engine, small):
    L = nat.lib()
    case, _, A = small["planted"]
    arena = engine.arena(case["texts"])
    try:
        es = sites.EnzymeSet(case["enzymes"])
        st, msg = _status(lambda: arena.site_columns(0, 0, 300))
        assert st == nat.CRP_ERR_STATE and "no hit tables" in msg
        assert _status(arena.site_stats)[0] == nat.CRP_ERR_STATE
        n_plus, n_minus = arena.scan_score_device(20)
        st, msg = _status(lambda: arena.site_columns(n_plus, n_minus, 300))
        assert st == nat.CRP_ERR_STATE and "crp_sites_set_enzymes" in msg  # no enzyme set
        for motifs, what in (([], "1..32"), (["GGTCTC"] * 33, "1..32"), (["GGT"], "4..16"), (["G" * 17], "4..16"), (["GGTXTC"], "IUPAC"), (["GGT-TC"], "IUPAC")):
            st, msg = _status(lambda: arena.set_enzymes(motifs))
            assert st == nat.CRP_ERR_INVALID and what in msg, (motifs, msg)
        n_pos = (A["offsets"][-1] // 64 + (len(case["texts"][-1]) + 63) // 64 + 2) * 64
        for bounds in (([100, 50], [120, 90]), ([64, 100], [128, 200]), ([64], [64]), ([64], [n_pos + 64])):
            st, msg = _status(lambda: arena.set_enzymes(es, (np.array(bounds[0]), np.array(bounds[1]))))
            assert st == nat.CRP_ERR_INVALID and "bounds" in msg, bounds
        assert L.crp_sites_set_enzymes(None, 0, None, None, None, None, 0) == nat.CRP_ERR_INVALID
        assert L.crp_site_columns(None, 300, None, None) == nat.CRP_ERR_INVALID
        arena.set_enzymes(es)
        assert arena.site_stats()["rows"] == 0 and arena.site_stats()["enzymes"] == len(es)
        for flank in (15, 0, -1, 100001):
            st, msg = _status(lambda: arena.site_columns(n_plus, n_minus, flank))
            assert st == nat.CRP_ERR_INVALID and "16" in msg and "100000" in msg, flank
        first = arena.site_columns(n_plus, n_minus, 64)
        h = sel.ArenaSelect(arena, np.array([64], np.uint32), np.array([64 + len(case["texts"][0]) - 1], np.uint32))
        try:
            h.set_site_limits((1, 0))
            h.run(sel.Params(5))
            assert h.stats()["bytes_per_row"] == 20
            # a re-scan drops the column and keeps the planes
            n_plus, n_minus = arena.scan_score_device(20)
            assert arena.site_stats()["rows"] == 0
            st, msg = _status(lambda: h.run(sel.Params(5)))
            assert st == nat.CRP_ERR_STATE and "crp_site_columns" in msg
            again = arena.site_columns(n_plus, n_minus, 64)
            assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
            h.run(sel.Params(5))
            # a new set drops the column
            arena.set_enzymes(sites.EnzymeSet([("six", "GAATTC")]))
            st, msg = _status(lambda: h.run(sel.Params(5)))
            assert st == nat.CRP_ERR_STATE and "crp_site_columns" in msg
            h.set_site_limits(None)  # cleared: the plain selection again
            h.run(sel.Params(5))
            assert h.stats()["bytes_per_row"] == 12
            h.set_site_limits((0, 0))
            h.run(sel.Params(5))
            assert h.stats()["bytes_per_row"] == 12
        finally:
            h.close()
        # guide lengths outside 1 .. 50
        n_plus, n_minus = arena.scan_score_device(0)
        st, msg = _status(lambda: arena.site_columns(n_plus, n_minus, 300))
        assert st == nat.CRP_ERR_INVALID and "guide length 0" in msg
    finally:
        arena.close()


# ---------------------------------------------------------------------------------------------- on the GPU: the plain selection
def _genes(A):
    """Gene ranges over the random case's arena: whole texts, halves and a few hundred letters."""
    lo, hi = [], []
    for t0, t1 in A["bounds"]:
        n = t1 - t0
        for a, b in ((0, n - 1), (0, n // 2), (n // 3, n // 3 + 400)):
            lo.append(t0 + a)
            hi.append(min(t0 + b, t1 - 1))
    return np.array(lo, np.uint32), np.array(hi, np.uint32)


PLAIN_LIMITS = [(31, 0), (0x7F << 25, 0), (0, 0xFFFFFFFF), (0, 1 << 27 | 1 << 20), (0x7F << 25, 0xFFFFFFFF)]


@pytest.fixture(scope="module")
def scanned(engine, random_case):
    case, A = random_case
    arena = engine.arena(case["texts"])
    try:
        n_plus, n_minus = arena.scan_score_device(20)
        cols = arena.fetch(n_plus, n_minus)
        tables = dict(pos_plus=cols[0], score_plus=cols[2], pos_minus=cols[3], score_minus=cols[5])
        assert np.array_equal(cols[0], A["pos_plus"]) and np.array_equal(cols[3], A["pos_minus"])
        arena.set_enzymes(sites.EnzymeSet())
        got = arena.site_columns(n_plus, n_minus, 64)
        want = cases.reference(case, A, 64)
        assert np.array_equal(got[0], want["plus"]["value"]) and np.array_equal(got[1], want["minus"]["value"])
    except BaseException:
        arena.close()
        raise
    yield dict(arena=arena, tables=tables, col=want, genes=_genes(A))
    arena.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("limits", PLAIN_LIMITS, ids=["forbid=%x,need=%x" % l for l in PLAIN_LIMITS])
def test_gpu_plain_selection_honours_the_limits(scanned, limits, k):
    lo, hi = scanned["genes"]
    h = sel.ArenaSelect(scanned["arena"], lo, hi)
    try:
        h.set_site_limits(limits)
        h.run(sel.Params(k, 0.1))
        got = h.fetch()
        assert h.stats()["bytes_per_row"] == 20
    finally:
        h.close()
    also = {s: ref.passes_numpy(scanned["col"][s]["value"], *limits) for s in ("plus", "minus")}
    cds = dict(feat_plus=also["plus"].astype(np.uint32), feat_minus=also["minus"].astype(np.uint32), flags=np.array([0, 1], np.uint8))
    want = sref.select_numpy(scanned["tables"], lo, hi, k, 0.1, None, cds)
    plain = sref.select_numpy(scanned["tables"], lo, hi, k, 0.1)
    for g, w, name in zip(got, want, ("n_in", "n_pass", "sel")):
        assert np.array_equal(np.asarray(g, np.uint32), np.asarray(w, np.uint32)), name
    assert int(want[1].sum()) < int(plain[1].sum()) and int(want[1].sum()) > 0


# ---------------------------------------------------------------------------------------------- the site term under every kernel
SITE_FLANK = 64
FOUR_CUTTERS = 0x7F << 25  # MspI .. RsaI and the three of SiteMatrix: a third of the rows of the case genome hold one in their guide
SITE_TERMS = dict(forbid=dict(sites=(FOUR_CUTTERS, 0)), need=dict(sites=(0, 0xFFFFFFFF)), both=dict(sites=(31, 0xFFFFFFFF)),
                  others=dict(sites=(FOUR_CUTTERS, 0), props=tm.THRESHOLDS["properties"]["props"], variants=tm.THRESHOLDS["variants"]["variants"]))
PASSES_NOTHING = {("family", "others")}


def site_limits_of(kernel, term):
    out = dict(joined=True) if kernel in tm.READS_THE_JOIN else {}
    if term is not None:
        out.update(SITE_TERMS[term])
    return out


class SiteMatrix(tm.Matrix):
    """test_select_predicate_matrix's Matrix with one more column -- the site masks of the built-in set at SITE_FLANK, from
    site_reference -- and one more key of the limits: sites = (forbid, need)."""

    def __init__(self, case, planted=()):
        super().__init__(case, planted)
        p = self.p
        size = p.offsets[-1] + ((case.lengths[-1] + 63) // 64 + 1) * 64
        buf = bytearray(size)
        for t, o in zip(case.contigs, p.offsets):
            buf[o:o + len(t)] = t
        self.bounds = [(o, o + n) for o, n in zip(p.offsets, case.lengths)]
        # the built-in set, its last three enzymes replaced by the six letters around the cut of the first pick of the splice,
        # the family and the edit kernel: on this genome none of their few rows has an assay with a built-in enzyme
        arena = bytes(buf)
        self.enzymes = list(cases.BUILTIN[:29])
        for kernel in ("splice", "family", "edit"):
            picks = np.asarray(self.expected(kernel, site_limits_of(kernel, None), tm.K)[2]).ravel()
            for row in picks[picks != NONE].tolist():
                pos = int(p.tables["pos_minus" if row >> 31 else "pos_plus"][row & 0x7FFFFFFF])
                c = pos + 6 if row >> 31 else pos - 3
                motif = arena[c - 3:c + 3].decode().upper()
                if set(motif) <= set("ACGT") and motif not in [m for _, m in self.enzymes]:
                    self.enzymes.append(("cut_" + kernel, motif))
                    break
        assert len(self.enzymes) == 32
        motifs = [m for _, m in self.enzymes]
        self.site_cols = (ref.column_numpy(bytes(buf), self.bounds, p.tables["pos_plus"], False, tm.L, SITE_FLANK, motifs),
                          ref.column_numpy(bytes(buf), self.bounds, p.tables["pos_minus"], True, tm.L, SITE_FLANK, motifs))
        self.sites = np.concatenate(self.site_cols)

    def mask(self, limits):
        rest = {k: v for k, v in limits.items() if k != "sites"}
        m = super().mask(rest)
        return m & ref.passes_numpy(self.sites, *limits["sites"]) if "sites" in limits else m

    def want(self, kernel, term, k=tm.K):
        return self.expected(kernel, site_limits_of(kernel, term), k)


@pytest.fixture(scope="module")
def site_matrix(oracle, tmp_path_factory):
    return SiteMatrix(thp.Case(oracle, tmp_path_factory.mktemp("site_matrix")), tm.PLANTED)


@pytest.mark.parametrize("kernel", tm.KERNELS)
def test_no_site_cell_is_vacuous(site_matrix, kernel):
    """On the references alone: every term lowers n_pass in some gene and changes some gene's picks, and leaves passing rows
    in every cell but PASSES_NOTHING."""
    m = site_matrix
    base = m.want(kernel, None)
    for term in SITE_TERMS:
        got = m.want(kernel, term)
        a, b = tm.n_pass_of(kernel, got), tm.n_pass_of(kernel, base)
        assert (a <= b).all() and (a < b).any(), (kernel, term, "lowers n_pass nowhere")
        assert tm.picks_of(kernel, got) != tm.picks_of(kernel, base), (kernel, term, "changes no pick")
        assert (a > 0).any() or (kernel, term) in PASSES_NOTHING, (kernel, term, "passes nothing")
    if kernel == "plain":
        scored = m.cols["score"] != -1.0
        for forbid, need in ((FOUR_CUTTERS, 0), (0, 0xFFFFFFFF), (31, 0)):
            assert 5 < (ref.passes_numpy(m.sites, forbid, need) & scored).sum() < scored.sum() - 5, (forbid, need)
        assert (np.asarray(m.want(kernel, "forbid", tm.K_ALL)[2]) != NONE).sum(axis=1).max() > tm.K
        assert [n for n, _ in m.enzymes[29:]] == ["cut_splice", "cut_family", "cut_edit"]


class SiteDevice(tm.Device):
    """test_select_predicate_matrix's Device with the site column resident as well, checked against the reference's."""

    def __init__(self, engine, m):
        super().__init__(engine, m)
        try:
            self.arena.set_enzymes(sites.EnzymeSet(m.enzymes))
            n = m.n_plus
            got = self.arena.site_columns(n, len(m.sites) - n, SITE_FLANK)
            assert np.array_equal(got[0], m.site_cols[0]) and np.array_equal(got[1], m.site_cols[1])
        except BaseException:
            self.close()
            raise


@pytest.fixture(scope="module")
def site_dev(engine, site_matrix):
    d = SiteDevice(engine, site_matrix)
    yield d
    d.close()


@pytest.mark.gpu
@thp.SLICES
@pytest.mark.parametrize("term", list(SITE_TERMS))
@pytest.mark.parametrize("kernel", tm.KERNELS)
def test_gpu_site_cell(site_dev, site_matrix, kernel, term, slice_rows):
    """One cell: the kernel with its own limit and the term's masks on an ArenaSelect of the resident case genome, whole genes
    and slices of 64, every number against the kernel's reference over the rows the masks keep (test_select_predicate_matrix's
    test_gpu_cell, with the site limits set as well)."""
    from cropsr_amd import baseedit, coding
    dev, matrix, p = site_dev, site_matrix, site_matrix.p
    limits = site_limits_of(kernel, term)
    joined = dev.handles[0] if limits.get("joined") else None
    h = sel.ArenaSelect(dev.arena, p.lo, p.hi)
    try:
        if slice_rows:
            h.set_limits(slice_rows)
            h.set_pair_limits(slice_rows)
        tm._set_limits(h, dev, limits)
        h.set_site_limits(limits["sites"])
        if kernel in ("coding", "edit", "splice"):
            h.set_coding(dev.request.coding_layout(sel.arena_layout(dev.genome, 0)))
        if kernel == "coding":
            h.set_coding_limits(coding.Limits(*tm.CODING_LIMITS))
        elif kernel == "edit":
            h.set_edit_limits(baseedit.Window(*thp.WINDOW), baseedit.Limits(*tm.EDIT_LIMITS))
        elif kernel == "splice":
            h.set_splice_limits(baseedit.Window(*thp.WINDOW), "cbe", baseedit.SpliceLimits(*tm.SPLICE_LIMITS))
        elif kernel in ("family", "step"):
            g = np.asarray(p.gene, np.int64)
            h.set_family(dev.table.gene_family[g], np.array([dev.table.family_size(int(x)) for x in g], np.uint32))
            if kernel == "family":
                h.set_family_limits(sel.FamilyLimits(**tm.FAMILY_LIMITS))
            else:
                h.set_family_members(dev.table.gene_member[g])
        for k in ((1, tm.K, tm.K_ALL) if kernel == "plain" else (tm.K,)):
            what = "%s x %s, K = %d" % (kernel, term, k)
            want = matrix.want(kernel, term, k)
            if kernel == "pairs":
                h.run_pairs(tm._params(1, limits), sel.PairParams(k, *tm.PAIR_WINDOW), joined)
                tm._same(kernel, h.fetch_pairs(), want, what)
            elif kernel == "spaced":
                h.run_spaced(tm._params(k, limits), tm.SPACING, joined)
                tm._same(kernel, h.fetch_spaced(), want, what)
            elif kernel == "step":
                n_pass, steps = want
                for covered, best_want in steps:
                    best = h.family_step(tm._params(1, limits), joined, np.array(covered, np.uint64))
                    for f, w in enumerate(best_want):
                        if w is None:
                            assert best["gain"][f] == 0, (what, covered, f)
                            continue
                        got = (int(best["gain"][f]), int(best["key"][f]), int(best["cover"][f]), int(p.gene[int(best["gene"][f])]),
                               int(best["row"][f]) >> 31, int(best["row"][f]))
                        assert got == w and int(best["tie"][f]) & 1 == w[4], (what, covered, f)
                h.run(tm._params(1, limits), joined)
                assert np.array_equal(h.fetch()[1], np.asarray(n_pass, np.uint32)[np.asarray(p.gene, np.int64)]), what
            else:
                h.run(tm._params(k, limits), joined)
                tm._same(kernel, h.fetch(), want, what)
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------- on the GPU: end to end
@pytest.mark.gpu
@pytest.mark.parametrize("with_join", [False, True], ids=["plain", "inside-the-specificity-join"])
def test_gpu_genome_level_selection(engine, site_matrix, with_join):
    """scan_score(select=Request(enzymes=...)) in both places the kernel runs: right before the plain selection, and inside
    the specificity join's after_join hook.  The Selection carries the two masks of its rows."""
    from cropsr_amd import annotate
    c, m = site_matrix.case, site_matrix
    g = engine.genome(c.contigs)
    try:
        areq = annotate.Request(c.annotation, c.names, 0)
        req = sel.Request(sel.Params(tm.K), areq, enzymes=sites.EnzymeSet(m.enzymes), assay_flank=SITE_FLANK,
                          forbid_sites=[n for n, _ in m.enzymes[25:]], site_fields=True)
        assert req.site_limits == (FOUR_CUTTERS, 0)
        hits = g.scan_score(tm.L, specificity={} if with_join else None, select=req)
        assert np.array_equal(hits.sites[0][0], m.site_cols[0]) and np.array_equal(hits.sites[0][1], m.site_cols[1])
        S = hits.selection
        # (with the join a row without joined counts passes nowhere)
        n_in, n_pass, picked = m.expected("plain", dict(sites=(FOUR_CUTTERS, 0), **(dict(joined=True) if with_join else {})), tm.K)
        # (the Selection is per gene of the GFF; the layout rows of one arena are its genes in order here)
        assert np.array_equal(np.asarray(S.n_pass, np.uint32)[np.asarray(m.p.gene, np.int64)], n_pass)
        assert S.guide_sites is not None and len(S.guide_sites) == len(S.rows["position"]) == int((picked != NONE).sum()) > 0
        assert not (S.guide_sites & np.uint32(FOUR_CUTTERS)).any()
        rows = picked[picked != NONE]
        want = np.where(rows >> 31, m.site_cols[1][np.minimum(rows & 0x7FFFFFFF, len(m.site_cols[1]) - 1)],
                        m.site_cols[0][np.minimum(rows & 0x7FFFFFFF, len(m.site_cols[0]) - 1)])
        assert sorted(sites.pack(S.guide_sites, S.assay_enzymes).tolist()) == sorted(want.tolist())
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------- the command line
import csv
import hashlib
import io
import json

import select_cases
import test_repair_outcome as tro
from cropsr_amd import annotate, cli, rows


@pytest.fixture(scope="module")
def cli_case(oracle, tmp_path_factory):
    """tests/select_cases.py's genome and genes as files, and per host arena the reference's site columns of the built-in set."""
    c = select_cases.build(oracle)
    d = tmp_path_factory.mktemp("sites")
    c["gff_path"] = str(d / "genes.gff")
    with open(c["gff_path"], "w") as f:
        f.write(c["gff"])
    c["fasta_path"] = str(d / "genome.fa")
    with open(c["fasta_path"], "w") as f:  # one line per contig: read unformatted (dec = 0)
        f.write("".join(">%s\n%s\n" % (n, t.decode()) for n, t in zip(c["names"], c["contigs"]))[:-1])
    c["genes"] = sref.gff_genes(c["gff"])
    c["enzyme_file"] = str(d / "mine.tsv")
    with open(c["enzyme_file"], "w") as f:
        f.write("# two of the built-in set, one with IUPAC letters, and one that every guide holds\nAluI\tagct\nEcoRI\tGAATTC\nBstNI\tCCWGG\n\nevery\tNNNN\n")
    return c


def _site_arena(texts, hits, motifs, flank, l=20):
    """(tables, {plus, minus: packed column}, entries, offsets) of one host arena that holds the texts."""
    empty = [dict(repair_plus=np.zeros(len(h["pos_plus"]), np.uint64), repair_minus=np.zeros(len(h["pos_minus"]), np.uint64)) for h in hits]
    tables, _, entries, offsets = tro._host_arena(texts, list(range(len(texts))), hits, empty)
    buf = bytearray(offsets[-1] + ((len(texts[-1]) + 63) // 64 + 1) * 64)
    for t, o in zip(texts, offsets):
        buf[o:o + len(t)] = t
    bounds = [(o, o + len(t)) for t, o in zip(texts, offsets)]
    col = {s: ref.column_numpy(bytes(buf), bounds, tables["pos_" + s], s == "minus", l, flank, motifs) for s in ("plus", "minus")}
    return tables, col, entries, offsets


def _select_with(tables, col, lo, hi, K, forbid, need):
    also = {s: ref.passes_numpy(col[s], forbid, need) for s in ("plus", "minus")}
    cds = dict(feat_plus=also["plus"].astype(np.uint32), feat_minus=also["minus"].astype(np.uint32), flags=np.array([0, 1], np.uint8))
    return sref.select_numpy(tables, lo, hi, K, 0.0, None, cds)


class SitesOracleBackend(tro.SelectOracleBackend):
    """OracleBackend plus the `select` keyword, serving the site column and the two limits from the reference."""

    def scan(self, strings, l, offtarget=False, annotation=None, specificity=None, select=None, properties=False):
        out = tro.OracleBackend.scan(self, strings, l, offtarget=offtarget, annotation=annotation)
        assert specificity is None and not properties
        self.last_sites = None
        if select is None:
            return out
        texts = [bytes(s) for s in strings]
        req = select.annotation
        self.saw = (select.enzymes, select.assay_flank, select.site_limits, select.site_fields)
        if select.enzymes is None:
            tables, _, _, offsets = _site_arena(texts, out, [], 300)
            forbid = need = 0
            col = None
        else:
            tables, col, _, offsets = _site_arena(texts, out, select.enzymes.motifs, select.assay_flank)
            forbid, need = select.site_limits or (0, 0)
            self.last_sites = dict(planes_ms=0.0, rank_ms=0.0, kernel_ms=0.0, rows=int(col["plus"].size + col["minus"].size),
                                   enzymes=len(select.enzymes), flank=select.assay_flank, bytes=0)
        lo, hi, gene = req.gene_layout([(k, o, len(t)) for k, (t, o) in enumerate(zip(texts, offsets))])
        if col is None:
            n_in, n_pass, picked = sref.select_numpy(tables, lo, hi, select.params.k, select.params.min_score)
        else:
            n_in, n_pass, picked = _select_with(tables, col, lo, hi, select.params.k, forbid, need)
        part = dict(offsets=np.array(offsets, np.uint64), lengths=np.array([len(t) for t in texts], np.uint64), group=list(range(len(texts))),
                    gene=gene, n_in=n_in, n_pass=n_pass, sel=picked, **tables)
        if col is not None and select.site_fields:
            part.update(sites_plus=col["plus"], sites_minus=col["minus"])
        out = sel.HitList(out)
        out.selection = sel.assemble(req.annotation.genes()[0], select.params.k, [part])
        return out


def _wanted_rows(case, K, forbid, need, motifs, flank):
    """([(gene label, rank, passing, contig, end_pos, strand, packed value)] the reference selects, n_pass per layout row)."""
    tables, col, entries, _ = _site_arena(case["contigs"], case["hits"], motifs, flank)
    named = [(n, a, b, o) for n, (_, a, b, o) in zip(case["names"], entries)]
    lo, hi, gene = sref.layout(case["genes"], named, 0)
    n_in, n_pass, picked = _select_with(tables, col, lo, hi, K, forbid, need)
    n_before = np.cumsum([0] + [len(h["pos_plus"]) for h in case["hits"]])
    m_before = np.cumsum([0] + [len(h["pos_minus"]) for h in case["hits"]])
    want = []
    for at, g in enumerate(gene):
        for rank, packed in enumerate(picked[at]):
            if packed == NONE:
                break
            minus, r = int(packed) >> 31, int(packed) & 0x7FFFFFFF
            c = int(np.searchsorted(m_before if minus else n_before, r, "right") - 1)
            h = case["hits"][c]
            end = int(h["pos_minus"][r - m_before[c]]) + 3 if minus else int(h["pos_plus"][r - n_before[c]])
            want.append((int(g), rank, (case["genes"][int(g)][3], str(rank + 1), str(int(n_pass[at])), case["names"][c], str(end),
                                        "-" if minus else "+", int(col["minus" if minus else "plus"][r]))))
    return [w[2] for w in sorted(want, key=lambda w: w[:2])], n_pass, (tables, col, lo, hi)


def _check_file(case, got, K, forbid, need, names, motifs, flank, with_fields):
    want, n_pass, _ = _wanted_rows(case, K, forbid, need, motifs, flank)
    assert got[0] == ["gene", "rank", "passing"] + rows.HEADER[1:] + (sites.HEADER if with_fields else [])
    assert len(got) - 1 == len(want)
    for g, w in zip(got[1:], want):
        strand_at = 9 if len(g) - (2 if with_fields else 0) == len(rows.HEADER) + 2 else 8  # (an 11-field row has no cutsite field)
        assert (g[0], g[1], g[2], g[6], g[8], g[strand_at + 1]) == w[:6], (g, w)
        v = w[6]
        assert not (v & 0xFFFFFFFF) & forbid and (not need or (v >> 32) & need)
        if with_fields:
            assert (g[-2], g[-1]) == (";".join(n for e, n in enumerate(names) if v >> e & 1), ";".join(n for e, n in enumerate(names) if v >> (32 + e) & 1)), (g, w)
    return n_pass


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


BUILTIN_NAMES = [n for n, _ in cases.BUILTIN]
BUILTIN_MOTIFS = [m for _, m in cases.BUILTIN]


def test_cli_over_the_oracle(cli_case, oracle, tmp_path, monkeypatch):
    case = cli_case
    backend = SitesOracleBackend(oracle)
    plain_main, plain_stdout = tro._run(case, tmp_path, monkeypatch, ["--select", "5"], tro.SelectOracleBackend(oracle), "plain.csv")
    _, unfiltered, (tables, col, lo, hi) = _wanted_rows(case, 5, 0, 0, BUILTIN_MOTIFS, 300)
    four = sum(1 << BUILTIN_NAMES.index(n) for n in ("MspI", "AluI"))
    runs = [(["--sites"], 0, 0, 300), (["--sites", "--select-no-site", "cloning"], 31, 0, 300),
            (["--sites", "--select-no-site", "mspi, AluI", "--select-assay", "any"], four, 0xFFFFFFFF, 300),
            (["--sites", "--select-assay", "TaqI,HinfI", "--assay-flank", "64"], 0, 1 << 28 | 1 << 30, 64)]
    for k, (flags, forbid, need, flank) in enumerate(runs):
        out, stdout = tro._run(case, tmp_path, monkeypatch, ["--select", "5", "--bench-json", str(tmp_path / "b.json")] + flags, backend, "run%d.csv" % k)
        assert stdout == plain_stdout and open(out, "rb").read() == open(plain_main, "rb").read()  # the main table does not change
        assert backend.saw[1:] == (flank, (forbid, need) if forbid or need else None, True) and backend.saw[0].builtin
        n_pass = _check_file(case, _read(out + ".selected.csv"), 5, forbid, need, BUILTIN_NAMES, BUILTIN_MOTIFS, flank, True)
        with open(tmp_path / "b.json") as f:
            stage = json.load(f)["sites"]
        assert stage["enzymes"] == 32 and stage["flank"] == flank and stage["rows"] == sum(h["pos_plus"].size + h["pos_minus"].size for h in case["hits"])
        if not (forbid or need):  # everything passes: the plain selection with two more fields
            assert np.array_equal(n_pass, unfiltered)
            assert [r[:-2] for r in _read(out + ".selected.csv")] == _read(plain_main + ".selected.csv")
            assert any(r[-2] for r in _read(out + ".selected.csv")[1:]) and any(r[-1] for r in _read(out + ".selected.csv")[1:])
        else:
            assert 0 < n_pass.sum() < unfiltered.sum()
    # limits alone: the kernel runs, the column stays where it is, no field is printed
    filt, _ = tro._run(case, tmp_path, monkeypatch, ["--select", "5", "--select-no-site", "cloning"], backend, "filt.csv")
    assert backend.saw[2:] == ((31, 0), False)
    _check_file(case, _read(filt + ".selected.csv"), 5, 31, 0, BUILTIN_NAMES, BUILTIN_MOTIFS, 300, False)
    assert _read(filt + ".selected.csv")[1:] == [r[:-2] for r in _read(str(tmp_path / "run1.csv") + ".selected.csv")[1:]]
    # exactly K rows: an enzyme and a gene with 2 .. 8 rows that have its assay
    inside = lambda g, s, back: (tables["pos_" + s].astype(np.int64) - back >= lo[g]) & (tables["pos_" + s].astype(np.int64) - back <= hi[g]) & (tables["score_" + s] != -1.0)
    found = None
    for g in range(len(lo)):
        for e in range(32):
            n = sum(int(((col[s][inside(g, s, back)] >> np.uint64(32 + e)) & np.uint64(1)).sum()) for s, back in (("plus", 3), ("minus", 0)))
            if 2 <= n <= 8 and found is None:
                found = (g, e, n)
    assert found is not None
    g, e, K = found
    out, _ = tro._run(case, tmp_path, monkeypatch, ["--select", str(K), "--sites", "--select-assay", BUILTIN_NAMES[e]], backend, "exact.csv")
    n_pass = _check_file(case, _read(out + ".selected.csv"), K, 0, 1 << e, BUILTIN_NAMES, BUILTIN_MOTIFS, 300, True)
    assert n_pass[g] == K
    # a set of one's own: its names in the fields, `every` in every guide, and forbidding it passes nothing
    own_names, own_motifs = ["AluI", "EcoRI", "BstNI", "every"], ["AGCT", "GAATTC", "CCWGG", "NNNN"]
    out, _ = tro._run(case, tmp_path, monkeypatch, ["--select", "5", "--sites", "--enzymes", case["enzyme_file"], "--select-no-site", "EcoRI"], backend, "own.csv")
    n_pass = _check_file(case, _read(out + ".selected.csv"), 5, 2, 0, own_names, own_motifs, 300, True)
    assert n_pass.sum() > 0 and all("every" in r[-2].split(";") for r in _read(out + ".selected.csv")[1:]) and not backend.saw[0].builtin
    out, _ = tro._run(case, tmp_path, monkeypatch, ["--select", "5", "--sites", "--enzymes", case["enzyme_file"], "--select-no-site", "every"], backend, "none.csv")
    assert _check_file(case, _read(out + ".selected.csv"), 5, 8, 0, own_names, own_motifs, 300, True).sum() == 0
    assert len(_read(out + ".selected.csv")) == 1 and open(out, "rb").read() == open(plain_main, "rb").read()


def test_cli_without_the_flags_every_byte_is_what_it_was(cli_case, oracle, tmp_path, monkeypatch, manifest):
    """A run without the new flags against a run on the same inputs over a backend that does not know the feature; and the
    main CSV against the golden one (md5_libm)."""
    from conftest import OracleBackend, golden_fasta_path, run_cli
    for k, extra in enumerate((["--select", "5"], ["--select", "3", "--select-min-score", "0.4", "--select-only"])):
        old, old_stdout = tro._run(cli_case, tmp_path, monkeypatch, extra, tro.SelectOracleBackend(oracle), "old%d.csv" % k)
        backend = SitesOracleBackend(oracle)
        new, new_stdout = tro._run(cli_case, tmp_path, monkeypatch, extra + ["--bench-json", str(tmp_path / ("b%d.json" % k))], backend, "new%d.csv" % k)
        assert backend.saw == (None, None, None, False) and old_stdout == new_stdout
        assert open(old + ".selected.csv", "rb").read() == open(new + ".selected.csv", "rb").read()
        if "--select-only" not in extra:
            assert open(old, "rb").read() == open(new, "rb").read()
        with open(tmp_path / ("b%d.json" % k)) as f:
            assert "sites" not in json.load(f)
    data, _ = run_cli(tmp_path, monkeypatch, golden_fasta_path("sample", tmp_path), OracleBackend(oracle), manifest["seed"])
    assert hashlib.md5(data).hexdigest() == manifest["cases"]["sample"]["md5_libm"]


CLI_REFUSALS = [
    (["--sites"], "--sites", "belongs to --select"),
    (["--enzymes", "FILE"], "--enzymes", "belongs to --select"),
    (["--select-no-site", "cloning"], "--select-no-site", "belongs to --select"),
    (["--select-assay", "any"], "--select-assay", "belongs to --select"),
    (["--assay-flank", "300"], "--assay-flank", "belongs to --select"),
    (["--sites", "-l", "0"], "--sites", "1..50"),
    (["--sites", "-l", "51"], "--sites", "1..50"),
    (["--select", "5", "--select-no-site", "EcoR1"], "--select-no-site", "no enzyme"),
    (["--select", "5", "--select-no-site", "BsaI,,BbsI"], "--select-no-site", "comma-separated"),
    (["--select", "5", "--select-no-site", "any"], "--select-no-site", "comma-separated"),
    (["--select", "5", "--select-assay", "nobody"], "--select-assay", "no enzyme"),
    (["--select", "5", "--select-assay", "cloning"], "--select-assay", "comma-separated"),
    (["--select", "5", "--enzymes", "FILE", "--select-no-site", "cloning"], "--select-no-site", "`cloning`"),
    (["--select", "5", "--enzymes", "FILE", "--select-assay", "BsaI"], "--select-assay", "no enzyme"),
    (["--select", "5", "--enzymes", "no/such.tsv", "--sites"], "--enzymes", "no such file"),
    (["--select", "5", "--enzymes", "BAD", "--sites"], "--enzymes", "line 2"),
    (["--select", "5", "--enzymes", "EMPTY", "--sites"], "--enzymes", "1..32"),
    (["--select", "5", "--sites", "--assay-flank", "7"], "--assay-flank", "8"),
    (["--select", "5", "--sites", "--assay-flank", "100001"], "--assay-flank", "100000"),
    (["--select", "5", "--sites", "--assay-flank", "-300"], "--assay-flank", "number of letters"),
    (["--select", "5", "--sites", "--assay-flank", "3e2"], "--assay-flank", "number of letters"),
    (["--select", "5", "--sites", "--gpus", "2"], "--select", "one GPU"),  # (the flags belong to --select, which refuses first)
    (["--select", "5", "--select-assay", "any", "--devices", "0,1"], "--select", "one GPU"),
]


@pytest.mark.parametrize("extra,flag,text", CLI_REFUSALS, ids=[" ".join(r[0]) for r in CLI_REFUSALS])
def test_cli_refusals_come_before_any_side_effect(cli_case, oracle, tmp_path, monkeypatch, extra, flag, text):
    class NoScan(tro.OracleBackend):
        def scan(self, *a, **k):
            raise AssertionError("a refused command line reached the scan")
    files = tmp_path.parent / (tmp_path.name + "_files")
    files.mkdir()
    (files / "bad.tsv").write_text("a\tGGTCTC\nb GGTCTC\n")
    (files / "empty.tsv").write_text("# nothing\n")
    swap = dict(FILE=cli_case["enzyme_file"], BAD=str(files / "bad.tsv"), EMPTY=str(files / "empty.tsv"))
    monkeypatch.chdir(tmp_path)
    argv = ["-f", cli_case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9", "-g", cli_case["gff_path"]] + [swap.get(x, x) for x in extra]
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=NoScan(oracle), out=io.StringIO())
    assert flag in str(e.value.code) and text in str(e.value.code), e.value.code
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra", [["--sites"], ["--select-no-site", "cloning"], ["--select-assay", "any"]], ids=["fields", "forbid", "need"])
def test_cli_refuses_a_launchers_ranks(cli_case, oracle, tmp_path, monkeypatch, extra):
    class Group:
        world, rank, local_rank = 2, 0, 0
    monkeypatch.chdir(tmp_path)
    argv = ["-f", cli_case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9", "-g", cli_case["gff_path"], "--select", "5"] + extra
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=SitesOracleBackend(oracle), out=io.StringIO(), group=Group())
    assert "2 ranks" in str(e.value.code)
    assert os.listdir(tmp_path) == []


@pytest.mark.gpu
def test_gpu_command_line_end_to_end(cli_case, tmp_path, monkeypatch):
    """The real backend: the selection file against the reference, the `sites` stage, and the main CSV's md5 equal to the run
    without the flags."""
    case = cli_case
    plain, plain_stdout = tro._run(case, tmp_path, monkeypatch, ["--select", "5"], None, "plain.csv")
    flags = ["--select", "5", "--sites", "--select-no-site", "cloning,AluI", "--select-assay", "any", "--assay-flank", "64",
             "--bench-json", str(tmp_path / "bench.json")]
    out, stdout = tro._run(case, tmp_path, monkeypatch, flags, None)
    assert hashlib.md5(open(out, "rb").read()).hexdigest() == hashlib.md5(open(plain, "rb").read()).hexdigest() and stdout == plain_stdout
    n_pass = _check_file(case, _read(out + ".selected.csv"), 5, 31 | 1 << 27, 0xFFFFFFFF, BUILTIN_NAMES, BUILTIN_MOTIFS, 64, True)
    assert n_pass.sum() > 0
    with open(tmp_path / "bench.json") as f:
        stage = json.load(f)["sites"]
    assert stage["kernel_ms"] > 0 and stage["planes_ms"] > 0 and stage["rank_ms"] > 0 and stage["flank"] == 64 and stage["enzymes"] == 32
    assert stage["rows"] == sum(h["pos_plus"].size + h["pos_minus"].size for h in case["hits"]) and stage["bytes"] > 0
    # limits alone print no field and select the same rows
    filt, _ = tro._run(case, tmp_path, monkeypatch, ["--select", "5", "--select-no-site", "cloning,AluI", "--select-assay", "any", "--assay-flank", "64"], None, "filt.csv")
    assert _read(filt + ".selected.csv")[1:] == [r[:-2] for r in _read(out + ".selected.csv")[1:]]
