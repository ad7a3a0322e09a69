"""Gene families of the self search (cropsr_amd/families.py, crp_search_self_set_families .. crp_search_self_family_*;
DESIGN.md section 23): the parser and its refusals, the family table and the per-arena rows against restatements, the two
statements of the definition on the case genome, and the ABI without a GPU; the device's family rows, their join and the
error codes against the reference, exactly, on the GPU; the selection with family limits at the default slices and with its
genes cut into slices of 64, alone and behind the predicate's other terms.  Everything compared is an integer."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import family_cases as cases
import family_reference as fref
import search_pair_reference as pref
import search_score_reference as sref
import search_self_reference as selfref
import select_reference as selref
from cropsr_amd import _native as nat
from cropsr_amd import annotate, families as fam
from cropsr_amd import search as srch

PATTERN, GUIDE_PATTERN = cases.PATTERN, cases.GUIDE_PATTERN
NONE = fam.NONE


class Case:
    def __init__(self, tmp):
        self.__dict__.update(cases.build())
        self.idents = [g[0] for g in self.genes]
        self.pairs = fref.parse(self.families)
        self.fam_names, self.gene_family, self.gene_member, self.sizes, self.unknown_found = fref.table(self.pairs, self.idents)
        self.gff_path = os.path.join(tmp, "case.gff")
        with open(self.gff_path, "w") as f:
            f.write(self.gff)
        self._rows = {}

    def rows(self, M, value_key, C):
        """The numpy reference, computed once per (M, scheme, C)."""
        key = (M, value_key, C)
        if key not in self._rows:
            self._rows[key] = fref.family_rows(self.contigs, PATTERN, M, GUIDE_PATTERN, self.genes, self.gene_family, self.gene_member, C,
                                               VALUES[value_key][1])
        return self._rows[key]

    def table(self):
        ann = annotate.Annotation(self.gff_path)
        return ann, fam.FamilyTable(fam.parse_families(self.families), ann.genes()[0])


_PAIR, _PAM = pref.random_table(np.random.default_rng(523), PATTERN, 3, (1, 2))
# key: (the score argument of search_self, the value argument of the reference)
VALUES = {"plain": (None, None), "hsu2013": ("hsu2013", ("weights", sref.W_HSU)),
          "pair": (srch.PairTable(_PAIR, (1, 2), _PAM), ("pair", _PAIR, (1, 2), _PAM))}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(str(tmp_path_factory.mktemp("families")))


# ------------------------------------------------------------------ the case genome (CPU)
def test_case_genome_carries_every_case(case):
    ref = case.rows(4, "hsu2013", 0)
    k, pos, strand = ref["cand"]
    owner, guide = ref["cand_owner"], ref["cand_guide"]
    cut = np.where(strand == 0, pos + 17, pos)
    gene = {ident: i for i, ident in enumerate(case.idents)}
    n_guides = lambda ident: int((guide & (owner == gene[ident])).sum())
    row_of = {s: r for r, s in enumerate(ref["sites"])}
    counts, cover = ref["fam_counts"], ref["fam_cover"]
    assert 60_000 <= sum(len(c) for c in case.contigs) <= 80_000 and len(case.contigs) == 8
    # the family of three on three contigs: the exact sites of A1 find A3's on the other strand and most of A2's
    a1 = [r for r, s in enumerate(ref["sites"]) if ref["site_gene"][r] == gene["A1"]]
    assert len(a1) > 100 and sum(cover[r] == 0b111 for r in a1) > 80 and sum(cover[r] == 0b101 for r in a1) > 5
    a3 = {(p, s) for kk, p, s in ref["sites"] if kk == 2}
    assert any(counts[r][0] >= 2 for r in a1) and any(counts[r][1] >= 1 for r in a1) and len(a3) > 100
    mid = a1[len(a1) // 2]  # (a site whose window lies inside the copied stretch)
    k0, p0, s0 = ref["sites"][mid]
    mirror = (3333 + cases.A_LEN - (p0 - 1001) - 23, 1 - s0)  # the same letters on A3's other strand
    assert k0 == 0 and mirror in a3
    # nested members: the inner one is first in the file and owns its part, the outer one the rest
    inner = owner[(k == 0) & (cut >= 3100) & (cut <= 3391)]
    assert inner.size > 50 and (inner == gene["B_inner"]).all() and n_guides("B_outer") > 30 and n_guides("B_inner") > 10
    # a gene overlapped by a gene of another family: the shared part belongs to the first
    shared = owner[(k == 0) & (cut >= 7500) & (cut <= 7900)]
    assert shared.size > 50 and (shared == gene["C1"]).all() and n_guides("D1") > 20
    # the single-member family with a tandem repeat: its own repeats are inside, at 0 and at 1 .. 4 mismatches
    e1 = [r for r in range(len(ref["sites"])) if ref["site_gene"][r] == gene["E1"]]
    assert sum(counts[r][0] > 0 for r in e1) > 5 and counts[e1][:, 1:].sum() > 10 and counts[e1][:, 3:].sum() > 0
    assert all(cover[r] == 1 for r in e1)
    # a name the GFF lacks, ends that are no multiple of 64
    assert case.unknown_found == sorted(case.unknown) and all((g[2] % 64, (g[3] + 1) % 64) != (0, 0) for g in case.genes)
    # sites that cut exactly at lo - 1, lo, hi and hi + 1 of F1, on both strands
    for at, inside in ((4999, False), (5000, True), (5777, True), (5778, False)):
        for st in (0, 1):
            c = np.nonzero((k == 0) & (cut == at) & (strand == st))[0]
            assert c.size == 1 and guide[c[0]] and (owner[c[0]] == gene["F1"]) == inside, (at, st)
    # members at a contig's first and last positions; the '-' window that the contig's end cuts is no candidate
    last = len(case.contigs[4]) - 1
    assert n_guides("G_first") > 10 and n_guides("G_last") > 10 and case.genes[gene["G_last"]][3] == last
    assert case.contigs[4][2992:2995] == b"CCA" and not ((k == 4) & (pos == 2992)).any()
    assert ((k == 4) & (owner == gene["G_first"]) & (cut < 64)).any()
    # members with 0, 1, 255, 256 and 257 guide sites
    assert [n_guides(i) for i in ("H0", "H1", "R255", "R256", "R257")] == [0, 1, 255, 256, 257]
    # NAG candidates inside members: they count, and never query or cover
    nag = ~guide & (owner >= 0)
    assert int(nag.sum()) > 500 and len(ref["sites"]) == int(guide.sum())
    plain = fref.family_rows(case.contigs, GUIDE_PATTERN, 4, GUIDE_PATTERN, case.genes, case.gene_family, case.gene_member, 0, None)
    assert plain["sites"] == ref["sites"] and (counts >= plain["fam_counts"]).all() and (counts > plain["fam_counts"]).any()
    assert plain["fam_cover"] == ref["fam_cover"]
    # a non-base inside a member: its windows are candidates, not guide sites
    nb = (k == 1) & (pos <= 2500) & (pos + 20 > 2500) & (strand == 0)
    assert nb.any() and not guide[nb].any() and (owner[nb] == gene["A2"]).any()
    # a family of exactly 64 tiny members; a gene in no family
    assert case.sizes[case.fam_names.index("tiny")] == 64 and case.gene_family[gene["T64"]] == NONE == case.gene_family[gene["lonely"]]
    assert any(n_guides("T%d" % j) > 0 for j in range(64))
    # inside never exceeds the whole: the self search's rows bound the family rows
    sites, _, full, hs = selfref.search_self(case.contigs, PATTERN, 4, 3, GUIDE_PATTERN, sref.W_HSU)
    assert sites == ref["sites"] and (counts <= full).all() and all(a <= b for a, b in zip(ref["fam_sum"], hs))
    out = [r for r in a1 if full[r][0] > counts[r][0]]
    assert len(out) > 10  # the copy of a piece of A1 in no gene: perfect hits outside the family
    assert row_of[(k0, p0, s0)] == mid


def test_numpy_and_loop_agree(case):
    a = case.rows(4, "hsu2013", 0)
    b = fref.family_rows_loop(case.contigs, PATTERN, 4, GUIDE_PATTERN, case.genes, case.gene_family, case.gene_member, 0, sref.W_HSU)
    assert a["sites"] == b[0] and a["site_family"].tolist() == b[1] and a["site_gene"].tolist() == b[2]
    assert a["fam_counts"].tolist() == b[3] and a["fam_sum"] == b[4] and a["fam_cover"] == b[5]
    assert sum(a["fam_sum"]) > 0 and int(a["fam_counts"][:, 3:].sum()) > 0
    # the cover limit widens the cover set and changes nothing else
    wide = case.rows(4, "hsu2013", 4)
    assert (wide["fam_counts"] == a["fam_counts"]).all() and wide["fam_sum"] == a["fam_sum"]
    assert all(w & c == c for w, c in zip(wide["fam_cover"], a["fam_cover"])) and wide["fam_cover"] != a["fam_cover"]
    short = {k: v for k, v in zip(("sites", "fam", "gene", "counts", "sum", "cover"),
                                  fref.family_rows_loop(case.contigs[:3], PATTERN, 2, GUIDE_PATTERN, case.genes[:10], case.gene_family,
                                                        case.gene_member, 2, None))}
    want = fref.family_rows(case.contigs[:3], PATTERN, 2, GUIDE_PATTERN, case.genes[:10], case.gene_family, case.gene_member, 2, None)
    assert short["sum"] is None and want["fam_sum"] is None and short["counts"] == want["fam_counts"].tolist()
    assert short["cover"] == want["fam_cover"]


# ------------------------------------------------------------------ parser, table, rows (CPU)
def test_parser_and_its_refusals(case, tmp_path):
    E = fam.FamilyInputError
    pairs = fam.parse_families(case.families)
    assert dict(pairs) == case.pairs and len(pairs) == len(case.pairs)  # (A1 named twice with one family: once)
    assert fam.parse_families(b"# c\n\ng1\tf\r\n  \ng2\tf\n") == [("g1", "f"), ("g2", "f")]
    for bad in ("g1\n", "g1\tf\tx\n", "g1 f\n", "g1\t\n", "\tf\n", "g1\tf\ng1\th\n"):
        with pytest.raises(E):
            fam.parse_families(bad)
    with pytest.raises(E) as e:
        fam.read_families(str(tmp_path / "missing.tsv"))
    assert "missing.tsv" in str(e.value)
    p = tmp_path / "f.tsv"
    p.write_text(case.families)
    assert fam.read_families(str(p)) == pairs


def test_family_table_against_restatement(case):
    ann, table = case.table()
    try:
        labels = ann.genes()[0]
        assert labels == ["gene:" + i for i in case.idents]
        assert table.names == case.fam_names and table.gene_family.tolist() == case.gene_family
        assert table.gene_member.tolist() == case.gene_member and table.size.tolist() == case.sizes
        assert table.n_unknown == len(case.unknown) == 2
        g = case.idents.index
        assert table.family_size(g("lonely")) == 1 and table.family_name(g("lonely")) == "" and table.family_size(g("A2")) == 3
        assert table.family_name(g("T5")) == "tiny" and table.family_size(g("T5")) == 64 and table.family_size(g("T64")) == 1
        assert table.member_labels(g("A2"), 0b101) == ["gene:A1", "gene:A3"] and table.member_labels(g("lonely"), 1) == []
        with pytest.raises(fam.FamilyInputError) as e:  # 65 members
            fam.FamilyTable(fam.parse_families(case.too_many), labels)
        assert "64" in str(e.value)
        with pytest.raises(ValueError):
            fref.table(fref.parse(case.too_many), case.idents)
        # the rows of an arena: the layout of the genes that have a family, by gene index
        req = annotate.Request(ann, case.names, 0)
        offsets = np.concatenate([[0], np.cumsum([len(c) + 7 for c in case.contigs])])[:-1]
        for which in ([0, 1, 2, 3, 4, 5, 6, 7], [0, 2], [7]):
            layout = [(t, int(offsets[t]), len(case.contigs[t])) for t in which]
            rows = fam.arena_rows(table, *req.gene_layout(layout))
            want = sorted((gi, int(offsets[kc]) + lo, int(offsets[kc]) + hi) for gi, (_, kc, lo, hi) in enumerate(case.genes)
                          if kc in which and case.gene_family[gi] != NONE)
            assert list(zip(rows.gene.tolist(), rows.lo.tolist(), rows.hi.tolist())) == want
            assert rows.family.tolist() == [case.gene_family[gi] for gi, _, _ in want]
            assert rows.member.tolist() == [case.gene_member[gi] for gi, _, _ in want]
            entries = [(case.names[t], 0, ln, off) for t, off, ln in layout]
            lo, hi, idx = selref.layout([(case.names[kc], a + 1, b + 1, None) for _, kc, a, b in case.genes], entries, 0)
            got = req.gene_layout(layout)
            assert (got[0].tolist(), got[1].tolist(), got[2].tolist()) == (list(lo), list(hi), list(idx))
    finally:
        ann.close()


def test_outside_values():
    counts = np.array([[3, 1], [2, 0], [0, 0]], np.uint32)
    fc = np.array([[2, 1], [0, 0], [0, 0]], np.uint32)
    hs, fs = np.array([10, 7, 0], np.uint64), np.array([4, 0, 0], np.uint64)
    mm0, out, hit = fam.outside(counts, hs, fc, fs, np.array([0b1011, 1, 1 << 63], np.uint64))
    assert mm0.tolist() == [1, 2, 0] and out.tolist() == [6, 7, 0] and hit.tolist() == [3, 1, 1]
    assert fam.outside(counts, None, fc, None, np.zeros(3, np.uint64))[1] is None
    # the per-(gene, row) statement of the reference: the row's family must be the gene's
    fam_of, sizes = [0, 1, fref.NONE], [3, 2]
    assert fref.selection_values(0, fam_of, sizes, 0, 3, 10, 2, 4, 0b1011) == (1, 6, 3, 3)
    assert fref.selection_values(1, fam_of, sizes, 0, 3, 10, 2, 4, 0b1011) == (3, 10, 1, 2)  # a row of an overlapping gene's family
    assert fref.selection_values(2, fam_of, sizes, fref.NONE, 3, 10, 0, 0, 0) == (3, 10, 1, 1)
    assert fref.passes_family((1, 6, 3, 3), "all", 1, 6) and not fref.passes_family((1, 6, 2, 3), "all")
    assert not fref.passes_family((1, 6, 3, 3), 2, 0) and not fref.passes_family((1, 6, 3, 3), None, None, 5)


def test_refusals_before_the_gpu(case):
    E = srch.SearchInputError
    for kw in (dict(family_cover_mm=4), dict(family_cover_mm=-1), dict(family_cover_mm=1.0)):
        with pytest.raises(E):
            srch.search_self(None, PATTERN, 3, 3, guide_pattern=GUIDE_PATTERN, families=[], **kw)
        with pytest.raises(E):
            srch.specificity_columns(None, 20, families=[], **kw)
    with pytest.raises(E):  # the owner is defined by the cut of a 3' PAM of 3 letters
        srch.search_self(None, "TTTV" + "N" * 20, 3, 4, families=[])


def test_library_declares_family_abi():
    L = nat.lib()
    with open(os.path.join(ROOT, "include", "cropsr_hip.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    c_types = {"crp_search_self *": ctypes.c_void_p, "const crp_search_self *": ctypes.c_void_p, "int": ctypes.c_int,
               "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "uint64_t *": nat.u64p, "uint32_t *": nat.u32p,
               "const uint32_t *": nat.u32p, "double *": nat.f64p}
    for name in ("set_families", "family_set_limits", "family_assign", "family_compare", "family_fetch", "family_join_hits", "family_stats"):
        sym = "crp_search_self_" + name
        m = re.search(r"int %s\(([^)]*)\);" % sym, header)
        assert m, sym
        want = [c_types[re.match(r"\s*(.*?)(\w+)\s*$", arg).group(1).strip()] for arg in m.group(1).split(",")]
        assert nat.SIGNATURES[sym] == (ctypes.c_int, want), sym
        assert hasattr(L, sym)
    c_types.update({"crp_select *": ctypes.c_void_p, "const crp_select *": ctypes.c_void_p, "const crp_select_family_limits *": ctypes.c_void_p})
    for sym in ("crp_select_set_family", "crp_select_set_family_limits", "crp_select_family_eval", "crp_select_family_stats"):
        m = re.search(r"int %s\(([^)]*)\);" % sym, header)
        assert m, sym
        want = [c_types[re.match(r"\s*(.*?)(\w+)\s*$", arg).group(1).strip()] for arg in m.group(1).split(",")]
        assert nat.SIGNATURES[sym] == (ctypes.c_int, want), sym
        assert hasattr(L, sym)
    m = re.search(r"typedef struct crp_select_family_limits \{([^}]*)\}", header)
    fields = [(n.strip(), {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}[t]) for t, names in
              re.findall(r"(uint64_t|uint32_t) ([^;]*);", m.group(1)) for n in names.split(",")]
    assert nat.SelectFamilyLimits._fields_ == fields and ctypes.sizeof(nat.SelectFamilyLimits) == 16
    assert re.search(r"#define CRP_SELECT_ALL_MEMBERS 0x%Xu" % nat.SELECT_ALL_MEMBERS, header)
    assert L.crp_abi_version() == nat.ABI_VERSION


# ------------------------------------------------------------------ the library (GPU)
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


MAX_WORDS = 450  # three arenas: chrA + chrB | chrD + rep + edge | runs + tiny + spare


def _device_rows(engine, case, M, score, C, max_words=None, limits=None, table=None):
    ann, tab = case.table()
    g = engine.genome(case.contigs, max_words=max_words)
    try:
        rows = fam.genome_rows(table or tab, g, annotate.Request(ann, case.names, 0))
        res = g.search_self(PATTERN, M, 3, guide_pattern=GUIDE_PATTERN, score=score, families=rows, family_cover_mm=C, family_limits=limits)
        return res, len(g.arenas)
    finally:
        g.close()
        ann.close()


def _assert_rows_equal(res, ref, scored):
    sites = list(zip(res.sites["contig"].tolist(), res.sites["position"].tolist(), (res.sites["strand"] == b"-").astype(int).tolist()))
    assert sites == ref["sites"]
    assert res.site_family.dtype == np.uint32 and (res.site_family == ref["site_family"]).all()
    assert (res.site_gene == ref["site_gene"]).all()
    assert res.fam_counts.dtype == np.uint32 and (res.fam_counts.astype(np.int64) == ref["fam_counts"]).all()
    assert res.fam_cover.dtype == np.uint64 and [int(x) for x in res.fam_cover] == ref["fam_cover"]
    if scored:
        assert res.fam_sum.dtype == np.uint64 and [int(x) for x in res.fam_sum] == ref["fam_sum"]
        assert (res.fam_sum <= res.hit_sum).all()
    else:
        assert res.fam_sum is None
    assert (res.fam_counts <= res.counts).all()
    none = res.site_family == NONE
    assert none.any() and not res.fam_counts[none].any() and not res.fam_cover[none].any()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [0, 3, 4])
@pytest.mark.parametrize("value", ["plain", "hsu2013", "pair"])
def test_gpu_family_rows_match_reference(engine, case, M, value):
    score = VALUES[value][0]
    for C in sorted({0, M}):
        ref = case.rows(M, value, C)
        for max_words in (None, MAX_WORDS):
            res, n_arenas = _device_rows(engine, case, M, score, C, max_words)
            assert n_arenas == (1 if max_words is None else 3)
            _assert_rows_equal(res, ref, score is not None)
            assert res.stats["family_pairs"] > 0 and res.stats["family_compare_launches"] >= n_arenas
    if M == 4:
        assert int(ref["fam_counts"][:, 1:].sum()) > 100 and (value == "plain" or sum(ref["fam_sum"]) > 0)


@pytest.mark.gpu
def test_gpu_result_does_not_depend_on_the_cut(engine, case):
    ref = case.rows(4, "hsu2013", 4)
    whole, _ = _device_rows(engine, case, 4, "hsu2013", 4)
    for max_words in (None, MAX_WORDS):
        res, _ = _device_rows(engine, case, 4, "hsu2013", 4, max_words, limits=(1, 1))  # one item a launch, slices of 8 candidates
        _assert_rows_equal(res, ref, True)
        assert res.stats["family_compare_launches"] > 50 * whole.stats["family_compare_launches"]
        assert res.stats["family_pairs"] == whole.stats["family_pairs"]


@pytest.mark.gpu
def test_gpu_whole_contig_family_equals_self_search(engine, case, tmp_path):
    """One family whose members are one whole-contig gene per contig: every candidate is inside, so the family rows are the
    self search's own rows and nothing lies outside.  This holds the family compare against search_self_compare_kernel."""
    gff = tmp_path / "whole.gff"
    gff.write_text("".join("%s\ttest\tgene\t1\t%d\t.\t+\t.\tID=w%d\n" % (n, len(c), j) for j, (n, c) in enumerate(zip(case.names, case.contigs))))
    ann = annotate.Annotation(str(gff))
    table = fam.FamilyTable([("w%d" % j, "all") for j in range(len(case.names))], ann.genes()[0])
    try:
        for value, M, max_words in (("hsu2013", 4, MAX_WORDS), ("pair", 3, None), ("plain", 2, MAX_WORDS)):
            g = engine.genome(case.contigs, max_words=max_words)
            try:
                rows = fam.genome_rows(table, g, annotate.Request(ann, case.names, 0))
                res = g.search_self(PATTERN, M, 3, guide_pattern=GUIDE_PATTERN, score=VALUES[value][0], families=rows)
            finally:
                g.close()
            assert (res.site_family == 0).all() and len(res.sites) > 5000
            assert (res.fam_counts == res.counts).all() and int(res.counts.sum()) > 500
            if value != "plain":
                assert (res.fam_sum == res.hit_sum).all() and int(res.hit_sum.sum()) > 0
            mm0, hs, _ = fam.outside(res.counts, res.hit_sum, res.fam_counts, res.fam_sum, res.fam_cover)
            assert not mm0.any() and (hs is None or not hs.any())
            assert (res.site_gene == res.sites["contig"]).all()
    finally:
        ann.close()


@pytest.mark.gpu
def test_gpu_joined_family_columns(engine, case):
    ref = case.rows(3, "hsu2013", 0)
    row_of = {s: r for r, s in enumerate(ref["sites"])}
    ann, table = case.table()
    try:
        for max_words in (None, MAX_WORDS):
            g = engine.genome(case.contigs, max_words=max_words)
            try:
                rows = fam.genome_rows(table, g, annotate.Request(ann, case.names, 0))
                hits = g.scan_score(20, specificity=dict(families=rows))
                tables = [hits.contig(k) for k in range(len(case.contigs))]
                plain = g.scan_score(20, specificity={})
            finally:
                g.close()
            assert hits.columns.stats["family_pairs"] > 0 and "family_pairs" not in plain.columns.stats
            n_joined = n_unjoined = 0
            for k in range(len(case.contigs)):
                h, cols, old = tables[k], hits.columns[k], plain.columns[k]
                for strand, name in ((0, "plus"), (1, "minus")):
                    # the existing join's columns are what they are without families
                    assert (cols["self_counts_" + name] == old["self_counts_" + name]).all()
                    assert (cols["self_sum_" + name] == old["self_sum_" + name]).all()
                    pos = h["pos_" + name].astype(np.int64)
                    start = pos - 20 if strand == 0 else pos
                    r = np.array([row_of.get((k, int(p), strand), -1) for p in start.tolist()], dtype=np.int64)
                    joined = r >= 0
                    assert (joined == (cols["self_counts_" + name][:, 0] != nat.SELF_UNJOINED_COUNT)).all()
                    fcnt, fsum = cols["fam_counts_" + name], cols["fam_sum_" + name]
                    fcov, ffam = cols["fam_cover_" + name], cols["site_family_" + name]
                    assert fcnt.dtype == np.uint32 and fsum.dtype == fcov.dtype == np.uint64 and ffam.dtype == np.uint32
                    assert (fcnt[~joined] == nat.SELF_UNJOINED_COUNT).all() and (fsum[~joined] == nat.SELF_UNJOINED_SUM).all()
                    assert not fcov[~joined].any() and (ffam[~joined] == NONE).all()
                    rj = r[joined]
                    assert (fcnt[joined].astype(np.int64) == ref["fam_counts"][rj]).all()
                    assert [int(x) for x in fsum[joined]] == [ref["fam_sum"][i] for i in rj.tolist()]
                    assert [int(x) for x in fcov[joined]] == [ref["fam_cover"][i] for i in rj.tolist()]
                    assert (ffam[joined] == ref["site_family"][rj]).all()
                    n_joined += int(joined.sum())
                    n_unjoined += int((~joined).sum())
            # (a guide site that the scan's tables do not list has no row to join: a few at the contigs' ends)
            assert len(ref["sites"]) - 40 < n_joined <= len(ref["sites"]) and n_unjoined > 0
    finally:
        ann.close()


@pytest.mark.gpu
def test_gpu_calls_out_of_order_and_refusals(engine, case):
    L = nat.lib()
    ann, table = case.table()
    g = engine.genome(case.contigs)
    handles = []
    try:
        rows = fam.genome_rows(table, g, annotate.Request(ann, case.names, 0))[0]
        h = srch.ArenaSelfSearch(g.arenas[0], PATTERN, GUIDE_PATTERN, 3, 3)
        handles.append(h)
        ctx = g.arenas[0]._engine._ctx
        u32 = lambda a: np.ascontiguousarray(a, np.uint32).ctypes.data_as(nat.u32p)
        cols = [np.ascontiguousarray(c, np.uint32) for c in (rows.lo, rows.hi, rows.family, rows.member)]
        args = [c.ctypes.data_as(nat.u32p) for c in cols]
        out = np.zeros(h.sizes()[2], np.uint32)
        # nothing set: every later call is a state error, with a text
        assert L.crp_search_self_family_assign(h._h) == nat.CRP_ERR_STATE and b"families" in L.crp_last_error(ctx)
        assert L.crp_search_self_family_compare(h._h, h._h) == nat.CRP_ERR_STATE
        assert L.crp_search_self_family_fetch(h._h, u32(out), None, None, None, None, out.size) == nat.CRP_ERR_STATE
        assert L.crp_search_self_family_join_hits(h._h, 20, *([None] * 8)) == nat.CRP_ERR_STATE
        # refusals of set_families: the cover limit above M, a 65th member, the family id that means none
        assert L.crp_search_self_set_families(h._h, *args, len(rows), 4) == nat.CRP_ERR_INVALID and b"cover" in L.crp_last_error(ctx)
        assert L.crp_search_self_set_families(h._h, *args, len(rows), -1) == nat.CRP_ERR_INVALID
        bad = cols[3].copy()
        bad[-1] = 64
        assert L.crp_search_self_set_families(h._h, args[0], args[1], args[2], u32(bad), len(rows), 0) == nat.CRP_ERR_INVALID
        assert b"64" in L.crp_last_error(ctx)
        none = cols[2].copy()
        none[0] = NONE
        assert L.crp_search_self_set_families(h._h, args[0], args[1], u32(none), args[3], len(rows), 0) == nat.CRP_ERR_INVALID
        assert L.crp_search_self_set_families(h._h, None, args[1], args[2], args[3], len(rows), 0) == nat.CRP_ERR_INVALID
        assert L.crp_search_self_set_families(None, *args, len(rows), 0) == nat.CRP_ERR_INVALID
        # set, not assigned: compare, fetch and join still refuse
        h.set_families(rows, 3)
        assert L.crp_search_self_family_compare(h._h, h._h) == nat.CRP_ERR_STATE
        assert L.crp_search_self_family_fetch(h._h, u32(out), None, None, None, None, out.size) == nat.CRP_ERR_STATE
        before = h.stats()["device_bytes"]
        n = sum(h.sizes()[:2])
        assert h.family_stats()["family_bytes"] == n * (4 * 4 + 8 + 8 + 4 + 4) + len(rows) * 24
        h.family_assign()
        assert L.crp_search_self_family_fetch(h._h, u32(out), None, None, None, None, out.size - 1) == nat.CRP_ERR_CAPACITY
        assert L.crp_search_self_family_join_hits(h._h, 20, *([None] * 8)) == nat.CRP_ERR_INVALID  # no tables of a scan
        assert L.crp_search_self_family_stats(h._h, None, 7) == nat.CRP_ERR_INVALID
        # a handle of another geometry or M does not compare
        other = srch.ArenaSelfSearch(g.arenas[0], PATTERN, GUIDE_PATTERN, 3, 2)
        handles.append(other)
        assert L.crp_search_self_family_compare(h._h, other._h) == nat.CRP_ERR_INVALID
        cas12a = srch.ArenaSelfSearch(g.arenas[0], "TTTV" + "N" * 20, "TTTV" + "N" * 20, 4, 3)
        handles.append(cas12a)
        assert L.crp_search_self_set_families(cas12a._h, *args, len(rows), 0) == nat.CRP_ERR_INVALID and b"PAM" in L.crp_last_error(ctx)
        # the budget counts the family columns
        small = srch.ArenaSelfSearch(g.arenas[0], PATTERN, GUIDE_PATTERN, 3, 3, budget=h.needed)
        handles.append(small)
        assert L.crp_search_self_set_families(small._h, *args, len(rows), 0) == nat.CRP_ERR_CAPACITY and b"budget" in L.crp_last_error(ctx)
        # taking families off gives the bytes back; an arena without family genes is fine
        h.set_families(None)
        assert h.stats()["device_bytes"] == before - n * 40 - len(rows) * 24 and L.crp_search_self_family_assign(h._h) == nat.CRP_ERR_STATE
        empty = fam.ArenaRows(*[np.zeros(0, np.uint32)] * 5)
        h.set_families(empty)
        h.family_assign()
        h.family_compare(h)
        owner, family, counts, sums, cover = h.family_fetch()
        assert (owner == NONE).all() and (family == NONE).all() and not counts.any() and not sums.any() and not cover.any()
    finally:
        for x in handles:
            x.close()
        g.close()
        ann.close()


# ------------------------------------------------------------------ the selection (CPU: limits and refusals; GPU: against a loop)
def test_family_limits_and_request_refusals():
    from cropsr_amd import select as sel
    lim = sel.FamilyLimits("all", 0, 0.5)
    assert lim.astuple() == (sel.max_hit_sum_for(0.5), 0, nat.SELECT_ALL_MEMBERS) and sel.max_hit_sum_for(0.5) == 1 << 30
    assert sel.FamilyLimits().astuple() == (sel.NO_BOUND_SUM, sel.NO_BOUND_MM0, 0) and sel.FamilyLimits(3).min_members == 3
    # the predicate against a loop on synthetic columns
    rng = np.random.default_rng(8)
    mm0, hs = rng.integers(0, 3, 200).astype(np.uint32), rng.choice(np.array([0, 1 << 29, 1 << 31], np.uint64), 200)
    hit, size = rng.integers(1, 5, 200).astype(np.uint32), rng.integers(1, 5, 200).astype(np.uint32)
    for args in (("all", 0, 0.5), (2, None, None), (None, 1, None), (None, None, 0.75), (4, 0, 1.0)):
        lim = sel.FamilyLimits(*args)
        bound = None if args[2] is None else sel.max_hit_sum_for(args[2])
        want = [fref.passes_family((int(a), int(b), int(c), int(d)), args[0], args[1], bound) for a, b, c, d in zip(mm0, hs, hit, size)]
        assert lim.passes(mm0, hs, hit, size).tolist() == want and 0 < sum(want) < 200
    for bad in (dict(min_members=0), dict(min_members=65), dict(min_members="most"), dict(min_members=1.5), dict(max_perfect_outside=-1),
                dict(max_perfect_outside=0.5), dict(min_specificity_outside=1.5)):
        with pytest.raises(ValueError):
            sel.FamilyLimits(**bad)
    table, params = object(), sel.Params(5)
    assert sel.Request(params, None, families=table).family_limits is None
    with pytest.raises(ValueError):  # a family limit without a family table
        sel.Request(params, None, min_members=2)
    from cropsr_amd import baseedit, coding
    for other in (dict(coding_limits=coding.Limits(0, 50)), dict(edit_limits=baseedit.Limits()), dict(splice_limits=baseedit.SpliceLimits()),
                  dict(pairs=sel.PairParams(3))):
        with pytest.raises(ValueError):
            sel.Request(params, None, families=table, max_perfect_outside=0, **other)


def _reference_selection(case, tables, columns, fam_ref, row_of, K, max_perfect=None, max_hit_sum=None, limits=(None, None, None),
                         also=None, min_score=0.0):
    """Per gene (n_in, n_pass, [(contig, position, strand, (outside_mm0, outside_hit_sum, members_hit, family_size), the site's
    row in the reference)], [each row's index in its contig's strand table]): a plain
    loop over the genes and the rows of their contig's tables; the plain joined columns are the device's (tests/
    test_specificity_join.py holds them), the family columns the reference's.  min_score and also(contig, strand, row index of
    the contig's strand table) -> bool are the predicate's other terms: a row passes only if they hold as well."""
    out = []
    more = lambda kc, strand, i, x: float(x) >= float(min_score) and (also is None or bool(also(kc, strand, i)))
    for g, (_, kc, lo, hi) in enumerate(case.genes):
        rows = []
        for strand, name in ((0, "plus"), (1, "minus")):
            pos, score = tables[kc]["pos_" + name], tables[kc]["score_" + name]
            if columns is None:  # (no specificity join: every scored row of the gene passes the joined terms)
                cuts = [int(p) - (0 if strand else 3) for p in pos.tolist()]
                rows += [(more(kc, strand, i, score[i]), -int(np.float64(score[i]).view(np.uint64)), cuts[i], strand, int(pos[i]), None, None, i)
                         for i in range(pos.size) if score[i] != -1.0 and lo <= cuts[i] <= hi]
                continue
            c0, hs = columns[kc]["self_counts_" + name][:, 0], columns[kc]["self_sum_" + name]
            for i in range(pos.size):
                cut = int(pos[i]) - 3 if strand == 0 else int(pos[i])
                if score[i] == -1.0 or not lo <= cut <= hi:
                    continue
                r = row_of.get((kc, int(pos[i]) - 20 if strand == 0 else int(pos[i]), strand))
                joined = int(c0[i]) != nat.SELF_UNJOINED_COUNT
                assert joined == (r is not None)
                values, ok = None, joined
                if joined:
                    values = fref.selection_values(g, case.gene_family, case.sizes, int(fam_ref["site_family"][r]), int(c0[i]), int(hs[i]),
                                                   int(fam_ref["fam_counts"][r][0]), fam_ref["fam_sum"][r], fam_ref["fam_cover"][r])
                    ok = ((max_perfect is None or int(c0[i]) <= max_perfect) and (max_hit_sum is None or int(hs[i]) <= max_hit_sum)
                          and fref.passes_family(values, *limits) and more(kc, strand, i, score[i]))
                rows.append((ok, -int(np.float64(score[i]).view(np.uint64)), cut, strand, int(pos[i]), values, r, i))
        passing = sorted(r[1:] for r in rows if r[0])
        out.append((len(rows), len(passing), [(kc, p, st, v, r) for _, _, st, p, v, r, _ in passing[:K]], [r[-1] for r in passing[:K]]))
    return out


def _check_selection_file(case, got, want, fam_ref):
    """The rows of a selection file written with --families against the reference's selection: gene, rank, passing and the
    seven family fields; returns the number of lines."""
    from cropsr_amd.cli import FAMILY_HEADER
    assert got[0][:3] == ["gene", "rank", "passing"] and got[0][-7:] == FAMILY_HEADER
    at = 1
    for gi, (_, n_pass, rows, _) in enumerate(want):
        f = case.gene_family[gi]
        for rank, (kc, pos, strand, values, r_) in enumerate(rows):
            line = got[at]
            applies = f != NONE and int(fam_ref["site_family"][r_]) == f
            members = [i for i, (ff, m) in zip(case.idents, zip(case.gene_family, case.gene_member))
                       if ff == f and (fam_ref["fam_cover"][r_] >> m) & 1] if applies else [case.idents[gi]]
            assert line[:3] == ["gene:" + case.idents[gi], str(rank + 1), str(n_pass)], (gi, rank)
            assert line[-7:] == ["" if f == NONE else case.fam_names[f], str(values[3]), str(values[2]), ";".join("gene:" + m for m in members),
                                 str(values[0]), "%.6f" % (values[1] / float(1 << 30)), "%.6f" % sref.specificity([values[1]])[0]]
            at += 1
    assert at == len(got)
    return at


SLICES = pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
CUT_GENES = ("A1", "A2", "A3", "R255", "R256", "R257", "B_outer")  # more than 64 rows each: cut and merged at slices of 64


def _assert_selection_equals(case, got, want):
    """A device Selection with family fields against _reference_selection's rows, field by field."""
    assert got.n_in.tolist() == [w[0] for w in want] and got.n_pass.tolist() == [w[1] for w in want]
    at = 0
    for gi, (_, _, rows, _) in enumerate(want):
        for rank, (kc, pos, strand, values, _) in enumerate(rows):
            row = got.rows[at]
            assert (row["gene"], row["rank"], row["contig"], row["position"], row["strand"]) == (gi, rank + 1, kc, pos, b"+-"[strand:strand + 1])
            assert (int(got.outside_mm0[at]), int(got.outside_hit_sum[at]), int(got.members_hit[at]), int(got.family_size[at])) == values
            members = got.members[at]
            assert len(members) == values[2] and all(m in got.labels for m in members)
            if values[2] == 1 and case.gene_family[gi] == NONE:
                assert members == [got.labels[gi]]
            at += 1
    assert at == len(got.rows)


def _run_lengths(case, tables):
    """Rows of every gene's two runs in its contig's tables, scored or not: what the kernel's runs hold (tests/test_select.py
    has the same restatement per arena; a gene here lies in one contig, so in one arena)."""
    out = []
    for _, kc, lo, hi in case.genes:
        cp, cm = tables[kc]["pos_plus"].astype(np.int64) - 3, tables[kc]["pos_minus"].astype(np.int64)
        out.append(int(((cp >= lo) & (cp <= hi)).sum() + ((cm >= lo) & (cm <= hi)).sum()))
    return np.array(out)


def _assert_the_case_cuts(case, tables, stats, slice_rows):
    """At slices of 64 the genes of more than 64 rows go through the merge, the named ones among them; merged_genes is their
    number, summed over the arenas (select.sum_stats).  At the default nothing is cut."""
    n = _run_lengths(case, tables)
    if slice_rows is None:
        assert n.max() < 65536 and stats["merged_genes"] == 0
        return
    assert all(n[case.idents.index(i)] > slice_rows for i in CUT_GENES)
    assert stats["merged_genes"] == int((n > slice_rows).sum()) >= len(CUT_GENES)
    assert stats["items"] == int(np.maximum(1, -(-n // slice_rows)).sum())


@pytest.mark.gpu
@SLICES
def test_gpu_selection_with_family_limits(engine, case, slice_rows):
    from cropsr_amd import select as sel
    fam_ref = case.rows(3, "hsu2013", 0)
    row_of = {s: r for r, s in enumerate(fam_ref["sites"])}
    gene = {ident: i for i, ident in enumerate(case.idents)}
    ann, table = case.table()
    g = engine.genome(case.contigs, max_words=MAX_WORDS)
    try:
        areq = annotate.Request(ann, case.names, 0)
        plain = g.scan_score(20, specificity={})
        tables = [plain.contig(k) for k in range(len(case.contigs))]
        s1_sums = None

        def run(K, params=None, **limits):
            req = sel.Request(sel.Params(K, **(params or {})), areq, slice_rows, families=table, **limits)
            got = g.scan_score(20, specificity={}, select=req).selection
            bound = None if limits.get("min_specificity_outside") is None else sel.max_hit_sum_for(limits["min_specificity_outside"])
            p = params or {}
            want = _reference_selection(case, tables, plain.columns, fam_ref, row_of, K, p.get("max_perfect"),
                                        None if p.get("min_specificity") is None else sel.max_hit_sum_for(p["min_specificity"]),
                                        (limits.get("min_members"), limits.get("max_perfect_outside"), bound))
            _assert_selection_equals(case, got, want)
            _assert_the_case_cuts(case, tables, got.stats, slice_rows)
            return got, want

        for K in (1, 5, 64):
            # the reference first: on the three-member family plain max_perfect 0 passes nothing, the family limit the shared guides
            got, want = run(K, params=dict(max_perfect=0))
            assert all(want[gene[i]][1] == 0 and want[gene[i]][0] > 100 for i in ("A1", "A3"))
            got, want = run(K, max_perfect_outside=0)
            assert all(100 < want[gene[i]][1] < want[gene[i]][0] for i in ("A1", "A3"))
            for members in (2, "all"):
                got, want = run(K, min_members=members)
                n_a1, n_f1 = want[gene["A1"]], want[gene["F1"]]
                assert 0 < n_a1[1] and (members == 2 or n_a1[1] < n_a1[0])  # (some of A1's guides miss the drifted copy A2)
                assert n_f1[0] > 50 and (n_f1[1] == 0 if members == 2 else n_f1[1] > 50)  # a family of one: 'all' is 1
                assert want[gene["lonely"]][1] == (0 if members == 2 else want[gene["lonely"]][0]) and want[gene["lonely"]][0] > 0
            # the overlapping-gene rows: D1's rows in C1's range belong to C1's family and count as plain rows for D1
            if K == 64:
                _, free_want = run(K)
                assert any(7500 <= (p - 3 if st == 0 else p) <= 7900 and v[2:] == (1, 2) for _, p, st, v, _ in free_want[gene["D1"]][2])
                assert any(v[3] == 1 and v[2] == 1 for _, _, _, v, _ in free_want[gene["lonely"]][2])  # a gene in no family
            # a specificity outside the family that nothing of S1 reaches, and one that exactly K of its rows reach
            got, want = run(K, min_specificity_outside=1.0)
            assert want[gene["S1"]][1] == 0 and want[gene["S1"]][0] >= 6 and want[gene["A2"]][1] > 100
            if s1_sums is None:
                free, _ = run(64)
                s1_sums = sorted(int(x) for x, gi in zip(free.outside_hit_sum, free.rows["gene"]) if gi == gene["S1"])
                assert len(s1_sums) >= 6 and s1_sums[0] > 0
                assert s1_sums[0] < s1_sums[1] and s1_sums[4] < s1_sums[5]  # the case genome: no tie at the K-th sum, K = 1, 5
            if K < 64:
                threshold = float(srch.specificity(np.uint64(s1_sums[K - 1])))
                got, want = run(K, min_specificity_outside=threshold)
                assert want[gene["S1"]][1] == K == int((got.rows["gene"] == gene["S1"]).sum())
        # family fields without limits: nothing is filtered
        free, _ = run(5)
        base = g.scan_score(20, specificity={}, select=sel.Request(sel.Params(5), areq)).selection
        assert (free.rows == base.rows).all() and (free.n_pass == base.n_pass).all() and base.outside_mm0 is None
        assert free.stats["family_select_ms"] == 0.0 and run(5, min_members=2)[0].stats["family_select_ms"] > 0.0
    finally:
        g.close()
        ann.close()


@pytest.mark.gpu
def test_gpu_more_genes_than_one_launch(engine, case):
    """The family kernel behind the driver's launch loop (crp_select_run hands every launch `d_items + first`): the genes of a
    one-arena build tiled to more than 2^20 (tests/select_scale_cases.py), their family ids and sizes taken through the tiling,
    under min_members = 2 and max_perfect_outside = 0.  At the default slices the second launch begins at gene 2^20; at slices
    of 64 a cut gene's pieces -- the genes of 255, 256 and 257 sites are among the cut ones -- lie on both sides of every launch
    boundary.  n_in, n_pass and sel whole, against the loop statement's selection of the base genes taken through the tiling."""
    import select_scale_cases as scale
    from cropsr_amd import select as sel
    K, G = 5, scale.G
    fam_ref = case.rows(3, "hsu2013", 0)
    row_of = {s: r for r, s in enumerate(fam_ref["sites"])}
    ann, table = case.table()
    g = engine.genome(case.contigs)
    try:
        assert len(g.arenas) == 1 and g.groups == [list(range(len(case.contigs)))]
        areq = annotate.Request(ann, case.names, 0)
        plain = g.scan_score(20, specificity={})
        tables = [plain.contig(k) for k in range(len(case.contigs))]
        want = _reference_selection(case, tables, plain.columns, fam_ref, row_of, K, limits=(2, 0, None))
        # (the limits pass a row and fail a row of the three homeologs: test_gpu_selection_with_family_limits shows each alone)
        assert all(0 < want[case.idents.index(i)][1] < want[case.idents.index(i)][0] for i in ("A1", "A3"))
        # the reference per layout row, sel packed as the device packs it: strand << 31 | the row in the arena's strand table
        lo, hi, gene = areq.gene_layout(sel.arena_layout(g, 0))
        gi = np.asarray(gene, dtype=np.int64)
        assert sorted(gi.tolist()) == list(range(len(case.genes)))  # whole contigs in one arena: one layout row a gene
        before = [np.cumsum([0] + [len(t["pos_" + name]) for t in tables]) for name in ("plus", "minus")]
        n_base = gi.size
        base = [np.zeros(n_base, np.uint32), np.zeros(n_base, np.uint32), np.full((n_base, K), NONE, np.uint32)]
        for r, x in enumerate(gi.tolist()):
            base[0][r], base[1][r] = want[x][0], want[x][1]
            for rank, ((kc, _, strand, _, _), index) in enumerate(zip(want[x][2], want[x][3])):
                base[2][r, rank] = strand << 31 | (int(before[strand][kc]) + index)
        total = _run_lengths(case, tables)[gi]
        assert sorted(total[[gi.tolist().index(case.idents.index(i)) for i in ("R255", "R256", "R257")]].tolist()) == [255, 256, 257]
        family = np.asarray(table.gene_family)[gi]
        size = np.array([table.family_size(int(x)) for x in gi], np.uint32)
        done = []

        ids = scale.tiling(range(n_base), G, scale.boundary_start(total, list(range(n_base)), 64))
        assert scale.straddles(total[ids], 64)

        def after_join(a, handle, cols, family_joined=None):
            for slice_rows in (None, 64):
                cut = scale.host_cut(total[ids], slice_rows or 65536)
                h = sel.ArenaSelect(g.arenas[0], lo[ids], hi[ids])
                try:
                    if slice_rows:
                        h.set_limits(slice_rows)
                    h.set_family(family[ids], size[ids])
                    h.set_family_limits(sel.FamilyLimits(2, 0))
                    h.run(sel.Params(K), handle)
                    got, stats, fstats = h.fetch(), h.stats(), h.family_stats()
                finally:
                    h.close()
                for x, w, name in zip(got, base, ("n_in", "n_pass", "sel")):
                    assert np.array_equal(x, w[ids]), (slice_rows, name, int((x != w[ids]).reshape(G, -1).any(axis=1).sum()))
                assert stats["items"] == cut["items"] and stats["launches"] == -(-cut["items"] // scale.MAX_ITEMS) >= 2
                assert stats["merged_genes"] == cut["cut_genes"] and fstats["family_select_ms"] > 0
                if slice_rows is None:
                    assert stats["items"] == G and stats["launches"] == 2
                else:
                    assert stats["items"] > G and cut["cut_genes"] > 0
            done.append(True)

        g._scan_score(20, False, False, True, None)
        srch.specificity_columns(g, 20, after_join=after_join, families=fam.genome_rows(table, g, areq))
        assert done
    finally:
        g.close()
        ann.close()


# ------------------------------------------------------------------ family limits with the predicate's other terms
# CDS rows for require_cds, on a copy of the case GFF (family_cases.build()'s text stays what the other tests read): parts of
# the three homeologs and of the nested pair
CDS_ROWS = (("chrA", 1201, 1700, "A1.cds"), ("chrB", 2250, 2900, "A2.cds"), ("chrD", 3500, 4100, "A3.cds"), ("chrA", 2900, 3300, "B.cds"))
FAMILY_LIMITS = dict(min_members=2, max_perfect_outside=0)
REPAIR_LIMITS = dict(min_mh=300, min_oof=55)


def _property_limits():
    from test_select_pairs import PROPERTY_LIMITS as L
    return dict(gc_min=L.gc_min, gc_max=L.gc_max, max_run=L.max_run, max_t_run=L.max_t_run, max_stem=L.max_stem)


def _combinations():
    """name -> (Params' keywords, Request's keywords): each of the other terms with the family limits, and all at once."""
    one = {"min-score": (dict(min_score=0.2), {}), "specificity": (dict(max_perfect=1, min_specificity=0.3), {}),
           "cds": (dict(require_cds=True), {}), "properties": ({}, _property_limits()), "repair": ({}, dict(REPAIR_LIMITS))}
    everything = ({}, {})
    for params, request in one.values():
        everything[0].update(params)
        everything[1].update(request)
    return dict(one, all=everything)


COMBINATIONS = ("min-score", "specificity", "cds", "properties", "repair", "all")


class Combined:
    """The case with CDS rows, and per contig the truth of the other terms for the rows of given tables: the packed
    properties and repair scores from the references (tests/guide_properties_reference.py, tests/repair_reference.py) and the
    CDS verdict from the annotation's label flags (oracle/annotate_oracle.host_join over the rows, select_reference.cds_flags
    over the strings)."""

    def __init__(self, case, tmp):
        self.case = case
        self.gff_path = os.path.join(tmp, "case_cds.gff")
        with open(self.gff_path, "w") as f:
            f.write(case.gff + "".join("%s\ttest\tCDS\t%d\t%d\t.\t+\t0\tID=%s\n" % (n, lo + 1, hi + 1, i) for n, lo, hi, i in CDS_ROWS))
        self.ann = annotate.Annotation(self.gff_path)
        assert self.ann.genes()[0] == ["gene:" + i for i in case.idents]  # the genes are what they were
        self.table = fam.FamilyTable(fam.parse_families(case.families), self.ann.genes()[0])
        self._want = {}

    def close(self):
        self.ann.close()

    def truth(self, tables):
        import guide_properties_reference as gpref
        import repair_reference as rref
        from oracle import annotate_oracle
        flags = selref.cds_flags([self.ann.strings[k] for k in range(len(self.ann.strings))])
        assert 0 < flags.sum() < flags.size
        out = []
        for k, (name, text) in enumerate(zip(self.case.names, self.case.contigs)):
            h = tables[k]
            feat = annotate_oracle.host_join(self.ann, name, 0, 0, h, 20, len(text))
            t = {}
            for strand, s in ((0, "plus"), (1, "minus")):
                ids = np.asarray(feat[strand]).astype(np.int64)
                t["cds_" + s] = (ids != NONE) & (np.concatenate([flags, [0]])[np.where(ids == NONE, flags.size, ids)] != 0)
                t["props_" + s] = gpref.column_numpy(text, h["pos_" + s], bool(strand), 20)
                t["repair_" + s] = rref.column_numpy(text, h["pos_" + s], bool(strand), 30)
            out.append(t)
        return out

    def want(self, key, tables, columns, name):
        """_reference_selection at K = 5 for a combination (None: the family limits alone), once per key; the assertion that
        the combination's own terms pass a row and fail a row of some family gene that the family limits alone pass is made
        here, on the reference, before any device result is looked at."""
        from cropsr_amd import select as sel
        import guide_properties_reference as gpref
        import repair_reference as rref
        if (key, name) in self._want:
            return self._want[(key, name)]
        case = self.case
        fam_ref = case.rows(3, "hsu2013", 0)
        row_of = {s: r for r, s in enumerate(fam_ref["sites"])}
        limits = (FAMILY_LIMITS["min_members"], FAMILY_LIMITS["max_perfect_outside"], None)
        if name is None:
            out = _reference_selection(case, tables, columns, fam_ref, row_of, 5, limits=limits)
        else:
            if (key, "truth") not in self._want:
                self._want[(key, "truth")] = self.truth(tables)
            truth = self._want[(key, "truth")]
            params, request = _combinations()[name]
            strands = ("plus", "minus")
            terms = []
            if params.get("require_cds"):
                terms.append(lambda kc, st, i: truth[kc]["cds_" + strands[st]][i])
            if "gc_min" in request:
                lim = tuple(request[k] for k in ("gc_min", "gc_max", "max_run", "max_t_run", "max_stem"))
                terms.append(lambda kc, st, i: gpref.limits_pass(truth[kc]["props_" + strands[st]][i:i + 1], lim)[0])
            if "min_mh" in request:
                lim2 = (request["min_mh"], request["min_oof"])
                terms.append(lambda kc, st, i: rref.limits_pass(truth[kc]["repair_" + strands[st]][i:i + 1], lim2)[0])
            out = _reference_selection(case, tables, columns, fam_ref, row_of, 5, params.get("max_perfect"),
                                       None if params.get("min_specificity") is None else sel.max_hit_sum_for(params["min_specificity"]),
                                       limits, also=lambda kc, st, i: all(t(kc, st, i) for t in terms), min_score=params.get("min_score", 0.0))
            alone = self.want(key, tables, columns, None)
            in_family = [gi for gi in range(len(case.genes)) if case.gene_family[gi] != NONE]
            assert all(out[gi][1] <= alone[gi][1] and out[gi][0] == alone[gi][0] for gi in range(len(case.genes)))
            assert any(0 < out[gi][1] < alone[gi][1] for gi in in_family), name
        self._want[(key, name)] = out
        return out


@pytest.fixture(scope="module")
def combined(case, tmp_path_factory):
    c = Combined(case, str(tmp_path_factory.mktemp("families_cds")))
    yield c
    c.close()


def _oracle_view(case, orc):
    """The tables of every contig from the CPU oracle and the plain joined columns from the CPU self search, as
    FamilyOracleBackend.scan has them: what the loop statement needs without a GPU."""
    import specificity_join_cases as jcases
    tables = [orc.scan_score(t, 20) for t in case.contigs]
    sites, _, counts, hs = selfref.search_self(case.contigs, PATTERN, 3, 3, GUIDE_PATTERN, sref.W_HSU)
    arr = np.empty(len(sites), srch.SELF_SITE_DTYPE)
    arr["contig"], arr["position"] = [s[0] for s in sites], [s[1] for s in sites]
    arr["strand"] = [b"+-"[s[2]:s[2] + 1] for s in sites]
    return tables, jcases.join_fast(tables, arr, counts.astype(np.uint32), np.array(hs, np.uint64), 20)


def test_combined_limits_pass_and_fail_rows_on_the_reference(case, combined, oracle):
    """Every combination of test_gpu_family_limits_combined_with_the_other_limits, on the CPU's tables and columns: its terms
    take rows of a family gene away that the family limits alone pass, and leave some (Combined.want asserts it)."""
    tables, columns = _oracle_view(case, oracle)
    alone = combined.want("cpu", tables, columns, None)
    gene = {ident: i for i, ident in enumerate(case.idents)}
    assert all(alone[gene[i]][1] > 50 for i in ("A1", "A2", "A3")) and alone[gene["F1"]][1] == 0
    for name in COMBINATIONS:
        want = combined.want("cpu", tables, columns, name)
        assert sum(w[1] for w in want) > 0
    everything = combined.want("cpu", tables, columns, "all")
    for name in COMBINATIONS[:-1]:  # all at once is at most each
        assert all(a[1] <= w[1] for a, w in zip(everything, combined.want("cpu", tables, columns, name)))


@pytest.mark.gpu
@SLICES
@pytest.mark.parametrize("name", COMBINATIONS)
def test_gpu_family_limits_combined_with_the_other_limits(engine, case, combined, name, slice_rows):
    """min_members = 2 and max_perfect_outside = 0 behind min_score, the specificity thresholds, require_cds, the property
    limits and the repair limits, one at a time and all at once, at K = 5, with whole genes and with genes cut into slices."""
    from cropsr_amd import select as sel
    g = engine.genome(case.contigs, max_words=MAX_WORDS)
    try:
        areq = annotate.Request(combined.ann, case.names, 0)
        plain = g.scan_score(20, specificity={})
        tables = [plain.contig(k) for k in range(len(case.contigs))]
        want = combined.want("gpu", tables, plain.columns, name)  # (asserts on the reference that the terms pass and fail rows)
        params, request = _combinations()[name]
        req = sel.Request(sel.Params(5, **params), areq, slice_rows, families=combined.table, **dict(FAMILY_LIMITS, **request))
        got = g.scan_score(20, specificity={}, select=req).selection
        _assert_selection_equals(case, got, want)
        _assert_the_case_cuts(case, tables, got.stats, slice_rows)
        assert got.stats["family_select_ms"] > 0.0
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_selection_refusals(engine, case):
    from cropsr_amd import select as sel
    L = nat.lib()
    ann, table = case.table()
    g = engine.genome(case.contigs)
    handles = []
    try:
        areq = annotate.Request(ann, case.names, 0)
        g.scan_score(20)
        lo, hi, gene_idx = areq.gene_layout(sel.arena_layout(g, 0))
        s = sel.ArenaSelect(g.arenas[0], lo, hi)
        handles.append(s)
        ctx = g.arenas[0]._engine._ctx
        params = sel.Params(5).native()
        lim = nat.SelectFamilyLimits(0, 0, 2)
        assert L.crp_select_set_family_limits(s._h, ctypes.byref(nat.SelectFamilyLimits(0, 0, 65))) == nat.CRP_ERR_INVALID
        assert L.crp_select_set_family_limits(s._h, ctypes.byref(lim)) == nat.CRP_OK
        assert L.crp_select_run(s._h, ctypes.byref(params), None) == nat.CRP_ERR_STATE and b"crp_select_set_family" in L.crp_last_error(ctx)
        fam_ids = np.zeros(lo.size, np.uint32)
        ones = np.ones(lo.size, np.uint32)
        u32 = lambda a: a.ctypes.data_as(nat.u32p)
        assert L.crp_select_set_family(s._h, u32(fam_ids), u32(ones), lo.size - 1) == nat.CRP_ERR_INVALID
        assert L.crp_select_set_family(s._h, u32(fam_ids), u32(np.zeros(lo.size, np.uint32)), lo.size) == nat.CRP_ERR_INVALID
        assert L.crp_select_set_family(s._h, u32(fam_ids), u32(ones), lo.size) == nat.CRP_OK
        assert L.crp_select_run(s._h, ctypes.byref(params), None) == nat.CRP_ERR_STATE  # no self-search handle
        h = srch.ArenaSelfSearch(g.arenas[0], PATTERN, GUIDE_PATTERN, 3, 3)
        handles.append(h)
        h.join_hits(20, fetch=False)
        assert L.crp_select_run(s._h, ctypes.byref(params), h._h) == nat.CRP_ERR_STATE and b"family" in L.crp_last_error(ctx)
        q = np.zeros(1, np.uint32)
        out64 = np.zeros(1, np.uint64)
        assert L.crp_select_family_eval(s._h, h._h, u32(q), u32(q), 1, u32(q.copy()), out64.ctypes.data_as(nat.u64p), u32(q.copy()),
                                        u32(q.copy()), out64.copy().ctypes.data_as(nat.u64p)) == nat.CRP_ERR_STATE
        s.set_coding_limits(__import__("cropsr_amd.coding", fromlist=["Limits"]).Limits(0, 50))
        assert L.crp_select_run(s._h, ctypes.byref(params), h._h) in (nat.CRP_ERR_STATE, nat.CRP_ERR_UNSUPPORTED)
        s.set_coding_limits(None)
        pp = sel.PairParams(3).native()
        assert L.crp_select_run_pairs(s._h, ctypes.byref(params), ctypes.byref(pp), h._h) == nat.CRP_ERR_UNSUPPORTED
        assert L.crp_select_family_stats(s._h, None, 3) == nat.CRP_ERR_INVALID
    finally:
        for x in handles:
            x.close()
        g.close()
        ann.close()


# ------------------------------------------------------------------ the command line
def test_cli_refuses_before_any_side_effect(case, tmp_path):
    import subprocess
    import sys
    fa = tmp_path / "g.fa"
    fa.write_text(">c1\nACGT\n")
    gff = tmp_path / "g.gff"
    gff.write_text(case.gff)
    ok, bad, two = tmp_path / "ok.tsv", tmp_path / "bad.tsv", tmp_path / "two.tsv"
    ok.write_text(case.families)
    bad.write_text("A1\thomeo\textra\n")
    two.write_text("A1\thomeo\nA1\tother\n")
    out = tmp_path / "o.csv"
    base = ["-f", str(fa), "-g", str(gff), "-o", str(out)]
    full = base + ["--select", "5", "--specificity", "--families", str(ok)]
    cases_ = [(base + ["--select", "5", "--specificity", "--select-min-members", "2"], "belongs to --families"),
              (base + ["--select", "5", "--specificity", "--family-cover-mismatches", "1"], "belongs to --families"),
              (base + ["--select", "5", "--specificity", "--select-max-perfect-outside", "0"], "belongs to --families"),
              (base + ["--select", "5", "--specificity", "--select-min-specificity-outside", "0.5"], "belongs to --families"),
              (base + ["--specificity", "--families", str(ok)], "belongs to --select"),
              (base + ["--select", "5", "--families", str(ok)], "--specificity"),
              (["-f", str(fa), "-o", str(out), "--select", "5", "--specificity", "--families", str(ok)], "-g"),
              (full[:-1] + [str(tmp_path / "none.tsv")], "cannot read"),
              (full[:-1] + [str(bad)], "line 1"), (full[:-1] + [str(two)], "line 2"),
              (full + ["--family-cover-mismatches", "4"], "0..3"), (full + ["--family-cover-mismatches", "x"], "0..3"),
              (full + ["--select-min-members", "0"], "1..64"), (full + ["--select-min-members", "65"], "1..64"),
              (full + ["--select-min-members", "most"], "1..64"), (full + ["--select-max-perfect-outside", "-1"], "count"),
              (full + ["--select-min-specificity-outside", "1.5"], "0..1"),
              (full + ["--select-min-members", "2", "--select-coding-min", "5"], "one or the other"),
              (full + ["--select-max-perfect-outside", "0", "--select-stop"], "one or the other"),
              (full + ["--select-min-members", "all", "--select-splice", "donor"], "one or the other"),
              (full + ["--select-min-members", "2", "--select-pairs", "3"], "--select-pairs"),
              (full + ["--devices", "0,1"], "one GPU")]
    for args, word in cases_:
        r = subprocess.run([sys.executable, "-m", "cropsr_amd"] + args, cwd=ROOT, capture_output=True, text=True,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode != 0 and "cropsr_amd:" in r.stderr and word in r.stderr, (args, r.stderr)
        assert not out.exists() and not (tmp_path / "o.csv.selected.csv").exists()


@pytest.mark.gpu
def test_gpu_cli_end_to_end(engine, case, tmp_path):
    import csv
    import subprocess
    import sys
    fa = tmp_path / "case.fa"
    fa.write_bytes(b"\n".join(b">" + n.encode() + b"\n" + c for n, c in zip(case.names, case.contigs)))  # (one line a contig: dec = 0)
    fam_file = tmp_path / "families.tsv"
    fam_file.write_text(case.families)
    out = tmp_path / "guides.csv"
    cmd = [sys.executable, "-m", "cropsr_amd", "-f", str(fa), "-g", case.gff_path, "-o", str(out), "--cas9", "--specificity", "--select", "5",
           "--families", str(fam_file), "--select-min-members", "all", "--select-max-perfect-outside", "0"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))  # (run beside the files it writes)
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "2 names of" in r.stderr  # the names the GFF lacks, reported once
    with open(str(out) + ".selected.csv", newline="") as f:
        got = list(csv.reader(f))
    # what the file must hold: the reference's selection over the tables of the same scan
    fam_ref = case.rows(3, "hsu2013", 0)
    row_of = {s: r_ for r_, s in enumerate(fam_ref["sites"])}
    g = engine.genome(case.contigs)
    try:
        plain = g.scan_score(20, specificity={})
        tables = [plain.contig(k) for k in range(len(case.contigs))]
    finally:
        g.close()
    want = _reference_selection(case, tables, plain.columns, fam_ref, row_of, 5, limits=("all", 0, None))
    assert _check_selection_file(case, got, want, fam_ref) > 20
    assert sum(1 for line in got[1:] if line[0] == "gene:A1") == 5
    # without --families every byte of both files is what it was
    import hashlib
    md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest()
    base = [c for c in cmd if c not in ("--families", str(fam_file), "--select-min-members", "all", "--select-max-perfect-outside", "0")]
    free = cmd[:cmd.index("--select-min-members")]
    for variant in (base, free):
        r = subprocess.run(variant + ["--seed", "7"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(str(out) + ".selected.csv", newline="") as f:
            rows_ = list(csv.reader(f))
        if variant is base:
            main_md5, base_rows = md5(str(out)), rows_
            assert base_rows[0][-1] != "outside_specificity"
        else:  # --families alone adds fields and filters nothing: the main table and the old fields are the same bytes
            assert md5(str(out)) == main_md5 and [line[:-7] for line in rows_] == base_rows


# ------------------------------------------------------------------ the command line over the oracle backend (CPU)
from conftest import OracleBackend  # noqa: E402


class FamilyOracleBackend(OracleBackend):
    """OracleBackend plus `specificity` (the CPU references' self search, joined in numpy) and `select` with a family table: the
    selection by the loop statement (_reference_selection) over the family reference's rows."""

    def __init__(self, orc, case):
        OracleBackend.__init__(self, orc)
        self.case, self.selected = case, []

    def scan(self, strings, l, offtarget=False, annotation=None, specificity=None, select=None):
        import specificity_join_cases as jcases
        from cropsr_amd import select as sel
        case = self.case
        out = OracleBackend.scan(self, strings, l, offtarget=offtarget, annotation=annotation)
        assert [bytes(s) for s in strings] == case.contigs
        columns = None
        if specificity is not None:
            assert (specificity["max_mm"], specificity["candidate_pam"], specificity["score"]) == (3, "NRG", "hsu2013")
            sites, _, counts, hs = selfref.search_self(case.contigs, PATTERN, 3, 3, GUIDE_PATTERN, sref.W_HSU)
            arr = np.empty(len(sites), srch.SELF_SITE_DTYPE)
            arr["contig"], arr["position"] = [s[0] for s in sites], [s[1] for s in sites]
            arr["strand"] = [b"+-"[s[2]:s[2] + 1] for s in sites]
            columns = jcases.join_fast(out, arr, counts.astype(np.uint32), np.array(hs, np.uint64), l)
            for h, cols in zip(out, columns):
                h.update(cols)
        if select is None:
            return out
        table, lim, p = select.families, select.family_limits, select.params
        fam_ref = case.rows(3, "hsu2013", select.family_cover_mm if table is not None else 0)
        row_of = {s: r for r, s in enumerate(fam_ref["sites"])}
        limits = (None, None, None)
        if lim is not None:
            limits = ("all" if lim.min_members == nat.SELECT_ALL_MEMBERS else lim.min_members or None,
                      None if lim.max_mm0_outside == sel.NO_BOUND_MM0 else lim.max_mm0_outside,
                      None if lim.max_hit_sum_outside == sel.NO_BOUND_SUM else lim.max_hit_sum_outside)
        want = _reference_selection(case, out, columns, fam_ref, row_of, p.k, p.max_mm0, p.max_hit_sum, limits)
        self.selected.append((want, fam_ref))
        labels = select.annotation.annotation.genes()[0]
        rows = np.empty(sum(len(w[2]) for w in want), sel.ROW_DTYPE)
        values, members, at = [], [], 0
        for gi, (_, _, picked, index) in enumerate(want):
            for rank, ((kc, pos, strand, v, r), i) in enumerate(zip(picked, index)):
                score = out[kc]["score_minus" if strand else "score_plus"][i]
                rows[at] = (gi, rank + 1, kc, pos, b"+-"[strand:strand + 1], score, i)
                values.append(v)
                if table is not None:
                    f = int(table.gene_family[gi])
                    applies = f != NONE and int(fam_ref["site_family"][r]) == f
                    members.append(table.member_labels(gi, fam_ref["fam_cover"][r]) if applies else [labels[gi]])
                at += 1
        selection = sel.Selection(labels, np.array([w[0] for w in want]), np.array([w[1] for w in want]), rows)
        if table is not None:
            selection.outside_mm0, selection.members_hit, selection.family_size = (np.array([v[j] for v in values], np.uint32) for j in (0, 2, 3))
            selection.outside_hit_sum, selection.members = np.array([v[1] for v in values], np.uint64), members
        out = sel.HitList(out)
        out.selection = selection
        return out


def _run_cli(case, tmp_path, monkeypatch, extra, backend, name):
    import io
    from cropsr_amd import cli
    monkeypatch.chdir(tmp_path)
    fa = tmp_path / "case.fa"
    fa.write_bytes(b"\n".join(b">" + n.encode() + b"\n" + c for n, c in zip(case.names, case.contigs)))  # (one line a contig: dec = 0)
    out_csv = str(tmp_path / name)
    argv = ["-f", str(fa), "-g", case.gff_path, "-o", out_csv, "--cas9", "--seed", "11", "--each-contig-once"] + list(extra)
    cli.run(cli.build_parser().parse_args(argv), backend=backend, out=io.StringIO())
    return out_csv


def _md5(path):
    import hashlib
    with open(path, "rb") as f:
        return hashlib.md5(f.read()).hexdigest()


def test_cli_family_fields_over_the_oracle(case, oracle, tmp_path, monkeypatch, capsys):
    import csv
    from test_select import SelectingOracleBackend
    from test_specificity_join import JoinBackend
    fam_file = tmp_path / "families.tsv"
    fam_file.write_text(case.families)
    backend = FamilyOracleBackend(oracle, case)
    read = lambda path: list(csv.reader(open(path, newline="")))
    # without --families every byte is what the earlier backends' runs give: the main CSV and the selection file, by md5
    old = _run_cli(case, tmp_path, monkeypatch, ["--select", "5"], SelectingOracleBackend(oracle), "old.csv")
    new = _run_cli(case, tmp_path, monkeypatch, ["--select", "5"], backend, "new.csv")
    assert _md5(old) == _md5(new) and _md5(old + ".selected.csv") == _md5(new + ".selected.csv")
    joined = _run_cli(case, tmp_path, monkeypatch, ["--specificity"], JoinBackend(oracle), "joined.csv")
    plain = _run_cli(case, tmp_path, monkeypatch, ["--specificity", "--select", "5"], backend, "plain.csv")
    assert _md5(joined) == _md5(plain) and read(plain + ".selected.csv")[0][-1] != "outside_specificity"
    capsys.readouterr()
    # --families alone: seven more fields, nothing filtered, the main CSV and the old fields the same bytes
    free = _run_cli(case, tmp_path, monkeypatch, ["--specificity", "--select", "5", "--families", str(fam_file)], backend, "free.csv")
    assert "2 names of" in capsys.readouterr().err  # the names the GFF lacks, reported once
    assert _md5(free) == _md5(plain)
    got, was = read(free + ".selected.csv"), read(plain + ".selected.csv")
    assert [line[:-7] for line in got] == was and len(got) > 200
    assert _check_selection_file(case, got, *backend.selected[-1]) == len(got)
    assert any(line[-7] == "" and line[-6:-3] == ["1", "1", line[0]] for line in got[1:])  # a gene in no family: empty, size 1, itself
    # the limits and the cover limit reach the selection; the file holds the reference's rows and values
    strict = _run_cli(case, tmp_path, monkeypatch, ["--specificity", "--select", "5", "--families", str(fam_file), "--select-min-members", "all",
                                                    "--select-max-perfect-outside", "0", "--select-min-specificity-outside", "0.9",
                                                    "--family-cover-mismatches", "2"], backend, "strict.csv")
    req_want, req_ref = backend.selected[-1]
    assert req_ref is case.rows(3, "hsu2013", 2) and _md5(strict) == _md5(plain)
    got = read(strict + ".selected.csv")
    assert 20 < _check_selection_file(case, got, req_want, req_ref) < len(was)
    assert sum(1 for line in got[1:] if line[0] == "gene:A1") == 5 and all(line[-3] == "0" for line in got[1:])
    # a family of 65 members ends the run before the output file is touched
    many = tmp_path / "many.tsv"
    many.write_text(case.too_many)
    with pytest.raises(SystemExit) as e:
        _run_cli(case, tmp_path, monkeypatch, ["--specificity", "--select", "5", "--families", str(many)], backend, "many.csv")
    assert "64" in str(e.value) and not (tmp_path / "many.csv").exists() and not (tmp_path / "many.csv.selected.csv").exists()


# ------------------------------------------------------------------ tools/family_bench.py: its host check, without a GPU
def test_family_bench_host_check_equals_reference(case):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import family_bench as fb
    texts = [fb.CODE[np.frombuffer(c, np.uint8)] for c in case.contigs]
    genes = [(kc, lo, hi) for _, kc, lo, hi in case.genes]
    scheme = srch.check_specificity(20, 3)[3]
    for C in (0, 2):
        ref = case.rows(3, "hsu2013", C)
        rng = np.random.default_rng(C)
        for f in range(len(case.fam_names)):
            mine = np.nonzero(ref["site_family"] == f)[0]
            rows = rng.choice(mine, min(12, mine.size), replace=False).tolist()
            got = fb.host_family_rows(texts, genes, case.gene_family, case.gene_member, f, [ref["sites"][r] for r in rows], 3, C, scheme)
            for r, (family, counts, total, cover) in zip(rows, got):
                assert family == f and counts.tolist() == ref["fam_counts"][r].tolist(), (f, r)
                assert total == ref["fam_sum"][r] and cover == ref["fam_cover"][r], (f, r)
        # a site of another family, a candidate that is no guide site, a place without a site: no row
        other = int(np.nonzero(ref["site_family"] == 1)[0][0])
        k, pos, strand = ref["cand"]
        nag = int(np.nonzero(~ref["cand_guide"] & (ref["cand_owner"] == 0))[0][0])
        for site in (ref["sites"][other], (int(k[nag]), int(pos[nag]), int(strand[nag])), (7, 5, 0)):
            assert fb.host_family_rows(texts, genes, case.gene_family, case.gene_member, 0, [site], 3, C, scheme)[0][0] == NONE
    # the planted families: later members carry the first member's letters, a few substituted
    strings = [bytearray(np.random.default_rng(1).choice(np.frombuffer(b"ACGT", np.uint8), 4000).tobytes()) for _ in range(2)]
    rows = [("g%d" % i, i % 2, 100 + 400 * i, 100 + 400 * i + 299) for i in range(8)]
    pairs = fb.plant_families(strings, rows, 4, 0.05, np.random.default_rng(2), dec=1)
    assert sorted(pairs) == sorted([("g%d" % i, "fam%d" % (i % 2)) for i in range(8)])
    first = bytes(strings[0][100:400])
    for i in (2, 4, 6):
        copy = bytes(strings[i % 2][100 + 400 * i:100 + 400 * i + 300])
        assert 0 < sum(a != b for a, b in zip(first, copy)) < 40
    assert fb.valu_per_pair()[0] == fb.FAMILY_VALU_PER_PAIR  # what DESIGN section 23 quotes: 40 VALU per 8 pairs
