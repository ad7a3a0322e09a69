"""The greedy family sets (cropsr_amd/family_sets.py, crp_select_family_step) against
tests/family_set_reference.py on the case genome of tests/family_set_cases.py.  The passing rows of every gene -- the
candidates -- come from test_families.py's loop statement of the selection, the family rows from family_reference.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import family_reference as fref
import family_set_cases as cases
import family_set_reference as sref_sets
import select_scale_cases as scale
from test_families import VALUES, FamilyOracleBackend, _oracle_view, _reference_selection, _run_cli, _run_lengths, _md5
from cropsr_amd import _native as nat
from cropsr_amd import annotate, families as fam
from cropsr_amd import search as srch

PATTERN, GUIDE_PATTERN = cases.PATTERN, cases.GUIDE_PATTERN
NONE = fam.NONE
EVERY = 10 ** 9  # a K that keeps every passing row


class Case:
    def __init__(self, tmp):
        self.__dict__.update(cases.build())
        self.idents = [g[0] for g in self.genes]
        self.pairs = fref.parse(self.families)
        self.fam_names, self.gene_family, self.gene_member, self.sizes, _ = fref.table(self.pairs, self.idents)
        self.gff_path = os.path.join(tmp, "case.gff")
        with open(self.gff_path, "w") as f:
            f.write(self.gff)
        self._rows, self._cands = {}, {}
        self.unknown, self.too_many = [], ""

    def rows(self, M, value_key, C):
        """The numpy family reference, computed once per (M, scheme, C); an unscored one gets sums of 0, as the device has them."""
        key = (M, value_key, C)
        if key not in self._rows:
            r = fref.family_rows(self.contigs, PATTERN, M, GUIDE_PATTERN, self.genes, self.gene_family, self.gene_member, C, VALUES[value_key][1])
            if r["fam_sum"] is None:
                r["fam_sum"] = [0] * len(r["sites"])
            self._rows[key] = r
        return self._rows[key]

    def table(self):
        ann = annotate.Annotation(self.gff_path)
        return ann, fam.FamilyTable(fam.parse_families(self.families), ann.genes()[0])

    def family(self, name):
        return self.fam_names.index(name)

    def gene(self, ident):
        return self.idents.index(ident)

    def candidates(self, key, tables, columns, fam_ref, arenas, limits=(None, None, None)):
        """(candidates, n_pass per gene) of the reference, once per key: every passing row of every family gene."""
        if key not in self._cands:
            row_of = {s: r for r, s in enumerate(fam_ref["sites"])}
            want = _reference_selection(self, tables, columns, fam_ref, row_of, EVERY, limits=limits)
            passing = [[(kc, pos, st, r, i) for (kc, pos, st, _, r), i in zip(w[2], w[3])] for w in want]
            arena_of = {k: a for a, group in enumerate(arenas) for k in group}
            key_of = lambda kc, st, i: int(np.float64(tables[kc]["score_minus" if st else "score_plus"][i]).view(np.uint64))
            cands = sref_sets.candidates(self.genes, self.gene_family, self.gene_member, passing, fam_ref, arena_of, key_of)
            self._cands[key] = (cands, [w[1] for w in want])
        return self._cands[key]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(str(tmp_path_factory.mktemp("family_sets")))


ONE_ARENA = [list(range(len(cases.NAMES)))]


@pytest.fixture(scope="module")
def cpu(case, oracle):
    """The CPU's tables and joined columns of the case genome (M = 3, hsu2013), and the reference's candidates over them."""
    tables, columns = _oracle_view(case, oracle)
    fam_ref = case.rows(3, "hsu2013", 0)
    free = case.candidates("cpu", tables, columns, fam_ref, cases.ARENAS_OF_THREE)
    strict = case.candidates("cpu-limits", tables, columns, fam_ref, cases.ARENAS_OF_THREE, limits=(None, 0, None))
    return dict(tables=tables, columns=columns, fam_ref=fam_ref, free=free, strict=strict)


def _by_family(picks):
    out = {}
    for p in picks:
        out.setdefault(p["family"], []).append(p)
    return out


# ------------------------------------------------------------------ the case genome (CPU)
def test_case_genome_carries_every_case(case, cpu):
    cands, n_pass = cpu["free"]
    picks, complete = sref_sets.greedy_loop(cands, case.sizes, 64)
    sets = _by_family(picks)
    f, g = case.family, case.gene
    assert 30_000 <= sum(len(c) for c in case.contigs) <= 45_000 and len(case.contigs) == 6
    assert len(case.fam_names) == 14 and case.gene_family[g("free")] == NONE
    # one guide suffices: three exact copies, complete in one step
    assert len(sets[f("one")]) == 1 and sets[f("one")][0]["gain"] == 3 and complete[f("one")]
    # gain beats score: the best-scoring candidate has gain 1, the pick a lower score and gain 2; exactly two steps
    mine = [c for c in cands if c[0] == f("gain")]
    top = max(mine, key=lambda c: c[6])
    first, second = sets[f("gain")]
    assert bin(top[7]).count("1") == 1 and first["gain"] == 2 and first["key"] < top[6] and second["gain"] == 1 and complete[f("gain")]
    assert not any(bin(c[7]).count("1") == 3 for c in mine)
    # ties: on the gain with different scores (the runner-up of `one`), and bit-equal pairs on gain and score, three ways
    gains3 = sorted((c[6] for c in cands if c[0] == f("one") and bin(c[7]).count("1") == 3), reverse=True)
    assert len(gains3) > 10 and gains3[0] > gains3[3]
    twin, strands, apart = sets[f("twin")][0], sets[f("strands")][0], sets[f("apart")][0]
    assert twin["tied"] == 3 and twin["gene"] == g("W1") and twin["cut"] < 2700 and twin["gain"] == 2  # the smallest cut; W2 comes first in the file
    assert g("W2") < g("W1") and len(sets[f("twin")]) == 1
    assert strands["tied"] == 2 and strands["gene"] == g("TS1") and g("TS2") < g("TS1") and strands["gain"] == 2
    other = [c for c in cands if c[0] == f("strands") and c[6] == strands["key"] and c[5] == g("TS2")]
    assert len(other) == 1 and other[0][4] != strands["strand"]  # its partner lies on the other strand
    assert apart["tied"] == 2 and (apart["contig"], apart["arena"], apart["gene"]) == (1, 0, g("TA1"))
    assert [c[1] for c in cands if c[0] == f("apart") and c[6] == apart["key"]] == [0, 1]  # one in either arena
    # cannot complete: K2 has no row, the set ends on gain 0; `three` needs three steps
    assert n_pass[g("K2")] == 0 and n_pass[g("K1")] > 10 and len(sets[f("stuck")]) == 1 and not complete[f("stuck")]
    assert [p["gain"] for p in sets[f("three")]] == [1, 1, 1] and complete[f("three")]
    for S in (1, 2):
        few, done = sref_sets.greedy_loop(cands, case.sizes, S)
        assert len(_by_family(few)[f("three")]) == S and not done[f("three")] and done[f("one")]
    # no passing row at all: no pick
    assert n_pass[g("N1")] == n_pass[g("N2")] == 0 and f("none") not in sets and not complete[f("none")]
    # 64 members: 64 steps of gain 1, every member has a row and no row covers two; the high bits decide half of the picks
    tiny = sets[f("tiny")]
    assert case.sizes[f("tiny")] == 64 and len(tiny) == 64 and all(p["gain"] == 1 for p in tiny) and complete[f("tiny")]
    assert tiny[-1]["covered"] == (1 << 64) - 1 and sum(1 for p in tiny[:32] if p["cover"] >> 32) > 5
    few, done = sref_sets.greedy_loop(cands, case.sizes, 63)
    assert len(_by_family(few)[f("tiny")]) == 63 and not done[f("tiny")]
    # wave-trip edges: members with 0, 1, 63, 64 and 65 passing rows; E0 cannot be covered
    assert [n_pass[g(i)] for i in ("E0", "E1", "E63", "E64", "E65")] == [0, 1, 63, 64, 65]
    assert len(sets[f("trips")]) == 4 and not complete[f("trips")]
    # overlapping members: a row of the overlap is a candidate of O1 and of O2, and for O2 both bits are in c
    lap = sets[f("lap")][0]
    both = [c for c in cands if c[0] == f("lap") and 6200 <= c[3] <= 6400]
    assert len(both) > 20 and len(both) == 2 * len({(c[3], c[4]) for c in both})
    assert lap["gene"] == g("O2") and lap["cover"] == 0b11 and 6200 <= lap["cut"] <= 6400 and len(sets[f("lap")]) == 1
    # a member inside another family's gene: its candidates cover it alone, although V2 holds a copy of its block
    v1 = [c for c in cands if c[5] == g("V1")]
    v2 = [c for c in cands if c[5] == g("V2")]
    assert len(v1) > 10 and all(c[7] == 0b01 for c in v1) and all(c[7] == 0b10 for c in v2) and [p["gain"] for p in sets[f("v")]] == [1, 1]
    assert sum(int(cpu["fam_ref"]["site_family"][r]) == f("z") for r, s in enumerate(cpu["fam_ref"]["sites"]) if s[0] == 0 and 7120 <= s[1] <= 7290) > 10
    # family limits: with max_perfect_outside = 0 the candidate picked first fails, and the set changes
    strict, strict_pass = cpu["strict"]
    loose_pick = sets[f("lim")][0]
    tight = _by_family(sref_sets.greedy_loop(strict, case.sizes, 64)[0])[f("lim")]
    assert not any(c[0] == f("lim") and (c[2], c[3], c[4]) == (loose_pick["contig"], loose_pick["cut"], loose_pick["strand"]) for c in strict)
    assert tight[0]["key"] < loose_pick["key"] and tight[0]["gain"] == 2 and 0 < strict_pass[g("L1")] < n_pass[g("L1")]


def test_numpy_and_loop_agree(case, cpu):
    for name in ("free", "strict"):
        cands, _ = cpu[name]
        for S in (1, 2, 5, 63, 64):
            assert sref_sets.greedy_numpy(cands, case.sizes, S) == sref_sets.greedy_loop(cands, case.sizes, S)
    cands = cpu["free"][0]
    for covered in (0, 1, 0xFFFFFFFF00000000, 0x5555555555555555):
        for f in range(len(case.sizes)):
            mine = [c for c in cands if c[0] == f]
            assert sref_sets.best_numpy(mine, covered) == sref_sets.best_loop(mine, covered)


def test_candidates_are_the_rows_behind_n_pass(case, cpu):
    for name in ("free", "strict"):
        cands, n_pass = cpu[name]
        per_gene = np.bincount([c[5] for c in cands], minlength=len(case.genes))
        for g in range(len(case.genes)):
            assert per_gene[g] == (n_pass[g] if case.gene_family[g] != NONE else 0)
        assert len({(c[5], c[2], c[3], c[4]) for c in cands}) == len(cands)  # each (gene, row) once
    assert case.gene_family[case.gene("free")] == NONE and cpu["free"][1][case.gene("free")] > 0


# ------------------------------------------------------------------ the step past one launch (2^20 items): the list and its reference
LATE_FAMILIES = ("gain", "three")  # more than one step each: they have a best candidate under both covered words


def _family_best_gene(cands, covered, f):
    mine = [c for c in cands if c[0] == f]
    b = sref_sets.best_loop(mine, covered[f])
    return None if b is None else mine[b][5]


def _late_case(case, cands, total, n_genes=scale.G, head=scale.MAX_ITEMS + 64):
    """The gene list of the step past one launch, in indices of case.genes: the family genes that have rows, tiled by
    select_scale_cases.late_list so that the genes holding the best candidate of LATE_FAMILIES -- under nothing covered and
    under what the reference greedy's first pick covers -- occur first behind position 2^20.  total: rows per gene."""
    F = len(case.sizes)
    base = [g for g in range(len(case.genes)) if case.gene_family[g] != NONE and total[g] > 0]
    after = {f: ps[-1]["covered"] for f, ps in _by_family(sref_sets.greedy_loop(cands, case.sizes, 1)[0]).items()}
    words = [[0] * F, [after.get(f, 0) for f in range(F)]]
    late = sorted({_family_best_gene(cands, w, case.family(name)) for w in words for name in LATE_FAMILIES})
    assert None not in late and len(late) >= 2
    glist = scale.late_list(base, late, n_genes, head)
    return dict(base=base, late=late, glist=glist, words=words, first=scale.first_occurrence(glist, len(case.genes)))


def _expected_step(case, cands, covered, first, place):
    """Per family the record crp_select_family_step returns for a handle over the list: best_loop over the base candidates with
    each candidate's gene relabelled to the first position of its gene in the list.  This is exact: the copies of a gene are
    equal in gain, key and tie -- they are the same table rows --, so among them the order's last term, the smaller layout
    row, decides for the first copy; and two different genes compare as their first copies do.  place(contig, cut, strand,
    index) -> (tie, row) as the device packs them, or None (then they are left out of the record)."""
    out = []
    for f in range(len(case.sizes)):
        mine = [c[:5] + (int(first[c[5]]),) + c[6:] for c in cands if c[0] == f]
        assert all(c[5] >= 0 for c in mine)
        b = sref_sets.best_loop(mine, covered[f])
        if b is None:
            out.append(dict(gain=0, key=0, cover=0, gene=NONE, tie=NONE, row=NONE))
            continue
        _, _, contig, cut, strand, gene, key, cover, _, index = mine[b]
        tie, row = place(contig, cut, strand, index) if place else (None, None)
        out.append(dict(gain=bin(cover & ~covered[f]).count("1"), key=key, cover=cover, gene=gene, tie=tie, row=row))
    return out


def test_the_late_list_puts_the_best_genes_behind_the_first_launch(case, cpu):
    """On the CPU's candidates, before any device is asked: the list's properties, the families whose best candidate lies
    behind item 2^20 and those whose best lies in front of it, and the relabelling argument by brute force on a short list."""
    cands = cpu["free"][0]
    total = _run_lengths(case, cpu["tables"])
    L = _late_case(case, cands, total)
    base, late, glist, first = L["base"], L["late"], L["glist"], L["first"]
    # late_list: G genes, the late genes first at or above 2^20 + 64, every other base gene in the first cycle, all in the tail
    assert glist.size == scale.G and set(glist.tolist()) == set(base) and len(base) > 30
    assert all(first[g] >= scale.MAX_ITEMS + 64 for g in late) and all(0 <= first[g] < len(base) for g in base if g not in late)
    assert not np.isin(glist[:scale.MAX_ITEMS + 64], late).any() and set(glist[scale.MAX_ITEMS + 64:].tolist()) == set(base)
    assert all(glist[first[g]] == g for g in base) and all(first[g] == -1 for g in range(len(case.genes)) if g not in base)
    # one item a gene at the default slices (items == G, two launches), more at slices of 64
    assert (total[glist] > 0).all() and int((-(-total[glist] // 64)).sum()) > scale.G > scale.MAX_ITEMS
    for covered in L["words"]:
        best = {f: _family_best_gene(cands, covered, f) for f in range(len(case.sizes))}
        behind = [f for f, g in best.items() if g is not None and g in late]
        front = [f for f, g in best.items() if g is not None and g not in late]
        assert len(behind) >= 2 and len(front) >= 2 and set(case.family(n) for n in LATE_FAMILIES) <= set(behind)
        # (the second launch holds items of the `front` families too: the tail tiles every base gene)
        want = _expected_step(case, cands, covered, first, None)
        assert all(want[f]["gene"] >= scale.MAX_ITEMS for f in behind) and all(want[f]["gene"] < len(base) for f in front)
    assert L["words"][1] != L["words"][0] and sum(1 for w in L["words"][1] if w) >= 10
    # the relabelling against brute force: a short list, every copy of every candidate with its own position as its gene
    S = _late_case(case, cands, total, n_genes=3 * len(base) + 7, head=len(base) + 5)
    copies = [c[:5] + (p,) + c[6:] for p, g in enumerate(S["glist"].tolist()) for c in cands if c[5] == g]
    for covered in S["words"]:
        want = _expected_step(case, cands, covered, S["first"], None)
        for f in range(len(case.sizes)):
            mine = [c for c in copies if c[0] == f]
            b = _best_with_copies(mine, covered[f])
            assert (None if b is None else (b[5], b[6], b[7])) == (None if want[f]["gain"] == 0 else (want[f]["gene"], want[f]["key"], want[f]["cover"]))


def _best_with_copies(cands, covered):
    """best_loop's order over candidates among which copies of one table row occur (equal in everything but the gene): a
    plain minimum over the order's terms."""
    live = [c for c in cands if bin(c[7] & ~covered).count("1")]
    if not live:
        return None
    return min(live, key=lambda c: (-bin(c[7] & ~covered).count("1"), -c[6], c[1], c[2], c[3] << 1 | c[4], c[5]))


def test_host_helpers():
    from cropsr_amd import family_sets as fs
    assert fs.full_words([1, 3, 63, 64]).tolist() == [1, 7, (1 << 63) - 1, (1 << 64) - 1]
    rec = lambda gain, key: np.array([(key, 1, gain, 0, 0, 0)], dtype=nat.FAMILY_STEP_BEST_DTYPE)
    for a, b, want in (((2, 5), (2, 5), 0), ((1, 9), (2, 1), 1), ((2, 5), (2, 6), 1), ((0, 0), (0, 7), 0), ((0, 0), (1, 0), 1)):
        arena, best = fs.merge_arenas([rec(*a), rec(*b)])
        assert arena.tolist() == [want] and best["gain"][0] == max(a[0], b[0])


def test_library_declares_family_set_abi():
    with open(os.path.join(ROOT, "include", "cropsr_hip.h")) as f:
        header = f.read()
    L = nat.lib()
    for name in ("crp_select_set_family_members", "crp_select_family_step", "crp_select_family_step_stats"):
        assert re.search(r"\bint %s\(" % name, header) and hasattr(L, name)
    assert "#define CRP_FAMILY_SET_MAX_STEPS 64" in header and nat.FAMILY_SET_MAX_STEPS == 64
    assert re.search(r"typedef struct crp_family_step_best \{\s*uint64_t key, cover;\s*uint32_t gain, tie, row, gene;\s*\} crp_family_step_best;", header)
    assert np.dtype(nat.FAMILY_STEP_BEST_DTYPE).itemsize == 32
    assert int(re.search(r"#define CRP_ABI_VERSION (\d+)", header).group(1)) == 6  # additions only


def test_request_refusals(case):
    from cropsr_amd import baseedit, coding
    from cropsr_amd import select as sel
    ann, table = case.table()
    try:
        areq = annotate.Request(ann, case.names, 0)
        p = sel.Params(5)
        assert sel.Request(p, areq, families=table, family_sets=4).family_sets == 4
        assert sel.Request(p, areq, families=table).family_sets is None
        for kw, word in ((dict(family_sets=4), "family table"), (dict(families=table, family_sets=0), "1..64"),
                         (dict(families=table, family_sets=65), "1..64"), (dict(families=table, family_sets="4"), "1..64"),
                         (dict(families=table, family_sets=4, coding_limits=coding.Limits(0, 50)), "one or the other"),
                         (dict(families=table, family_sets=4, edit_limits=baseedit.Limits(0, 50, 3)), "one or the other"),
                         (dict(families=table, family_sets=4, splice_limits=baseedit.SpliceLimits(0, 50, 3, "any")), "one or the other"),
                         (dict(families=table, family_sets=4, pairs=sel.PairParams(3)), "one or the other")):
            with pytest.raises(ValueError) as e:
                sel.Request(p, areq, **kw)
            assert word in str(e.value), kw
    finally:
        ann.close()


def test_cli_refuses_before_any_side_effect(case, tmp_path):
    import subprocess
    import sys
    fa = tmp_path / "g.fa"
    fa.write_text(">c1\nACGT\n")
    gff = tmp_path / "g.gff"
    gff.write_text(case.gff)
    ok = tmp_path / "ok.tsv"
    ok.write_text(case.families)
    out = tmp_path / "o.csv"
    base = ["-f", str(fa), "-g", str(gff), "-o", str(out)]
    full = base + ["--select", "5", "--specificity", "--families", str(ok)]
    cases_ = [(base + ["--select", "5", "--specificity", "--family-sets", "4"], "belongs to --families"),
              (base + ["--specificity", "--family-sets", "4"], "belongs to --select"),
              (base + ["--select", "5", "--families", str(ok), "--family-sets", "4"], "--specificity"),
              (full + ["--family-sets-output", str(tmp_path / "s.csv")], "belongs to --family-sets"),
              (full + ["--family-sets", "0"], "1..64"), (full + ["--family-sets", "65"], "1..64"), (full + ["--family-sets", "x"], "1..64"),
              (full + ["--family-sets", "4", "--select-coding-min", "5"], "one or the other"),
              (full + ["--family-sets", "4", "--select-stop"], "one or the other"),
              (full + ["--family-sets", "4", "--select-splice", "donor"], "one or the other"),
              (full + ["--family-sets", "4", "--select-pairs", "3"], "--select-pairs")]
    for args, word in cases_:
        r = subprocess.run([sys.executable, "-m", "cropsr_amd"] + args, cwd=ROOT, capture_output=True, text=True,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode != 0 and "cropsr_amd:" in r.stderr and word in r.stderr, (args, r.stderr)
        assert not out.exists() and not (tmp_path / "o.csv.selected.csv").exists() and not (tmp_path / "o.csv.family_sets.csv").exists()
        assert not (tmp_path / "s.csv").exists()


# ------------------------------------------------------------------ the command line over the oracle backend (CPU)
def _expected_file(case, picks, complete, main_rows, outside):
    """The family-sets file of the reference's picks: the main table's fields come from the main CSV's own line of the row
    (found by chromosome, cut site and strand), the outside values from outside(pick)."""
    from cropsr_amd import cli, rows
    at = {name: main_rows[0].index(name) for name in ("chromosome", "cutsite", "strand")}
    by_place = {(line[at["chromosome"]], line[at["cutsite"]], line[at["strand"]]): line[1:] for line in main_rows[1:]}
    out = [cli.FAMILY_SET_HEADER + main_rows[0][1:] + cli.FAMILY_SET_TAIL]
    before = {}
    for p in picks:
        f = p["family"]
        new = p["covered"] & ~before.get(f, 0)
        before[f] = p["covered"]
        members = [i for i, (ff, m) in zip(case.idents, zip(case.gene_family, case.gene_member)) if ff == f and new >> m & 1]
        assert len(members) == p["gain"]
        # (the main table's cutsite is the reference's: i - 3 on '+', j on '-')
        place = (case.names[p["contig"]], str(p["cut"]), "-" if p["strand"] else "+")
        mm0, hs = outside(p)
        out.append([case.fam_names[f], str(case.sizes[f]), str(p["step"]), str(p["gain"]), str(bin(p["covered"]).count("1")),
                    str(int(complete[f])), ";".join("gene:" + m for m in members), "gene:" + case.idents[p["gene"]]] + by_place[place]
                   + [str(mm0), "%.6f" % (hs / float(1 << 30)), "%.6f" % srch.specificity(np.uint64(hs))])
    assert rows.HEADER[1:] == main_rows[0][1:len(rows.HEADER)]
    return out


class SetsOracleBackend(FamilyOracleBackend):
    """FamilyOracleBackend plus select.family_sets: the reference's greedy sets over the same tables, as a Selection carries them."""

    def scan(self, strings, l, offtarget=False, annotation=None, specificity=None, select=None):
        from cropsr_amd import select as sel
        out = FamilyOracleBackend.scan(self, strings, l, offtarget=offtarget, annotation=annotation, specificity=specificity, select=select)
        if select is None or select.family_sets is None:
            return out
        case = self.case
        self.columns = [{k: v for k, v in h.items() if k.startswith("self_")} for h in out]
        lim = select.family_limits
        limits = (None, None, None) if lim is None else (None, None if lim.max_mm0_outside == sel.NO_BOUND_MM0 else lim.max_mm0_outside, None)
        fam_ref = self.selected[-1][1]
        cands, _ = case.candidates(("backend", limits), list(out), self.columns, fam_ref,
                                   ONE_ARENA, limits)
        picks, complete = sref_sets.greedy_loop(cands, case.sizes, select.family_sets)
        self.sets = (picks, complete, cands)
        arr = np.empty(len(picks), sel.FAMILY_SET_DTYPE)
        for at, p in enumerate(picks):
            score = out[p["contig"]]["score_minus" if p["strand"] else "score_plus"][p["index"]]
            arr[at] = (p["family"], p["step"], p["gene"], p["contig"], p["position"], b"+-"[p["strand"]:p["strand"] + 1], score, p["index"], p["gain"],
                       p["cover"], p["covered"])
        values = [self.outside(p) for p in picks]
        s = out.selection
        s.family_sets, s.family_complete = arr, np.array(complete, bool)
        s.family_sets_stats = dict(outside_mm0=np.array([v[0] for v in values], np.uint32), outside_hit_sum=np.array([v[1] for v in values], np.uint64))
        return out

    def outside(self, p):
        """(outside_mm0, outside_hit_sum) of a pick for its gene, by family_reference.selection_values over the columns."""
        case, fam_ref = self.case, self.selected[-1][1]
        r = {s: i for i, s in enumerate(fam_ref["sites"])}[(p["contig"], p["position"] if p["strand"] else p["position"] - 20, p["strand"])]
        cols = self.columns[p["contig"]]
        name = "minus" if p["strand"] else "plus"
        v = fref.selection_values(p["gene"], case.gene_family, case.sizes, int(fam_ref["site_family"][r]), int(cols["self_counts_" + name][p["index"], 0]),
                                  int(cols["self_sum_" + name][p["index"]]), int(fam_ref["fam_counts"][r][0]), fam_ref["fam_sum"][r], fam_ref["fam_cover"][r])
        return v[0], v[1]


def test_cli_family_sets_over_the_oracle(case, oracle, tmp_path, monkeypatch, capsys):
    import csv
    fam_file = tmp_path / "families.tsv"
    fam_file.write_text(case.families)
    backend = SetsOracleBackend(oracle, case)
    read = lambda path: list(csv.reader(open(path, newline="")))
    common = ["--specificity", "--select", "5", "--families", str(fam_file)]
    # without --family-sets every byte is what the family backend's run gives: the main CSV and the selection file, by md5
    old = _run_cli(case, tmp_path, monkeypatch, common, FamilyOracleBackend(oracle, case), "old.csv")
    assert not os.path.exists(old + ".family_sets.csv")
    capsys.readouterr()
    new = _run_cli(case, tmp_path, monkeypatch, common + ["--family-sets", "4"], backend, "new.csv")
    err = capsys.readouterr().err
    assert _md5(old) == _md5(new) and _md5(old + ".selected.csv") == _md5(new + ".selected.csv")
    picks, complete, _ = backend.sets
    sets = _by_family(picks)
    n_done = sum(1 for f in sets if complete[f])
    assert "--family-sets 4: 14 families, %d complete, %d incomplete, 1 without a passing guide" % (n_done, len(sets) - n_done) in err
    assert n_done >= 8 and len(sets) - n_done >= 3  # (stuck, trips and -- at S = 4 -- tiny stay incomplete)
    got = read(new + ".family_sets.csv")
    assert got == _expected_file(case, picks, complete, read(new), backend.outside) and len(got) == len(picks) + 1 == 24
    assert [line[0] for line in got[1:]] == [case.fam_names[p["family"]] for p in picks] and "none" not in {line[0] for line in got[1:]}
    # the limits reach the sets, and the file goes where --family-sets-output says
    where = tmp_path / "elsewhere.csv"
    strict = _run_cli(case, tmp_path, monkeypatch, common + ["--family-sets", "64", "--select-max-perfect-outside", "0", "--family-sets-output", str(where)],
                      backend, "strict.csv")
    picks, complete, _ = backend.sets
    assert not os.path.exists(strict + ".family_sets.csv")
    got = read(str(where))
    assert got == _expected_file(case, picks, complete, read(strict), backend.outside) and all(line[-3] == "0" for line in got[1:])
    assert sum(1 for line in got[1:] if line[0] == "tiny") == 64


# ------------------------------------------------------------------ tools/family_sets_bench.py: its host check, without a GPU
def test_bench_host_check_equals_reference(case, cpu):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import family_sets_bench as fsb
    texts = [fsb.fb.CODE[np.frombuffer(c, np.uint8)] for c in case.contigs]
    genes = [(kc, lo, hi) for _, kc, lo, hi in case.genes]
    ann, table = case.table()
    ann.close()
    tables = [dict(t, **c) for t, c in zip(cpu["tables"], cpu["columns"])]
    for S in (4, 64):
        sets = _by_family(sref_sets.greedy_loop(cpu["free"][0], case.sizes, S)[0])
        done = sref_sets.greedy_loop(cpu["free"][0], case.sizes, S)[1]
        for f in range(len(case.fam_names)):
            cands, where = fsb.family_candidates(f, table, genes, tables, cpu["columns"], texts, genes, case.gene_family, case.gene_member, 3)
            picks, complete = fsb.host_family_set(cands, case.sizes[f], S)
            have = [(step,) + where[i] + (gain, cands[i][4], covered) for step, i, gain, covered in picks]
            want = [(p["step"], p["gene"], p["contig"], p["position"], p["strand"], p["gain"], p["cover"], p["covered"]) for p in sets.get(f, [])]
            assert have == want and complete == done[f], (S, f)


# ------------------------------------------------------------------ the device
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


class Device:
    """The device's tables and plain joined columns of the case genome per (M, scheme), fetched once: what the reference's
    candidates are computed over (tests/test_specificity_join.py holds the columns)."""

    def __init__(self, engine, case):
        self.engine, self.case, self._plain = engine, case, {}

    def plain(self, M, value):
        if (M, value) not in self._plain:
            g = self.engine.genome(self.case.contigs)
            try:
                plain = g.scan_score(20, specificity=dict(max_mm=M, score=VALUES[value][0]))
                self._plain[(M, value)] = ([plain.contig(k) for k in range(len(self.case.contigs))], plain.columns)
            finally:
                g.close()
        return self._plain[(M, value)]

    def candidates(self, M, value, C, arenas, strict):
        tables, columns = self.plain(M, value)
        return self.case.candidates(("gpu", M, value, C, len(arenas), strict), tables, columns, self.case.rows(M, value, C), arenas,
                                    (None, 0, None) if strict else (None, None, None))


@pytest.fixture(scope="module")
def device(engine, case):
    return Device(engine, case)


def _assert_sets_equal(case, got, want_picks, want_complete):
    assert got.family_sets.dtype == __import__("cropsr_amd.select", fromlist=["x"]).FAMILY_SET_DTYPE
    have = [(int(p["family"]), int(p["step"]), int(p["gene"]), int(p["contig"]), int(p["position"]), p["strand"], int(p["index"]), int(p["gain"]),
             int(p["cover"]), int(p["covered"]), int(np.float64(p["score"]).view(np.uint64))) for p in got.family_sets]
    want = [(p["family"], p["step"], p["gene"], p["contig"], p["position"], b"+-"[p["strand"]:p["strand"] + 1], p["index"], p["gain"], p["cover"],
             p["covered"], p["key"]) for p in want_picks]
    assert have == want
    assert got.family_complete.tolist() == list(want_complete)


CONFIGS = [(0, "plain", 0), (0, "hsu2013", 0), (3, "plain", 0), (3, "plain", 3), (3, "hsu2013", 0), (3, "hsu2013", 3)]
# (S, slice_rows, max_words, family limits): every S, both slicings, one arena and three, with and without limits, each twice
RUNS = [(64, None, None, False), (2, 64, cases.MAX_WORDS, True), (1, 64, None, False), (63, None, cases.MAX_WORDS, True),
        (64, 64, cases.MAX_WORDS, False), (1, None, None, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,value,C", CONFIGS, ids=["M%d-%s-C%d" % c for c in CONFIGS])
def test_gpu_family_sets_match_reference(engine, case, device, M, value, C):
    from cropsr_amd import select as sel
    ann, table = case.table()
    try:
        areq = annotate.Request(ann, case.names, 0)
        for S, slice_rows, max_words, strict in RUNS:
            g = engine.genome(case.contigs, max_words=max_words)
            try:
                arenas = cases.ARENAS_OF_THREE if max_words else ONE_ARENA
                assert g.groups == arenas
                cands, n_pass = device.candidates(M, value, C, arenas, strict)
                want_picks, want_complete = sref_sets.greedy_loop(cands, case.sizes, S)
                limits = dict(max_perfect_outside=0) if strict else {}
                req = sel.Request(sel.Params(5), areq, slice_rows, families=table, family_cover_mm=C, family_sets=S, **limits)
                got = g.scan_score(20, specificity=dict(max_mm=M, score=VALUES[value][0]), select=req).selection
                assert got.n_pass.tolist() == n_pass  # the candidates are the rows behind n_pass
                _assert_sets_equal(case, got, want_picks, want_complete)
                st = got.family_sets_stats
                assert st["plan_builds"] == len(arenas) and 1 <= st["steps"] <= S and st["step_ms"] > 0.0 and st["pick_ms"] > 0.0
                assert st["steps"] == min(S, max(p["step"] for p in want_picks) + 1)  # (one more step finds nothing, unless S ends it)
                n_rows = np.array([g_[3] - g_[2] for g_ in case.genes])  # (items: at least one per family gene with rows)
                assert st["items"] >= sum(1 for gi, n in enumerate(n_pass) if n and case.gene_family[gi] != NONE) and n_rows.size
                if slice_rows == 64:
                    assert st["items"] > sum(1 for gi, n in enumerate(n_pass) if n and case.gene_family[gi] != NONE)
            finally:
                g.close()
    finally:
        ann.close()


def _with_joined_handles(engine, case, max_words, body, M=3, value="hsu2013", C=0):
    """Runs body(genome, hits, handles, areq, table) while every arena's self-search handle is open with both joins."""
    ann, table = case.table()
    g = engine.genome(case.contigs, max_words=max_words)
    done = []
    try:
        areq = annotate.Request(ann, case.names, 0)
        hits = g._scan_score(20, False, False, True, None)
        handles = {}

        def after_join(a, handle, cols, family_joined=None):
            handles[a] = handle
            if len(handles) == len(g.arenas):
                body(g, hits, handles, areq, table)
                done.append(True)

        srch.specificity_columns(g, 20, max_mm=M, score=VALUES[value][0], after_join=after_join, families=fam.genome_rows(table, g, areq),
                                 family_cover_mm=C)
        assert done
    finally:
        g.close()
        ann.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_words", [None, cases.MAX_WORDS], ids=["one-arena", "three-arenas"])
def test_gpu_step_by_step(engine, case, device, max_words):
    """crp_select_family_step's proposals, arena by arena, against the reference's best of that arena for a given covered:
    nothing covered, what the greedy has covered after one and after two steps, the high bits only, and all ones."""
    from cropsr_amd import select as sel
    arenas = cases.ARENAS_OF_THREE if max_words else ONE_ARENA
    cands, _ = device.candidates(3, "hsu2013", 0, arenas, False)
    F = len(case.sizes)
    words = [[0] * F, [0xFFFFFFFF00000000] * F, [(1 << 64) - 1] * F, [0x5555555555555555] * F]
    for S in (1, 2):
        after = {f: ps[-1]["covered"] for f, ps in _by_family(sref_sets.greedy_loop(cands, case.sizes, S)[0]).items()}
        words.append([after.get(f, 0) for f in range(F)])

    def body(g, hits, handles, areq, table):
        assert g.groups == arenas
        for slice_rows in (None, 64):
            for a in range(len(g.arenas)):
                lo, hi, gene = areq.gene_layout(sel.arena_layout(g, a))
                s = sel.ArenaSelect(g.arenas[a], lo, hi)
                try:
                    if slice_rows:
                        s.set_limits(slice_rows)
                    gi = np.asarray(gene, dtype=np.int64)
                    s.set_family(table.gene_family[gi], np.array([table.family_size(int(x)) for x in gi], np.uint32))
                    s.set_family_members(table.gene_member[gi])
                    for n, covered in enumerate(words):
                        best = s.family_step(sel.Params(1), handles[a], np.array(covered, np.uint64))
                        want = sref_sets.arena_best(cands, case.sizes, covered, a)
                        for f in range(F):
                            if want[f] is None:
                                assert best["gain"][f] == 0, (a, n, f)
                                continue
                            w = want[f]
                            assert (int(best["gain"][f]), int(best["key"][f]), int(best["cover"][f]), int(gi[best["gene"][f]])) == \
                                (w["gain"], w["key"], w["cover"], w["gene"]), (a, n, f)
                            assert int(best["row"][f]) >> 31 == w["strand"] and int(best["tie"][f]) & 1 == w["strand"]
                        st = s.family_step_stats()
                        assert st["plan_builds"] == 1 and st["step_ms"] > 0 and st["bytes_per_row"] == 48.0  # built once over all steps
                    assert not best["gain"][case.family("tiny")] or covered[case.family("tiny")] != (1 << 64) - 1
                    # another parameter set, other slices: a new plan each; the same again: none
                    s.family_step(sel.Params(1, min_score=0.5), handles[a], np.zeros(F, np.uint64))
                    assert s.family_step_stats()["plan_builds"] == 2
                    s.set_limits(128)
                    s.family_step(sel.Params(1, min_score=0.5), handles[a], np.zeros(F, np.uint64))
                    s.family_step(sel.Params(1, min_score=0.5), handles[a], np.zeros(F, np.uint64))
                    assert s.family_step_stats()["plan_builds"] == 3
                finally:
                    s.close()

    _with_joined_handles(engine, case, max_words, body)


@pytest.mark.gpu
def test_gpu_step_past_one_launch(engine, case, device):
    """crp_select_family_step over more than 2^20 items: its loop hands the second launch `d_set_items + first` and
    `d_set_prop + first`, and the pick kernel reads the proposals by absolute slot.  The handle's genes are _late_case's list:
    for LATE_FAMILIES the best candidate's gene occurs first behind item 2^20, so the second launch writes the winning
    proposal; for the other families the winner lies in the first launch while the second holds items of theirs too.  Every
    field of every family's record against _expected_step, with nothing covered and with the greedy's first pick covered, at
    the default slices (one item a gene) and at slices of 64."""
    from cropsr_amd import select as sel
    cands, _ = device.candidates(3, "hsu2013", 0, ONE_ARENA, False)
    tables, _ = device.plain(3, "hsu2013")
    total = _run_lengths(case, tables)
    L = _late_case(case, cands, total)
    glist, F = L["glist"], len(case.sizes)
    before = [np.cumsum([0] + [len(t["pos_" + name]) for t in tables]) for name in ("plus", "minus")]

    def body(g, hits, handles, areq, table):
        assert g.groups == ONE_ARENA
        offsets = [int(o) for o in g.arenas[0].offsets]  # (one arena: the contigs in genome order)
        place = lambda contig, cut, strand, index: ((offsets[contig] + cut) << 1 | strand, strand << 31 | (int(before[strand][contig]) + index))
        lo, hi, gene = areq.gene_layout(sel.arena_layout(g, 0))
        gi = np.asarray(gene, dtype=np.int64)
        assert sorted(gi.tolist()) == list(range(len(case.genes)))  # whole contigs in one arena: one layout row a gene
        row_of_gene = np.empty(gi.size, np.int64)
        row_of_gene[gi] = np.arange(gi.size)
        lay = row_of_gene[glist]
        size = np.array([table.family_size(x) for x in range(len(case.genes))], np.uint32)
        for slice_rows in (None, 64):
            items = int(np.maximum(1, -(-total[glist] // (slice_rows or 65536))).sum())
            s = sel.ArenaSelect(g.arenas[0], lo[lay], hi[lay])
            try:
                if slice_rows:
                    s.set_limits(slice_rows)
                s.set_family(np.asarray(table.gene_family)[glist], size[glist])
                s.set_family_members(np.asarray(table.gene_member)[glist])
                for n, covered in enumerate(L["words"]):
                    best = s.family_step(sel.Params(1), handles[0], np.array(covered, np.uint64))
                    want = _expected_step(case, cands, covered, L["first"], place)
                    for f in range(F):
                        for field in ("gain", "key", "cover", "gene", "tie", "row"):
                            assert int(best[field][f]) == want[f][field], (slice_rows, n, case.fam_names[f], field)
                    assert sum(1 for w in want if w["gain"] and w["gene"] >= scale.MAX_ITEMS) >= 2
                    assert sum(1 for w in want if w["gain"] and w["gene"] < scale.MAX_ITEMS) >= 2
                    st = s.family_step_stats()
                    assert st["items"] == items and st["plan_builds"] == 1
                assert items == scale.G if slice_rows is None else items > scale.G
            finally:
                s.close()

    _with_joined_handles(engine, case, None, body)


@pytest.mark.gpu
def test_gpu_calls_out_of_order_and_error_codes(engine, case):
    from cropsr_amd import baseedit, coding
    from cropsr_amd import select as sel
    L = nat.lib()

    def body(g, hits, handles, areq, table):
        ctx = g.arenas[0]._engine._ctx
        lo, hi, gene = areq.gene_layout(sel.arena_layout(g, 0))
        gi = np.asarray(gene, dtype=np.int64)
        F = len(table.names)
        s = sel.ArenaSelect(g.arenas[0], lo, hi)
        bare = srch.ArenaSelfSearch(g.arenas[0], PATTERN, GUIDE_PATTERN, 3, 3)
        try:
            bare.join_hits(20, fetch=False)
            covered, best = np.zeros(F, np.uint64), np.zeros(F, nat.FAMILY_STEP_BEST_DTYPE)
            u32, u64 = (lambda a: a.ctypes.data_as(nat.u32p)), (lambda a: a.ctypes.data_as(nat.u64p))
            params = sel.Params(1).native()
            step = lambda p=params, h=handles[0], n=F: L.crp_select_family_step(s._h, ctypes.byref(p), h._h if h is not None else None, u64(covered), n,
                                                                                 best.ctypes.data_as(ctypes.c_void_p))
            err = lambda: L.crp_last_error(ctx)
            members = np.ascontiguousarray(table.gene_member[gi])
            assert step() == nat.CRP_ERR_STATE and b"crp_select_set_family" in err()
            assert L.crp_select_set_family_members(s._h, u32(members), members.size) == nat.CRP_ERR_STATE and b"crp_select_set_family" in err()
            s.set_family(table.gene_family[gi], np.array([table.family_size(int(x)) for x in gi], np.uint32))
            assert step() == nat.CRP_ERR_STATE and b"crp_select_set_family_members" in err()
            assert L.crp_select_set_family_members(s._h, u32(members), members.size - 1) == nat.CRP_ERR_INVALID
            assert L.crp_select_set_family_members(s._h, u32(np.full(members.size, 64, np.uint32)), members.size) == nat.CRP_ERR_INVALID and b"64" in err()
            assert L.crp_select_set_family_members(s._h, None, members.size) == nat.CRP_ERR_INVALID
            s.set_family_members(members)
            assert step(h=None) == nat.CRP_ERR_STATE and b"joined" in err()
            assert step(h=bare) == nat.CRP_ERR_STATE and b"family" in err()
            assert step(h=handles[1]) == nat.CRP_ERR_INVALID and b"another arena" in err()
            assert step(p=nat.SelectParams(float("nan"), sel.NO_BOUND_SUM, sel.NO_BOUND_MM0, 1, 0, 0)) == nat.CRP_ERR_INVALID and b"min_score" in err()
            assert step(n=1) == nat.CRP_ERR_INVALID and b"family" in err()  # a gene's family id is not below n_families
            model = areq.coding_layout(sel.arena_layout(g, 0))
            s.set_coding(model)
            for put, clear in ((lambda: s.set_coding_limits(coding.Limits(0, 50)), lambda: s.set_coding_limits(None)),
                               (lambda: s.set_edit_limits(None, baseedit.Limits(0, 50, 3)), lambda: s.set_edit_limits(None, None)),
                               (lambda: s.set_splice_limits(None, "cbe", baseedit.SpliceLimits(0, 50, 3, "any")), lambda: s.set_splice_limits(None, "cbe", None))):
                put()
                assert step() == nat.CRP_ERR_UNSUPPORTED and b"one kernel per predicate" in err()
                clear()
            assert L.crp_select_family_step(None, ctypes.byref(params), handles[0]._h, u64(covered), F, best.ctypes.data_as(ctypes.c_void_p)) == nat.CRP_ERR_INVALID
            assert L.crp_select_family_step(s._h, ctypes.byref(params), handles[0]._h, None, F, best.ctypes.data_as(ctypes.c_void_p)) == nat.CRP_ERR_INVALID
            assert L.crp_select_family_step_stats(s._h, None, 7) == nat.CRP_ERR_INVALID
            assert step() == nat.CRP_OK and best["gain"][case.family("one")] == 3
            # the families set again: the member bits are gone with them; cleared members likewise
            s.set_family(table.gene_family[gi], np.array([table.family_size(int(x)) for x in gi], np.uint32))
            assert step() == nat.CRP_ERR_STATE and b"crp_select_set_family_members" in err()
            s.set_family_members(members)
            assert step() == nat.CRP_OK
            s.set_family_members(None)
            assert step() == nat.CRP_ERR_STATE
            # a plain selection on the same handle is what it was
            s.run(sel.Params(5), handles[0])
            assert s.fetch()[1][0] > 0
        finally:
            bare.close()
            s.close()

    _with_joined_handles(engine, case, cases.MAX_WORDS, body)


@pytest.mark.gpu
def test_gpu_cli_end_to_end(engine, case, device, tmp_path):
    import csv
    import subprocess
    import sys
    fa = tmp_path / "case.fa"
    fa.write_bytes(b"\n".join(b">" + n.encode() + b"\n" + c for n, c in zip(case.names, case.contigs)))  # (one line a contig: dec = 0)
    fam_file = tmp_path / "families.tsv"
    fam_file.write_text(case.families)
    out = tmp_path / "guides.csv"
    cmd = [sys.executable, "-m", "cropsr_amd", "-f", str(fa), "-g", case.gff_path, "-o", str(out), "--cas9", "--specificity", "--select", "5",
           "--families", str(fam_file), "--seed", "7", "--each-contig-once"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))  # (run beside the files it writes)
    r = subprocess.run(cmd + ["--family-sets", "64"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    cands, _ = device.candidates(3, "hsu2013", 0, ONE_ARENA, False)
    picks, complete = sref_sets.greedy_loop(cands, case.sizes, 64)
    n_done = int(sum(complete))
    assert "--family-sets 64: 14 families, %d complete, %d incomplete, 1 without a passing guide" % (n_done, 13 - n_done) in r.stderr
    read = lambda path: list(csv.reader(open(path, newline="")))
    got, main_rows = read(str(out) + ".family_sets.csv"), read(str(out))
    tables, columns = device.plain(3, "hsu2013")
    fam_ref = case.rows(3, "hsu2013", 0)
    row_of = {s: i for i, s in enumerate(fam_ref["sites"])}

    def outside(p):
        rr = row_of[(p["contig"], p["position"] if p["strand"] else p["position"] - 20, p["strand"])]
        name = "minus" if p["strand"] else "plus"
        v = fref.selection_values(p["gene"], case.gene_family, case.sizes, int(fam_ref["site_family"][rr]),
                                  int(columns[p["contig"]]["self_counts_" + name][p["index"], 0]), int(columns[p["contig"]]["self_sum_" + name][p["index"]]),
                                  int(fam_ref["fam_counts"][rr][0]), fam_ref["fam_sum"][rr], fam_ref["fam_cover"][rr])
        return v[0], v[1]

    assert got == _expected_file(case, picks, complete, main_rows, outside) and len(got) > 80
    # without --family-sets every byte of the other two files is what it was, and there is no third
    import hashlib
    md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest()
    with_sets = md5(str(out)), md5(str(out) + ".selected.csv")
    os.remove(str(out) + ".family_sets.csv")
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (md5(str(out)), md5(str(out) + ".selected.csv")) == with_sets and not os.path.exists(str(out) + ".family_sets.csv")
