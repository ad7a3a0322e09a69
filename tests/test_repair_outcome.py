"""--repair-scores: the microhomology and out-of-frame score of every hit's cut (cropsr_amd/repair.py, csrc/crp_repair.hip)
and the selection's two repair limits.  The definition is restated twice in tests/repair_reference.py; the genome comes
from tests/repair_cases.py, the genes of the selection tests from tests/select_cases.py.

A planted segment's PAM lies inside its own window from a flank of 5 on (GG at p = F + 4, F + 5 of a '+' row), so the
hand values of pure windows (A x 60, a window without a base) are checked on the definitions without a GPU, and on the
GPU the planted rows are compared with the reference like every other row."""
import csv
import ctypes
import io
import json
import math
import os

import numpy as np
import pytest

from conftest import OracleBackend

import guide_properties_cases as pcases
import guide_properties_reference as pref
import repair_cases as cases
import repair_reference as ref
import select_cases
import select_reference as sref
from cropsr_amd import _native as nat
from cropsr_amd import annotate, cli, repair, rows
from cropsr_amd import search as srch
from cropsr_amd import select as sel

NONE = 0xFFFFFFFF
EVERYTHING = (0, 0)
NOTHING = (1 << 20, 0)  # mh stays below 2^20
ALL_FLANKS = (2, 3, 5, 16, 30, 31, 32)


def _pair(v):
    return int(v) & 0xFFFFFFFF, int(v) >> 32


# ---------------------------------------------------------------------------------------------- without a GPU
def _test_windows(F, rng):
    out = []
    for alphabet in ("ACGT", "ACGTN", "AC", "GT", "G", "A"):
        for _ in range(6 if F > 16 else 12):
            out.append("".join(rng.choice(list(alphabet), 2 * F)))
    for unit_len in (1, 2, 3, 4):
        for _ in range(3):
            unit = "".join(rng.choice(list("ACGT"), unit_len))
            out.append((unit * (2 * F))[:2 * F])
    return out


@pytest.mark.parametrize("F", ALL_FLANKS)
def test_enumeration_equals_the_diagonal_form(F):
    rng = np.random.default_rng(100 + F)
    windows = _test_windows(F, rng)
    # the numpy statement sees the same windows as rows of one text: window k is a '+' row with cut at its middle
    text = ("N" * 70).join(windows)
    pos = np.array([k * (2 * F + 70) + F + 3 for k in range(len(windows))])
    col = ref.column_numpy(text.encode(), pos, False, F)
    for k, t in enumerate(windows):
        w = ref.as_window(t)
        want = ref.score_enumerate(w, F)
        assert ref.score_diagonals(w, F) == want, (F, t)
        assert _pair(col[k]) == want, (F, t)
        assert ref.window(text, int(pos[k]), False, F) == w and ref.window(text, int(pos[k]) - 9, True, F) == w
        assert want[1] <= want[0] < 1 << 20


def test_known_values():
    assert ref.score_enumerate(ref.as_window("G" * 64), 32) == ref.score_diagonals(ref.as_window("G" * 64), 32) == (507528, 338390)
    assert ref.score_enumerate(ref.as_window("A" * 60), 30) == ref.score_diagonals(ref.as_window("A" * 60), 30) == (240389, 160100)
    for F, left, d, letters in ((30, 28, 3, "AC"), (30, 10, 25, "GC"), (32, 0, 32, "AT"), (32, 30, 32, "TA"), (16, 14, 2, "CG"), (2, 0, 2, "GA"),
                                (30, 0, 58, "AC"), (32, 30, 2, "GG")):
        w = ["N"] * (2 * F)
        w[left:left + 2] = letters
        w[left + d:left + d + 2] = letters
        gc = sum(ch in "CG" for ch in letters)
        v = ref.W[d] * (2 + gc)
        got = ref.score_enumerate(ref.as_window("".join(w)), F)
        assert got == ref.score_diagonals(ref.as_window("".join(w)), F) == (v, v if d % 3 else 0), (F, left, d)
    for unit in ("ACT", "GAT", "CGT"):  # a pure repeat of three distinct letters: every microhomology is a multiple of 3 long
        for F in (16, 30, 32):
            mh, oof = ref.score_diagonals(ref.as_window((unit * 30)[:2 * F]), F)
            assert oof == 0 and mh > 0
    # a run that would go on across the cut ends at p = F - 1; one that starts in front of max(0, F - d) starts there
    F = 30
    w = ["N"] * 60
    w[21:34] = "ACTACTACTACTA"  # m_3 holds for p = 21 .. 30, but the range of d = 3 is [27, 30): ACT; d = 6: p = 24 .. 27, d = 9: p = 21 .. 24
    got = ref.score_diagonals(ref.as_window("".join(w)), F)
    assert got == ref.score_enumerate(ref.as_window("".join(w)), F) == (4 * ref.W[3] + 5 * ref.W[6] + 5 * ref.W[9], 0)
    w = ["N"] * 60
    w[19:23], w[29:33] = "TTCA", "TTCA"  # d = 10: p = 19 pairs with p + d = 29 < F, outside the range
    assert ref.score_diagonals(ref.as_window("".join(w)), F) == ref.score_enumerate(ref.as_window("".join(w)), F) == (ref.W[10] * 4,) * 2
    # a non-base splits a run; a piece of length 1 adds nothing
    w = ["N"] * 60
    w[22:29], w[36:43] = "ACGRACG", "ACGAACG"
    assert ref.score_diagonals(ref.as_window("".join(w)), F)[0] >= 2 * 5 * ref.W[14]
    w = ["N"] * 60
    w[22:26], w[36:40] = "ACRG", "ACAG"
    assert ref.score_diagonals(ref.as_window("".join(w)), F) == ref.score_enumerate(ref.as_window("".join(w)), F) == (3 * ref.W[14],) * 2
    # case is ignored, U is A, lower-case u and IUPAC letters are no bases; void positions are non-bases
    assert ref.as_window("acgtUuNRZ") == ["A", "C", "G", "T", "A", None, None, None, None]
    assert ref.window(b"ACGTACGT", 5, False, 3) == [None, "A", "C", "G", "T", "A"] and ref.window(b"ACGTACGT", 0, True, 3) == ["T", "A", "C", "G", "T", None]
    assert ref.cut(10, False) == 7 and ref.cut(10, True) == 16
    assert repair.unpack(repair.pack([507528], [338390]))[0][0] == 507528 and repair.unpack(repair.pack([507528], [338390]))[1][0] == 338390
    mh, pct = repair.scores(np.array([507528 | 338390 << 32, 0], np.uint64))
    assert mh.tolist() == [50752.8, 0.0] and pct.tolist() == [(100 * 338390) / 507528, -1.0]
    assert repair.fields(240389 | 160100 << 32) == ("24038.9", (100 * 160100) / 240389) and repair.fields(0) == ("0.0", -1)
    assert repair.fields(7 | 7 << 32) == ("0.7", 100.0)


@pytest.mark.parametrize("F", ALL_FLANKS)
def test_reverse_complement_leaves_the_pair_unchanged(F):
    rng = np.random.default_rng(7 + F)
    comp = {"A": "T", "T": "A", "C": "G", "G": "C", "N": "N"}
    for t in _test_windows(F, rng)[::2]:
        rc = "".join(comp[ch] for ch in reversed(t))
        assert ref.score_diagonals(ref.as_window(t), F) == ref.score_diagonals(ref.as_window(rc), F), t


def test_weight_table_is_the_formula():
    assert len(repair.WEIGHTS) == 63 and list(repair.WEIGHTS) == ref.W[1:]
    for d in range(1, 64):
        assert repair.WEIGHTS[d - 1] == int(math.floor(1000.0 * math.exp(-d / 20.0) + 0.5))
    assert [repair.WEIGHTS[d - 1] for d in (1, 2, 3, 20, 63)] == [951, 905, 861, 368, 43]
    path = os.path.join(os.path.dirname(repair.__file__), "csrc", "microhomology_weights.def")
    body = [ln for ln in open(path) if not ln.startswith("//")]
    assert [int(v) for v in "".join(body).replace(",", " ").split()] == list(repair.WEIGHTS)


def test_thresholds_are_converted_exactly():
    assert [repair.parse_min_mh(t) for t in ("0", "12", "12.5", "0.1", "0.0", "50752.8", " 7 ")] == [0, 120, 125, 1, 0, 507528, 70]
    for bad in ("", ".", ".5", "12.", "12.55", "1e3", "-1", "+1", "12,5", "0x10", "١٢", "nan"):
        with pytest.raises(ValueError):
            repair.parse_min_mh(bad)
    col = repair.pack([0, 0, 100, 100, 100, 3, 3], [0, 0, 100, 50, 49, 1, 2])
    assert repair.Limits(0, 0).passes(col).all() and repair.Limits().astuple() == (0, 0)
    assert repair.Limits(None, 100).passes(col).tolist() == [False, False, True, False, False, False, False]  # mh = 0 fails under PCT > 0
    assert repair.Limits(None, 50).passes(col).tolist() == [False, False, True, True, False, False, True]    # 100 * 2 >= 50 * 3, 100 * 1 < 50 * 3
    assert repair.Limits(None, 1).passes(col).tolist() == [False, False, True, True, True, True, True]
    assert repair.Limits(100, None).passes(col).tolist() == [False, False, True, True, True, False, False]
    assert repair.Limits(101, 0).passes(col).sum() == 0
    assert np.array_equal(repair.Limits(3, 34).passes(col), ref.limits_pass(col, (3, 34)))
    for bad in (dict(min_oof=101), dict(min_oof=-1), dict(min_mh=-1), dict(min_mh=1 << 32)):
        with pytest.raises(ValueError):
            repair.Limits(**bad)
    for bad in (1, 33, 0, -2):
        with pytest.raises(ValueError):
            repair.check_flank(bad)
    assert repair.check_flank(2) == 2 and repair.check_flank(32) == 32
    req = sel.Request(sel.Params(5), None)
    assert not req.runs_repair and req.repair_limits is None and req.repair_flank is None
    req = sel.Request(sel.Params(5), None, min_oof=60)
    assert req.runs_repair and req.flank == 30 and req.repair_flank is None and req.repair_limits.astuple() == (0, 60)
    req = sel.Request(sel.Params(5), None, repair_flank=16, min_mh=125)
    assert req.flank == req.repair_flank == 16 and req.repair_limits.astuple() == (125, 0)
    with pytest.raises(ValueError):
        sel.Request(sel.Params(5), None, repair_flank=33)


def test_library_declares_the_abi():
    text = open(os.path.join(os.path.dirname(nat.__file__), "..", "include", "cropsr_hip.h")).read()
    assert "#define CRP_ABI_VERSION 6" in text
    for name in ("crp_repair_scores", "crp_repair_scores_stats", "crp_select_set_repair_limits"):
        assert hasattr(nat.lib(), name) and name in nat.SIGNATURES and name + "(" in text
    assert ctypes.sizeof(nat.SelectRepairLimits) == 8 and ctypes.sizeof(nat.SelectParams) == 32
    assert nat.lib().crp_repair_scores(None, 30, None, None) == nat.CRP_ERR_INVALID


# ---------------------------------------------------------------------------------------------- the case genome
@pytest.fixture(scope="module")
def genome():
    """The case genome, and per (guide length, flank) the kept positions and the reference's columns (numpy statement)."""
    texts = cases.contigs()
    pos_cache, cache = {}, {}

    def at(l, F):
        if l not in pos_cache:
            pos_cache[l] = [cases.kept(t, l) for t in texts]
        if (l, F) not in cache:
            cache[l, F] = [dict(pos_plus=p, pos_minus=m, repair_plus=ref.column_numpy(t, p, False, F), repair_minus=ref.column_numpy(t, m, True, F))
                           for t, (p, m) in zip(texts, pos_cache[l])]
        return cache[l, F]

    return dict(texts=texts, at=at)


def test_loop_equals_numpy_on_the_case_genome(genome):
    for F in (2, 16, 32):
        for t, per in zip(genome["texts"][:2], genome["at"](1, F)):
            for minus, s in ((False, "plus"), (True, "minus")):
                pos = per["pos_" + s]
                pick = np.unique(np.concatenate([np.arange(0, pos.size, 331 if F > 2 else 47), np.arange(min(4, pos.size)),
                                                 np.arange(max(0, pos.size - 8), pos.size)]))
                assert np.array_equal(ref.column_loop(t, pos[pick], minus, F), per["repair_" + s][pick]), (F, s)


def test_the_case_genome_contains_the_cases(genome):
    texts = genome["texts"]
    offsets, off = [], 64
    for t in texts:  # one arena: 64-aligned texts, one separator word between them
        offsets.append(off)
        off += ((len(t) + 63) // 64 + 1) * 64
    planted = cases.plant_positions()
    for F in cases.FLANKS:
        per20, per1 = genome["at"](20, F), genome["at"](1, F)
        starts = {s: set() for s in ("plus", "minus")}
        for t, o, h in zip(texts, offsets, per20):
            starts["plus"].update(((h["pos_plus"].astype(np.int64) + o - 3 - F) & 63).tolist())
            starts["minus"].update(((h["pos_minus"].astype(np.int64) + o + 6 - F) & 63).tolist())
        for s in starts:  # a window that starts at plane bit 0; the last start inside one word and the first that straddles two
            assert {0, 64 - 2 * F, (65 - 2 * F) & 63, 63} <= starts[s], (F, s)
        for t, h in zip(texts, per1):  # '-' rows at the end of EVERY contig: the contig end cuts the window by 1 .. F letters
            over = h["pos_minus"].astype(np.int64) + 6 + F - len(t)
            assert set(range(1, F + 1)) <= set(over.tolist())
        # the first rows: the smallest cut - F there is, 3 - F, reaches into the leading void word but never below arena position 0
        assert int(per1[0]["pos_plus"][0]) == 6 and int(per1[0]["pos_minus"][0]) == 2 and offsets[0] + 3 - 32 >= 0
        assert int(per20[0]["pos_plus"][0]) == 25
        h0 = per20[0]
        value = {}
        for name, (i, j) in planted.items():
            r, m = int(np.searchsorted(h0["pos_plus"], i)), int(np.searchsorted(h0["pos_minus"], j))
            assert h0["pos_plus"][r] == i and h0["pos_minus"][m] == j, (F, name)
            assert h0["repair_plus"][r] == h0["repair_minus"][m], (F, name)  # a window and its reverse complement
            value[name] = _pair(h0["repair_plus"][r])
        assert value["no_base"] == (0, 0)
        if F == 32:
            assert value["poly_g"] == (507528, 338390)
        if F in (2, 3):  # (the PAM is still outside the window)
            assert value["poly_a"] == ref.score_diagonals(ref.as_window("A" * (2 * F)), F)
        if F >= 16:
            for d in cases.TWOMER_D:
                assert value["twomer_d%d" % d] == (3 * ref.W[d], 3 * ref.W[d] if d % 3 else 0)
            assert value["unit3"][1] == 0 < value["unit3"][0] and value["across_cut"][1] == 0 < value["across_cut"][0]
            assert value["range_start"] == (4 * ref.W[10],) * 2 and value["piece_of_one"] == (3 * ref.W[14],) * 2
            assert value["unit2"][0] > 0 and value["unit4"][0] > 0 and value["split_run"][0] >= 10 * ref.W[14]
        # soft-masking: the rows of the copy's upper-case core equal the rows of the all-upper-case stretch
        pos = h0["pos_plus"].astype(np.int64)
        a = np.flatnonzero((pos >= cases.MASK_AT + 150) & (pos < cases.MASK_AT + 247))
        b = np.flatnonzero((pos >= cases.MASK_COPY + 150) & (pos < cases.MASK_COPY + 247))
        assert a.size == b.size >= 3 and np.array_equal(pos[a] - cases.MASK_AT, pos[b] - cases.MASK_COPY)
        assert np.array_equal(h0["repair_plus"][a], h0["repair_plus"][b])
        if F >= 16:  # N runs and single IUPAC letters inside windows
            inside = lambda lo, hi: ((pos - 3 - F < hi) & (pos - 3 + F > lo)).any()
            assert inside(10000, 10012) and sum(inside(10500 + 37 * k, 10501 + 37 * k) for k in range(13)) >= 5
    for n_rows in pcases.TABLE_ROWS:
        plus, minus = cases.kept(pcases.exact_table(n_rows), 20)
        assert plus.size == n_rows and minus.size == 0


# ---------------------------------------------------------------------------------------------- the selection's reference
@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    """tests/select_cases.py's genome and genes, with the reference's repair columns (flank 30) and property columns."""
    c = select_cases.build(oracle)
    d = tmp_path_factory.mktemp("repair")
    c["gff_path"] = str(d / "genes.gff")
    with open(c["gff_path"], "w") as f:
        f.write(c["gff"])
    c["fasta_path"] = str(d / "genome.fa")
    with open(c["fasta_path"], "w") as f:  # one line per contig: read unformatted (dec = 0)
        f.write("".join(">%s\n%s\n" % (n, t.decode()) for n, t in zip(c["names"], c["contigs"]))[:-1])
    c["annotation"] = annotate.Annotation(c["gff_path"])
    c["genes"] = sref.gff_genes(c["gff"])
    c["repair"] = [dict(repair_plus=ref.column_numpy(t, h["pos_plus"], False, 30), repair_minus=ref.column_numpy(t, h["pos_minus"], True, 30))
                   for t, h in zip(c["contigs"], c["hits"])]
    c["props"] = [dict(props_plus=pref.column_numpy(t, h["pos_plus"], False, 20), props_minus=pref.column_numpy(t, h["pos_minus"], True, 20))
                  for t, h in zip(c["contigs"], c["hits"])]
    return c


def _arena_tables(hits, cols, offsets, keys, dtype):
    cat = lambda src, key, dt, add: np.concatenate([h[key].astype(dt) + (dt(o) if add else dt(0)) for h, o in zip(src, offsets)])
    tables = dict(pos_plus=cat(hits, "pos_plus", np.uint32, True), score_plus=cat(hits, "score_plus", np.float64, False),
                  pos_minus=cat(hits, "pos_minus", np.uint32, True), score_minus=cat(hits, "score_minus", np.float64, False))
    return tables, {k: cat(cols, k, dtype, False) for k in keys}


REPAIR_KEYS = ("repair_plus", "repair_minus")


def _host_arena(texts, names, hits, cols):
    offsets, off = [], 64
    for t in texts:
        offsets.append(off)
        off += ((len(t) + 63) // 64 + 1) * 64
    tables, cols = _arena_tables(hits, cols, offsets, REPAIR_KEYS, np.uint64)
    return tables, cols, [(n, 0, len(t), o) for n, t, o in zip(names, texts, offsets)], offsets


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("n_in", "n_pass", "sel")):
        assert np.array_equal(np.asarray(g, np.uint32), np.asarray(w, np.uint32)), (what, name)


def _exactly_k(tables, cols, lo, hi, K):
    """(limits, gene): repair limits under which exactly K rows of the gene with most rows pass, from the reference's columns."""
    g = int(sref.select_numpy(tables, lo, hi, 1)[0].argmax())
    mh = []
    for s, back in (("plus", 3), ("minus", 0)):
        c = tables["pos_" + s].astype(np.int64) - back
        inside = (c >= lo[g]) & (c <= hi[g]) & (tables["score_" + s] != -1.0)
        mh.append((cols["repair_" + s][inside] & np.uint64(0xFFFFFFFF)).astype(np.int64))
    mh = np.sort(np.concatenate(mh))[::-1]
    if mh.size <= K or mh[K - 1] == mh[K]:
        return None, g
    return (int(mh[K - 1]), 0), g  # the K-th largest mh as the bound: the next one is smaller


def test_selection_numpy_statement_equals_the_plain_loop(case):
    tables, cols, entries, _ = _host_arena(case["contigs"], case["names"], case["hits"], case["repair"])
    lo, hi, _ = sref.layout(case["genes"], entries, 0)
    pick = np.arange(0, len(lo), 4)
    for limits in ((20000, 60), (0, 67), (35000, 0), (0, 100), EVERYTHING, NOTHING):
        got = ref.select_numpy(tables, lo[pick], hi[pick], 5, 0.3, None, None, cols, limits)
        _same(got, ref.select_loop(tables, lo[pick], hi[pick], 5, 0.3, cols, limits), str(limits))
        if limits == EVERYTHING:
            _same(got, sref.select_numpy(tables, lo[pick], hi[pick], 5, 0.3))
        if limits == NOTHING:
            assert got[1].sum() == 0 and got[0].sum() > 0
    full = ref.select_numpy(tables, lo, hi, 5, 0.0, None, None, cols, (20000, 60))
    plain = sref.select_numpy(tables, lo, hi, 5)
    assert np.array_equal(full[0], plain[0]) and (full[1] <= plain[1]).all() and 0 < full[1].sum() < plain[1].sum()
    limits, g = _exactly_k(tables, cols, lo, hi, 5)
    assert limits is not None and ref.select_numpy(tables, lo, hi, 5, 0.0, None, None, cols, limits)[1][g] == 5


# ---------------------------------------------------------------------------------------------- the command line
class SelectOracleBackend(OracleBackend):
    """OracleBackend plus the `select` keyword as it was before the repair scores: the selection by the numpy statement
    over one host arena.  It does not know the feature: a request's repair fields are not looked at."""
    knows_repair = False

    def scan(self, strings, l, offtarget=False, annotation=None, specificity=None, select=None, properties=False):
        out = OracleBackend.scan(self, strings, l, offtarget=offtarget, annotation=annotation)
        assert specificity is None and not properties  # (the oracle has no self search)
        if select is None:
            return out
        assert select.property_limits is None
        texts = [bytes(s) for s in strings]
        F = select.flank if self.knows_repair else 30
        cols = [dict(repair_plus=ref.column_numpy(t, h["pos_plus"], False, F), repair_minus=ref.column_numpy(t, h["pos_minus"], True, F))
                for t, h in zip(texts, out)]
        tables, cols, _, offsets = _host_arena(texts, list(range(len(texts))), out, cols)
        req = select.annotation
        lo, hi, gene = req.gene_layout([(k, o, len(t)) for k, (t, o) in enumerate(zip(texts, offsets))])
        limits = select.repair_limits.astuple() if self.knows_repair and select.repair_limits is not None else None
        self.ran_repair = self.knows_repair and select.runs_repair
        n_in, n_pass, picked = ref.select_numpy(tables, lo, hi, select.params.k, select.params.min_score, None, None, cols, limits)
        part = dict(offsets=np.array(offsets, np.uint64), lengths=np.array([len(t) for t in texts], np.uint64), group=list(range(len(texts))),
                    gene=gene, n_in=n_in, n_pass=n_pass, sel=picked, **tables)
        if self.knows_repair and select.repair_flank is not None:
            part.update(cols)
        out = sel.HitList(out)
        out.selection = sel.assemble(req.annotation.genes()[0], select.params.k, [part])
        return out


class RepairOracleBackend(SelectOracleBackend):
    """The same, serving `repair` and the limits from the reference."""
    knows_repair = True


def _run(case, tmp_path, monkeypatch, extra, backend, name="out.csv"):
    monkeypatch.chdir(tmp_path)
    out_csv = str(tmp_path / name)
    argv = ["-f", case["fasta_path"], "-g", case["gff_path"], "-o", out_csv, "--cas9", "--seed", "11", "--each-contig-once"] + list(extra)
    buf = io.StringIO()
    cli.run(cli.build_parser().parse_args(argv), backend=backend, out=buf)
    return out_csv, buf.getvalue()


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def _wanted_selection(case, K, limits, F=30):
    """[(gene label, rank, passing, contig name, end_pos, strand, packed repair value)] the reference selects."""
    cols = case["repair"] if F == 30 else [dict(repair_plus=ref.column_numpy(t, h["pos_plus"], False, F), repair_minus=ref.column_numpy(t, h["pos_minus"], True, F))
                                           for t, h in zip(case["contigs"], case["hits"])]
    tables, cols, entries, _ = _host_arena(case["contigs"], case["names"], case["hits"], cols)
    lo, hi, gene = sref.layout(case["genes"], entries, 0)
    n_in, n_pass, picked = ref.select_numpy(tables, lo, hi, K, 0.0, None, None, cols, limits)
    n_before = np.cumsum([0] + [len(h["pos_plus"]) for h in case["hits"]])
    m_before = np.cumsum([0] + [len(h["pos_minus"]) for h in case["hits"]])
    want = []
    for row_of_layout, g in enumerate(gene):
        for rank, packed in enumerate(picked[row_of_layout]):
            if packed == NONE:
                break
            minus, r = int(packed) >> 31, int(packed) & 0x7FFFFFFF
            c = int(np.searchsorted(m_before if minus else n_before, r, "right") - 1)
            h = case["hits"][c]
            end = int(h["pos_minus"][r - m_before[c]]) + 3 if minus else int(h["pos_plus"][r - n_before[c]])
            value = int(cols["repair_minus" if minus else "repair_plus"][r])
            want.append((int(g), rank, (case["genes"][int(g)][3], str(rank + 1), str(int(n_pass[row_of_layout])), case["names"][c], str(end),
                                        "-" if minus else "+", value)))
    return [w[2] for w in sorted(want, key=lambda w: w[:2])], n_pass


def _check_selection_file(case, got, K, limits, with_fields, F=30):
    want, n_pass = _wanted_selection(case, K, limits, F)
    assert got[0] == ["gene", "rank", "passing"] + rows.HEADER[1:] + (repair.HEADER if with_fields else [])
    assert len(got) - 1 == len(want)
    for g, w in zip(got[1:], want):
        strand_at = 9 if len(g) - (2 if with_fields else 0) == len(rows.HEADER) + 2 else 8  # (an 11-field row has no cutsite field)
        assert (g[0], g[1], g[2], g[6], g[8], g[strand_at + 1]) == w[:6], (g, w)
        if with_fields:
            mh, oof = _pair(w[6])
            assert g[-2] == "%d.%d" % divmod(mh, 10) and g[-1] == (repr((100 * oof) / mh) if mh else "-1"), (g, w)
            assert mh >= limits[0] and 100 * oof >= limits[1] * mh
    return n_pass


def test_cli_over_the_oracle(case, oracle, tmp_path, monkeypatch):
    backend = RepairOracleBackend(oracle)
    tables, cols, entries, _ = _host_arena(case["contigs"], case["names"], case["hits"], case["repair"])
    lo, hi, _ = sref.layout(case["genes"], entries, 0)
    exact, g = _exactly_k(tables, cols, lo, hi, 5)
    mh_text = "%d.%d" % divmod(exact[0], 10)
    plain_main, plain_stdout = _run(case, tmp_path, monkeypatch, ["--select", "5"], SelectOracleBackend(oracle), "plain.csv")
    unfiltered = sref.select_numpy(tables, lo, hi, 5)[1]
    for k, (flags, limits) in enumerate(((["--repair-scores"], EVERYTHING),
                                        (["--repair-scores", "--select-min-oof", "60", "--select-min-mh", "2000"], (20000, 60)),
                                        (["--repair-scores", "--select-min-mh", "200000.0"], (2000000, 0)),   # passes nothing
                                        (["--repair-scores", "--select-min-oof", "0", "--select-min-mh", "0"], EVERYTHING),
                                        (["--repair-scores", "--select-min-mh", mh_text], exact))):            # exactly K in the largest gene
        out, stdout = _run(case, tmp_path, monkeypatch, ["--select", "5", "--bench-json", str(tmp_path / "b.json")] + flags, backend, "run%d.csv" % k)
        assert backend.ran_repair and stdout == plain_stdout
        assert open(out, "rb").read() == open(plain_main, "rb").read()  # the main table does not change
        n_pass = _check_selection_file(case, _read(out + ".selected.csv"), 5, limits, True)
        if limits == EVERYTHING:
            assert np.array_equal(n_pass, unfiltered)
            assert [r[:-2] for r in _read(out + ".selected.csv")] == _read(plain_main + ".selected.csv")
        elif limits[0] == 2000000:
            assert n_pass.sum() == 0 and len(_read(out + ".selected.csv")) == 1
        elif limits == exact:
            assert n_pass[g] == 5
        else:
            assert 0 < n_pass.sum() < unfiltered.sum()
    # a filter alone runs the kernel and prints no field; another flank gives other scores
    filt, _ = _run(case, tmp_path, monkeypatch, ["--select", "5", "--select-min-oof", "60", "--select-min-mh", "2000"], backend, "filt.csv")
    assert backend.ran_repair
    _check_selection_file(case, _read(filt + ".selected.csv"), 5, (20000, 60), False)
    assert _read(filt + ".selected.csv")[1:] == [r[:-2] for r in _read(str(tmp_path / "run1.csv") + ".selected.csv")[1:]]
    f16, _ = _run(case, tmp_path, monkeypatch, ["--select", "5", "--repair-scores", "--repair-flank", "16", "--select-min-oof", "60"], backend, "f16.csv")
    _check_selection_file(case, _read(f16 + ".selected.csv"), 5, (0, 60), True, F=16)


def test_cli_without_the_flags_every_byte_is_what_it_was(case, oracle, tmp_path, monkeypatch, manifest):
    """A run without the new flags against a run on the same inputs over a backend that does not know the feature; and the
    main CSV against the golden one (md5_libm)."""
    import hashlib
    from conftest import golden_fasta_path, run_cli
    for k, extra in enumerate((["--select", "5"], ["--select", "3", "--select-min-score", "0.4", "--select-only"])):
        old, old_stdout = _run(case, tmp_path, monkeypatch, extra, SelectOracleBackend(oracle), "old%d.csv" % k)
        backend = RepairOracleBackend(oracle)
        new, new_stdout = _run(case, tmp_path, monkeypatch, extra, backend, "new%d.csv" % k)
        assert not backend.ran_repair and old_stdout == new_stdout
        assert open(old + ".selected.csv", "rb").read() == open(new + ".selected.csv", "rb").read()
        if "--select-only" not in extra:
            assert open(old, "rb").read() == open(new, "rb").read()
    data, _ = run_cli(tmp_path, monkeypatch, golden_fasta_path("sample", tmp_path), OracleBackend(oracle), manifest["seed"])
    assert hashlib.md5(data).hexdigest() == manifest["cases"]["sample"]["md5_libm"]


REFUSALS = [
    (["--repair-scores"], "belongs to --select"),
    (["--repair-flank", "30"], "belongs to --select"),
    (["--select-min-oof", "60"], "belongs to --select"),
    (["--select-min-mh", "12.5"], "belongs to --select"),
    (["--select", "5", "--repair-flank", "30"], "--repair-flank belongs to"),
    (["--select", "5", "--repair-scores", "--repair-flank", "1"], "2..32"),
    (["--select", "5", "--repair-scores", "--repair-flank", "33"], "2..32"),
    (["--select", "5", "--select-min-oof", "50", "--repair-flank", "-4"], "2..32"),
    (["--select", "5", "--repair-scores", "--repair-flank", "3x"], "2..32"),
    (["--select", "5", "--select-min-oof", "101"], "0..100"),
    (["--select", "5", "--select-min-oof", "-1"], "0..100"),
    (["--select", "5", "--select-min-oof", "50.5"], "0..100"),
    (["--select", "5", "--select-min-oof", "half"], "0..100"),
    (["--select", "5", "--select-min-mh", "12.55"], "one fractional digit"),
    (["--select", "5", "--select-min-mh", "-3"], "one fractional digit"),
    (["--select", "5", "--select-min-mh", "1e3"], "one fractional digit"),
    (["--select", "5", "--select-min-mh", "."], "one fractional digit"),
    (["--select", "5", "--repair-scores", "--gpus", "2"], "one GPU"),
    (["--select", "5", "--select-min-oof", "60", "--gpus", "2"], "one GPU"),
    (["--select", "5", "--repair-scores", "--devices", "0,1"], "one GPU"),
    (["--select", "5", "--select-min-mh", "10", "--devices", "0,1"], "one GPU"),
]


@pytest.mark.parametrize("extra,text", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_cli_refusals_come_before_any_side_effect(case, oracle, tmp_path, monkeypatch, extra, text):
    monkeypatch.chdir(tmp_path)
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9", "-g", case["gff_path"]] + extra
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=RepairOracleBackend(oracle), out=io.StringIO())
    assert "--select" in str(e.value.code) and text in str(e.value.code)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra", [["--select", "5", "--repair-scores"], ["--select", "5", "--select-min-oof", "60"]], ids=["scores", "filter"])
def test_cli_refuses_a_launchers_ranks(case, oracle, tmp_path, monkeypatch, extra):
    class Group:
        world, rank, local_rank = 2, 0, 0
    monkeypatch.chdir(tmp_path)
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9", "-g", case["gff_path"]] + extra
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=RepairOracleBackend(oracle), out=io.StringIO(), group=Group())
    assert "--select" in str(e.value.code) and "2 ranks" in str(e.value.code)
    assert os.listdir(tmp_path) == []


# ---------------------------------------------------------------------------------------------- on the GPU
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_arenas", [1, 3], ids=["one-arena", "three-arenas"])
@pytest.mark.parametrize("l", [20, 1], ids=["l20", "l1"])
def test_gpu_columns_equal_the_reference(engine, genome, l, n_arenas):
    """Row by row, at every flank.  The scan at guide length 1 keeps the rows nearest to the contig ends: the first '+' row
    (cut at 3: the window reaches into the arena's leading void) and '-' rows whose window the contig end cuts by 1 .. F
    letters, at the end of every contig -- the last contig of an arena included, whose windows meet the words past the
    text."""
    g = engine.genome(genome["texts"], max_words=None if n_arenas == 1 else 600)
    try:
        assert len(g.arenas) == n_arenas
        hits = g.scan_score(l)
        counts = [(h.n_plus, h.n_minus) for h in hits.per_arena]
        for F in cases.FLANKS:
            cols = g.repair_scores(counts, F)
            assert g.repair_stats["rows"] == hits.n_plus + hits.n_minus and g.repair_stats["flank"] == F and g.repair_stats["kernel_ms"] > 0
            want = genome["at"](l, F)
            for a, group in enumerate(g.groups):
                for s, key in enumerate(REPAIR_KEYS):
                    w = np.concatenate([want[k][key] for k in group])
                    assert np.array_equal(getattr(hits.per_arena[a], "pos_" + key[7:]) - 0, np.concatenate(
                        [want[k]["pos_" + key[7:]] + np.uint32(g.arenas[a].offsets[j]) for j, k in enumerate(group)])), (F, a, key)
                    got = cols[a][s]
                    bad = np.flatnonzero(got != w)
                    assert bad.size == 0, (F, a, key, bad[:5], got[bad[:5]], w[bad[:5]])
        via_scan = g.scan_score(l, repair=30)
        again = genome["at"](l, 30)
        assert len(via_scan.repair) == n_arenas and "repair_plus" not in via_scan.contig(0)
        for a, group in enumerate(g.groups):
            for s, key in enumerate(REPAIR_KEYS):
                assert np.array_equal(via_scan.repair[a][s], np.concatenate([again[k][key] for k in group]))
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", pcases.TABLE_ROWS)
def test_gpu_exact_tables_and_an_empty_strand(engine, n_rows):
    text = pcases.exact_table(n_rows)
    arena = engine.arena([text])
    try:
        n_plus, n_minus = arena.scan_score_device(20)
        assert (n_plus, n_minus) == (n_rows, 0)
        pos = arena.fetch(n_plus, n_minus)[0].astype(np.int64) - int(arena.offsets[0])
        for F in cases.FLANKS:
            rp, rm = arena.repair_scores(n_plus, n_minus, F)
            assert rm.size == 0 and np.array_equal(rp, ref.column_numpy(text, pos, False, F)), F
            st = arena.repair_scores_stats()
            assert st["rows"] == n_rows and st["flank"] == F and st["kernel_ms"] > 0
    finally:
        arena.close()


@pytest.mark.gpu
def test_gpu_calls_out_of_order(engine):
    L = nat.lib()
    text = b"ACGTTGCAAGGCCTTAGGACCA" * 60
    arena = engine.arena([text])
    empty = engine.arena([b"ATATATATATATATATATATATATATATATATATATATAT"])
    try:
        def status(fn):
            with pytest.raises(nat.CropsrHipError) as e:
                fn()
            return e.value.status, str(e.value)

        assert status(lambda: arena.repair_scores(0, 0))[0] == nat.CRP_ERR_STATE  # no tables
        assert status(arena.repair_scores_stats)[0] == nat.CRP_ERR_STATE
        n_plus, n_minus = arena.scan_score_device(20)
        for flank in (1, 33, 0, -5):
            st, msg = status(lambda: arena.repair_scores(n_plus, n_minus, flank))
            assert st == nat.CRP_ERR_INVALID and "2..32" in msg
        assert status(arena.repair_scores_stats)[0] == nat.CRP_ERR_STATE
        h = sel.ArenaSelect(arena, [0, 100], [50, 900])
        limits = repair.Limits(min_mh=10000, min_oof=50)
        h.set_repair_limits(limits)
        st, msg = status(lambda: h.run(sel.Params(5)))
        assert st == nat.CRP_ERR_STATE and "crp_repair_scores" in msg  # limits without a column
        bad = nat.SelectRepairLimits(0, 101)
        assert L.crp_select_set_repair_limits(h._h, ctypes.byref(bad)) == nat.CRP_ERR_INVALID
        assert arena.repair_scores(n_plus, n_minus, 30, fetch=False) is None  # NULL pointers: the column stays on the device
        rp, rm = arena.repair_scores(n_plus, n_minus, 30)
        cols = arena.fetch(n_plus, n_minus)
        off = int(arena.offsets[0])
        assert np.array_equal(rp, ref.column_numpy(text, cols[0].astype(np.int64) - off, False, 30))
        assert np.array_equal(rm, ref.column_numpy(text, cols[3].astype(np.int64) - off, True, 30))
        tables = dict(pos_plus=cols[0], score_plus=cols[2], pos_minus=cols[3], score_minus=cols[5])
        h.run(sel.Params(5))
        _same(h.fetch(), ref.select_numpy(tables, [0, 100], [50, 900], 5, 0.0, None, None, dict(repair_plus=rp, repair_minus=rm), limits.astuple()))
        assert h.stats()["bytes_per_row"] == 20
        arena.scan_score_device(20)  # a re-scan: the column belongs to the earlier tables
        assert status(arena.repair_scores_stats)[0] == nat.CRP_ERR_STATE
        st, msg = status(lambda: h.run(sel.Params(5)))
        assert st == nat.CRP_ERR_STATE and "crp_repair_scores" in msg
        h.set_repair_limits(None)  # cleared: the plain selection again
        h.run(sel.Params(5))
        _same(h.fetch(), sref.select_numpy(tables, [0, 100], [50, 900], 5))
        assert h.stats()["bytes_per_row"] == 12
        h.close()
        assert empty.scan_score_device(20) == (0, 0)  # empty tables are fine
        rp, rm = empty.repair_scores(0, 0, 30)
        assert rp.size == rm.size == 0 and empty.repair_scores_stats()["rows"] == 0
    finally:
        arena.close()
        empty.close()


@pytest.fixture(scope="module", params=[1, 3], ids=["one-arena", "three-arenas"])
def scanned(request, engine, case):
    """select_cases' genome with tables, annotation ids, repair and property columns and joined specificity columns
    resident, and per arena the reference's view of the same."""
    g = engine.genome(case["contigs"], max_words=None if request.param == 1 else 600)
    assert len(g.arenas) == request.param
    areq = annotate.Request(case["annotation"], case["names"], 0)
    hits = g.scan_score(20)
    counts = [(h.n_plus, h.n_minus) for h in hits.per_arena]
    feats = g.annotate(areq, counts)
    g.guide_properties(counts, fetch=False)
    dev = g.repair_scores(counts, 30)
    pattern, gp, M, scheme = srch.check_specificity(20, 3)
    handles = []
    srch._self_handles(g, pattern, gp, srch.SPECIFICITY_PAM_LEN, M, scheme, None, None, handles)
    srch._self_compare_all(handles, M)
    arenas = []
    for a, (arena, group) in enumerate(zip(g.arenas, g.groups)):
        offsets = [int(o) for o in arena.offsets]
        tables, cols = _arena_tables([case["hits"][k] for k in group], [case["repair"][k] for k in group], offsets, REPAIR_KEYS, np.uint64)
        _, props = _arena_tables([case["hits"][k] for k in group], [case["props"][k] for k in group], offsets, ("props_plus", "props_minus"), np.uint32)
        for key in tables:
            assert np.array_equal(tables[key].view(np.uint8), getattr(hits.per_arena[a], key).view(np.uint8)), key
        assert np.array_equal(dev[a][0], cols["repair_plus"]) and np.array_equal(dev[a][1], cols["repair_minus"])
        entries = [(case["names"][k], 0, int(arena.lengths[j]), int(arena.offsets[j])) for j, k in enumerate(group)]
        lo, hi, gene = sref.layout(case["genes"], entries, 0)
        cp, sp, cm, sm = handles[a].join_hits(20)
        arenas.append(dict(tables=tables, repair=cols, props=props, lo=lo, hi=hi, gene=gene,
                           spec=dict(counts_plus=cp, sum_plus=sp, counts_minus=cm, sum_minus=sm),
                           cds=dict(feat_plus=feats[a][0], feat_minus=feats[a][1], flags=case["annotation"].cds_flags())))
    yield dict(genome=g, request=areq, handles=handles, arenas=arenas)
    for h in handles:
        h.close()
    g.close()


def _device(s, a, K, slice_rows, limits, min_score=0.0, spec=None, cds=False, prop_limits=(None,) * 5):
    params = sel.Params(K, min_score, require_cds=cds)
    if spec is not None:
        params.max_mm0, params.max_hit_sum = spec["max_mm0"], spec["max_hit_sum"]
    req = sel.Request(params, s["request"], slice_rows, *prop_limits, min_mh=limits[0], min_oof=limits[1])
    _, _, _, n_in, n_pass, picked, stats = sel.select_arena(s["genome"], a, req, s["handles"][a] if spec is not None else None)
    return (n_in, n_pass, picked), stats


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
@pytest.mark.parametrize("K", (1, 5, 64))
def test_gpu_selection_with_limits_equals_the_reference(scanned, K, slice_rows):
    s = scanned
    exact = 0
    for a, A in enumerate(s["arenas"]):
        args = (A["tables"], A["lo"], A["hi"], K, 0.0, None, None, A["repair"])
        for limits in ((20000, 60), (0, 67), (0, 100), (35000, 0), NOTHING, EVERYTHING):
            got, stats = _device(s, a, K, slice_rows, limits)
            _same(got, ref.select_numpy(*args, limits), "arena %d %r" % (a, limits))
            assert stats["bytes_per_row"] == 20
            if limits == NOTHING:
                assert (got[1] == 0).all() and (got[2] == NONE).all() and got[0].sum() > 0
            if limits == EVERYTHING:
                _same(got, sref.select_numpy(A["tables"], A["lo"], A["hi"], K))
        limits, g = _exactly_k(A["tables"], A["repair"], A["lo"], A["hi"], K)
        if limits is not None:
            got, _ = _device(s, a, K, slice_rows, limits)
            _same(got, ref.select_numpy(*args, limits), "exactly K")
            assert got[1][g] == K and (got[2][g] != NONE).all()
            exact += 1
    assert exact >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
def test_gpu_limits_with_property_limits_joined_columns_and_cds(scanned, slice_rows):
    s = scanned
    spec = dict(max_mm0=2, max_hit_sum=1 << 34)
    limits, prop_limits = (15000, 55), (6, 15, 4, 3, 5)
    total = 0
    for a, A in enumerate(s["arenas"]):
        got, stats = _device(s, a, 5, slice_rows, limits, 0.2, spec, cds=True, prop_limits=prop_limits)
        also = dict(plus=pref.limits_pass(A["props"]["props_plus"], prop_limits), minus=pref.limits_pass(A["props"]["props_minus"], prop_limits))
        want = ref.select_numpy(A["tables"], A["lo"], A["hi"], 5, 0.2, dict(A["spec"], **spec), A["cds"], A["repair"], limits, also)
        _same(got, want, "arena %d" % a)
        assert stats["bytes_per_row"] == 40
        without = ref.select_numpy(A["tables"], A["lo"], A["hi"], 5, 0.2, dict(A["spec"], **spec), A["cds"], also=also)
        assert (want[1] <= without[1]).all()
        total += int(without[1].sum() - want[1].sum())
    assert total > 0


@pytest.mark.gpu
def test_gpu_genome_level_call_runs_the_kernel_before_the_selection(engine, case):
    g = engine.genome(case["contigs"], max_words=600)
    try:
        areq = annotate.Request(case["annotation"], case["names"], 0)
        params = lambda: sel.Params(5, 0.2, max_perfect=0, min_specificity=0.5)
        # limits alone: the kernel runs inside the join's hook, nothing is fetched
        hits = g.scan_score(20, specificity=dict(max_mm=3), select=sel.Request(params(), areq, min_mh=15000, min_oof=55))
        S = hits.selection
        assert hits.repair is None and S.mh is None and g.repair_stats["rows"] == hits.n_plus + hits.n_minus and g.repair_stats["flank"] == 30
        with_cols = g.scan_score(20, specificity=dict(max_mm=3), select=sel.Request(params(), areq, min_mh=15000, min_oof=55, repair_flank=30))
        T = with_cols.selection
        assert S.rows.tobytes() == T.rows.tobytes() and np.array_equal(S.n_pass, T.n_pass) and 0 < S.n_pass.sum()
        loose = g.scan_score(20, specificity=dict(max_mm=3), select=sel.Request(params(), areq))
        assert loose.selection.n_pass.sum() > S.n_pass.sum() and loose.selection.mh is None and loose.repair is None
        assert T.mh.size == T.oof.size == T.rows.size
        for r, mh, oof in zip(T.rows, T.mh, T.oof):  # every selected row carries the reference's pair and keeps the limits
            v = case["repair"][int(r["contig"])]["repair_plus" if r["strand"] == b"+" else "repair_minus"][int(r["index"])]
            assert _pair(v) == (int(mh), int(oof)) and mh >= 15000 and 100 * int(oof) >= 55 * int(mh)
        # the plain place: no specificity join
        plain = g.scan_score(20, select=sel.Request(sel.Params(5), areq, repair_flank=16))
        assert plain.selection.mh.size == plain.selection.rows.size and g.repair_stats["flank"] == 16
        for a, group in enumerate(g.groups):
            for s_, key in enumerate(("plus", "minus")):
                want = np.concatenate([ref.column_numpy(case["contigs"][k], case["hits"][k]["pos_" + key], key == "minus", 16) for k in group])
                assert np.array_equal(plain.repair[a][s_], want)
        with pytest.raises(ValueError):
            g.scan_score(20, repair=33)
        with pytest.raises(ValueError):
            g.scan_score(20, repair=30, select=sel.Request(sel.Params(5), areq, repair_flank=16))
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_command_line_end_to_end(case, tmp_path, monkeypatch):
    flags = ["--select", "5", "--repair-scores", "--select-min-oof", "60", "--select-min-mh", "2000", "--bench-json", str(tmp_path / "bench.json")]
    out, _ = _run(case, tmp_path, monkeypatch, flags, None)
    n_pass = _check_selection_file(case, _read(out + ".selected.csv"), 5, (20000, 60), True)
    assert n_pass.sum() > 0
    with open(tmp_path / "bench.json") as f:
        stage = json.load(f)["repair"]
    assert stage["kernel_ms"] > 0 and stage["flank"] == 30 and stage["wall_s"] > 0
    assert stage["rows"] == sum(h["pos_plus"].size + h["pos_minus"].size for h in case["hits"])
