"""The pair-table hit score of the off-target search (search.py PairTable / --score-table, crp_search_set_pair_scheme,
crp_search_self_set_pair_scheme; DESIGN.md section 15, Pair tables): the definition stated twice, hand-made answers, the
tie to the position-weight scheme, refusals, the file parser, the converter, TSV bytes, the ABI and the two kernels'
static ISA without a GPU; the device's sums against the loop reference, exactly, on the GPU."""
import ctypes
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import search_pair_reference as pref
import search_reference as ref
import search_score_reference as sref
from cropsr_amd import _native as nat
from cropsr_amd import search as srch
from test_search import CAS12A, PAM_LEN, SACAS9, SPCAS9, SPCAS9_NAG, TSV_GENOME, _as_tuples, _planted_genome, _queries_for, _tsv_case
from test_search_score import CAS12A_20, _figures, _sites_array, search_isa  # noqa: F401  (search_isa: a fixture)
from test_search_self import _genome, _queries_of_rows, self_isa  # noqa: F401  (self_isa: a fixture)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import cfd_to_table  # noqa: E402
import emit_isa_budget as isa  # noqa: E402

ONE = 1 << 30
P_OF = dict(PAM_LEN)
P_OF[CAS12A_20] = 4
# the PAM offsets each pattern is run with: letters other than N only
OFFSETS = {SPCAS9: (1, 2), SPCAS9_NAG: (1, 2), SACAS9: (2, 3, 4), CAS12A: (3,), CAS12A_20: ()}


def _table(pattern, seed):
    """(PairTable, pair, offsets, pam) of a pattern: random and asymmetric, with exact 0 and 1 entries."""
    pair, pam = pref.random_table(np.random.default_rng(500 + seed), pattern, P_OF[pattern], OFFSETS[pattern])
    return srch.PairTable(pair, OFFSETS[pattern], pam), pair, OFFSETS[pattern], pam


# ------------------------------------------------------------------ the definition (CPU)
def test_two_statements_of_the_definition_agree():
    rng = np.random.default_rng(11)
    n_cases = 0
    for G in (17, 20, 21, 23):
        for pam3 in (True, False):
            for k in range(4):
                P = 4
                pam_letters = "NGRT" if pam3 else "TTVN"  # one N: never an offset
                pattern = "N" * G + pam_letters if pam3 else pam_letters + "N" * G
                free = [o for o in range(P) if pam_letters[o] != "N"]
                offsets = tuple(sorted(rng.choice(free, k, replace=False).tolist()))
                pair, pam = pref.random_table(rng, pattern, P, offsets)
                sc = srch.make_scheme(pattern, P, srch.PairTable(pair, offsets, pam))
                gpos, pam_at = pref.guide_positions(pattern, P)
                assert sc.g_positions().tolist() == gpos and sc.pam_positions == tuple(pam_at + o for o in offsets)
                qc, scodes, at, want = [], [], [], []
                for n in range(9):
                    for rep in range(12):
                        query = list("N" * len(pattern))
                        for p in gpos:
                            query[p] = str(rng.choice(list("ACGT")))
                        if rep % 4 == 3:  # a shorter guide: N at the PAM-distal end
                            query[gpos[0]] = query[gpos[1]] = "N"
                        site = list(query)
                        for p in range(len(pattern)):
                            if site[p] == "N":
                                site[p] = str(rng.choice(list(ref.IUPAC_SETS.get(pattern[p], "ACGT"))))
                        compared = [p for p in gpos if query[p] != "N"]
                        for p in rng.choice(compared, n, replace=False):
                            site[p] = str(rng.choice([b for b in "ACGT" if b != site[p]]))
                        if n and rep % 6 == 5:
                            site[[p for p in compared if site[p] != query[p]][0]] = "?"  # a non-base at a mismatch
                        want.append(pref.value_loop("".join(query), "".join(site), pattern, P, pair, offsets, pam))
                        qc.append([("ACGTN".index(query[p])) for p in gpos])
                        scodes.append([("ACGT?".index(site[p])) for p in gpos])
                        at.append(sum("ACGT".index(site[pam_at + o]) << (2 * (k - 1 - j)) for j, o in enumerate(offsets)))
                        if n == 0 or "?" in site:
                            assert want[-1] == 0
                got = srch.pair_values(np.array(qc), np.array(scodes), np.array(at), sc)
                assert got.dtype == np.uint64 and got.tolist() == want, (G, pam3, k)
                assert max(want) <= ONE and sum(1 for v in want if v) > 20  # (not a comparison of zeros)
                n_cases += len(want)
    assert n_cases == 4 * 2 * 4 * 9 * 12


def _one_site(pattern, P, query, site, table):
    """The single site of a one-contig genome, its value by the package's site route and by the loop."""
    contig = site.encode()
    counts, s = ref.search([contig], pattern, [query], 8)
    sites = _sites_array(s)
    assert sites.size == 1
    sc = srch.make_scheme(pattern, P, table)
    v = srch.hit_values(sites, [query], [contig], sc).tolist()
    want = pref.value_loop(query, site.upper(), pattern, P, table.pair, table.pam_offsets, table.pam)
    assert v == [want]
    return v[0], int(sites["mismatches"][0])


def test_known_answers():
    guide = "ACGTTGCAACGTTGCAACGT"
    pair = np.full((20, 4, 4), 0.5)
    pair[19, 3, 0] = 0.3      # query T facing site A, next to the PAM
    pair[19, 3, 1] = 0.7      # query T facing site C there: the same mask, another letter
    pair[19, 0, 3] = 0.9      # (the transposed entry: must not be the one that is read)
    pam = np.zeros(16)
    pam["ACGT".index("G") * 4 + "ACGT".index("G")] = 1.0
    pam["ACGT".index("A") * 4 + "ACGT".index("G")] = 0.25
    t3 = srch.PairTable(pair, (1, 2), pam)
    q3 = srch.check_query(SPCAS9_NAG, guide, 3)
    # a single mismatch next to a 3' PAM: exactly rint(pair * pam * 2^30)
    v_a, mm = _one_site(SPCAS9_NAG, 3, q3, guide[:19] + "A" + "TGG", t3)
    assert mm == 1 and v_a == int(np.rint(0.3 * 1.0 * ONE))
    # the same mask, another site letter: what the position-only scheme cannot tell apart
    v_c, mm = _one_site(SPCAS9_NAG, 3, q3, guide[:19] + "C" + "TGG", t3)
    assert mm == 1 and v_c == int(np.rint(0.7 * 1.0 * ONE)) and v_c != v_a
    # the same site behind AG and GG differs by the PAM entry
    v_ag, _ = _one_site(SPCAS9_NAG, 3, q3, guide[:19] + "A" + "TAG", t3)
    assert v_ag == int(np.rint(0.3 * 0.25 * ONE)) and v_a == int(np.rint(np.float64(0.3) * 1.0 * ONE))
    # a non-base at a mismatching position: counted, worth 0; no mismatch: 0
    v_n, mm = _one_site(SPCAS9_NAG, 3, q3, guide[:19] + "N" + "TGG", t3)
    assert (v_n, mm) == (0, 1)
    assert _one_site(SPCAS9_NAG, 3, q3, guide + "TGG", t3) == (0, 0)
    # two mismatches multiply in ascending g, then the PAM
    v2, mm = _one_site(SPCAS9_NAG, 3, q3, "C" + guide[1:19] + "A" + "TAG", t3)
    assert mm == 2 and v2 == int(np.rint(0.5 * 0.3 * 0.25 * ONE))
    # a PAM on the 5' side: g = 19 is the position next to it, the guide's first letter
    pair5 = np.full((20, 4, 4), 0.5)
    pair5[19, 0, 2] = 0.3     # query A facing site G at the guide's first letter
    pam5 = np.array([0.6, 0.7, 0.8, 0.0])  # TTTV: the V letter, offset 3 (A, C, G; T cannot be)
    t5 = srch.PairTable(pair5, (3,), pam5)
    q5 = srch.check_query(CAS12A_20, guide, 4)
    v5, mm = _one_site(CAS12A_20, 4, q5, "TTTC" + "G" + guide[1:], t5)
    assert mm == 1 and v5 == int(np.rint(0.3 * 0.7 * ONE))
    v5b, _ = _one_site(CAS12A_20, 4, q5, "TTTC" + guide[:19] + "A", t5)  # the PAM-distal end: g = 0
    assert v5b == int(np.rint(0.5 * 0.7 * ONE))
    # a '-' strand site reads like its '+' twin
    rc = (guide[:19] + "A" + "TAG").translate(str.maketrans("ACGT", "TGCA"))[::-1].encode()
    counts, s = ref.search([rc], SPCAS9_NAG, [q3], 8)
    sites = _sites_array(s)
    assert sites.size == 1 and sites["strand"][0] == b"-"
    assert srch.hit_values(sites, [q3], [rc], srch.make_scheme(SPCAS9_NAG, 3, t3)).tolist() == [v_ag]


def test_pair_table_of_position_factors_is_the_weights_scheme_without_shape():
    rng = np.random.default_rng(5)
    for pattern, P in ((SPCAS9, 3), (CAS12A, 4)):
        G = len(pattern) - P
        w = np.round(rng.random(G), 3)
        weights = srch.make_scheme(pattern, P, w.tolist())
        weights.shape = np.ones_like(weights.shape)  # the spread term switched off
        pair = np.repeat((1.0 - w)[:, None, None], 4, axis=1).repeat(4, axis=2)
        sc = srch.make_scheme(pattern, P, srch.PairTable(pair))
        masks, qc, scodes = [], [], []
        for n in range(9):
            for _ in range(30):
                gs = rng.choice(G, n, replace=False)
                q = rng.integers(0, 4, G)
                s = q.copy()
                s[gs] = (q[gs] + rng.integers(1, 4, n)) % 4
                masks.append(sum(1 << int(g) for g in gs))
                qc.append(q)
                scodes.append(s)
        got = srch.pair_values(np.array(qc), np.array(scodes), np.zeros(len(masks), np.int64), sc)
        assert got.tolist() == srch.mask_values(masks, weights).tolist()


# ------------------------------------------------------------------ refusals, the parser, the converter (CPU)
def test_refusals():
    E = srch.SearchInputError
    q = srch.check_query(SPCAS9, "ACGTACGTACGTACGTACGT", 3)
    good = np.full((20, 4, 4), 0.5)
    pam = np.full(16, 0.5)
    assert isinstance(srch.check_score(SPCAS9, 3, srch.PairTable(good, (1, 2), pam), [q]), srch.PairScheme)
    assert srch.check_score(SPCAS9, 3, srch.PairTable(good), [q]).pam.tolist() == [1.0]
    for bad in (1.5, -0.1, float("nan"), float("inf")):
        p = good.copy()
        p[7, 1, 2] = bad
        with pytest.raises(E):
            srch.make_scheme(SPCAS9, 3, srch.PairTable(p))
        pm = pam.copy()
        pm[5] = bad
        with pytest.raises(E):
            srch.make_scheme(SPCAS9, 3, srch.PairTable(good, (1, 2), pm))
    diag = good.copy()
    diag[:, np.arange(4), np.arange(4)] = np.nan  # the diagonal is ignored
    assert (srch.make_scheme(SPCAS9, 3, srch.PairTable(diag)).pair[:, 0, 0] == 1.0).all()
    for table in (srch.PairTable(good[:19]), srch.PairTable(np.full((21, 4, 4), 0.5)),  # wrong G
                  srch.PairTable(np.full((20, 4, 3), 0.5)), srch.PairTable("x"),
                  srch.PairTable(good, (0, 1), pam),          # offset 0 is the N of NGG
                  srch.PairTable(good, (2, 1), pam), srch.PairTable(good, (1, 1), pam),  # not strictly ascending
                  srch.PairTable(good, (1, 3), pam), srch.PairTable(good, (-1, 2), pam),  # out of range
                  srch.PairTable(good, (1, 2), np.full(4, 0.5)), srch.PairTable(good, (1, 2)), srch.PairTable(good, (), pam),
                  srch.PairTable(good, (1.0, 2), pam)):
        with pytest.raises(E):
            srch.make_scheme(SPCAS9, 3, table)
    with pytest.raises(E):  # more than 3 offsets
        srch.make_scheme(SACAS9, 6, srch.PairTable(np.full((21, 4, 4), 0.5), (2, 3, 4, 5), np.full(256, 0.5)))
    with pytest.raises(E):  # no PAM length
        srch.check_score(SPCAS9, None, srch.PairTable(good), [q])
    with pytest.raises(E):  # a base at a PAM position of a query
        srch.check_score(SPCAS9, 3, srch.PairTable(good), ["ACGTACGTACGTACGTACGTNGG"])
    with pytest.raises(E):
        srch.check_self(SPCAS9, 3, 3, None, srch.PairTable(good[:19]))
    assert isinstance(srch.check_self(SPCAS9_NAG, 3, 3, SPCAS9, srch.PairTable(good, (1, 2), pam))[4], srch.PairScheme)


def _table_text(pair, offsets, pam, skip=None):
    lines = ["# a pair table"]
    if offsets:
        lines.append("pam-offsets " + " ".join(str(o) for o in offsets) + "   # inside the PAM")
        k = len(offsets)
        for i, v in enumerate(pam):
            if v:
                lines.append("pam %s %r" % ("".join("ACGT"[(i >> (2 * (k - 1 - j))) & 3] for j in range(k)), float(v)))
    for g in range(pair.shape[0]):
        for a in range(4):
            for b in range(4):
                if a != b and (g, a, b) != skip:
                    lines.append("pair %d %s %s %r  # g, query, site" % (g, "ACGT"[a], "acgt"[b], float(pair[g, a, b])))
    return "\n".join(lines) + "\n"


def test_parse_pair_table():
    E = srch.SearchInputError
    t, pair, offsets, pam = _table(SPCAS9_NAG, 3)
    got = srch.parse_pair_table(_table_text(pair, offsets, pam))
    sc, want = srch.make_scheme(SPCAS9_NAG, 3, got), srch.make_scheme(SPCAS9_NAG, 3, t)
    assert (sc.pair == want.pair).all() and sc.pam_offsets == (1, 2) and (sc.pam == want.pam).all()
    assert (pam == 0).any()  # an unlisted combination is 0
    none = srch.parse_pair_table(_table_text(pair, (), None).encode())
    assert none.pam is None and tuple(none.pam_offsets) == () and srch.make_scheme(SPCAS9, 3, none).pam.tolist() == [1.0]
    with pytest.raises(E):  # a missing pair entry
        srch.parse_pair_table(_table_text(pair, offsets, pam, skip=(7, 2, 1)))
    text = _table_text(pair, offsets, pam)
    for bad in (text + "pair 3 A C 0.5\n", text + "pair 3 A C\n", text + "pair x A C 0.5\n", text + "pair 3 A N 0.5\n",
                text + "pair 40 A C 0.5\n", text + "pam TT 0.5\n", text + "pam A 0.5\n", text + "pam-offsets 1 2\n", text + "weights 1\n",
                text + "pair 3 A C zero\n", "pam-offsets 1 2\npam AG 0.25\n", _table_text(pair, (), None) + "pam AG 0.5\n"):
        with pytest.raises(E):
            srch.parse_pair_table(bad)
    with pytest.raises(E):  # a table for 20 positions on a guide region of 21
        srch.make_scheme(SACAS9, 6, got)
    with pytest.raises(E):  # values are checked against the pattern, not by the parser alone
        srch.make_scheme(SPCAS9, 3, srch.parse_pair_table(text.replace("pam-offsets 1 2", "pam-offsets 0 2")))
    with pytest.raises(E):
        srch.make_scheme(SPCAS9, 3, srch.parse_pair_table(text.replace("pam TT 1.0", "pam TT 1.5") + "pair 0 A A 0.5\n"))


def _synthetic_cfd(rng):
    """The two dictionaries in the publication's key format, with synthetic numbers."""
    mm = {}
    for pos in range(1, 21):
        for r in "ACGU":
            for d in "ACGT":
                if ("T" if r == "U" else r) != cfd_to_table.COMPLEMENT[d]:  # (a match has no entry)
                    mm["r%s:d%s,%d" % (r, d, pos)] = round(float(rng.random()), 6)
    pam = {a + b: round(float(rng.random()), 6) for a in "ACGT" for b in "ACGT"}
    pam["GG"] = 1.0
    return mm, pam


def test_converter_on_a_synthetic_dictionary(tmp_path):
    mm, pam = _synthetic_cfd(np.random.default_rng(3))
    assert len(mm) == 240
    (tmp_path / "mm.pkl").write_bytes(pickle.dumps(mm))
    (tmp_path / "pam.json").write_text(json.dumps(pam))
    out = tmp_path / "cfd.txt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cfd_to_table.py"), str(tmp_path / "mm.pkl"), str(tmp_path / "pam.json"),
                        "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sc = srch.make_scheme(SPCAS9_NAG, 3, srch.parse_pair_table(out.read_text()))
    assert sc.pam_offsets == (1, 2) and sc.pair.shape == (20, 4, 4)
    # rU:dG,20: the guide's T (U as RNA) facing a site C (d is its complement), next to the PAM
    assert sc.pair[19, "ACGT".index("T"), "ACGT".index("C")] == mm["rU:dG,20"]
    assert sc.pair[0, "ACGT".index("A"), "ACGT".index("G")] == mm["rA:dC,1"]
    assert sc.pair[4, "ACGT".index("G"), "ACGT".index("T")] == mm["rG:dA,5"]
    assert sc.pam["ACGT".index("A") * 4 + "ACGT".index("G")] == pam["AG"] and sc.pam[2 * 4 + 2] == 1.0
    # refusals: a key outside the format, a missing entry
    bad = dict(mm)
    bad["rX:dG,20"] = 0.5
    with pytest.raises(ValueError):
        cfd_to_table.convert(bad, pam)
    short = dict(mm)
    del short["rU:dG,20"]
    with pytest.raises(ValueError):
        cfd_to_table.convert(short, pam)
    with pytest.raises(ValueError):
        cfd_to_table.convert(mm, {"NGG": 1.0})
    (tmp_path / "short.json").write_text(json.dumps(short))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cfd_to_table.py"), str(tmp_path / "short.json"), str(tmp_path / "pam.json"),
                        "-o", str(tmp_path / "no.txt")], capture_output=True, text=True)
    assert r.returncode == 2 and not (tmp_path / "no.txt").exists()


def test_cli_refuses_bad_table_input_before_the_gpu(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">c1\nACGT\n")
    gd = tmp_path / "g.txt"
    gd.write_text("ACGTACGTACGTACGTACGT\n")
    pamq = tmp_path / "pam.txt"
    pamq.write_text("ACGTACGTACGTACGTACGTNGG\n")
    t, pair, offsets, pam = _table(SPCAS9_NAG, 1)
    good = tmp_path / "t.txt"
    good.write_text(_table_text(pair, offsets, pam))
    missing = tmp_path / "missing.txt"
    missing.write_text(_table_text(pair, offsets, pam, skip=(3, 0, 1)))
    big = tmp_path / "big.txt"
    big.write_text(_table_text(pair, offsets, pam).replace("pair 3 A c ", "pair 3 A c 1"))  # a value above 1
    on_n = tmp_path / "on_n.txt"
    on_n.write_text(_table_text(pair, offsets, pam).replace("pam-offsets 1 2", "pam-offsets 0 2"))
    w20 = tmp_path / "w20.txt"
    w20.write_text(" ".join(["0.5"] * 20) + "\n")
    out, cnt = tmp_path / "o.tsv", tmp_path / "c.tsv"
    base = ["--pattern", SPCAS9_NAG, "--guides", str(gd), "--pam-length", "3", "-o", str(out)]
    self_base = ["--pattern", SPCAS9_NAG, "--self", "--pam-length", "3", "-m", "2", "-o", str(out)]
    cases = [["--pattern", SPCAS9_NAG, "--guides", str(gd), "-o", str(out), "--score-table", str(good)],  # no --pam-length
             base + ["--score-table", str(good), "--score", "hsu2013"], base + ["--score-table", str(good), "--weights", str(w20)],
             base + ["--score-table", str(missing)], base + ["--score-table", str(big)], base + ["--score-table", str(on_n)],
             base + ["--score-table", str(tmp_path / "none.txt")], base + ["--score-table", str(w20)],
             ["--pattern", SPCAS9_NAG, "--guides", str(pamq), "--pam-length", "3", "-o", str(out), "--score-table", str(good)],
             ["--pattern", SACAS9, "--guides", str(gd), "--pam-length", "6", "-o", str(out), "--score-table", str(good)],  # G = 21
             base + ["--score-table", str(good), "--no-sites", "--counts", str(cnt)],
             self_base + ["--score-table", str(missing)], self_base + ["--score-table", str(on_n)],
             self_base + ["--score-table", str(good), "--score", "hsu2013"],
             ["--pattern", SACAS9, "--self", "--pam-length", "6", "-m", "2", "-o", str(out), "--score-table", str(good)]]
    for args in cases:
        cmd = [sys.executable, "-m", "cropsr_amd.search", "-f", str(fa)] + args
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 2 and "error:" in r.stderr, (args, r.stderr)
        assert not out.exists() and not cnt.exists()


# ------------------------------------------------------------------ TSV bytes (CPU)
def test_scored_tsv_bytes():
    queries, counts, sites = _tsv_case()
    names, contig_names = ["g1"], ["c1", "c2"]
    pair = np.full((20, 4, 4), 0.5)
    pair[11, 3, 2] = 0.8   # the second site: query T facing a non-base at g = 11 ...
    pair[19, 0, 3] = 0.25  # ... and query A facing T at g = 19
    pam = np.zeros(16)
    pam[2 * 4 + 2] = 0.5   # GG
    sc = srch.make_scheme(SPCAS9, 3, srch.PairTable(pair, (1, 2), pam))
    v = srch.hit_values(sites, queries, TSV_GENOME, sc)
    assert v.tolist() == [0, 0]  # no mismatches; a non-base at a mismatching position
    # the same genome with a base there
    genome = [TSV_GENOME[0], TSV_GENOME[1].replace(b"N", b"C")]  # '-' strand: the oriented site holds G at g = 11
    counts, s = ref.search(genome, SPCAS9, queries, 2)
    sites = _sites_array(s)
    v = srch.hit_values(sites, queries, genome, sc)
    h = 0.8 * 0.25 * 0.5
    assert v.tolist() == [0, int(np.rint(h * ONE))]
    res = srch.SearchResult(counts, sites, (0, 0), np.array([int(v.sum())], dtype=np.uint64))
    text = srch.format_scored_sites(names, queries, contig_names, genome, res, sc)
    assert text == ("name\tquery\tcontig\tposition\tstrand\tmismatches\tsite\thit_score\n"
                    "g1\tACGTACGTACGTACGTACGANNN\tc1\t2\t+\t0\tACGTACGTACGTACGTACGAAGG\t\n"
                    "g1\tACGTACGTACGTACGTACGANNN\tc2\t0\t-\t2\tACGTACGTACGgACGTACGtAGG\t%.6f\n" % h)
    ctext = srch.format_scored_counts(names, queries, res)
    assert ctext == ("name\tquery\tmm0\tmm1\tmm2\thit_sum\tspecificity\n"
                     "g1\tACGTACGTACGTACGTACGANNN\t1\t0\t1\t%.6f\t%.6f\n" % (h, 1.0 / (1.0 + h)))
    rows = _as_tuples(sites)
    strings = [srch.site_string(genome[k], pos, "+-"[st], queries[q]) for q, k, pos, st, _ in rows]
    assert text == sref.format_sites(names, queries, contig_names, rows, strings, v.tolist())
    assert ctext == sref.format_counts(names, queries, counts, [int(v.sum())])


# ------------------------------------------------------------------ ABI and ISA (CPU)
def test_library_declares_pair_abi():
    L = nat.lib()
    with open(os.path.join(ROOT, "include", "cropsr_hip.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    assert ("int crp_search_set_pair_scheme(crp_search *search, const double *pair, int n_factor, int pam_side, const int *pam_offsets, "
            "int n_pam_offsets, const double *pam);") in header
    assert ("int crp_search_self_set_pair_scheme(crp_search_self *self, const double *pair, int n_factor, const int *pam_offsets, "
            "int n_pam_offsets, const double *pam);") in header
    assert hasattr(L, "crp_search_set_pair_scheme") and hasattr(L, "crp_search_self_set_pair_scheme")
    assert nat.SIGNATURES["crp_search_set_pair_scheme"] == (ctypes.c_int, [ctypes.c_void_p, nat.f64p, ctypes.c_int, ctypes.c_int, nat.i32p,
                                                                           ctypes.c_int, nat.f64p])
    assert nat.SIGNATURES["crp_search_self_set_pair_scheme"] == (ctypes.c_int, [ctypes.c_void_p, nat.f64p, ctypes.c_int, nat.i32p, ctypes.c_int,
                                                                                nat.f64p])
    assert re.search(r"#define CRP_SEARCH_PAIR_MAX_PAM %d\b" % nat.SEARCH_PAIR_MAX_PAM, header)
    assert nat.SEARCH_PAIR_MAX_PAM == srch.MAX_PAM_OFFSETS == 3
    assert L.crp_abi_version() == 6 == nat.ABI_VERSION


def test_pair_kernel_static_isa(search_isa):  # noqa: F811
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    scored = _figures(search_isa, "search_score_compare_kernel")
    pair = _figures(search_isa, "search_pair_compare_kernel")
    print("search_score_compare_kernel", scored, "\nsearch_pair_compare_kernel", pair)
    assert pair["scratch"] == 0 and pair["vgpr_spills"] == 0
    assert pair["loop_valu"] == scored["loop_valu"]  # the sibling kernel of the same build, not a constant
    assert pair["f64"] > 0 and pair["atomics_x2"] == scored["atomics_x2"]
    asm, remarks = search_isa
    mangled = next(m.group(1) for m in re.finditer(r"^(_ZN3crp\S*search_pair_compare_kernelE\S*):", asm, re.M))
    res = isa.resources(remarks, mangled)
    assert int(res["SGPRs Spill"]) == 0
    # DESIGN section 15 quotes what the test prints
    assert "search_pair_compare_kernel: %d VGPRs, %s waves per SIMD, %d VALU" % (pair["vgprs"], res["Occupancy [waves/SIMD]"], pair["valu"]) in design
    assert "no-hit loop of %d VALU" % pair["loop_valu"] in design


def test_self_pair_kernel_static_isa(self_isa):  # noqa: F811
    asm, remarks = self_isa
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    fig = {}
    for name in (r"search_self_compare_kernelILb1E", r"search_self_pair_compare_kernelE"):
        mangled = next(m.group(1) for m in re.finditer(r"^(_ZN3crp\S*\d+%s\S*):" % name, asm, re.M))
        res = isa.resources(remarks, mangled)
        assert int(res["ScratchSize [bytes/lane]"]) == 0 and int(res["VGPRs Spill"]) == 0 and int(res["SGPRs Spill"]) == 0
        blocks = isa.blocks_of(asm, mangled)
        loop = [b for b in blocks if sum(i.startswith("v_bcnt_u32_b32") for i in b[3]) == 8]  # 8 pairs per trip
        assert len(loop) == 1 and loop[0][3][-1].startswith("s_cbranch")
        ins = loop[0][3]
        assert sum(i.startswith("s_load_dwordx8") for i in ins) == 3
        assert not any(i.startswith(("global_", "flat_", "buffer_", "ds_", "scratch_")) for i in ins)
        fig[name] = (int(res["VGPRs"]), res["Occupancy [waves/SIMD]"], isa.counts(ins)["valu"])
        print(name, "%d VGPRs, %s waves per SIMD, no-hit loop: %d VALU per 8 pairs" % fig[name])
    sibling, pair = fig["search_self_compare_kernelILb1E"], fig["search_self_pair_compare_kernelE"]
    assert pair[2] == sibling[2]  # the sibling kernel of the same build, not a constant
    assert "search_self_pair_compare_kernel: %d VGPRs, %s waves per SIMD" % pair[:2] in design


# ------------------------------------------------------------------ the library (GPU)
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def _case(pattern, seed, n_queries=20, chars=300_000, n_contigs=14, max_mm=8):
    rng = np.random.default_rng(2000 + seed)
    P = P_OF[pattern]
    G = len(pattern) - P
    queries = [srch.check_query(pattern, "".join(rng.choice(list("ACGT"), G)), P) for _ in range(n_queries)]
    queries[-1] = srch.check_query(pattern, "".join(rng.choice(list("ACGT"), G - 2)), P)  # a short guide next to the PAM
    contigs = _planted_genome(rng, pattern, chars, n_contigs, queries[:14] + queries[-1:], max_mm)
    # one more contig: query 0's site with a non-base at a mismatching position, on both strands
    lo, hi, pam3 = srch.guide_region(pattern, P)
    site = [q if q != "N" else str(rng.choice(list(ref.IUPAC_SETS.get(c, "ACGT")))) for q, c in zip(queries[0], pattern)]
    site[lo + 5], site[lo + 9] = "N", "ACGT"[("ACGT".index(site[lo + 9]) + 1) % 4]
    s = "".join(site).encode()
    contigs.append(b"TT" + s + b"TTTT" + s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1] + b"TT")
    return P, queries, contigs


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,seed", [(SPCAS9, 1), (SPCAS9_NAG, 2), (SACAS9, 3), (CAS12A, 4), (CAS12A_20, 5)])
def test_gpu_hit_sums_match_reference(engine, pattern, seed):
    P, queries, contigs = _case(pattern, seed)
    table, pair, offsets, pam = _table(pattern, seed)
    scheme = srch.make_scheme(pattern, P, table)
    g = engine.genome(contigs)
    try:
        for M in (4, 8):
            want_counts, s, want_sum = pref.search(contigs, pattern, queries, M, P, pair, offsets, pam)
            res = g.search(pattern, queries, M, pam_len=P, score=table)
            print(pattern, M, "hit_sum", [int(x) for x in res.hit_sum], "want", want_sum)
            assert res.hit_sum.dtype == np.uint64 and [int(x) for x in res.hit_sum] == want_sum, (pattern, M)
            assert sum(want_sum) > 0 and sum(1 for x in want_sum if x) >= 10
            assert res.specificity.tolist() == sref.specificity(want_sum)
            plain = g.search(pattern, queries, M, pam_len=P)
            assert (res.counts == plain.counts).all() and (res.counts == want_counts).all()
            assert (res.sites == plain.sites).all() and res.sites.size == int(want_counts.sum())
            # the planted non-base sites are counted and worth nothing
            zero = (s["query"] == 0) & (s["contig"] == len(contigs) - 1) & (s["mismatches"] > 0)
            assert int(zero.sum()) == 2 and (s["value"][zero] == 0).all()
            # the device's sums against the host's values of the fetched sites: another route to the same integers
            v = srch.hit_values(res.sites, queries, contigs, scheme)
            assert v.tolist() == s["value"].tolist()
            for q in range(len(queries)):
                assert sum(int(x) for x in v[res.sites["query"] == q].tolist()) == int(res.hit_sum[q]), (pattern, M, q)
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_hit_sums_do_not_depend_on_the_cut(engine):
    rng = np.random.default_rng(32)
    queries = _queries_for(rng, SPCAS9_NAG, 300)
    contigs = _planted_genome(rng, SPCAS9_NAG, 700_000, 20, queries[:40], 4)
    table, pair, offsets, pam = _table(SPCAS9_NAG, 7)
    want_counts, s, want_sum = pref.search(contigs, SPCAS9_NAG, queries, 4, 3, pair, offsets, pam)
    assert int(want_counts.sum()) > 16 * 4
    one = engine.genome(contigs)
    many = engine.genome(contigs, max_words=3000)
    try:
        assert len(many.arenas) > 3 and len(one.arenas) == 1
        uncut = one.search(SPCAS9_NAG, queries, 4, pam_len=3, score=table)
        assert [int(x) for x in uncut.hit_sum] == want_sum and (uncut.counts == want_counts).all()
        for g, budget in ((many, None), (one, 1), (many, 1)):
            res = g.search(SPCAS9_NAG, queries, 4, pam_len=3, score=table, budget=budget)
            assert (res.hit_sum == uncut.hit_sum).all() and (res.counts == uncut.counts).all(), budget
            assert (res.sites == uncut.sites).all()
        h = srch.ArenaSearch(one.arenas[0], SPCAS9_NAG)
        try:
            h.set_scheme(srch.make_scheme(SPCAS9_NAG, 3, table))
            h.set_limits(batch_queries=7, first_site_slots=16)
            st, counts, n, hit_sum = h.run_scored(queries, 4, 1 << 40)
            assert st == nat.CRP_OK and n == int(want_counts.sum()) and (counts == want_counts).all()
            assert h.stats()["compare_launches"] == 2 * 43  # the site list grew once: a hit must not be added twice
            assert [int(x) for x in hit_sum] == want_sum
        finally:
            h.close()
    finally:
        one.close()
        many.close()


@pytest.mark.gpu
def test_gpu_score_only_and_abi_states(engine):
    P, queries, contigs = _case(SPCAS9_NAG, 9, n_queries=12, chars=200_000, n_contigs=6, max_mm=4)
    queries.append("N" * 23)  # every candidate hits with n = 0
    table, pair, offsets, pam = _table(SPCAS9_NAG, 9)
    want_counts, s, want_sum = pref.search(contigs, SPCAS9_NAG, queries, 4, 3, pair, offsets, pam)
    assert want_sum[-1] == 0 and int(want_counts[-1, 0]) > 1000 and sum(want_sum) > 0
    g = engine.genome(contigs)
    L = nat.lib()
    try:
        res = g.search(SPCAS9_NAG, queries, 4, pam_len=3, score=table, sites=False)
        assert res.sites.size == 0 and (res.counts == want_counts).all() and [int(x) for x in res.hit_sum] == want_sum
        h = srch.ArenaSearch(g.arenas[0], SPCAS9_NAG)
        try:
            sc = srch.make_scheme(SPCAS9_NAG, 3, table)
            blob = "".join(queries).encode()
            Q = len(queries)
            counts = np.zeros((Q, 5), dtype=np.uint32)
            hit_sum = np.zeros(Q, dtype=np.uint64)
            n = ctypes.c_uint64()
            args = (blob, Q, 4, 0, counts.ctypes.data_as(nat.u32p), ctypes.byref(n), hit_sum.ctypes.data_as(nat.u64p))
            assert L.crp_search_run_scored(h._h, *args) == nat.CRP_ERR_STATE  # nothing set
            h.set_scheme(sc)
            assert L.crp_search_run_scored(h._h, *args) == nat.CRP_ERR_CAPACITY  # site_cap 0: exact counts and sums
            assert n.value == int(want_counts.sum()) and (counts == want_counts).all() and [int(x) for x in hit_sum] == want_sum
            # setting one scheme clears the other, either way round
            hsu = srch.make_scheme(SPCAS9_NAG, 3, "hsu2013")
            h.set_scheme(hsu)
            st, c, m, hs_hsu = h.run_scored(queries, 4, 0)
            factor, shape = sref.tables(sref.W_HSU)
            assert [int(x) for x in hs_hsu] == sref.search(contigs, SPCAS9_NAG, queries, 4, 3, factor, shape)[2]
            h.set_scheme(sc)
            st, c, m, hs = h.run_scored(queries, 4, 0)
            assert [int(x) for x in hs] == want_sum
            h.set_scheme(None)
            assert L.crp_search_run_scored(h._h, *args) == nat.CRP_ERR_STATE
            # misuse: a refused table sets nothing
            p_ok, G, offs, k, pam_p = sc.native_args()
            three, five = nat.SEARCH_PAM_3PRIME, nat.SEARCH_PAM_5PRIME
            assert L.crp_search_set_pair_scheme(None, p_ok, 20, three, offs, 2, pam_p) == nat.CRP_ERR_INVALID
            assert L.crp_search_set_pair_scheme(h._h, p_ok, 20, 2, offs, 2, pam_p) == nat.CRP_ERR_INVALID
            assert L.crp_search_set_pair_scheme(h._h, p_ok, 20, five, offs, 2, pam_p) == nat.CRP_ERR_INVALID  # the region is not all N there
            assert L.crp_search_set_pair_scheme(h._h, p_ok, 0, three, offs, 2, pam_p) == nat.CRP_ERR_INVALID
            assert L.crp_search_set_pair_scheme(h._h, p_ok, 20, three, offs, 4, pam_p) == nat.CRP_ERR_INVALID
            assert L.crp_search_set_pair_scheme(h._h, p_ok, 20, three, None, 2, pam_p) == nat.CRP_ERR_INVALID
            for bad_offs in ((0, 2), (2, 1), (1, 1), (1, 3), (-1, 2)):
                bo = np.array(bad_offs, dtype=np.intc)
                assert L.crp_search_set_pair_scheme(h._h, p_ok, 20, three, bo.ctypes.data_as(nat.i32p), 2, pam_p) == nat.CRP_ERR_INVALID
            for bad in (1.5, -0.5, float("nan"), float("inf")):
                pb = sc.pair.copy().reshape(-1)
                pb[(3 * 4 + 1) * 4 + 2] = bad
                assert L.crp_search_set_pair_scheme(h._h, pb.ctypes.data_as(nat.f64p), 20, three, offs, 2, pam_p) == nat.CRP_ERR_INVALID
                mb = sc.pam.copy()
                mb[6] = bad
                assert L.crp_search_set_pair_scheme(h._h, p_ok, 20, three, offs, 2, mb.ctypes.data_as(nat.f64p)) == nat.CRP_ERR_INVALID
            assert L.crp_search_run_scored(h._h, *args) == nat.CRP_ERR_STATE
            assert L.crp_search_set_pair_scheme(h._h, p_ok, 20, three, offs, 2, pam_p) == nat.CRP_OK
            base_in_pam = ("A" * 20 + "NGG").encode()
            assert L.crp_search_run_scored(h._h, base_in_pam, 1, 4, 0, None, ctypes.byref(n), hit_sum.ctypes.data_as(nat.u64p)) == nat.CRP_ERR_INVALID
            st, c, m = h.run(queries, 4, 1 << 40)  # an unscored run on the same handle is untouched by the table
            assert st == nat.CRP_OK and (c == want_counts).all()
        finally:
            h.close()
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_scored_bulge_search(engine):
    P, queries, contigs = _case(SPCAS9_NAG, 12, n_queries=10, chars=150_000, n_contigs=6, max_mm=4)
    table, pair, offsets, pam = _table(SPCAS9_NAG, 12)
    g = engine.genome(contigs)
    try:
        plain = g.search(SPCAS9_NAG, queries, 4, pam_len=3, score=table)
        unscored = g.search_bulges(SPCAS9_NAG, queries, 4, 3, 1, 1)
        res = g.search_bulges(SPCAS9_NAG, queries, 4, 3, 1, 1, score=table)
        assert (res.hit_sum == plain.hit_sum).all() and int(plain.hit_sum.sum()) > 0  # kind none only
        assert [int(x) for x in res.hit_sum] == pref.search(contigs, SPCAS9_NAG, queries, 4, 3, pair, offsets, pam)[2]
        assert (res.counts == unscored.counts).all() and (res.sites == unscored.sites).all() and (res.sites["kind"] != 0).any()
        v = srch.hit_values(res.sites, queries, contigs, srch.make_scheme(SPCAS9_NAG, 3, table))
        assert (v[res.sites["kind"] != 0] == 0).all()
        for q in range(len(queries)):
            assert sum(int(x) for x in v[res.sites["query"] == q].tolist()) == int(res.hit_sum[q])
    finally:
        g.close()


def _assert_self_equals_given_guides(g, pattern, P, M, table, gp=None, **kw):
    res = g.search_self(pattern, M, P, guide_pattern=gp, score=table, **kw)
    queries = _queries_of_rows(res, pattern, P)
    ref_res = g.search(pattern, queries, M, pam_len=P, score=table, sites=False)
    want = ref_res.counts.astype(np.int64)
    want[:, 0] -= 1
    assert (res.counts.astype(np.int64) == want).all(), (pattern, M)
    bad = np.nonzero(res.hit_sum != ref_res.hit_sum)[0]
    assert bad.size == 0, (pattern, M, bad[:5], res.hit_sum[bad[:5]], ref_res.hit_sum[bad[:5]])
    return res, ref_res


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,gp,seed", [(SPCAS9, None, 1), (SPCAS9_NAG, SPCAS9, 2), (SACAS9, None, 3), (CAS12A_20, None, 4),
                                             (CAS12A, None, 5)])
def test_gpu_self_search_rows_equal_the_given_guides_search(engine, pattern, gp, seed):
    rng = np.random.default_rng(8000 + seed)
    contigs = _genome(rng, pattern, 60_000, 9, families=40)
    P = P_OF[pattern]
    table, pair, offsets, pam = _table(pattern, seed)
    g = engine.genome(contigs)
    try:
        for M in range(5):
            res, ref_res = _assert_self_equals_given_guides(g, pattern, P, M, table, gp)
            assert len(res.sites) > 200
            if M >= 2:
                assert int(res.counts[:, 1:].sum()) > 100 and int(res.hit_sum.sum()) > 0
            if M == 3:  # and a sample of rows against the loop reference
                rows = rng.choice(len(res.sites), 25, replace=False).tolist()
                queries = _queries_of_rows(res, pattern, P)
                want = pref.search(contigs, pattern, [queries[r] for r in rows], M, P, pair, offsets, pam)[2]
                assert [int(res.hit_sum[r]) for r in rows] == want
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_self_search_does_not_depend_on_the_cut(engine):
    rng = np.random.default_rng(33)
    contigs = _genome(rng, SPCAS9_NAG, 700_000, 20, families=60)
    table = _table(SPCAS9_NAG, 21)[0]
    one = engine.genome(contigs)
    many = engine.genome(contigs, max_words=3000)
    try:
        assert len(many.arenas) >= 3 and len(one.arenas) == 1
        uncut, _ = _assert_self_equals_given_guides(one, SPCAS9_NAG, 3, 4, table, SPCAS9)
        assert int(uncut.hit_sum.sum()) > 0
        cut = many.search_self(SPCAS9_NAG, 4, 3, guide_pattern=SPCAS9, score=table)  # guides of one arena, buckets of another
        low = one.search_self(SPCAS9_NAG, 4, 3, guide_pattern=SPCAS9, score=table, pairs_per_launch=1 << 18)
        both = many.search_self(SPCAS9_NAG, 4, 3, guide_pattern=SPCAS9, score=table, pairs_per_launch=1 << 18)
        assert low.stats["compare_launches"] >= 20
        for res in (cut, low, both):
            assert (res.sites == uncut.sites).all() and (res.guides == uncut.guides).all()
            assert (res.counts == uncut.counts).all() and (res.hit_sum == uncut.hit_sum).all()
        # the other scheme on the same genome is untouched
        hsu = one.search_self(SPCAS9_NAG, 4, 3, guide_pattern=SPCAS9, score="hsu2013")
        assert (hsu.counts == uncut.counts).all() and (hsu.hit_sum != uncut.hit_sum).any()
    finally:
        one.close()
        many.close()


@pytest.mark.gpu
def test_gpu_cli_end_to_end(tmp_path):
    genome = [TSV_GENOME[0], TSV_GENOME[1].replace(b"N", b"C"), b"TTACGTACGTACGTACGTACGCAAGTT"]
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">c1 first\n" + genome[0][:14] + b"\n" + genome[0][14:] + b"\n>c2\n" + genome[1] + b"\n>c3\n" + genome[2] + b"\n")
    gd = tmp_path / "guides.txt"
    gd.write_text("ACGTACGTACGTACGTACGA g1\nCGTACGTACGTACGTACG g2\n")
    names = ["g1", "g2"]
    queries = [srch.check_query(SPCAS9_NAG, "ACGTACGTACGTACGTACGA", 3), srch.check_query(SPCAS9_NAG, "CGTACGTACGTACGTACG", 3)]
    table, pair, offsets, pam = _table(SPCAS9_NAG, 40)
    pam[0 * 4 + 2] = 0.25  # AG: the site of c3
    tf = tmp_path / "table.txt"
    tf.write_text(_table_text(pair, offsets, pam))
    counts, s, hit_sum = pref.search(genome, SPCAS9_NAG, queries, 3, 3, pair, offsets, pam)
    rows = list(zip(*[s[f].tolist() for f in ref.SITE_FIELDS]))
    strings = [srch.site_string(genome[k], pos, "+-"[st], queries[q]) for q, k, pos, st, _ in rows]
    assert sum(hit_sum) > 0 and any(k == 2 for _, k, _, _, _ in rows)
    base = [sys.executable, "-m", "cropsr_amd.search", "-f", str(fa), "--pattern", SPCAS9_NAG, "--pam-length", "3", "-m", "3",
            "--score-table", str(tf)]
    out, cnt = tmp_path / "sites.tsv", tmp_path / "counts.tsv"
    r = subprocess.run(base + ["--guides", str(gd), "-o", str(out), "--counts", str(cnt)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert out.read_text() == sref.format_sites(names, queries, ["c1", "c2", "c3"], rows, strings, s["value"].tolist())
    assert cnt.read_text() == sref.format_counts(names, queries, counts, hit_sum)
    only = tmp_path / "only.tsv"
    out.unlink()
    r = subprocess.run(base + ["--guides", str(gd), "--no-sites", "--counts", str(only)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert only.read_text() == cnt.read_text() and not out.exists()
    # --self: every row is the given-guides search of its own query
    r = subprocess.run(base + ["--self", "--guide-pattern", SPCAS9, "-o", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln.split("\t") for ln in out.read_text().splitlines()]
    assert lines[0] == ["contig", "position", "strand", "guide", "n0", "n1", "n2", "n3", "hit_sum", "specificity"] and len(lines) > 2
    for row in lines[1:]:
        q = srch.check_query(SPCAS9_NAG, row[3], 3)
        c, _, hs = pref.search(genome, SPCAS9_NAG, [q], 3, 3, pair, offsets, pam)
        assert [int(x) for x in row[4:8]] == [int(c[0][0]) - 1] + [int(x) for x in c[0][1:]]
        assert row[8] == "%.6f" % (hs[0] / float(ONE)) and row[9] == "%.6f" % (1.0 / (1.0 + hs[0] / float(ONE)))
