"""--pairs-distinct: KP pairs per gene that share no guide (cropsr_amd/select.py, csrc/crp_select_pairs_distinct.hip,
DESIGN.md section 29).  The definition is restated twice in tests/select_pairs_distinct_reference.py -- in numpy by rounds
and as the plain walk with a set of taken rows; the genome and its genes are tests/select_pairs_cases.py's, and the helpers
that build its arenas are tests/test_select_pairs.py's, unchanged.

  distinct   walk the qualifying pairs of a gene in the pairs' order; take a pair iff neither of its two
             rows is a row of a pair already taken; stop at KP taken.  A row is a table row of one strand (row | strand <<
             31); a row taken as a shuts out pairs that offer it as b, and the other way round."""
import csv
import ctypes
import hashlib
import io
import json
import os

import numpy as np
import pytest

from conftest import OracleBackend

import select_pairs_cases as pcases
import select_pairs_distinct_reference as dref
import select_pairs_reference as pref
import select_reference as ref
import test_select_pairs as tp
from cropsr_amd import _native as nat
from cropsr_amd import annotate, cli, properties, repair
from cropsr_amd import search as srch
from cropsr_amd import select as sel

KPS = (1, 5, 64)
NONE = 0xFFFFFFFF
WINDOWS = tp.WINDOWS
ANY_50_500, ANY_1_40, OUT_30_54 = (50, 500, 0xF, False), (1, 40, 0xF, False), (30, 54, pref.PAM_OUT, False)
# without --pairs-distinct, of the commit before this option existed: --select 5 --select-min-score 0.3 --select-pairs 4
# --pairs-frameshift --pairs-min-distance 40 --pairs-max-distance 700 over the oracle backend
MD5_MAIN, MD5_SELECTED, MD5_PAIRS = "b496e88bec88c12150b6ff1781733727", "84319f73e0e5d9b445f24329167a9d5a", "a854a539008d087f2a3f813d3032c391"


@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    c = pcases.build(oracle)
    d = tmp_path_factory.mktemp("select_pairs_distinct")
    c["gff_path"] = str(d / "genes.gff")
    with open(c["gff_path"], "w") as f:
        f.write(c["gff"])
    c["fasta_path"] = str(d / "genome.fa")
    with open(c["fasta_path"], "w") as f:  # one line per contig: read unformatted (dec = 0)
        f.write("".join(">%s\n%s\n" % (n, t.decode()) for n, t in zip(c["names"], c["contigs"]))[:-1])
    c["annotation"] = annotate.Annotation(c["gff_path"])
    c["genes"] = ref.gff_genes(c["gff"])
    return c


@pytest.fixture(scope="module")
def host(case):
    """The case genome as one host arena: tables, layout rows, their ids, and a cache of ordered pair lists per window."""
    tables, entries, offsets = tp._host_arena(case)
    lo, hi, gene = ref.layout(case["genes"], entries, 0)
    return dict(tables=tables, lo=lo, hi=hi, gene=gene, ids=[case["ids"][int(x)] for x in gene], ordered={})


def _ordered(host, window):
    if window not in host["ordered"]:
        dmin, dmax, mask, fs = window
        host["ordered"][window] = dref.ordered_pairs(host["tables"], host["lo"], host["hi"], dmin, dmax, mask, fs)
    return host["ordered"][window]


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("n_pass", "n_pairs", "n_distinct", "pairs")):
        assert np.array_equal(np.asarray(g, np.uint64), np.asarray(w, np.uint64)), (what, name)


def _first(want, KP):
    """The result at KP from the reference's at 64: the walk never goes back, so the first KP picks are a prefix."""
    return want[0], want[1], np.minimum(want[2], KP), want[3][:, :KP]


# ---------------------------------------------------------------------------------------------- without a GPU
def test_numpy_by_rounds_equals_the_plain_walk(host):
    tables, lo, hi = host["tables"], host["lo"], host["hi"]
    ok = pref.eligible_numpy(tables)
    size = np.array([len(tp._rows_of(tables, a, b, ok)) for a, b in zip(lo, hi)])
    pick = np.flatnonzero(size <= 300)  # (the walk's pair loop is quadratic)
    assert pick.size >= 30 and size[pick].max() > 129 and (size[pick] == 0).any()
    rng = np.random.default_rng(9)
    spec, cds = {}, {}
    for s in ("plus", "minus"):
        n = len(tables["pos_" + s])
        counts = rng.integers(0, 3, (n, 4)).astype(np.uint32)
        sums = rng.integers(0, 1 << 33, n).astype(np.uint64)
        un = rng.random(n) < 0.1
        counts[un], sums[un] = NONE, np.uint64(0xFFFFFFFFFFFFFFFF)
        spec["counts_" + s], spec["sum_" + s] = counts, sums
        feat = rng.integers(0, 9, n).astype(np.uint32)
        feat[rng.random(n) < 0.3] = NONE
        cds["feat_" + s] = feat
    cds["flags"] = (rng.random(9) < 0.6).astype(np.uint8)
    spec.update(max_mm0=1, max_hit_sum=1 << 32)
    also = dict(plus=rng.random(len(tables["pos_plus"])) < 0.8, minus=rng.random(len(tables["pos_minus"])) < 0.8)
    taken = 0
    for dmin, dmax, mask, fs in WINDOWS:
        for KP in (5, 64):
            a = dref.distinct_numpy(tables, lo[pick], hi[pick], KP, dmin, dmax, mask, fs)
            b = dref.distinct_walk(tables, lo[pick], hi[pick], KP, dmin, dmax, mask, fs)
            _same(a, b, (dmin, dmax, mask, fs, KP))
            taken += int(a[2].sum())
    assert taken > 2000
    a = dref.distinct_numpy(tables, lo[pick], hi[pick], 64, 20, 400, 0xF, True, 0.3, spec, cds, also)
    b = dref.distinct_walk(tables, lo[pick], hi[pick], 64, 20, 400, 0xF, True, 0.3, spec, cds, also)
    _same(a, b, "all terms")
    assert a[2].sum() > 30 and (a[0] < dref.distinct_numpy(tables, lo[pick], hi[pick], 1, 20, 400)[0]).any()


def test_counts_order_and_kp_one(host):
    """For every window: n_pass and n_pairs are the pair selection's, KP = 1 is the pair selection's KP = 1, no row occurs
    twice in a gene's picks, the picks are in the pairs' order, and n_distinct keeps its bound."""
    tables, lo, hi = host["tables"], host["lo"], host["hi"]
    for window in WINDOWS:
        dmin, dmax, mask, fs = window
        plain = pref.pairs_numpy(tables, lo, hi, 1, dmin, dmax, mask, fs)
        one = dref.distinct_numpy(tables, lo, hi, 1, dmin, dmax, mask, fs)
        assert np.array_equal(one[0], plain[0]) and np.array_equal(one[1], plain[1]) and np.array_equal(one[3], plain[2])
        assert np.array_equal(one[2], (plain[1] > 0).astype(np.uint32))
        ranks = []
        got = dref.distinct_numpy(tables, lo, hi, 64, dmin, dmax, mask, fs, ranks=ranks)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
        assert (got[2] <= np.minimum(np.minimum(64, got[1]), got[0] // 2)).all()
        for g, r in enumerate(ranks):
            rows_g = got[3][g][:got[2][g]].ravel().tolist()
            assert len(set(rows_g)) == len(rows_g) and NONE not in rows_g and r == sorted(r)
            assert (got[3][g][got[2][g]:] == NONE).all()
            for KP in (1, 5):  # a smaller KP is a prefix
                assert dref.rounds_of(*_ordered(host, window)[g][1:], KP) == r[:KP]


def _struck_out(A, B, KP):
    """The plain top KP with every pair struck out that shares a row with ANY better pair: NOT the definition."""
    kept, seen = [], set()
    for i in range(min(KP, A.size)):
        if int(A[i]) not in seen and int(B[i]) not in seen:
            kept.append(i)
        seen.update((int(A[i]), int(B[i])))
    return kept


def _chained(A, B, ranks):
    """The picks that share a row with a better pair the walk rejected."""
    picks = set(ranks)
    return [i for i in ranks if any(j not in picks and {int(A[j]), int(B[j])} & {int(A[i]), int(B[i])} for j in range(i))]


def _figures(host, window, KP):
    """Over the layout rows: (rows whose picks differ from the plain top KP, rows that run out of distinct pairs before
    min(KP, n_pairs), the deepest plain rank a pick comes from and its gene, the rejections by kind, summed)."""
    differ = early = 0
    deepest, kinds = (0, None), {}
    for g, (_, A, B) in enumerate(_ordered(host, window)):
        r = dref.rounds_of(A, B, KP)
        differ += r != list(range(min(KP, A.size)))
        early += len(r) < min(KP, A.size)
        if r and r[-1] > deepest[0]:
            deepest = (r[-1], host["ids"][g])
        for kind, n in dref.rejections(A, B, r).items():
            kinds[kind] = kinds.get(kind, 0) + n
    return differ, early, deepest, kinds


def _assert_the_genome_contains_the_cases(host):
    """On the reference's own rows: the counts are pinned, so a genome that has lost a case fails here and does not pass
    quietly.  A rejection is counted under every kind that holds for it, on the walk down to the gene's last pick."""
    ids = host["ids"]
    assert len(ids) == 40
    ok = pref.eligible_numpy(host["tables"])  # genes with 0, 1, 2 and 3 eligible rows
    assert sorted(len(tp._rows_of(host["tables"], a, b, ok)) for a, b in zip(host["lo"], host["hi"]))[:8] == [0, 1, 1, 1, 2, 2, 2, 3]
    differ, early, deepest, kinds = _figures(host, ANY_50_500, 5)
    assert (differ, early, deepest) == (27, 3, (88, "repeat_core"))
    # the four kinds of rejection: shared a, shared b, a row taken as b and offered as a, and the reverse
    assert kinds == {dref.SHARED_A: 208, dref.SHARED_B: 231, dref.B_AS_A: 102, dref.A_AS_B: 116, "both": 31}
    assert _figures(host, ANY_50_500, 64)[:3] == (27, 12, (5895, "p_run64"))  # a pick at a plain rank far beyond 64
    assert _figures(host, ANY_1_40, 5)[:3] == (32, 6, (36, "one_strand"))
    differ, early, deepest, kinds = _figures(host, OUT_30_54, 5)
    assert (differ, early, deepest) == (22, 5, (12, "by_parent"))
    # under pam-out a is always a '-' row and b a '+' row: only the first two kinds can occur
    assert kinds[dref.SHARED_A] == 31 and kinds[dref.SHARED_B] == 17 and kinds[dref.B_AS_A] == kinds[dref.A_AS_B] == kinds["both"] == 0
    by = {i: k for k, i in enumerate(ids)}
    op = _ordered(host, ANY_50_500)

    def gene(name, KP=5):
        n, A, B = op[by[name]]
        r = dref.rounds_of(A, B, KP)
        return n, A, B, r, dref.rejections(A, B, r)

    n, A, B, r, kinds = gene("first_rows")  # all four kinds in one gene
    assert r == [0, 5, 13, 29, 36] and min(kinds[k] for k in (dref.SHARED_A, dref.SHARED_B, dref.B_AS_A, dref.A_AS_B)) > 0
    assert gene("nested")[4]["both"] == 2  # pairs rejected on both of their rows
    n, A, B, r, _ = gene("p_run5")  # ends early: 2 of its 8 pairs
    assert (A.size, r) == (8, [0, 5])
    n, A, B, r, _ = gene("one_strand")
    assert (A.size, r) == (1, [0]) and n >= 3
    # the greedy list is not "the plain top KP with sharers struck out" (a pair struck when it shares a row with ANY better
    # pair): a pair that shares a row only with a REJECTED better pair is taken -- the pair-level sibling of section 26's chain
    n, A, B, r, _ = gene("p_run64")
    assert r == [0, 5, 13, 23, 37] and _struck_out(A, B, 38) != r and _chained(A, B, r)
    assert sum(bool(_chained(A, B, dref.rounds_of(A, B, 5))) for _, A, B in op) == 25
    # repeat_core: hundreds of pairs tie on both scores, the boundaries decide which one takes the rows
    n, A, B, r, kinds = gene("repeat_core")
    assert A.size == 2750 and r == [0, 11, 44, 55, 88]
    t = host["tables"]

    def keys_of(i):
        ks = [int(t["score_minus" if int(p) >> 31 else "score_plus"][int(p) & 0x7FFFFFFF].view(np.uint64)) for p in (A[i], B[i])]
        return min(ks), max(ks)
    assert keys_of(0) == keys_of(11) == keys_of(10) and len({keys_of(i) for i in range(89)}) < 10
    # rows with equal boundaries on the two strands, both picked by one gene: different guides
    c = {}
    for g, (_, A, B) in enumerate(_ordered(host, ANY_1_40)):
        rows_g = [int(x) for i in dref.rounds_of(A, B, 64) for x in (A[i], B[i])]
        cs = [int(t["pos_minus"][x & 0x7FFFFFFF]) + 6 if x >> 31 else int(t["pos_plus"][x]) - 3 for x in rows_g]
        c[g] = len(cs) - len(set(cs))
    assert sum(c.values()) > 0


def test_the_genome_contains_the_cases(host):
    _assert_the_genome_contains_the_cases(host)


def test_the_bench_tools_host_check_equals_the_reference(host):
    """tools/pairs_distinct_bench.py checks sampled genes of the device's result against its own numpy statement: that one
    against the reference, on the case genome."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "pairs_distinct_bench.py")
    spec = importlib.util.spec_from_file_location("pairs_distinct_bench", path)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    t = host["tables"]
    cols = (t["pos_plus"], t["score_plus"], t["pos_minus"], t["score_minus"])
    for _, KP, dmin, dmax, orientation in bench.SETS + (("", 64, 1, 40, "any"),):
        mask = sel.ORIENTATIONS[orientation]
        _same(bench.host_distinct(cols, host["lo"], host["hi"], KP, dmin, dmax, mask),
              dref.distinct_numpy(t, host["lo"], host["hi"], KP, dmin, dmax, mask), "KP=%d %d..%d %s" % (KP, dmin, dmax, orientation))


def test_pair_params_refusals():
    p = sel.PairParams(5)
    assert p.distinct is False and sel.PairParams(5, 50, 500, False, "any").distinct is False  # positional callers are untouched
    q = sel.PairParams(7, 3, 9, True, "pam-out", distinct=True)
    assert q.distinct is True and (q.k, q.dmin, q.dmax, q.frameshift, q.mask) == (7, 3, 9, True, 4)
    n = q.native()
    assert (n.k, n.dmin, n.dmax, n.orientation_mask, n.frameshift) == (7, 3, 9, 4, 1)  # the native parameters keep their layout
    for bad in (dict(k=0), dict(k=65), dict(k=5, dmin=0), dict(k=5, dmin=60, dmax=50), dict(k=5, dmax=65536), dict(k=5, orientation="sideways"),
                dict(k=5, orientation=0), dict(k=5, orientation=16)):
        with pytest.raises(ValueError):
            sel.PairParams(distinct=True, **bad)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="distinct"):
            sel.PairParams(5, distinct=bad)


def _greedy_by_hand(cand, KP):
    out, taken = [], set()
    for c in sorted(cand):
        if len(out) < KP and c[-2] not in taken and c[-1] not in taken:
            out.append(c)
            taken.update(c[-2:])
    return out


def test_assemble_pairs_for_a_gene_in_two_texts():
    """A gene met in two texts: the merge of the per-text greedy lists in the pairs' order is the greedy over the union, and
    the summed n_distinct is capped at KP."""
    offsets, tables, lo, hi, gene = tp._two_text_arena()
    KP = 3
    n_pass, n_pairs, n_distinct, pairs = dref.distinct_numpy(tables, lo, hi, KP, 10, 300)
    assert n_pairs.tolist() == [6, 6, 6] and n_distinct.tolist() == [2, 2, 2]  # four rows a text: two disjoint pairs at the most
    n_in, _, picked = ref.select_numpy(tables, lo, hi, 2)
    part = dict(offsets=offsets, lengths=np.array([1000, 1000], np.uint64), group=[4, 7], gene=gene, n_in=n_in, n_pass=n_pass, sel=picked,
                pair_n_pairs=n_pairs, pair_list=pairs, pair_n_distinct=n_distinct, **tables)
    got, total, rep = sel.assemble_pairs(2, KP, [part])
    assert total.tolist() == [12, 6] and rep is None
    assert sel.assemble_n_distinct(2, KP, [part]).tolist() == [3, 2]  # gene 0: 2 + 2, capped at KP
    # by hand: every pair of the two texts, none across them; rows of different texts are different rows
    cand = []
    for t, (first, n) in enumerate(((0, 3), (3, 3))):
        rows_t = [(int(p) - 3, 0, s, k) for k, (p, s) in enumerate(zip(tables["pos_plus"], tables["score_plus"])) if first <= k < first + n]
        rows_t += [(int(tables["pos_minus"][t]) + 6, 1, tables["score_minus"][t], t)]
        for ca, sa, xa, ra in rows_t:
            for cb, sb, xb, rb in rows_t:
                if 10 <= cb - ca <= 300:
                    cand.append((-min(xa, xb), -max(xa, xb), ca, cb, sa * 2 + sb, t, cb - ca, xa, xb, (sa, ra), (sb, rb)))
    want = _greedy_by_hand(cand, KP)
    assert len(want) == 3 and {c[5] for c in want} == {0, 1}
    g0 = got[got["gene"] == 0]
    assert g0["rank"].tolist() == [1, 2, 3] and got[got["gene"] == 1]["rank"].tolist() == [1, 2]
    for r, c in zip(g0, want):
        assert r["contig"] == [4, 7][c[5]] and r["deletion_length"] == c[6] and r["score_a"] == c[7] and r["score_b"] == c[8]
    plain = sel.assemble_pairs(2, KP, [dict(part, pair_list=pref.pairs_numpy(tables, lo, hi, KP, 10, 300)[2])])[0]
    assert plain[plain["gene"] == 0].tobytes() != g0.tobytes()  # the plain top three share a guide


# ---------------------------------------------------------------------------------------------- the command line
class DistinctOracleBackend(OracleBackend):
    """OracleBackend plus the `select` keyword with pairs, plain or distinct: the selections by the numpy statements over
    one host arena -- what select_arena does with the device."""

    def scan(self, strings, l, offtarget=False, annotation=None, specificity=None, select=None):
        out = OracleBackend.scan(self, strings, l, offtarget=offtarget, annotation=annotation)
        if select is None:
            return out
        assert specificity is None and not select.params.require_cds and select.property_limits is None and select.repair_limits is None
        texts = [bytes(s) for s in strings]
        offsets, off = [], 64
        for t in texts:
            offsets.append(off)
            off += ((len(t) + 63) // 64 + 1) * 64
        tables = tp._arena_tables(out, offsets)
        req = select.annotation
        lo, hi, gene = req.gene_layout([(k, o, len(t)) for k, (t, o) in enumerate(zip(texts, offsets))])
        n_in, n_pass, picked = ref.select_numpy(tables, lo, hi, select.params.k, select.params.min_score)
        part = dict(offsets=np.array(offsets, np.uint64), lengths=np.array([len(t) for t in texts], np.uint64), group=list(range(len(texts))),
                    gene=gene, n_in=n_in, n_pass=n_pass, sel=picked, **tables)
        labels = req.annotation.genes()[0]
        out = sel.HitList(out)
        S = out.selection = sel.assemble(labels, select.params.k, [part])
        q = select.pairs
        if q is not None and q.distinct:
            _, part["pair_n_pairs"], part["pair_n_distinct"], part["pair_list"] = dref.distinct_numpy(
                tables, lo, hi, q.k, q.dmin, q.dmax, q.mask, q.frameshift, select.params.min_score)
            S.n_pairs_distinct = sel.assemble_n_distinct(len(labels), q.k, [part])
        elif q is not None:
            _, part["pair_n_pairs"], part["pair_list"] = pref.pairs_numpy(tables, lo, hi, q.k, q.dmin, q.dmax, q.mask, q.frameshift,
                                                                          select.params.min_score)
        if q is not None:
            S.pairs, S.n_pairs, S.pairs_repair = sel.assemble_pairs(len(labels), q.k, [part])
        return out


def _expected_pairs_file(case, main_rows, n_pairs, pairs, gene):
    """The pairs file's bytes from the main CSV's own rows and a reference's picks (layout rows x KP x 2)."""
    by_key = {(r[4], r[6], r[8]): r for r in main_rows[1:] if len(r) >= 12}  # (chromosome, end_pos, strand)
    n_before = np.cumsum([0] + [len(h["pos_plus"]) for h in case["hits"]])
    m_before = np.cumsum([0] + [len(h["pos_minus"]) for h in case["hits"]])

    def guide(packed):
        minus, r = int(packed) >> 31, int(packed) & 0x7FFFFFFF
        c = int(np.searchsorted(m_before if minus else n_before, r, "right") - 1)
        h = case["hits"][c]
        pos = int(h["pos_minus"][r - m_before[c]]) if minus else int(h["pos_plus"][r - n_before[c]])
        main = by_key[(case["names"][c], str(pos + 3 if minus else pos), "-" if minus else "+")]
        score = float(h["score_minus"][r - m_before[c]] if minus else h["score_plus"][r - n_before[c]])  # (from the hit table, as the writer takes it)
        assert abs(score - float(main[9])) < 1e-15
        return pref.boundary(pos, bool(minus)), case["names"][c], [main[5], main[6], main[7], main[8], main[2], score]

    want = []
    for row_of_layout, g in enumerate(gene):
        for rank in range(pairs.shape[1]):
            if pairs[row_of_layout, rank, 0] == NONE:
                break
            (ca, chrom, fa), (cb, _, fb) = guide(pairs[row_of_layout, rank, 0]), guide(pairs[row_of_layout, rank, 1])
            want.append((int(g), rank, [case["genes"][int(g)][3], str(rank + 1), str(int(n_pairs[row_of_layout])), str(cb - ca),
                                        str(int((cb - ca) % 3 == 0)), chrom] + fa + fb))
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(["gene", "rank", "qualifying_pairs", "deletion_length", "in_frame", "chromosome"]
               + [n + s for s in ("_a", "_b") for n in ("start_pos", "end_pos", "cutsite", "strand", "sequence", "on_site_score")])
    for _, _, fields in sorted(want, key=lambda x: x[:2]):  # genes in GFF order, ranks in pick order
        w.writerow(fields)
    return buf.getvalue().encode(), len(want)


PLAIN_ARGS = ["--select", "5", "--select-min-score", "0.3", "--select-pairs", "4", "--pairs-frameshift", "--pairs-min-distance", "40",
              "--pairs-max-distance", "700"]


def _md5(path):
    with open(path, "rb") as f:
        return hashlib.md5(f.read()).hexdigest()


def test_cli_pairs_file_over_the_oracle(case, host, oracle, tmp_path, monkeypatch):
    plain, plain_out = tp._run(case, tmp_path, monkeypatch, PLAIN_ARGS, DistinctOracleBackend(oracle), "plain.csv")
    # without the flag every output byte is what it was before the option existed
    assert (_md5(plain), _md5(plain + ".selected.csv"), _md5(plain + ".pairs.csv")) == (MD5_MAIN, MD5_SELECTED, MD5_PAIRS)
    out, stdout = tp._run(case, tmp_path, monkeypatch, PLAIN_ARGS + ["--pairs-distinct"], DistinctOracleBackend(oracle))
    assert (_md5(out), _md5(out + ".selected.csv")) == (MD5_MAIN, MD5_SELECTED) and _md5(out + ".pairs.csv") != MD5_PAIRS
    assert stdout.replace("out.csv", "plain.csv") == plain_out
    n_pass, n_pairs, n_distinct, pairs = dref.distinct_numpy(host["tables"], host["lo"], host["hi"], 4, 40, 700, 0xF, True, 0.3)
    want, n = _expected_pairs_file(case, tp._read(out), n_pairs, pairs, host["gene"])
    assert n == int(n_distinct.sum()) > 60
    with open(out + ".pairs.csv", "rb") as f:
        assert f.read() == want  # bytes: the columns are the plain file's, rank is the pick order, qualifying_pairs stays n_pairs
    rows_got = tp._read(out + ".pairs.csv")
    assert rows_got[0] == tp._read(plain + ".pairs.csv")[0]
    def most_shared(rows):
        """How often the most used guide of a gene occurs in its pairs (a gene's block starts at rank 1: two genes may share a label)."""
        count, block = {}, 0
        for r in rows:
            block += r[1] == "1"
            for at in (6, 12):
                key = (block, r[5], r[at + 1], r[at + 3])
                count[key] = count.get(key, 0) + 1
        return max(count.values())

    assert most_shared(rows_got[1:]) == 1  # no guide twice in a gene
    shared = {0: most_shared(tp._read(plain + ".pairs.csv")[1:])}
    assert max(shared.values()) > 1  # the plain file does share guides


REFUSALS = [
    (["--pairs-distinct"], "belongs to --select-pairs"),
    (["--select", "5", "--pairs-distinct"], "belongs to --select-pairs"),
    (["--select-pairs", "5", "--pairs-distinct"], "--select-pairs belongs to --select"),
    (["--select", "5", "--select-pairs", "0", "--pairs-distinct"], "1..64"),
    (["--select", "5", "--select-pairs", "65", "--pairs-distinct"], "1..64"),
    (["--select", "5", "--select-pairs", "5", "--pairs-distinct", "--pairs-min-distance", "0"], "1 <= dmin"),
    (["--select", "5", "--select-pairs", "5", "--pairs-distinct", "--pairs-max-distance", "65536"], "65535"),
    (["--select", "5", "--select-pairs", "5", "--pairs-distinct", "--pairs-orientation", "sideways"], "pam-out"),
    (["--select", "5", "--select-pairs", "5", "--pairs-distinct", "-l", "19"], "-l 20"),
    (["--select", "5", "--select-pairs", "5", "--pairs-distinct", "--gpus", "2"], "one GPU"),
    (["--select", "5", "--select-pairs", "5", "--pairs-distinct", "--select-coding-min", "5"], "--select-pairs"),
    (["--select", "5", "--select-pairs", "5", "--pairs-distinct", "--select-stop"], "--select-pairs"),
    (["--select", "5", "--select-pairs", "5", "--pairs-distinct", "--select-splice", "donor"], "--select-pairs"),
]


@pytest.mark.parametrize("extra,text", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_cli_refusals_come_before_any_side_effect(case, oracle, tmp_path, monkeypatch, extra, text):
    monkeypatch.chdir(tmp_path)
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9", "-g", case["gff_path"]] + extra
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=DistinctOracleBackend(oracle), out=io.StringIO())
    assert "--select" in str(e.value.code) and text in str(e.value.code)
    assert os.listdir(tmp_path) == []


# ---------------------------------------------------------------------------------------------- on the GPU
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module", params=[1, 3], ids=["one-arena", "three-arenas"])
def scanned(request, engine, case, host):
    _assert_the_genome_contains_the_cases(host)  # no GPU test runs on a genome that has lost one of them
    s = tp._scanned(engine, case, None if request.param == 1 else 600)
    assert len(s["genome"].arenas) == request.param
    tp._assert_the_genome_contains_the_cases(s)  # the sizes, run lengths and ties of the pair tests' genes
    yield s
    for h in s["handles"]:
        h.close()
    s["genome"].close()


def _reference(s, a, window, min_score=0.0, spec=None, cds=False, limits=False):
    """distinct_numpy at KP = 64 for arena a, computed once per set of arguments."""
    key = ("distinct", a, window, min_score, None if spec is None else tuple(sorted(spec.items())), cds, limits)
    if key not in s["cache"]:
        A = s["arenas"][a]
        dmin, dmax, mask, fs = window
        s["cache"][key] = dref.distinct_numpy(A["tables"], A["lo"], A["hi"], 64, dmin, dmax, mask, fs, min_score,
                                              None if spec is None else dict(A["spec"], **spec), A["cds"] if cds else None,
                                              A["also"] if limits else None)
    return s["cache"][key]


def _handle(s, a, pair_slice_rows=None, cds=False, limits=False, genes=None, per_launch=None):
    A = s["arenas"][a]
    lo, hi = (A["lo"], A["hi"]) if genes is None else (A["lo"][genes], A["hi"][genes])
    h = sel.ArenaSelect(s["genome"].arenas[a], lo, hi)
    if cds:
        h.set_flags(A["cds"]["flags"])
    if limits:
        h.set_property_limits(tp.PROPERTY_LIMITS)
        h.set_repair_limits(tp.REPAIR_LIMITS)
    if pair_slice_rows:
        h.set_pair_limits(pair_slice_rows)
    if per_launch:
        h.set_pair_distinct_limits(per_launch)
    return h


def _params(min_score=0.0, spec=None, cds=False):
    params = sel.Params(1, min_score, require_cds=cds)
    if spec is not None:
        params.max_mm0, params.max_hit_sum = spec["max_mm0"], spec["max_hit_sum"]
    return params


def _device(s, a, KP, window, pair_slice_rows=None, min_score=0.0, spec=None, cds=False, limits=False, genes=None, per_launch=None):
    h = _handle(s, a, pair_slice_rows, cds, limits, genes, per_launch)
    try:
        dmin, dmax, mask, fs = window
        h.run_pairs_distinct(_params(min_score, spec, cds), sel.PairParams(KP, dmin, dmax, fs, mask), s["handles"][a] if spec is not None else None)
        return h.fetch_pairs_distinct(), h.pairs_distinct_stats()
    finally:
        h.close()


def _launch_bound(stats, KP, per_launch=1 << 20):
    """At most 2 KP + 3 launches per block of items."""
    return stats["launches"] <= (2 * KP + 3) * max(1, -(-int(stats["items"]) // per_launch))


@pytest.mark.gpu
@pytest.mark.parametrize("pair_slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
@pytest.mark.parametrize("KP", KPS)
def test_gpu_distinct_pairs_equal_the_reference(scanned, KP, pair_slice_rows):
    """Every window and mask of the pair tests -- 1 .. 1 and 1 .. 40 (overlapping protospacers, equal-boundary rows), 50 ..
    500 with and without frameshift, 30 .. 54 pam-out and pam-in, each single mask bit at 1 .. 300 -- over every gene of the
    case genome: 0, 1, 2 and 3 eligible rows, one-strand genes, the *_run63/64/65/129 genes, repeat_core."""
    s = scanned
    for a, A in enumerate(s["arenas"]):
        n = tp._eligible_counts(A).sum(axis=1)
        for window in WINDOWS:
            got, stats = _device(s, a, KP, window, pair_slice_rows)
            want = _first(_reference(s, a, window), KP)
            _same(got, want, "arena %d window %r" % (a, window))
            assert stats["qualifying_pairs"] == float(want[1].sum()) and stats["pairs_taken"] == float(want[2].sum())
            assert stats["pair_evaluations"] >= stats["qualifying_pairs"] and stats["items"] >= len(A["lo"])
            assert _launch_bound(stats, KP) and stats["launches"] >= 3
            assert stats["distinct_rounds"] <= KP and (stats["cut_genes"] > 0) == (stats["distinct_rounds"] > 0)
        if pair_slice_rows == 64 and len(s["arenas"]) == 1:
            assert (n > 64).sum() > 10 and stats["cut_genes"] > 10  # cut genes: the host rounds ran
        if pair_slice_rows is None and len(s["arenas"]) == 1:
            assert stats["cut_genes"] >= 1 and stats["items"] > len(A["lo"])  # whole_c1, also at the default


@pytest.mark.gpu
def test_gpu_kp_one_is_the_pair_run_of_the_same_handle(scanned):
    s = scanned
    for a, A in enumerate(s["arenas"]):
        for pair_slice_rows in (None, 64):
            h = _handle(s, a, pair_slice_rows)
            try:
                for dmin, dmax, mask, fs in (ANY_50_500, ANY_1_40, OUT_30_54):
                    q = sel.PairParams(1, dmin, dmax, fs, mask)
                    h.run_pairs(_params(), q)
                    h.run_pairs_distinct(_params(), q)
                    n_pass, n_pairs, pairs = h.fetch_pairs()
                    got = h.fetch_pairs_distinct()
                    assert got[0].tobytes() == n_pass.tobytes() and got[1].tobytes() == n_pairs.tobytes() and got[3].tobytes() == pairs.tobytes()
                    assert np.array_equal(got[2], (n_pairs > 0).astype(np.uint32)) and n_pairs.sum() > 0
            finally:
                h.close()


def _run_rows(A, k):
    return tp._run_rows(A, k)


@pytest.mark.gpu
def test_gpu_every_pair_of_a_contig(scanned):
    """1 .. 65 535 on whole_c1: millions of pairs, one gene cut into three items at the default slicing and forty at 64, so
    it goes through the host rounds at both -- and, at 2 items a launch, with its pieces in different launches of every round."""
    s = scanned
    done = 0
    for a, A in enumerate(s["arenas"]):
        if "whole_c1" not in A["ids"]:
            continue
        k = A["ids"].index("whole_c1")
        genes = np.array([k])
        want = dref.distinct_numpy(A["tables"], A["lo"][genes], A["hi"][genes], 64, 1, 65535)
        assert want[1][0] > 2000000 and want[2][0] == 64
        for rows_per_item, per_launch in ((None, None), (64, None), (64, 2)):
            got, stats = _device(s, a, 64, (1, 65535, 0xF, False), rows_per_item, genes=genes, per_launch=per_launch)
            _same(got, want, "whole_c1 %r %r" % (rows_per_item, per_launch))
            items = -(-(_run_rows(A, k)) // (rows_per_item or 1024))
            assert stats["items"] == items > 2 and stats["cut_genes"] == 1 and stats["distinct_rounds"] == 64
            blocks = -(-items // (per_launch or 1 << 20))
            assert stats["launches"] == 2 + 64 * (blocks + 1) and _launch_bound(stats, 64, per_launch or 1 << 20)
            if per_launch:
                assert blocks >= 20
            assert stats["pair_evaluations"] >= float(want[1][0])
        done += 1
    assert done == 1


@pytest.mark.gpu
def test_gpu_set_pair_distinct_limits_over_all_genes(scanned):
    """2 items a launch over every gene at slices of 64: whole genes and pieces of cut genes on both sides of launch boundaries."""
    s = scanned
    L = nat.lib()
    for a, A in enumerate(s["arenas"]):
        got, stats = _device(s, a, 5, ANY_50_500, 64, per_launch=2)
        _same(got, _first(_reference(s, a, ANY_50_500), 5), "arena %d" % a)
        assert _launch_bound(stats, 5, 2) and stats["launches"] > stats["items"] / 2
        h = _handle(s, a)
        try:
            assert L.crp_select_set_pair_distinct_limits(h._h, (1 << 20) + 1) == nat.CRP_ERR_INVALID
            assert L.crp_select_set_pair_distinct_limits(h._h, 1 << 20) == nat.CRP_OK and L.crp_select_set_pair_distinct_limits(h._h, 0) == nat.CRP_OK
        finally:
            h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair_slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
def test_gpu_all_predicate_terms(scanned, pair_slice_rows):
    """Joined columns at M = 3 with their sentinel rows, require_cds, property and repair limits, all at once and one by one."""
    s = scanned
    window = (20, 2000, 0xF, True)
    TERMS = (dict(min_score=0.5), dict(spec=dict(max_mm0=0, max_hit_sum=sel.max_hit_sum_for(0.5))), dict(cds=True), dict(limits=True))
    total = lambda at, **terms: sum(int(_reference(s, a, window, **terms)[at].sum()) for a in range(len(s["arenas"])))
    assert 0 < total(0, **tp.ALL_TERMS) < min(total(0, **terms) for terms in TERMS) and max(total(0, **terms) for terms in TERMS) < total(0)
    assert total(2, **tp.ALL_TERMS) > 20
    for a, A in enumerate(s["arenas"]):
        for KP in (5, 64):
            got, _ = _device(s, a, KP, window, pair_slice_rows, **tp.ALL_TERMS)
            _same(got, _first(_reference(s, a, window, **tp.ALL_TERMS), KP), "arena %d" % a)
        for terms in TERMS:
            got, _ = _device(s, a, 5, window, pair_slice_rows, **terms)
            _same(got, _first(_reference(s, a, window, **terms), 5), "arena %d %r" % (a, sorted(terms)))
        if "n_run" in A["ids"]:  # sentinel rows of the join inside a gene: in it, never eligible
            k = A["ids"].index("n_run")
            everything = dict(max_mm0=NONE, max_hit_sum=0xFFFFFFFFFFFFFFFF)
            joined_only = _reference(s, a, window, spec=everything)
            assert joined_only[0][k] < _reference(s, a, window)[0][k]
            got, _ = _device(s, a, 5, window, pair_slice_rows, spec=everything)
            _same(got, _first(joined_only, 5), "joined only")


@pytest.mark.gpu
def test_gpu_thresholds_that_leave_no_row_and_exactly_two(scanned):
    s = scanned
    twos = 0
    for a, A in enumerate(s["arenas"]):
        got, stats = _device(s, a, 5, ANY_50_500, min_score=2.0)
        assert (got[0] == 0).all() and (got[1] == 0).all() and (got[2] == 0).all() and (got[3] == NONE).all()
        assert stats["pair_evaluations"] == 0 and stats["qualifying_pairs"] == 0 and stats["pairs_taken"] == 0
        # the second highest score of a gene as the threshold: exactly two of its rows pass, one pair at the most
        t, ok = A["tables"], pref.eligible_numpy(A["tables"])
        for name in ("first_rows", "p_run64", "nested"):
            if name not in A["ids"]:
                continue
            k = A["ids"].index(name)
            keys = sorted((r[2] for r in tp._rows_of(t, A["lo"][k], A["hi"][k], ok)), reverse=True)
            if keys[1] == keys[2]:
                continue
            threshold = float(np.array([keys[1]], np.uint64).view(np.float64)[0])
            for window in ((1, 65535, 0xF, False), ANY_50_500):
                want = dref.distinct_numpy(t, A["lo"], A["hi"], 5, *window, min_score=threshold)
                assert want[0][k] == 2 and want[2][k] <= 1
                for pair_slice_rows in (None, 64):
                    got, _ = _device(s, a, 5, window, pair_slice_rows, min_score=threshold)
                    _same(got, want, "two rows left in %s" % name)
            assert dref.distinct_numpy(t, A["lo"], A["hi"], 5, 1, 65535, min_score=threshold)[2][k] == 1
            twos += 1
    assert twos >= 2


def _arena_case(engine, case):
    """The case contigs as one arena of their own (its tables may be scanned again), with the reference's view of it."""
    arena = engine.arena(case["contigs"])
    n_plus, n_minus = arena.scan_score_device(20)
    tables = dict(zip(("pos_plus", "_", "score_plus", "pos_minus", "__", "score_minus"), arena.fetch(n_plus, n_minus)))
    tables = {k: v for k, v in tables.items() if not k.startswith("_")}
    entries = [(n, 0, int(ln), int(o)) for n, ln, o in zip(case["names"], arena.lengths, arena.offsets)]
    lo, hi, gene = ref.layout(case["genes"], entries, 0)
    return arena, tables, lo, hi


@pytest.mark.gpu
def test_gpu_one_handle_through_every_run(engine, case):
    """Plain selection, plain pairs, distinct pairs, spaced, distinct pairs with a smaller KP, a rescan: after every step the
    handle's distinct result equals the reference and a fresh handle's, and the other runs' results stay what they were."""
    import select_spacing_reference as sp
    arena, tables, lo, hi = _arena_case(engine, case)
    try:
        h = sel.ArenaSelect(arena, lo, hi)
        h.set_pair_limits(64)
        params = sel.Params(5, 0.3)
        want_sel = ref.select_numpy(tables, lo, hi, 5, 0.3)
        want_pairs = pref.pairs_numpy(tables, lo, hi, 5, 50, 500, min_score=0.3)
        want_spaced = sp.spaced_numpy(tables, lo, hi, 5, 40, 0.3)
        want = {KP: dref.distinct_numpy(tables, lo, hi, KP, 50, 500, min_score=0.3) for KP in (64, 3)}

        def fresh(KP):
            f = sel.ArenaSelect(arena, lo, hi)
            try:
                f.set_pair_limits(64)
                f.run_pairs_distinct(params, sel.PairParams(KP, 50, 500))
                return f.fetch_pairs_distinct()
            finally:
                f.close()

        def check(KP, what):
            got = h.fetch_pairs_distinct()
            _same(got, want[KP], what)
            for g, f in zip(got, fresh(KP)):
                assert g.tobytes() == f.tobytes(), what

        h.run(params)
        h.run_pairs(params, sel.PairParams(5, 50, 500))
        h.run_pairs_distinct(params, sel.PairParams(64, 50, 500))
        check(64, "after select and pairs")
        tp._same(h.fetch_pairs(), want_pairs, "pairs after distinct")
        for g, w in zip(h.fetch(), want_sel):
            assert np.array_equal(g, w)
        h.run_spaced(params, 40)
        check(64, "after spaced")
        for g, w in zip(h.fetch_spaced(), want_spaced):
            assert np.array_equal(g, w)
        h.run_pairs_distinct(params, sel.PairParams(3, 50, 500))
        check(3, "a smaller KP")
        tp._same(h.fetch_pairs(), want_pairs, "pairs after the second distinct run")
        for g, w in zip(h.fetch_spaced(), want_spaced):
            assert np.array_equal(g, w)
        h.run_pairs(params, sel.PairParams(5, 50, 500))  # the plain run writes the shared pass keys; the distinct results are its own
        check(3, "after another plain pair run")
        arena.scan_score_device(20)  # a rescan: the same tables again, a new run on them
        h.run_pairs_distinct(params, sel.PairParams(64, 50, 500))
        check(64, "after a rescan")
        h.close()
    finally:
        arena.close()


@pytest.mark.gpu
def test_gpu_calls_out_of_order_and_error_codes(engine):
    from cropsr_amd import baseedit, coding
    L = nat.lib()
    arena = engine.arena([b"ACGTTGCAAGGCCTTAGGACCA" * 60])
    try:
        h = sel.ArenaSelect(arena, [0, 100], [50, 900])

        def status(fn):
            with pytest.raises(nat.CropsrHipError) as e:
                fn()
            return e.value.status, str(e.value)

        pp = sel.PairParams(5, 10, 200)
        run = lambda params=sel.Params(5), q=pp, handle=None: h.run_pairs_distinct(params, q, handle)
        assert status(h.fetch_pairs_distinct)[0] == nat.CRP_ERR_STATE                  # nothing has run
        assert L.crp_select_fetch_pairs_distinct(h._h, None, None, None, None) == nat.CRP_ERR_STATE
        st, text = status(run)
        assert st == nat.CRP_ERR_STATE and "guide length 20" in text and "crp_select_run_pairs_distinct" in text  # no tables
        arena.scan_score_device(19)
        assert status(run)[0] == nat.CRP_ERR_STATE                                       # a scan at another length
        n_plus, n_minus = arena.scan_score_device(20)
        st, text = status(lambda: run(sel.Params(5, require_cds=True)))
        assert st == nat.CRP_ERR_STATE and "crp_select_set_flags" in text
        h.set_flags(np.ones(3, np.uint8))
        st, text = status(lambda: run(sel.Params(5, require_cds=True)))
        assert st == nat.CRP_ERR_STATE and "crp_annotate_lookup" in text
        h.set_property_limits(properties.Limits(gc_min=5))                             # limits without their column
        st, text = status(run)
        assert st == nat.CRP_ERR_STATE and "crp_guide_properties" in text
        h.set_property_limits(None)
        h.set_repair_limits(repair.Limits(min_mh=10))
        st, text = status(run)
        assert st == nat.CRP_ERR_STATE and "crp_repair_scores" in text
        h.set_repair_limits(None)
        pattern, gp, M, scheme = srch.check_specificity(20, 3)
        handle = srch.ArenaSelfSearch(arena, pattern, gp, 3, M)
        try:
            st, text = status(lambda: run(handle=handle))
            assert st == nat.CRP_ERR_STATE and "joined" in text
        finally:
            handle.close()
        p = nat.SelectParams(0.0, 0, 0, 5, 0, 0)
        for bad, word in ((nat.SelectPairParams(0, 10, 200, 0xF, 0), "k must be"), (nat.SelectPairParams(65, 10, 200, 0xF, 0), "k must be"),
                          (nat.SelectPairParams(5, 0, 200, 0xF, 0), "distances"), (nat.SelectPairParams(5, 201, 200, 0xF, 0), "distances"),
                          (nat.SelectPairParams(5, 10, 65536, 0xF, 0), "distances"), (nat.SelectPairParams(5, 10, 200, 0, 0), "mask"),
                          (nat.SelectPairParams(5, 10, 200, 16, 0), "mask")):
            for fn in (L.crp_select_run_pairs_distinct, L.crp_select_run_pairs):  # one host function checks both
                assert fn(h._h, ctypes.byref(p), ctypes.byref(bad), None) == nat.CRP_ERR_INVALID
                assert word in L.crp_last_error(engine._ctx).decode()
        good = nat.SelectPairParams(5, 10, 200, 0xF, 0)
        assert L.crp_select_run_pairs_distinct(None, ctypes.byref(p), ctypes.byref(good), None) == nat.CRP_ERR_INVALID
        assert L.crp_select_run_pairs_distinct(h._h, None, ctypes.byref(good), None) == nat.CRP_ERR_INVALID
        assert L.crp_select_run_pairs_distinct(h._h, ctypes.byref(p), None, None) == nat.CRP_ERR_INVALID
        assert L.crp_select_set_pair_distinct_limits(None, 0) == nat.CRP_ERR_INVALID
        out = np.zeros(13)
        assert L.crp_select_pairs_distinct_stats(h._h, out.ctypes.data_as(nat.f64p), 13) == nat.CRP_ERR_INVALID
        assert status(h.fetch_pairs_distinct)[0] == nat.CRP_ERR_STATE                  # a failed run leaves nothing to fetch
        # the limits that are relative to the gene: refused as the plain pair run refuses them, with its code
        for put, clear, word in ((lambda: h.set_coding_limits(coding.Limits(5, 65)), lambda: h.set_coding_limits(None), "coding limits"),
                                 (lambda: h.set_edit_limits(None, baseedit.Limits(0, 50, 3)), lambda: h.set_edit_limits(None, None), "edit limits"),
                                 (lambda: h.set_splice_limits(None, "cbe", baseedit.SpliceLimits(0, 50, 3, "any")),
                                  lambda: h.set_splice_limits(None, "cbe", None), "splice limits")):
            put()
            for fn in (run, lambda: h.run_pairs(sel.Params(5), pp)):
                st, text = status(fn)
                assert st == nat.CRP_ERR_UNSUPPORTED and word in text
            clear()
        run(q=sel.PairParams(64, 10, 200))
        tables = dict(zip(("pos_plus", "_", "score_plus", "pos_minus", "__", "score_minus"), arena.fetch(n_plus, n_minus)))
        want = dref.distinct_numpy(tables, [0, 100], [50, 900], 64, 10, 200)
        assert want[1][1] > 64 and want[2][1] > 2
        _same(h.fetch_pairs_distinct(), want)
        assert L.crp_select_fetch_pairs_distinct(h._h, None, None, None, None) == nat.CRP_OK  # any pointer may be NULL
        n_distinct = np.zeros(2, np.uint32)
        assert L.crp_select_fetch_pairs_distinct(h._h, None, None, n_distinct.ctypes.data_as(nat.u32p), None) == nat.CRP_OK
        assert np.array_equal(n_distinct, want[2])
        assert status(h.fetch_pairs)[0] == nat.CRP_ERR_STATE                           # the plain pair run has results of its own: none yet
        arena.scan_score_device(20)                                                    # a re-scan: the same tables again, a new run on them
        run(q=sel.PairParams(64, 10, 200))
        _same(h.fetch_pairs_distinct(), want)
        h.close()
    finally:
        arena.close()


@pytest.mark.gpu
def test_gpu_genome_level_call(engine, case):
    """Genome.scan_score(select=Request(pairs=PairParams(distinct=True))): the distinct run instead of the plain pair run."""
    g = engine.genome(case["contigs"], max_words=600)
    try:
        request = annotate.Request(case["annotation"], case["names"], 0)
        params = sel.Params(5, 0.2, max_perfect=0, min_specificity=0.5, require_cds=True)
        pp = sel.PairParams(5, 40, 900, True, distinct=True)
        hits = g.scan_score(20, specificity=dict(max_mm=3), select=sel.Request(params, request, pairs=pp, pair_slice_rows=64, repair_flank=30, min_mh=100))
        S = hits.selection
        parts = []
        for a, (arena, group) in enumerate(zip(g.arenas, g.groups)):
            h = hits.per_arena[a]
            tables = dict(pos_plus=h.pos_plus, score_plus=h.score_plus, pos_minus=h.pos_minus, score_minus=h.score_minus)
            entries = [(case["names"][k], 0, int(arena.lengths[j]), int(arena.offsets[j])) for j, k in enumerate(group)]
            lo, hi, gene = ref.layout(case["genes"], entries, 0)
            cols = [hits.columns[k] for k in group]
            spec = dict(counts_plus=np.concatenate([c["self_counts_plus"] for c in cols]), sum_plus=np.concatenate([c["self_sum_plus"] for c in cols]),
                        counts_minus=np.concatenate([c["self_counts_minus"] for c in cols]), sum_minus=np.concatenate([c["self_sum_minus"] for c in cols]),
                        max_mm0=0, max_hit_sum=1 << 30)
            fp, fm = arena.annotate_lookup(h.n_plus, h.n_minus)
            cds = dict(feat_plus=fp, feat_minus=fm, flags=case["annotation"].cds_flags())
            lim = repair.Limits(min_mh=100)
            also = dict(plus=lim.passes(hits.repair[a][0]), minus=lim.passes(hits.repair[a][1]))
            n_pass, n_pairs, n_distinct, pairs = dref.distinct_numpy(tables, lo, hi, 5, 40, 900, 0xF, True, 0.2, spec, cds, also)
            n_in, _, picked = ref.select_numpy(tables, lo, hi, 5, 0.2, spec, cds)  # (only n_in and the shape are used below)
            parts.append(dict(offsets=arena.offsets, lengths=arena.lengths, group=group, gene=gene, n_in=n_in, n_pass=n_pass, sel=picked,
                              pair_n_pairs=n_pairs, pair_list=pairs, pair_n_distinct=n_distinct, repair_plus=hits.repair[a][0],
                              repair_minus=hits.repair[a][1], **tables))
        W, total, rep = sel.assemble_pairs(len(S.labels), 5, parts)
        assert np.array_equal(S.n_pairs, total) and total.sum() > 20 and W.size > 10
        assert S.pairs.tobytes() == W.tobytes() and np.array_equal(S.pairs_repair, rep)
        taken = sel.assemble_n_distinct(len(S.labels), 5, parts)
        assert np.array_equal(S.n_pairs_distinct, taken) and np.array_equal(np.bincount(W["gene"], minlength=len(S.labels)), taken)
        assert S.pairs_stats["items"] > 0 and S.pairs_stats["qualifying_pairs"] == float(total.sum()) and S.pairs_stats["pairs_taken"] >= taken.sum()
        assert "distinct_items_ms" in S.pairs_stats and "merge_ms" not in S.pairs_stats  # the distinct run INSTEAD of the plain one
        for label in range(len(S.labels)):  # no guide twice in a gene
            mine = S.pairs[S.pairs["gene"] == label]
            guides = [(r["contig"], r["strand_" + x], r["index_" + x]) for r in mine for x in "ab"]
            assert len(set(guides)) == len(guides)
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_command_line_end_to_end(case, host, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    out_csv = str(tmp_path / "out.csv")
    argv = ["-f", case["fasta_path"], "-g", case["gff_path"], "-o", out_csv, "--cas9", "--seed", "11", "--each-contig-once"] + PLAIN_ARGS + [
        "--pairs-distinct", "--bench-json", str(tmp_path / "bench.json")]
    cli.run(cli.build_parser().parse_args(argv), out=io.StringIO())
    n_pass, n_pairs, n_distinct, pairs = dref.distinct_numpy(host["tables"], host["lo"], host["hi"], 4, 40, 700, 0xF, True, 0.3)
    want, n = _expected_pairs_file(case, tp._read(out_csv), n_pairs, pairs, host["gene"])
    with open(out_csv + ".pairs.csv", "rb") as f:
        got = f.read()
    assert n > 60 and got == want
    with open(tmp_path / "bench.json") as f:
        stage = json.load(f)["pairs"]
    assert stage["distinct"] is True and stage["kp"] == 4 and stage["pairs_taken"] == n and stage["items"] > 0 and "distinct_items_ms" in stage


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["straddle", "top"])
def test_gpu_high_positions(engine, oracle, placement):
    """A gene's rows on either side of arena position 2^30 (straddle) and all rows within 2^20 of 2^31 (top), behind the filler
    contig of tests/high_position_cases.py: the tie word c_a << 32 | c_b and the packed rows at the top of their range."""
    import high_position_cases as hp
    c = hp.build(oracle)
    lengths = [len(t) for t in c["contigs"]]
    n = hp.filler_length(placement, lengths, int(nat.lib().crp_arena_max_words()))
    offsets = hp.offsets_of([n] + lengths)[0][1:]
    tables = hp.arena_tables(c["hits"], offsets)
    entries = [(name, 0, ln, o) for name, ln, o in zip(c["names"], lengths, offsets)]
    lo, hi, gene = ref.layout(ref.gff_genes(c["gff"]), entries, 0)
    tie = [i for i, _, _, _ in c["genes"]].index("tie")
    k = int(np.flatnonzero(gene == tie)[0])
    if placement == "straddle":
        assert int(lo[k]) < hp.TWO30 <= int(hi[k])
    else:
        assert hp.TWO31 - int(lo.min()) < 2**20
    text = hp.filler(n)
    genome = engine.genome([text] + c["contigs"])
    del text
    try:
        assert len(genome.arenas) == 1
        hits = genome.scan_score(20).per_arena[0]
        for key in tables:
            assert np.array_equal(tables[key].view(np.uint8), getattr(hits, key).view(np.uint8)), key
        for pair_slice_rows in (None, 64):
            h = sel.ArenaSelect(genome.arenas[0], lo, hi)
            try:
                if pair_slice_rows:
                    h.set_pair_limits(pair_slice_rows)
                for KP, dmin, dmax in ((5, 50, 500), (64, 1, 65535), (64, 1, 40)):
                    h.run_pairs_distinct(sel.Params(1), sel.PairParams(KP, dmin, dmax))
                    want = dref.distinct_numpy(tables, lo, hi, KP, dmin, dmax)
                    _same(h.fetch_pairs_distinct(), want, "%s KP %d %d..%d" % (placement, KP, dmin, dmax))
                    assert want[2].sum() > 5
                    if placement == "straddle" and dmax == 65535:  # pairs whose two rows lie on either side of 2^30
                        t = tables
                        cs = [[int(t["pos_minus"][int(x) & 0x7FFFFFFF]) if int(x) >> 31 else int(t["pos_plus"][int(x)]) for x in p]
                              for p in want[3][k][:want[2][k]]]
                        assert any(a < hp.TWO30 <= b for a, b in cs)
            finally:
                h.close()
    finally:
        genome.close()
