"""--select-pairs: the best KP deletion pairs of every gene (cropsr_amd/select.py, csrc/crp_select_pairs.hip, DESIGN.md
section 19).  The definition is restated twice in tests/select_pairs_reference.py; the genome and its genes come from
tests/select_pairs_cases.py (tests/select_cases.py plus a few genes)."""
import csv
import ctypes
import io
import os

import numpy as np
import pytest

from conftest import OracleBackend

import repair_reference
import select_pairs_cases as pcases
import select_pairs_reference as pref
import select_reference as ref
from cropsr_amd import _native as nat
from cropsr_amd import annotate, cli, properties, repair, rows
from cropsr_amd import search as srch
from cropsr_amd import select as sel

KPS = (1, 5, 64)
NONE = 0xFFFFFFFF
# (dmin, dmax, mask, frameshift)
WINDOWS = [(1, 1, 0xF, False), (1, 40, 0xF, False), (1, 40, 0xF, True), (50, 500, 0xF, False), (50, 500, 0xF, True),
           (30, 54, pref.PAM_OUT, False), (30, 54, pref.PAM_IN, False), (1, 300, 1, False), (1, 300, 2, True), (1, 300, 4, False),
           (1, 300, 8, False)]


@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    c = pcases.build(oracle)
    d = tmp_path_factory.mktemp("select_pairs")
    c["gff_path"] = str(d / "genes.gff")
    with open(c["gff_path"], "w") as f:
        f.write(c["gff"])
    c["fasta_path"] = str(d / "genome.fa")
    with open(c["fasta_path"], "w") as f:  # one line per contig: read unformatted (dec = 0)
        f.write("".join(">%s\n%s\n" % (n, t.decode()) for n, t in zip(c["names"], c["contigs"]))[:-1])
    c["annotation"] = annotate.Annotation(c["gff_path"])
    c["genes"] = ref.gff_genes(c["gff"])
    return c


def _arena_tables(hits, offsets):
    cat = lambda key, dt, add: np.concatenate([h[key].astype(dt) + (dt(o) if add else dt(0)) for h, o in zip(hits, offsets)])
    return dict(pos_plus=cat("pos_plus", np.uint32, True), score_plus=cat("score_plus", np.float64, False),
                pos_minus=cat("pos_minus", np.uint32, True), score_minus=cat("score_minus", np.float64, False))


def _host_arena(case):
    """All contigs as one arena laid out like the device's: 64-aligned texts, one separator word between them."""
    offsets, off = [], 64
    for t in case["contigs"]:
        offsets.append(off)
        off += ((len(t) + 63) // 64 + 1) * 64
    entries = [(n, 0, len(t), o) for n, t, o in zip(case["names"], case["contigs"], offsets)]
    return _arena_tables(case["hits"], offsets), entries, offsets


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("n_pass", "n_pairs", "pairs")):
        assert np.array_equal(np.asarray(g, np.uint64), np.asarray(w, np.uint64)), (what, name)


def _first(want, KP):
    """The result at KP from the reference's at 64: the order is total, so the first KP are a prefix."""
    return want[0], want[1], want[2][:, :KP]


def _rows_of(tables, lo, hi, ok):
    """(c, strand, score bits) of the eligible rows of one gene, by c."""
    out = []
    for s, name in enumerate(("plus", "minus")):
        pos = tables["pos_" + name].astype(np.int64)
        site = pos - 3 if s == 0 else pos
        inside = ok[name] & (site >= int(lo)) & (site <= int(hi))
        out += [(int(pref.boundary(p, s == 1)), s, int(k)) for p, k in zip(pos[inside], tables["score_" + name][inside].view(np.uint64))]
    return sorted(out)


# ---------------------------------------------------------------------------------------------- without a GPU
def test_numpy_statement_equals_the_plain_loop(case):
    tables, entries, _ = _host_arena(case)
    lo, hi, gene = ref.layout(case["genes"], entries, 0)
    ok = pref.eligible_numpy(tables)
    size = np.array([len(_rows_of(tables, a, b, ok)) for a, b in zip(lo, hi)])
    pick = np.flatnonzero(size <= 300)  # (the loop is quadratic)
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
    total = 0
    for dmin, dmax, mask, fs in WINDOWS:
        a = pref.pairs_numpy(tables, lo[pick], hi[pick], 5, dmin, dmax, mask, fs)
        b = pref.pairs_loop(tables, lo[pick], hi[pick], 5, dmin, dmax, mask, fs)
        _same(a, b, (dmin, dmax, mask, fs))
        total += int(a[1].sum())
    assert total > 10000
    a = pref.pairs_numpy(tables, lo[pick], hi[pick], 64, 20, 400, 0xF, True, 0.3, spec, cds, also)
    b = pref.pairs_loop(tables, lo[pick], hi[pick], 64, 20, 400, 0xF, True, 0.3, spec, cds, also)
    _same(a, b, "all terms")
    assert a[1].sum() > 100 and (a[0] < pref.pairs_numpy(tables, lo[pick], hi[pick], 1, 20, 400)[0]).any()


def test_boundary_is_the_repair_cut_and_not_the_cut_site():
    for pos in (3, 64, 1000, 12345):
        for minus in (False, True):
            assert pref.boundary(pos, minus) == repair_reference.cut(pos, minus)
    assert pref.boundary(100, True) != 100  # the CSV's cutsite of a '-' row is j


def test_nickase_offset_of_a_pam_out_pair_is_d_minus_34(oracle):
    """A hand-built PAM-out pair: a '-' guide (CCN + protospacer) on the left, a '+' guide (protospacer + NGG) on the
    right, `gap` letters between the protospacers' PAM-distal ends: D = gap + 34 at guide length 20."""
    rng = np.random.default_rng(3)
    rand = lambda n: rng.choice(np.frombuffer(b"AT", dtype=np.uint8), n).tobytes()  # (A/T only: no PAM by accident)
    for gap in (0, 7, 20):
        left = b"CCA" + rand(20)         # the '-' site: CCN at j, protospacer s[j + 3 : j + 23]
        right = rand(20) + b"AGG"        # the '+' site: protospacer s[i - 20 : i], NGG at i
        text = rand(40) + left + rand(gap) + right + rand(40)
        h = oracle.scan_score(text, 20)
        j, i = 40, 40 + 23 + gap + 20
        assert j in h["pos_minus"].tolist() and i in h["pos_plus"].tolist()
        # the protospacers' PAM-distal ends: s[j + 23) on the left, s[i - 20] on the right
        assert (i - 20) - (j + 23) == gap
        D = pref.boundary(i, False) - pref.boundary(j, True)
        assert D - 34 == gap
        tables = dict(pos_plus=h["pos_plus"], score_plus=np.where(h["score_plus"] == -1.0, 0.5, h["score_plus"]), pos_minus=h["pos_minus"],
                      score_minus=np.where(h["score_minus"] == -1.0, 0.5, h["score_minus"]))
        n_pass, n_pairs, pairs = pref.pairs_numpy(tables, [0], [len(text)], 5, gap + 34, gap + 34, pref.PAM_OUT)
        want = [h["pos_minus"].tolist().index(j) | 1 << 31, h["pos_plus"].tolist().index(i)]
        assert n_pairs[0] == 1 and pairs[0, 0].tolist() == want
        assert pref.pairs_numpy(tables, [0], [len(text)], 5, gap + 34, gap + 34, pref.PAM_IN)[1][0] == 0


def test_pair_params_refusals():
    p = sel.PairParams(5)
    assert (p.k, p.dmin, p.dmax, p.frameshift, p.mask) == (5, 50, 500, False, 0xF)
    assert sel.PairParams(1, 30, 54, True, "pam-out").mask == 4 and sel.PairParams(1, orientation="pam-in").mask == 2
    assert sel.PairParams(64, 1, 65535, orientation=8).mask == 8
    for bad in (dict(k=0), dict(k=65), dict(k=5, dmin=0), dict(k=5, dmin=60, dmax=50), dict(k=5, dmax=65536), dict(k=5, orientation="sideways"),
                dict(k=5, orientation=0), dict(k=5, orientation=16)):
        with pytest.raises(ValueError):
            sel.PairParams(**bad)
    q = sel.PairParams(7, 3, 9, True, "pam-out").native()
    assert (q.k, q.dmin, q.dmax, q.orientation_mask, q.frameshift) == (7, 3, 9, 4, 1)


def _two_text_arena():
    """One arena of two texts that both carry gene 0 (two contigs of one name), and gene 1 in the second text only."""
    offsets = np.array([64, 2048], np.uint64)
    pos_plus = np.array([100, 160, 260, 2100, 2180, 2300], np.uint32)
    score_plus = np.array([0.9, 0.88, 0.7, 0.8, 0.95, 0.6])
    pos_minus = np.array([120, 2120], np.uint32)
    score_minus = np.array([0.4, 0.85])
    tables = dict(pos_plus=pos_plus, score_plus=score_plus, pos_minus=pos_minus, score_minus=score_minus)
    lo, hi, gene = np.array([64, 2048, 2048], np.uint32), np.array([1063, 3047, 3047], np.uint32), np.array([0, 0, 1], np.uint64)
    return offsets, tables, lo, hi, gene


def test_assemble_pairs_for_a_gene_in_two_texts():
    offsets, tables, lo, hi, gene = _two_text_arena()
    KP = 3
    n_pass, n_pairs, pairs = pref.pairs_numpy(tables, lo, hi, KP, 10, 300)
    assert n_pairs.tolist() == [6, 6, 6] and (pairs != NONE).all()  # both texts fill their lists: the merge has to choose
    n_in, _, picked = ref.select_numpy(tables, lo, hi, 2)
    rp, rm = np.arange(6, dtype=np.uint64) + 100, np.arange(2, dtype=np.uint64) + 200
    part = dict(offsets=offsets, lengths=np.array([1000, 1000], np.uint64), group=[4, 7], gene=gene, n_in=n_in, n_pass=n_pass, sel=picked,
                pair_n_pairs=n_pairs, pair_list=pairs, repair_plus=rp, repair_minus=rm, **tables)
    got, total, rep = sel.assemble_pairs(2, KP, [part])
    assert total.tolist() == [12, 6]
    g0 = got[got["gene"] == 0]
    assert g0["rank"].tolist() == [1, 2, 3] and got[got["gene"] == 1]["rank"].tolist() == [1, 2, 3]
    # by hand: every pair of the two texts, none across them, in the definition's order
    cand = []
    for t, (first, n) in enumerate(((0, 3), (3, 3))):
        rows_t = [(int(pos_plus) - 3, 0, s, k) for k, (pos_plus, s) in enumerate(zip(tables["pos_plus"], tables["score_plus"])) if first <= k < first + n]
        rows_t += [(int(tables["pos_minus"][t]) + 6, 1, tables["score_minus"][t], t)]
        for ca, sa, xa, ra in rows_t:
            for cb, sb, xb, rb in rows_t:
                if 10 <= cb - ca <= 300:
                    cand.append((-min(xa, xb), -max(xa, xb), ca, cb, sa * 2 + sb, t, cb - ca, xa, xb))
    cand.sort()
    assert len(cand) == 12 and {c[5] for c in cand[:3]} == {0, 1}  # the first three come from both texts
    for r, c in zip(g0, cand[:3]):
        assert r["contig"] == [4, 7][c[5]] and r["deletion_length"] == c[6] and r["score_a"] == c[7] and r["score_b"] == c[8]
        base = int(offsets[c[5]])
        assert r["position_a"] == c[2] - base + (3 if r["strand_a"] == b"+" else -6) and r["position_b"] == c[3] - base + (3 if r["strand_b"] == b"+" else -6)
    # indices are local to the contig's table, and the repair values follow their rows
    second = got[(got["gene"] == 1)][0]
    assert second["contig"] == 7 and second["index_a"] < 3 and second["index_b"] < 3
    for r, (ra, rb) in zip(got, rep):
        t = [4, 7].index(int(r["contig"]))
        for side, v in (("a", ra), ("b", rb)):
            assert v == (200 + t if r["strand_" + side] == b"-" else 100 + 3 * t + r["index_" + side])


# ---------------------------------------------------------------------------------------------- on the GPU
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


PROPERTY_LIMITS = properties.Limits(gc_min=7, gc_max=14, max_run=4, max_t_run=3, max_stem=5)
REPAIR_LIMITS = repair.Limits(min_mh=300, min_oof=55)


def _scanned(engine, case, max_words):
    """A genome with its tables, annotation ids, joined specificity columns (M = 3), guide properties and repair scores
    resident, and per arena the reference's view of the same."""
    g = engine.genome(case["contigs"], max_words=max_words)
    request = annotate.Request(case["annotation"], case["names"], 0)
    hits = g.scan_score(20)
    counts = [(h.n_plus, h.n_minus) for h in hits.per_arena]
    feats = g.annotate(request, counts)
    props = g.guide_properties(counts)
    reps = g.repair_scores(counts, 30)
    pattern, gp, M, scheme = srch.check_specificity(20, 3)
    handles = []
    srch._self_handles(g, pattern, gp, srch.SPECIFICITY_PAM_LEN, M, scheme, None, None, handles)
    srch._self_compare_all(handles, M)
    arenas = []
    for a, (arena, group) in enumerate(zip(g.arenas, g.groups)):
        tables = _arena_tables([case["hits"][k] for k in group], [int(o) for o in arena.offsets])
        got = hits.per_arena[a]
        for key in tables:  # (the scan itself is pinned elsewhere; here it is the ground the selection stands on)
            assert np.array_equal(tables[key].view(np.uint8), getattr(got, key).view(np.uint8)), key
        entries = [(case["names"][k], 0, int(arena.lengths[j]), int(arena.offsets[j])) for j, k in enumerate(group)]
        lo, hi, gene = ref.layout(case["genes"], entries, 0)
        cp, sp, cm, sm = handles[a].join_hits(20)
        also = dict(plus=PROPERTY_LIMITS.passes(props[a][0]) & REPAIR_LIMITS.passes(reps[a][0]),
                    minus=PROPERTY_LIMITS.passes(props[a][1]) & REPAIR_LIMITS.passes(reps[a][1]))
        arenas.append(dict(tables=tables, lo=lo, hi=hi, gene=gene, ids=[case["ids"][int(x)] for x in gene], also=also,
                           spec=dict(counts_plus=cp, sum_plus=sp, counts_minus=cm, sum_minus=sm),
                           cds=dict(feat_plus=feats[a][0], feat_minus=feats[a][1], flags=case["annotation"].cds_flags())))
    return dict(genome=g, request=request, handles=handles, arenas=arenas, cache={})


@pytest.fixture(scope="module", params=[1, 3], ids=["one-arena", "three-arenas"])
def scanned(request, engine, case):
    s = _scanned(engine, case, None if request.param == 1 else 600)
    assert len(s["genome"].arenas) == request.param
    _assert_the_genome_contains_the_cases(s)
    yield s
    for h in s["handles"]:
        h.close()
    s["genome"].close()


ALL_TERMS = dict(min_score=0.2, spec=dict(max_mm0=2, max_hit_sum=1 << 34), cds=True, limits=True)


def _reference(s, a, window, min_score=0.0, spec=None, cds=False, limits=False):
    """pairs_numpy at KP = 64 for arena a, computed once per set of arguments."""
    key = (a, window, min_score, None if spec is None else tuple(sorted(spec.items())), cds, limits)
    if key not in s["cache"]:
        A = s["arenas"][a]
        dmin, dmax, mask, fs = window
        s["cache"][key] = pref.pairs_numpy(A["tables"], A["lo"], A["hi"], 64, dmin, dmax, mask, fs, min_score,
                                           None if spec is None else dict(A["spec"], **spec), A["cds"] if cds else None,
                                           A["also"] if limits else None)
    return s["cache"][key]


def _device(s, a, KP, window, pair_slice_rows=None, min_score=0.0, spec=None, cds=False, limits=False, genes=None):
    A = s["arenas"][a]
    lo, hi = (A["lo"], A["hi"]) if genes is None else (A["lo"][genes], A["hi"][genes])
    h = sel.ArenaSelect(s["genome"].arenas[a], lo, hi)
    try:
        params = sel.Params(1, min_score, require_cds=cds)
        if spec is not None:
            params.max_mm0, params.max_hit_sum = spec["max_mm0"], spec["max_hit_sum"]
        if cds:
            h.set_flags(A["cds"]["flags"])
        if limits:
            h.set_property_limits(PROPERTY_LIMITS)
            h.set_repair_limits(REPAIR_LIMITS)
        if pair_slice_rows:
            h.set_pair_limits(pair_slice_rows)
        dmin, dmax, mask, fs = window
        h.run_pairs(params, sel.PairParams(KP, dmin, dmax, fs, mask), s["handles"][a] if spec is not None else None)
        return h.fetch_pairs(), h.pairs_stats()
    finally:
        h.close()


def _eligible_counts(A):
    """Eligible rows (plain predicate) per strand of every gene of an arena."""
    t = A["tables"]
    ok = pref.eligible_numpy(t)
    out = []
    for lo, hi in zip(A["lo"], A["hi"]):
        rows_g = _rows_of(t, lo, hi, ok)
        out.append((sum(1 for r in rows_g if r[1] == 0), sum(1 for r in rows_g if r[1] == 1)))
    return np.array(out).reshape(-1, 2)


def _assert_the_genome_contains_the_cases(s):
    """On the reference's own rows: every size, edge and tie the GPU tests rely on is really there.  The `scanned` fixture
    calls it, so no test that takes the fixture runs on a genome that has lost one of them."""
    sizes, ids, classes, ties, edges, d0 = set(), [], set(), 0, set(), 0
    for a, A in enumerate(s["arenas"]):
        ids += A["ids"]
        by = {i: k for k, i in enumerate(A["ids"])}
        n = _eligible_counts(A)
        sizes.update(int(x) for x in n.sum(axis=1))
        t, ok = A["tables"], pref.eligible_numpy(A["tables"])
        for i in ("p_run63", "p_run64", "p_run65", "p_run129"):  # a-row trips +- 1 on the '+' strand, and likewise '-'
            if i in by:
                assert n[by[i]][0] == int(i[5:])
        for i in ("m_run63", "m_run64", "m_run65", "m_run129"):
            if i in by:
                assert n[by[i]][1] == int(i[5:])
        if "one_strand" in by:
            assert n[by["one_strand"]][0] >= 3 and n[by["one_strand"]][1] == 0
        if "plus_only" in by:
            assert tuple(n[by["plus_only"]]) == (1, 0)
        if "whole_c1" in by:
            assert n[by["whole_c1"]].sum() > 1024  # cut into several items at the default pair_slice_rows, too
        # n_pairs below, at and above KP = 5, at 50 .. 500 with frameshift
        fs = _reference(s, a, (50, 500, 0xF, True))
        classes.update(np.sign(fs[1].astype(np.int64) - 5)[fs[1] > 0].tolist())
        if (fs[1] == 0).any():
            classes.add("none")
        want = _reference(s, a, (50, 500, 0xF, False))
        if "repeat_core" in by:  # hundreds of pairs with equal min and max score: c_a and c_b decide, also at the boundary of every KP
            k = by["repeat_core"]
            top = want[2][k]

            def keys_of(pair):
                out = []
                for packed in pair:
                    minus, r = int(packed) >> 31, int(packed) & 0x7FFFFFFF
                    out.append(int(t["score_minus" if minus else "score_plus"][r].view(np.uint64)))
                return min(out), max(out)
            ks = [keys_of(p) for p in top]
            assert want[1][k] > 500
            for KP in (1, 5, 63):
                assert ks[KP - 1] == ks[KP]  # the KP-th and the next pair tie on both scores
            ties += 1
        # a partner run that starts at the gene's first row of a table, and one that ends at its last
        for k in range(len(A["lo"])):
            rows_g = _rows_of(t, A["lo"][k], A["hi"][k], ok)
            if len(rows_g) < 4:
                continue
            for strand in (0, 1):
                cs = [c for c, st, _ in rows_g if st == strand]
                if not cs:
                    continue
                for c, _, _ in rows_g:
                    inside = [x for x in cs if c + 50 <= x <= c + 500]
                    if inside and inside[0] == cs[0] and c < cs[0]:
                        edges.add("first")
                    if inside and inside[-1] == cs[-1]:
                        edges.add("last")
        if "palindrome" in by:  # two eligible rows with one CUT SITE -- their boundaries c lie 6 apart (i - 3 and j + 6, j = i - 3)
            k = by["palindrome"]
            rows_g = _rows_of(t, A["lo"][k], A["hi"][k], ok)
            assert len(rows_g) == 2 and rows_g[1][0] - rows_g[0][0] == 6 and (rows_g[0][1], rows_g[1][1]) == (0, 1)
        # rows with EQUAL c on the two strands (D = 0 must not pair): a '+' row at i and a '-' row at j = i - 9
        cp = set((t["pos_plus"].astype(np.int64) - 3)[ok["plus"]].tolist())
        d0 += len(cp & set((t["pos_minus"].astype(np.int64) + 6)[ok["minus"]].tolist()))
    assert {0, 1, 2} <= sizes
    assert classes >= {-1, 0, 1, "none"}
    assert ties == 1 and edges == {"first", "last"} and d0 > 10
    for i in ("one_strand", "short_pair", "repeat", "repeat_core", "whole_c1", "p_run63", "p_run64", "p_run65", "p_run129"):
        assert i in ids


@pytest.mark.gpu
def test_gpu_the_genome_contains_the_cases(scanned):
    """The case assertions by name (the fixture has made them already: a genome without its cases fails every GPU test)."""
    _assert_the_genome_contains_the_cases(scanned)


@pytest.mark.gpu
@pytest.mark.parametrize("pair_slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
@pytest.mark.parametrize("KP", KPS)
def test_gpu_pairs_equal_the_reference(scanned, KP, pair_slice_rows):
    s = scanned
    for a, A in enumerate(s["arenas"]):
        n = _eligible_counts(A).sum(axis=1)
        for window in WINDOWS:
            got, stats = _device(s, a, KP, window, pair_slice_rows)
            want = _reference(s, a, window)
            _same(got, _first(want, KP), "arena %d window %r" % (a, window))
            assert stats["qualifying_pairs"] == float(want[1].sum()) and stats["pair_evaluations"] >= stats["qualifying_pairs"]
            assert stats["launches"] >= 1 and stats["items"] >= len(A["lo"])
        if pair_slice_rows == 64 and len(s["arenas"]) == 1:
            assert (n > 64).sum() > 10 and stats["items"] > len(A["lo"]) + 10  # cut genes: the merge kernel ran
        want = _reference(s, a, (1, 1, 0xF, False))
        assert want[1].sum() > 0  # neighbouring boundaries exist, overlapping protospacers


@pytest.mark.gpu
def test_gpu_every_pair_of_a_contig(scanned):
    """1 .. 65 535 on whole_c1: every pair of a 20 kb contig qualifies, millions of them, one gene cut into pieces."""
    s = scanned
    done = 0
    for a, A in enumerate(s["arenas"]):
        if "whole_c1" not in A["ids"]:
            continue
        k = A["ids"].index("whole_c1")
        genes = np.array([k])
        want = pref.pairs_numpy(A["tables"], A["lo"][genes], A["hi"][genes], 64, 1, 65535)
        n = int(want[0][0])
        assert want[1][0] > 2000000 and want[1][0] <= n * (n - 1) // 2
        for rows_per_item in (None, 64):
            got, stats = _device(s, a, 64, (1, 65535, 0xF, False), rows_per_item, genes=genes)
            _same(got, want, "whole_c1")
            assert stats["items"] == -(-(_run_rows(A, k)) // (rows_per_item or 1024))
        done += 1
    assert done == 1


def _run_rows(A, k):
    """Rows of gene k's two runs, scored or not."""
    t = A["tables"]
    cp, cm = t["pos_plus"].astype(np.int64) - 3, t["pos_minus"].astype(np.int64)
    return int(((cp >= A["lo"][k]) & (cp <= A["hi"][k])).sum() + ((cm >= A["lo"][k]) & (cm <= A["hi"][k])).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("pair_slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
def test_gpu_all_predicate_terms_at_once(scanned, pair_slice_rows):
    """Joined columns with their sentinel rows, require_cds, property and repair limits together: a drift between the
    shared predicate and the select kernel's shows here (and in n_pass against the single-guide selection)."""
    s = scanned
    window = (20, 2000, 0xF, True)
    TERMS = (dict(min_score=0.5), dict(spec=dict(max_mm0=0, max_hit_sum=sel.max_hit_sum_for(0.5))), dict(cds=True), dict(limits=True))
    # on the reference's rows, over the whole genome: every term on its own takes rows away, all together take more and leave pairs
    total = lambda **terms: sum(int(_reference(s, a, window, **terms)[0].sum()) for a in range(len(s["arenas"])))
    plain_rows, all_rows = total(), total(**ALL_TERMS)
    assert 0 < all_rows < min(total(**terms) for terms in TERMS) and max(total(**terms) for terms in TERMS) < plain_rows
    assert sum(int(_reference(s, a, window, **ALL_TERMS)[1].sum()) for a in range(len(s["arenas"]))) > 50
    for a, A in enumerate(s["arenas"]):
        want = _reference(s, a, window, **ALL_TERMS)
        plain = _reference(s, a, window)
        for KP in (5, 64):
            got, _ = _device(s, a, KP, window, pair_slice_rows, **ALL_TERMS)
            _same(got, _first(want, KP), "arena %d" % a)
        for terms in TERMS:
            got, _ = _device(s, a, 5, window, pair_slice_rows, **terms)
            _same(got, _first(_reference(s, a, window, **terms), 5), "arena %d %r" % (a, sorted(terms)))
        if "n_run" in A["ids"]:  # sentinel rows of the join inside a gene: in it, never eligible
            k = A["ids"].index("n_run")
            joined_only = _reference(s, a, window, spec=dict(max_mm0=NONE, max_hit_sum=0xFFFFFFFFFFFFFFFF))
            assert joined_only[0][k] < plain[0][k]
            got, _ = _device(s, a, 5, window, pair_slice_rows, spec=dict(max_mm0=NONE, max_hit_sum=0xFFFFFFFFFFFFFFFF))
            _same(got, _first(joined_only, 5), "joined only")


@pytest.mark.gpu
def test_gpu_thresholds_that_leave_no_row(scanned):
    s = scanned
    for a, A in enumerate(s["arenas"]):
        got, stats = _device(s, a, 5, (50, 500, 0xF, False), min_score=2.0)
        assert (got[0] == 0).all() and (got[1] == 0).all() and (got[2] == NONE).all()
        assert stats["pair_evaluations"] == 0 and stats["qualifying_pairs"] == 0


@pytest.mark.gpu
def test_gpu_select_after_pairs_on_one_handle(scanned):
    """crp_select_run after crp_select_run_pairs: section 16's result, and the pairs' own stay fetchable."""
    s = scanned
    for a, A in enumerate(s["arenas"]):
        h = sel.ArenaSelect(s["genome"].arenas[a], A["lo"], A["hi"])
        try:
            h.set_pair_limits(64)
            h.run_pairs(sel.Params(1, 0.3), sel.PairParams(5, 50, 500))
            h.run(sel.Params(5, 0.3))
            n_in, n_pass, picked = h.fetch()
            want = ref.select_numpy(A["tables"], A["lo"], A["hi"], 5, 0.3)
            for g, w in zip((n_in, n_pass, picked), want):
                assert np.array_equal(g, w)
            pw = pref.pairs_numpy(A["tables"], A["lo"], A["hi"], 5, 50, 500, min_score=0.3)
            _same(h.fetch_pairs(), pw, "pairs after select")
            assert np.array_equal(pw[0], n_pass)  # one predicate: the two kernels count the same passing rows
        finally:
            h.close()


@pytest.mark.gpu
def test_gpu_calls_out_of_order(engine):
    L = nat.lib()
    arena = engine.arena([b"ACGTTGCAAGGCCTTAGGACCA" * 60])
    try:
        h = sel.ArenaSelect(arena, [0, 100], [50, 900])

        def status(fn):
            with pytest.raises(nat.CropsrHipError) as e:
                fn()
            return e.value.status, str(e.value)

        pp = sel.PairParams(5, 10, 200)
        assert status(h.fetch_pairs)[0] == nat.CRP_ERR_STATE                          # nothing has run
        st, text = status(lambda: h.run_pairs(sel.Params(5), pp))
        assert st == nat.CRP_ERR_STATE and "guide length 20" in text and "crp_select_run_pairs" in text  # no tables
        arena.scan_score_device(19)
        assert status(lambda: h.run_pairs(sel.Params(5), pp))[0] == nat.CRP_ERR_STATE   # a scan at another length
        n_plus, n_minus = arena.scan_score_device(20)
        st, text = status(lambda: h.run_pairs(sel.Params(5, require_cds=True), pp))
        assert st == nat.CRP_ERR_STATE and "crp_select_set_flags" in text
        h.set_flags(np.ones(3, np.uint8))
        st, text = status(lambda: h.run_pairs(sel.Params(5, require_cds=True), pp))
        assert st == nat.CRP_ERR_STATE and "crp_annotate_lookup" in text
        h.set_property_limits(properties.Limits(gc_min=5))                             # limits without their column
        st, text = status(lambda: h.run_pairs(sel.Params(5), pp))
        assert st == nat.CRP_ERR_STATE and "crp_guide_properties" in text
        h.set_property_limits(None)
        h.set_repair_limits(repair.Limits(min_mh=10))
        st, text = status(lambda: h.run_pairs(sel.Params(5), pp))
        assert st == nat.CRP_ERR_STATE and "crp_repair_scores" in text
        h.set_repair_limits(None)
        pattern, gp, M, scheme = srch.check_specificity(20, 3)
        handle = srch.ArenaSelfSearch(arena, pattern, gp, 3, M)
        try:
            st, text = status(lambda: h.run_pairs(sel.Params(5), pp, handle))
            assert st == nat.CRP_ERR_STATE and "joined" in text
        finally:
            handle.close()
        p = nat.SelectParams(0.0, 0, 0, 5, 0, 0)
        for bad, word in ((nat.SelectPairParams(0, 10, 200, 0xF, 0), "k must be"), (nat.SelectPairParams(65, 10, 200, 0xF, 0), "k must be"),
                          (nat.SelectPairParams(5, 0, 200, 0xF, 0), "distances"), (nat.SelectPairParams(5, 201, 200, 0xF, 0), "distances"),
                          (nat.SelectPairParams(5, 10, 65536, 0xF, 0), "distances"), (nat.SelectPairParams(5, 10, 200, 0, 0), "mask"),
                          (nat.SelectPairParams(5, 10, 200, 16, 0), "mask")):
            assert L.crp_select_run_pairs(h._h, ctypes.byref(p), ctypes.byref(bad), None) == nat.CRP_ERR_INVALID
            assert word in L.crp_last_error(engine._ctx).decode()
        assert L.crp_select_set_pair_limits(h._h, 63) == nat.CRP_ERR_INVALID
        assert status(h.fetch_pairs)[0] == nat.CRP_ERR_STATE                          # a failed run leaves nothing to fetch
        h.run_pairs(sel.Params(5), sel.PairParams(64, 10, 200))
        tables = dict(zip(("pos_plus", "_", "score_plus", "pos_minus", "__", "score_minus"), arena.fetch(n_plus, n_minus)))
        want = pref.pairs_numpy(tables, [0, 100], [50, 900], 64, 10, 200)
        assert want[1][1] > 64
        _same(h.fetch_pairs(), want)
        arena.scan_score_device(20)                                                    # a re-scan: the same tables again, a new run on them
        h.run_pairs(sel.Params(5), sel.PairParams(64, 10, 200))
        _same(h.fetch_pairs(), want)
        h.close()
    finally:
        arena.close()


@pytest.mark.gpu
def test_gpu_genome_level_call(engine, case):
    """Genome.scan_score(select=Request(pairs=...)): the pairs right after the single guides, inside the join's hook."""
    g = engine.genome(case["contigs"], max_words=600)
    try:
        request = annotate.Request(case["annotation"], case["names"], 0)
        params = sel.Params(5, 0.2, max_perfect=0, min_specificity=0.5, require_cds=True)
        pp = sel.PairParams(5, 40, 900, True)
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
            n_pass, n_pairs, pairs = pref.pairs_numpy(tables, lo, hi, 5, 40, 900, 0xF, True, 0.2, spec, cds, also)
            n_in, _, picked = ref.select_numpy(tables, lo, hi, 5, 0.2, spec, cds)  # (only n_in and the shape are used below)
            parts.append(dict(offsets=arena.offsets, lengths=arena.lengths, group=group, gene=gene, n_in=n_in, n_pass=n_pass, sel=picked,
                              pair_n_pairs=n_pairs, pair_list=pairs, repair_plus=hits.repair[a][0], repair_minus=hits.repair[a][1], **tables))
        W, total, rep = sel.assemble_pairs(len(S.labels), 5, parts)
        assert np.array_equal(S.n_pairs, total) and total.sum() > 20 and W.size > 10
        assert S.pairs.tobytes() == W.tobytes() and np.array_equal(S.pairs_repair, rep)
        assert np.array_equal(S.n_pass, np.bincount(np.concatenate([p["gene"] for p in parts]).astype(np.int64),
                                                    np.concatenate([p["n_pass"] for p in parts]), len(S.labels)).astype(np.int64))
        assert S.pairs_stats["items"] > 0 and S.pairs_stats["qualifying_pairs"] == float(total.sum())
        # a pair's guides are what the contig's own tables say at those indices, and D is the distance of their boundaries
        for r in S.pairs[:50]:
            hc = hits.contig(int(r["contig"]))
            c = []
            for side in "ab":
                strand = "plus" if r["strand_" + side] == b"+" else "minus"
                assert hc["pos_" + strand][r["index_" + side]] == r["position_" + side] and hc["score_" + strand][r["index_" + side]] == r["score_" + side]
                c.append(pref.boundary(int(r["position_" + side]), strand == "minus"))
            assert c[1] - c[0] == r["deletion_length"] and 40 <= r["deletion_length"] <= 900 and r["deletion_length"] % 3 != 0
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------- the command line
class PairingOracleBackend(OracleBackend):
    """OracleBackend plus the `select` keyword with pairs: both selections by the numpy statements over one host arena."""

    def scan(self, strings, l, offtarget=False, annotation=None, specificity=None, select=None):
        out = OracleBackend.scan(self, strings, l, offtarget=offtarget, annotation=annotation)
        if select is None:
            return out
        assert specificity is None and select.property_limits is None and select.repair_limits is None  # (the oracle has neither)
        texts = [bytes(s) for s in strings]
        offsets, off = [], 64
        for t in texts:
            offsets.append(off)
            off += ((len(t) + 63) // 64 + 1) * 64
        tables = _arena_tables(out, offsets)
        req = select.annotation
        lo, hi, gene = req.gene_layout([(k, o, len(t)) for k, (t, o) in enumerate(zip(texts, offsets))])
        cds = None
        if select.params.require_cds:
            from oracle import annotate_oracle
            feats = [annotate_oracle.host_join(req.annotation, req.names[k], req.starts[k], req.dec, h, l, len(t))
                     for k, (t, h) in enumerate(zip(texts, out))]
            cds = dict(feat_plus=np.concatenate([f[0] for f in feats]), feat_minus=np.concatenate([f[1] for f in feats]),
                       flags=req.annotation.cds_flags())
        n_in, n_pass, picked = ref.select_numpy(tables, lo, hi, select.params.k, select.params.min_score, None, cds)
        part = dict(offsets=np.array(offsets, np.uint64), lengths=np.array([len(t) for t in texts], np.uint64), group=list(range(len(texts))),
                    gene=gene, n_in=n_in, n_pass=n_pass, sel=picked, **tables)
        labels = req.annotation.genes()[0]
        out = sel.HitList(out)
        out.selection = sel.assemble(labels, select.params.k, [part])
        if select.pairs is not None:
            q = select.pairs
            _, part["pair_n_pairs"], part["pair_list"] = pref.pairs_numpy(tables, lo, hi, q.k, q.dmin, q.dmax, q.mask, q.frameshift,
                                                                          select.params.min_score, None, cds)
            S = out.selection
            S.pairs, S.n_pairs, S.pairs_repair = sel.assemble_pairs(len(labels), q.k, [part])
        return out


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


def _expected_pairs_file(case, main_rows, KP, dmin, dmax, mask, frameshift, min_score=0.0):
    """The pairs file's bytes from the main CSV's own rows and the numpy statement."""
    tables, entries, offsets = _host_arena(case)
    lo, hi, gene = ref.layout(case["genes"], entries, 0)
    n_pass, n_pairs, pairs = pref.pairs_numpy(tables, lo, hi, KP, dmin, dmax, mask, frameshift, min_score)
    by_key = {(r[4], r[6], r[8]): r for r in main_rows[1:] if len(r) >= 12}  # (chromosome, end_pos, strand)
    n_before = np.cumsum([0] + [len(h["pos_plus"]) for h in case["hits"]])
    m_before = np.cumsum([0] + [len(h["pos_minus"]) for h in case["hits"]])

    def guide(packed):
        minus, r = int(packed) >> 31, int(packed) & 0x7FFFFFFF
        c = int(np.searchsorted(m_before if minus else n_before, r, "right") - 1)
        h = case["hits"][c]
        pos = int(h["pos_minus"][r - m_before[c]]) if minus else int(h["pos_plus"][r - n_before[c]])
        main = by_key[(case["names"][c], str(pos + 3 if minus else pos), "-" if minus else "+")]
        # (the score from the hit table, as the writer takes it: the main table re-scores the last rows of a batch in the
        # reference's BLAS tail order, where the last digit may differ)
        score = float(h["score_minus"][r - m_before[c]] if minus else h["score_plus"][r - n_before[c]])
        assert abs(score - float(main[9])) < 1e-15
        return pref.boundary(pos, bool(minus)), case["names"][c], [main[5], main[6], main[7], main[8], main[2], score]

    want = []
    for row_of_layout, g in enumerate(gene):
        for rank in range(KP):
            if pairs[row_of_layout, rank, 0] == NONE:
                break
            (ca, chrom, fa), (cb, _, fb) = guide(pairs[row_of_layout, rank, 0]), guide(pairs[row_of_layout, rank, 1])
            want.append((int(g), rank, [case["genes"][int(g)][3], str(rank + 1), str(int(n_pairs[row_of_layout])), str(cb - ca),
                                        str(int((cb - ca) % 3 == 0)), chrom] + fa + fb))
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(["gene", "rank", "qualifying_pairs", "deletion_length", "in_frame", "chromosome"]
               + [n + s for s in ("_a", "_b") for n in ("start_pos", "end_pos", "cutsite", "strand", "sequence", "on_site_score")])
    for _, _, fields in sorted(want, key=lambda x: x[:2]):  # genes in GFF order
        w.writerow(fields)
    return buf.getvalue().encode(), len(want)


def test_cli_pairs_file_over_the_oracle(case, oracle, tmp_path, monkeypatch):
    plain, plain_out = _run(case, tmp_path, monkeypatch, ["--select", "5", "--select-min-score", "0.3"], PairingOracleBackend(oracle), "plain.csv")
    assert not os.path.exists(plain + ".pairs.csv")
    out, stdout = _run(case, tmp_path, monkeypatch, ["--select", "5", "--select-min-score", "0.3", "--select-pairs", "4", "--pairs-frameshift",
                                                      "--pairs-min-distance", "40", "--pairs-max-distance", "700"], PairingOracleBackend(oracle))
    for suffix in ("", ".selected.csv"):  # the main table and the selection file are what they were
        with open(plain + suffix, "rb") as a, open(out + suffix, "rb") as b:
            assert a.read() == b.read()
    assert stdout.replace("out.csv", "plain.csv") == plain_out
    want, n = _expected_pairs_file(case, _read(out), 4, 40, 700, 0xF, True, 0.3)
    assert n > 60
    with open(out + ".pairs.csv", "rb") as f:
        got = f.read()
    assert got == want  # bytes
    rows_got = _read(out + ".pairs.csv")
    assert all(int(r[3]) % 3 != 0 and r[4] == "0" and 40 <= int(r[3]) <= 700 for r in rows_got[1:])
    # pam-out to another file, default distances
    out2, _ = _run(case, tmp_path, monkeypatch, ["--select", "5", "--select-pairs", "2", "--pairs-orientation", "pam-out", "--pairs-output",
                                                 str(tmp_path / "p.csv")], PairingOracleBackend(oracle), "second.csv")
    assert not os.path.exists(out2 + ".pairs.csv")
    rows2 = _read(str(tmp_path / "p.csv"))
    want2, n2 = _expected_pairs_file(case, _read(out2), 2, 50, 500, pref.PAM_OUT, False)
    assert len(rows2) - 1 == n2 > 20 and all(r[9] == "-" and r[15] == "+" for r in rows2[1:])
    with open(str(tmp_path / "p.csv"), "rb") as f:
        assert f.read() == want2


def test_cli_default_output_is_unchanged_and_golden(oracle, tmp_path, monkeypatch, manifest):
    """Without the flags the main CSV is byte for byte the golden one (md5_libm)."""
    import hashlib
    from conftest import golden_fasta_path, run_cli
    data, _ = run_cli(tmp_path, monkeypatch, golden_fasta_path("sample", tmp_path), OracleBackend(oracle), manifest["seed"])
    assert hashlib.md5(data).hexdigest() == manifest["cases"]["sample"]["md5_libm"]
    assert not [n for n in os.listdir(tmp_path) if n.endswith(".pairs.csv") or n.endswith(".selected.csv")]


PAIR_REFUSALS = [
    (["--select-pairs", "5"], "--select-pairs belongs to --select"),
    (["--pairs-frameshift"], "belongs to --select-pairs"),
    (["--select", "5", "--pairs-min-distance", "10"], "belongs to --select-pairs"),
    (["--select", "5", "--pairs-max-distance", "10"], "belongs to --select-pairs"),
    (["--select", "5", "--pairs-orientation", "pam-out"], "belongs to --select-pairs"),
    (["--select", "5", "--pairs-output", "x.csv"], "belongs to --select-pairs"),
    (["--select", "5", "--select-pairs", "0"], "1..64"),
    (["--select", "5", "--select-pairs", "65"], "1..64"),
    (["--select", "5", "--select-pairs", "5", "--pairs-min-distance", "0"], "1 <= dmin"),
    (["--select", "5", "--select-pairs", "5", "--pairs-min-distance", "600"], "1 <= dmin"),
    (["--select", "5", "--select-pairs", "5", "--pairs-max-distance", "65536"], "65535"),
    (["--select", "5", "--select-pairs", "5", "--pairs-orientation", "sideways"], "pam-out"),
    (["--select", "5", "--select-pairs", "5", "-l", "19"], "-l 20"),
    (["--select", "5", "--select-pairs", "5", "--gpus", "2"], "one GPU"),
    (["--select", "5", "--select-pairs", "5", "--devices", "0,1"], "one GPU"),
    (["--select", "65", "--select-pairs", "5"], "1..64"),
]


@pytest.mark.parametrize("extra,text", PAIR_REFUSALS, ids=[" ".join(r[0]) for r in PAIR_REFUSALS])
def test_cli_refusals_come_before_any_side_effect(case, oracle, tmp_path, monkeypatch, extra, text):
    monkeypatch.chdir(tmp_path)
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9", "-g", case["gff_path"]] + extra
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=PairingOracleBackend(oracle), out=io.StringIO())
    assert "--select" in str(e.value.code) and text in str(e.value.code)
    assert os.listdir(tmp_path) == []


@pytest.mark.gpu
def test_gpu_command_line_end_to_end(case, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    out_csv = str(tmp_path / "out.csv")
    argv = ["-f", case["fasta_path"], "-g", case["gff_path"], "-o", out_csv, "--cas9", "--seed", "11", "--each-contig-once", "--specificity",
            "--select", "64", "--select-min-score", "0.2", "--select-max-perfect", "0", "--select-cds", "--repair-scores", "--select-pairs", "3",
            "--pairs-min-distance", "30", "--pairs-max-distance", "54", "--pairs-orientation", "pam-out", "--bench-json", str(tmp_path / "bench.json")]
    cli.run(cli.build_parser().parse_args(argv), out=io.StringIO())
    main, single, got = _read(out_csv), _read(out_csv + ".selected.csv"), _read(out_csv + ".pairs.csv")
    assert got[0][:6] == ["gene", "rank", "qualifying_pairs", "deletion_length", "in_frame", "chromosome"]
    assert got[0][-4:] == ["mh_score_a", "oof_score_a", "mh_score_b", "oof_score_b"] and len(got[0]) == 22 and len(got) > 10
    by_key = {(r[4], r[6], r[8]): r for r in main[1:] if len(r) == len(main[0])}
    for r in got[1:]:
        assert 30 <= int(r[3]) <= 54 and r[4] == str(int(int(r[3]) % 3 == 0)) and int(r[1]) <= min(3, int(r[2]))
        for at, strand in ((6, "-"), (12, "+")):
            m = by_key[(r[5], r[at + 1], r[at + 3])]
            assert r[at + 3] == strand and [r[at], r[at + 2], r[at + 4]] == [m[5], m[7], m[2]] and abs(float(r[at + 5]) - float(m[9])) < 1e-15
            assert float(r[at + 5]) >= 0.2 and m[main[0].index("self_mm0")] == "0"
        # D from the file's own fields: the '-' guide's boundary is its cutsite + 6, the '+' guide's its cutsite
        assert int(r[14]) - (int(r[8]) + 6) == int(r[3])
    # the repair fields are those the selection file prints for the same guide, where it holds it
    shown = {(r[6], r[8], r[10]): r[-2:] for r in single[1:]}
    hit = 0
    for r in got[1:]:
        for at, more in ((6, r[18:20]), (12, r[20:22])):
            k = (r[5], r[at + 1], r[at + 3])
            if k in shown:
                assert shown[k] == more
                hit += 1
    assert hit > 0
    import json
    with open(tmp_path / "bench.json") as f:
        stages = json.load(f)
    assert stages["pairs"]["items"] > 0 and stages["pairs"]["kp"] == 3 and stages["select"]["items"] > 0
