"""--select-min-spacing: K guides per gene whose cut sites lie at least D apart (cropsr_amd/select.py, DESIGN.md section
26, csrc/crp_select_spaced.hip).  The definition is restated twice in tests/select_spacing_reference.py -- by rounds in
numpy, as a walk in plain loops; the genome and its genes are those of tests/select_cases.py, and the device's columns
are made the way tests/test_select.py makes them.

Definition, per arena and per layout row g, after a scan at guide length 20: walk the passing rows of g -- those n_pass[g]
counts -- by higher score bits (unsigned 64-bit), then smaller cut site (i - 3 for '+', j for '-'), then '+' before '-';
take a row iff |cut - cut(p)| >= D for every row p already taken; stop at K taken.  n_pass does not depend on D,
n_spaced is the number taken, sel holds the rows taken in pick order (row | strand << 31), 0xFFFFFFFF beyond."""
import csv
import ctypes
import hashlib
import io
import json
import os

import numpy as np
import pytest

from conftest import OracleBackend

import select_cases as cases
import select_reference as ref
import select_spacing_reference as sp
import test_select as ts
from cropsr_amd import _native as nat
from cropsr_amd import annotate, cli, rows
from cropsr_amd import select as sel

KS = (1, 5, 64)
DS = (0, 1, 2, 20, 23, 40, 1000, 100000, (1 << 31) - 1)
NONE = 0xFFFFFFFF
# the main table and the selection file of `--select 5 --select-min-score 0.3` over the oracle backend, as the commit
# before the spaced selection wrote them (test_without_the_option_every_byte_is_what_it_was)
MD5_MAIN, MD5_SELECTED = "b496e88bec88c12150b6ff1781733727", "58656529d4d8db9b8077a06fbe5ad995"


@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    c = cases.build(oracle)
    d = tmp_path_factory.mktemp("select_spacing")
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
    """All contigs as one host arena: tables, the genes' layout rows and their ids, and a cache of reference results."""
    tables, entries, offsets = ts._host_arena(case)
    lo, hi, gene = ref.layout(case["genes"], entries, 0)
    ids = [case["ids"][int(g)] for g in gene]
    return dict(tables=tables, lo=lo, hi=hi, gene=gene, ids=ids, by={i: k for k, i in enumerate(ids)}, cache={})


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("n_pass", "n_spaced", "sel")):
        assert np.array_equal(np.asarray(g, np.uint32), np.asarray(w, np.uint32)), (what, name)


def _host_spaced(host, K, D):
    if (K, D) not in host["cache"]:
        host["cache"][(K, D)] = sp.spaced_numpy(host["tables"], host["lo"], host["hi"], K, D)
    return host["cache"][(K, D)]


def _cut(tables, packed):
    minus, r = int(packed) >> 31, int(packed) & 0x7FFFFFFF
    return int(tables["pos_minus"][r]) if minus else int(tables["pos_plus"][r]) - 3


# ---------------------------------------------------------------------------------------------- without a GPU
def test_numpy_statement_equals_the_plain_loop(host):
    tables, lo, hi = host["tables"], host["lo"], host["hi"]
    rng = np.random.default_rng(26)
    spec, cds = ts._synthetic_columns(tables, rng, 9)
    spec.update(max_mm0=1, max_hit_sum=1 << 32)
    pick = np.arange(0, len(lo), 3)  # (the loop visits every row for every gene: a spread of the genes is enough for it)
    for K, D in ((1, 20), (5, 0), (5, 1), (5, 23), (64, 20), (64, 1000), (64, (1 << 31) - 1)):
        _same(sp.spaced_numpy(tables, lo[pick], hi[pick], K, D), sp.spaced_loop(tables, lo[pick], hi[pick], K, D), "K=%d D=%d" % (K, D))
    _same(sp.spaced_numpy(tables, lo[pick], hi[pick], 64, 20, 0.55, spec, cds), sp.spaced_loop(tables, lo[pick], hi[pick], 64, 20, 0.55, spec, cds),
          "all thresholds")
    n_pass, n_spaced, picked = sp.spaced_numpy(tables, lo, hi, 5, 20, 0.55, spec, cds)
    assert (n_spaced <= np.minimum(n_pass, 5)).all() and ((picked != NONE).sum(axis=1) == n_spaced).all() and n_spaced.max() == 5


@pytest.mark.parametrize("K", KS)
def test_distance_zero_is_the_plain_selection(host, K):
    n_in, n_pass, picked = ref.select_numpy(host["tables"], host["lo"], host["hi"], K)
    got = _host_spaced(host, K, 0)
    _same(got, (n_pass, np.minimum(n_pass, K), picked), "D = 0")
    for D in DS[1:]:  # n_pass does not depend on D, and every pick clears every other
        n_pass_d, n_spaced, chosen = _host_spaced(host, K, D)
        assert np.array_equal(n_pass_d, n_pass) and (n_spaced <= np.minimum(n_pass, K)).all() and (n_spaced[n_pass > 0] >= 1).all()
        for g in np.flatnonzero(n_spaced > 1):
            cuts = np.sort([_cut(host["tables"], p) for p in chosen[g][:n_spaced[g]]])
            assert np.diff(cuts).min() >= D


def test_the_genome_contains_the_cases(host):
    """On the oracle's rows, before any device is looked at: every decision the GPU tests rely on is really there."""
    tables, lo, hi, by = host["tables"], host["lo"], host["hi"], host["by"]
    plain = lambda name, K: set(int(p) for p in ref.select_numpy(tables, lo[by[name]:by[name] + 1], hi[by[name]:by[name] + 1], K)[2][0] if p != NONE)
    one = lambda name, K, D: tuple(x[by[name]] for x in _host_spaced(host, K, D))
    # the palindrome's two rows share their cut site: at D = 1 the second is rejected at distance 0
    n_pass, n_spaced, picked = one("palindrome", 64, 1)
    assert (n_pass, n_spaced) == (2, 1) and picked[0] >> 31 == 0
    trace = sp.walk(tables, lo[by["palindrome"]], hi[by["palindrome"]], 64, 1)
    assert [(t[1], t[3], t[4]) for t in trace] == [(0, True, None), (1, False, 0)]
    assert one("palindrome", 64, 0)[1] == 2
    # fewer picks than K although enough rows pass
    n_pass, n_spaced, _ = one("p_run63", 64, 20)
    assert (n_pass, n_spaced) == (113, 27)
    # picks that the plain top K does not hold
    n_pass, n_spaced, picked = one("p_run129", 64, 20)
    assert (n_pass, n_spaced) == (257, 60) and len(set(picked[:n_spaced].tolist()) - plain("p_run129", 64)) == 20
    # a chain: a row within D of a REJECTED row and clear of every taken one is taken -- filtering the top K pairwise differs
    n_pass, n_spaced, picked = one("p_run5", 5, 23)
    assert (n_pass, n_spaced) == (11, 3)
    trace = sp.walk(tables, lo[by["p_run5"]], hi[by["p_run5"]], 5, 23)
    rejected = [t[0] for t in trace if not t[3]]
    chained = [t for t in trace if t[3] and t[4] is not None and any(abs(t[0] - r) < 23 for r in rejected[:trace.index(t)])]
    assert chained and chained[0][4] >= 23
    # ... and testing against the latest pick alone would take a row that an earlier pick forbids
    taken = [t[0] for t in trace if t[3]]
    assert any(not t[3] and abs(t[0] - [p for p in taken if trace.index(t) > [x[0] for x in trace].index(p)][-1]) >= 23 for t in trace[1:])
    # a row taken at exactly D and another rejected at exactly D - 1
    trace = sp.walk(tables, lo[by["nested"]], hi[by["nested"]], 64, 20)
    assert any(t[3] and t[4] == 20 for t in trace) and any(not t[3] and t[4] == 19 for t in trace)
    assert one("nested", 64, 20)[:2] == (131, 34)
    # the repeat: ties decide, and the picks leave the plain top K
    n_pass, n_spaced, picked = one("repeat", 5, 40)
    assert (n_pass, n_spaced) == (170, 5) and len(set(picked.tolist()) - plain("repeat", 5)) == 4
    scores = np.concatenate([tables["score_plus"], tables["score_minus"]]).view(np.uint64)
    assert len({int(scores[(int(p) & 0x7FFFFFFF) + (len(tables["pos_plus"]) if int(p) >> 31 else 0)]) for p in picked}) < 5
    # a gene of some 40 items at slices of 64: reaches K, stops early, takes one
    k = by["whole_c1"]
    assert _host_spaced(host, 64, 20)[0][k] == 2554
    assert [int(_host_spaced(host, 64, D)[1][k]) for D in (20, 1000, 100000)] == [64, 15, 1]
    # cuts near the arena's first position
    n_pass, n_spaced, picked = one("first_rows", 5, 20)
    assert n_spaced == 5 and min(_cut(tables, p) for p in picked) < 64 + 100
    # every D of the GPU tests changes something somewhere; no text has 100 000 letters, so from there on a gene gets one pick
    results = [_host_spaced(host, 64, D)[2].tobytes() for D in DS]
    assert len(set(results[:-1])) == len(DS) - 1 and results[-1] == results[-2]
    assert (_host_spaced(host, 64, DS[-1])[1] <= 1).all()


def test_the_bench_tools_host_check_equals_the_reference(host):
    """tools/spacing_bench.py checks sampled genes of the device's result against its own numpy statement: that one against
    the reference, on the case genome."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "spacing_bench.py")
    spec = importlib.util.spec_from_file_location("spacing_bench", path)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    t = host["tables"]
    cols = (t["pos_plus"], t["score_plus"], t["pos_minus"], t["score_minus"])
    for K, D in bench.SETS + ((5, 0), (64, 1)):
        _same(bench.host_spaced(cols, host["lo"], host["hi"], K, D), _host_spaced(host, K, D), "K=%d D=%d" % (K, D))


def test_request_refusals(case):
    request = annotate.Request(case["annotation"], case["names"], 0)
    params = sel.Params(5)
    from cropsr_amd import baseedit, coding
    assert sel.Request(params, request, min_spacing=20).min_spacing == 20 and sel.Request(params, request).min_spacing is None
    assert sel.Request(params, request, min_spacing=0).min_spacing == 0
    assert sel.Request(params, request, min_spacing=(1 << 31) - 1, coding=True, pairs=sel.PairParams(3)).min_spacing == (1 << 31) - 1
    for bad in (-1, 1 << 31, 2.5, "20", True):
        with pytest.raises(ValueError, match="min_spacing"):
            sel.Request(params, request, min_spacing=bad)
    for limits in (dict(coding_limits=coding.Limits(0, 100, 0)), dict(edit_limits=baseedit.Limits(0, 100, 20)),
                   dict(splice_limits=baseedit.SpliceLimits(0, 100, 20, "any")), dict(families=object(), min_members=2),
                   dict(families=object(), max_perfect_outside=0), dict(families=object(), min_specificity_outside=0.5)):
        with pytest.raises(ValueError, match="spaced selection"):
            sel.Request(params, request, min_spacing=20, **limits)


class SpacingOracleBackend(OracleBackend):
    """OracleBackend plus the `select` keyword, with min_spacing: the plain selection by select_numpy for n_in and n_pass, the
    rows by spaced_numpy, over one host arena -- what select_arena does with the device."""

    def scan(self, strings, l, offtarget=False, annotation=None, specificity=None, select=None):
        out = OracleBackend.scan(self, strings, l, offtarget=offtarget, annotation=annotation)
        if select is None:
            return out
        assert specificity is None and not select.params.require_cds
        texts = [bytes(s) for s in strings]
        offsets, off = [], 64
        for t in texts:
            offsets.append(off)
            off += ((len(t) + 63) // 64 + 1) * 64
        tables = ts._arena_tables(out, offsets)
        req = select.annotation
        lo, hi, gene = req.gene_layout([(k, o, len(t)) for k, (t, o) in enumerate(zip(texts, offsets))])
        n_in, n_pass, picked = ref.select_numpy(tables, lo, hi, select.params.k, select.params.min_score)
        if select.min_spacing is not None:
            spaced_pass, _, picked = sp.spaced_numpy(tables, lo, hi, select.params.k, select.min_spacing, select.params.min_score)
            assert np.array_equal(spaced_pass, n_pass)
        part = dict(offsets=np.array(offsets, np.uint64), lengths=np.array([len(t) for t in texts], np.uint64), group=list(range(len(texts))),
                    gene=gene, n_in=n_in, n_pass=n_pass, sel=picked, **tables)
        out = sel.HitList(out)
        out.selection = sel.assemble(req.annotation.genes()[0], select.params.k, [part])
        return out


def _expected_file_rows(case, main_rows, K, D, min_score):
    """The selection file from the main CSV's own rows and the reference's picks."""
    tables, entries, offsets = ts._host_arena(case)
    lo, hi, gene = ref.layout(case["genes"], entries, 0)
    n_pass, n_spaced, picked = sp.spaced_numpy(tables, lo, hi, K, D, min_score)
    by_key = {(r[4], r[6], r[8]): r for r in main_rows[1:] if len(r) >= 12}
    n_before = np.cumsum([0] + [len(h["pos_plus"]) for h in case["hits"]])
    m_before = np.cumsum([0] + [len(h["pos_minus"]) for h in case["hits"]])
    want = []
    for row_of_layout, g in enumerate(gene):
        for rank, packed in enumerate(picked[row_of_layout][:n_spaced[row_of_layout]]):
            minus, r = int(packed) >> 31, int(packed) & 0x7FFFFFFF
            c = int(np.searchsorted(m_before if minus else n_before, r, "right") - 1)
            h = case["hits"][c]
            end = int(h["pos_minus"][r - m_before[c]]) + 3 if minus else int(h["pos_plus"][r - n_before[c]])
            main = by_key[(case["names"][c], str(end), "-" if minus else "+")]
            want.append((int(g), rank, [case["genes"][int(g)][3], str(rank + 1), str(int(n_pass[row_of_layout]))] + main[1:]))
    return [w[2] for w in sorted(want, key=lambda w: w[:2])]  # genes in GFF order, ranks in pick order


def test_cli_selection_file_over_the_oracle(case, oracle, tmp_path, monkeypatch):
    out, _ = ts._run(case, tmp_path, monkeypatch, ["--select", "5", "--select-min-score", "0.3", "--select-min-spacing", "40"],
                     SpacingOracleBackend(oracle))
    main, got = ts._read(out), ts._read(out + ".selected.csv")
    assert got[0] == ["gene", "rank", "passing"] + rows.HEADER[1:]  # the columns do not change
    want = _expected_file_rows(case, main, 5, 40, 0.3)
    assert len(got) - 1 == len(want) and len(want) > 100
    for g, w in zip(got[1:], want):
        assert g[:11] == w[:11] and abs(float(g[11]) - float(w[11])) < 1e-15 and g[12:] == w[12:], (g, w)
    # the spacing changed the file: the plain selection's rows are others
    plain = ts._expected_selection_rows(case, main, 5, 0.3)
    assert [w[:11] for w in plain] != [w[:11] for w in want]
    # `passing` stays n_pass; the ranks of a gene count up from 1; the guides of one gene and one contig cut >= 40 apart
    for label in ("gene:repeat", "gene:whole_c1", "gene:p_run129"):
        mine = [r for r in got[1:] if r[0] == label]
        assert [int(r[1]) for r in mine] == list(range(1, len(mine) + 1)) and len({r[2] for r in mine}) == 1 and int(mine[0][2]) > 5
        cuts = sorted(int(r[9]) for r in mine)
        assert len(mine) == 5 and min(b - a for a, b in zip(cuts, cuts[1:])) >= 40


def _md5(path):
    with open(path, "rb") as f:
        return hashlib.md5(f.read()).hexdigest()


def test_without_the_option_every_byte_is_what_it_was(case, oracle, tmp_path, monkeypatch):
    plain, plain_out = ts._run(case, tmp_path, monkeypatch, ["--select", "5", "--select-min-score", "0.3"], SpacingOracleBackend(oracle), "plain.csv")
    assert (_md5(plain), _md5(plain + ".selected.csv")) == (MD5_MAIN, MD5_SELECTED)
    spaced, spaced_out = ts._run(case, tmp_path, monkeypatch, ["--select", "5", "--select-min-score", "0.3", "--select-min-spacing", "40"],
                                 SpacingOracleBackend(oracle), "spaced.csv")
    assert _md5(spaced) == MD5_MAIN and _md5(spaced + ".selected.csv") != MD5_SELECTED  # the main table is what it was
    assert plain_out.replace("plain.csv", "X") == spaced_out.replace("spaced.csv", "X")


REFUSALS = [
    (["--select-min-spacing", "20"], "belongs to --select"),
    (["--select", "5", "--select-min-spacing", "0"], "1..2147483647"),
    (["--select", "5", "--select-min-spacing", "-3"], "1..2147483647"),
    (["--select", "5", "--select-min-spacing", "2147483648"], "1..2147483647"),
    (["--select", "5", "--select-min-spacing", "20", "--select-coding-min", "5"], "coding-position filter"),
    (["--select", "5", "--select-min-spacing", "20", "--select-coding-max", "65"], "coding-position filter"),
    (["--select", "5", "--select-min-spacing", "20", "--select-transcripts", "50"], "coding-position filter"),
    (["--select", "5", "--select-min-spacing", "20", "--select-stop"], "stop-codon filter"),
    (["--select", "5", "--select-min-spacing", "20", "--select-stop-max", "50"], "stop-codon filter"),
    (["--select", "5", "--select-min-spacing", "20", "--select-splice", "donor"], "splice-site filter"),
    (["--select", "5", "--select-min-spacing", "20", "--select-splice-max", "50"], "splice-site filter"),
    (["--select", "5", "--select-min-spacing", "20", "--specificity", "--families", "@FAMILIES@", "--select-min-members", "2"], "family filter"),
    (["--select", "5", "--select-min-spacing", "20", "--specificity", "--families", "@FAMILIES@", "--select-max-perfect-outside", "0"],
     "family filter"),
]


@pytest.mark.parametrize("extra,text", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_cli_refusals_come_before_any_side_effect(case, oracle, tmp_path, tmp_path_factory, monkeypatch, extra, text):
    families = tmp_path_factory.mktemp("families") / "families.tsv"
    families.write_text("nested\tf1\nouter\tf1\n")
    monkeypatch.chdir(tmp_path)
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9", "-g", case["gff_path"]] + [str(families) if x == "@FAMILIES@" else x for x in extra]
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=SpacingOracleBackend(oracle), out=io.StringIO())
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
def scanned(request, engine, case):
    s = ts._scanned(engine, case, None if request.param == 1 else 600)
    assert len(s["genome"].arenas) == request.param
    yield s
    for h in s["handles"]:
        h.close()
    s["genome"].close()


def _reference(s, a, K, D, min_score=0.0, spec=None, cds=False):
    """spaced_numpy for arena a, computed once per set of arguments."""
    key = ("spaced", a, K, D, min_score, None if spec is None else tuple(sorted(spec.items())), cds)
    if key not in s["cache"]:
        A = s["arenas"][a]
        s["cache"][key] = sp.spaced_numpy(A["tables"], A["lo"], A["hi"], K, D, min_score, None if spec is None else dict(A["spec"], **spec),
                                          A["cds"] if cds else None)
    return s["cache"][key]


def _handle(s, a, slice_rows=None, cds=False):
    A = s["arenas"][a]
    h = sel.ArenaSelect(s["genome"].arenas[a], A["lo"], A["hi"])
    if cds:
        h.set_flags(A["cds"]["flags"])
    if slice_rows:
        h.set_limits(slice_rows)
    return h


def _params(K, min_score=0.0, spec=None, cds=False):
    params = sel.Params(K, min_score, require_cds=cds)
    if spec is not None:
        params.max_mm0, params.max_hit_sum = spec["max_mm0"], spec["max_hit_sum"]
    return params


def _device(s, a, K, D, slice_rows=None, min_score=0.0, spec=None, cds=False):
    h = _handle(s, a, slice_rows, cds)
    try:
        h.run_spaced(_params(K, min_score, spec, cds), D, s["handles"][a] if spec is not None else None)
        return h.fetch_spaced(), h.spaced_stats()
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
@pytest.mark.parametrize("K", KS)
def test_gpu_spaced_selection_equals_the_reference(scanned, K, slice_rows):
    s = scanned
    for a, A in enumerate(s["arenas"]):
        n_p, n_m = ts._run_lengths(A)
        cut_genes = int(((n_p + n_m) > (slice_rows or 65536)).sum())
        h = _handle(s, a, slice_rows)
        try:
            h.run(_params(K))
            plain = h.fetch()
            for D in DS:
                h.run_spaced(_params(K), D)
                got, stats = h.fetch_spaced(), h.spaced_stats()
                _same(got, _reference(s, a, K, D), "arena %d D %d" % (a, D))
                if D == 0:  # the plain selection's own rows, from the same handle
                    assert np.array_equal(got[2], plain[2]) and np.array_equal(got[0], plain[1])
                assert stats["spaced_cut_genes"] == cut_genes and stats["spaced_rounds"] <= (K if cut_genes else 0)
                # the bounded-launch rule: the two key launches, one for the whole genes, a step and a pick a round
                assert stats["spaced_launches"] <= 2 * K + 3 and stats["spaced_launches"] == 2 + 1 + 2 * stats["spaced_rounds"]
            _same(h.fetch(), plain, "the plain results stay")
        finally:
            h.close()
        if slice_rows == 64 and len(s["arenas"]) == 1:
            assert cut_genes > 10


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
def test_gpu_thresholds(scanned, slice_rows):
    s = scanned
    for a, A in enumerate(s["arenas"]):
        # nothing passes
        (n_pass, n_spaced, picked), _ = _device(s, a, 5, 20, slice_rows, min_score=2.0)
        assert (n_pass == 0).all() and (n_spaced == 0).all() and (picked == NONE).all()
        # exactly K pass in the arena's largest gene: min_score = its K-th best score, where the next one is lower
        n_in, _, _ = ref.select_numpy(A["tables"], A["lo"], A["hi"], 1)
        if n_in.max() < 100:
            continue
        g = int(n_in.argmax())
        t = A["tables"]
        scores = np.concatenate([t["score_plus"][(t["pos_plus"].astype(np.int64) - 3 >= A["lo"][g]) & (t["pos_plus"].astype(np.int64) - 3 <= A["hi"][g])],
                                 t["score_minus"][(t["pos_minus"] >= A["lo"][g]) & (t["pos_minus"] <= A["hi"][g])]])
        scores = np.sort(scores[scores != -1.0])[::-1]
        K = next(k for k in range(5, 60) if scores[k - 1] > scores[k])
        for D in (1, 20):
            want = _reference(s, a, K, D, float(scores[K - 1]))
            assert want[0][g] == K
            got, _ = _device(s, a, K, D, slice_rows, min_score=float(scores[K - 1]))
            _same(got, want, "exactly K pass, D %d" % D)
        assert _reference(s, a, K, 1, float(scores[K - 1]))[1][g] == K or len(s["arenas"]) > 1


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
@pytest.mark.parametrize("K", KS)
def test_gpu_specificity_columns_and_cds(scanned, K, slice_rows):
    """Joined columns at M = 3 with their sentinel rows, and require_cds, made as tests/test_select.py makes them."""
    s = scanned
    for a in range(len(s["arenas"])):
        for spec in (dict(max_mm0=NONE, max_hit_sum=0xFFFFFFFFFFFFFFFF),  # only "joined"
                     dict(max_mm0=0, max_hit_sum=sel.max_hit_sum_for(0.5))):
            got, _ = _device(s, a, K, 20, slice_rows, 0.2, spec)
            _same(got, _reference(s, a, K, 20, 0.2, spec), "spec arena %d" % a)
        spec = dict(max_mm0=2, max_hit_sum=1 << 34)
        got, _ = _device(s, a, K, 40, slice_rows, 0.0, spec, cds=True)
        want = _reference(s, a, K, 40, 0.0, spec, cds=True)
        _same(got, want, "cds arena %d" % a)
        by = {i: k for k, i in enumerate(s["arenas"][a]["ids"])}
        if "no_cds" in by:
            assert want[0][by["no_cds"]] == 0 and _reference(s, a, K, 40)[0][by["no_cds"]] > 0
        if "n_run" in by:  # the unjoined rows are in the gene and never pass
            assert _reference(s, a, K, 20, 0.0, dict(max_mm0=NONE, max_hit_sum=0xFFFFFFFFFFFFFFFF))[0][by["n_run"]] < _reference(s, a, K, 20)[0][by["n_run"]]


@pytest.mark.gpu
def test_gpu_one_handle_through_every_run(engine, case):
    """Plain, spaced, pairs, spaced with a smaller K, a rescan: after every step the result equals the reference and a fresh
    handle's, and the earlier results of the other runs stay."""
    import select_pairs_reference as pairs_ref
    s = ts._scanned(engine, case, None)
    try:
        A = s["arenas"][0]
        fresh = lambda K, D: _device(s, 0, K, D, 64)[0]
        h = _handle(s, 0, 64)
        try:
            h.run(_params(64))
            plain = h.fetch()
            ts._same(plain, ref.select_numpy(A["tables"], A["lo"], A["hi"], 64), "plain")
            h.run_spaced(_params(64), 20)
            got = h.fetch_spaced()
            _same(got, _reference(s, 0, 64, 20), "spaced")
            _same(got, fresh(64, 20), "spaced, a fresh handle")
            ts._same(h.fetch(), plain, "plain after spaced")
            h.run_pairs(_params(64), sel.PairParams(5, 50, 500))
            pairs = h.fetch_pairs()
            want = pairs_ref.pairs_numpy(A["tables"], A["lo"], A["hi"], 5, 50, 500)
            assert all(np.array_equal(g, w) for g, w in zip(pairs, want))
            _same(h.fetch_spaced(), got, "spaced after pairs")
            h.run_spaced(_params(5), 1000)  # the pass keys are shared with the pair run: written again by this run
            small = h.fetch_spaced()
            assert small[2].shape == (len(A["lo"]), 5)
            _same(small, _reference(s, 0, 5, 1000), "spaced, a smaller K")
            _same(small, fresh(5, 1000), "spaced, a smaller K, a fresh handle")
            assert all(np.array_equal(g, w) for g, w in zip(h.fetch_pairs(), pairs))
            ts._same(h.fetch(), plain, "plain after everything")
            # a rescan: the same tables again, the handle still good
            s["genome"].scan_score(20)
            h.run_spaced(_params(64), 23)
            _same(h.fetch_spaced(), _reference(s, 0, 64, 23), "after a rescan")
            _same(h.fetch_spaced(), fresh(64, 23), "after a rescan, a fresh handle")
        finally:
            h.close()
    finally:
        for handle in s["handles"]:
            handle.close()
        s["genome"].close()


@pytest.mark.gpu
def test_gpu_a_gene_longer_than_the_rows_a_wave_remembers(engine):
    """A whole gene keeps an out-for-good bit for the rows of its first 128 trips (8 192 rows) and tests the rows behind them
    against every pick: a gene of some 237 trips in one item, so that both kinds of rows hold candidates and picks, on the
    device's own tables; and the same genes at slices of 64, where nothing is remembered."""
    rng = np.random.default_rng(2026)
    text = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 120000).tobytes()
    arena = engine.arena([text])
    try:
        n_plus, n_minus = arena.scan_score_device(20)
        tables = dict(zip(("pos_plus", "_", "score_plus", "pos_minus", "__", "score_minus"), arena.fetch(n_plus, n_minus)))
        trips = (n_plus + 63) // 64, (n_minus + 63) // 64
        assert trips[0] < 128 < trips[0] + trips[1] - 20  # the border lies inside the '-' strand's rows
        first, end = int(arena.offsets[0]), int(arena.offsets[0]) + len(text) - 1
        lo = np.array([first, first, first + 60000, first + 100], np.uint32)
        hi = np.array([end, first + 50000, end, first + 110000], np.uint32)
        border = int(tables["pos_minus"][(128 - trips[0]) * 64])  # the first '-' row that is not remembered in the whole-contig gene
        for slice_rows in (None, 64):
            h = sel.ArenaSelect(arena, lo, hi)
            try:
                if slice_rows:
                    h.set_limits(slice_rows)
                for K, D in ((64, 0), (64, 20), (64, 1000), (64, 2400), (5, 40000)):
                    h.run_spaced(sel.Params(K), D)
                    want = sp.spaced_numpy(tables, lo, hi, K, D)
                    _same(h.fetch_spaced(), want, "slices %r K %d D %d" % (slice_rows, K, D))
                    if D in (1000, 2400):  # picks among the remembered rows and behind them, '-' rows on both sides of the border
                        minus = [int(tables["pos_minus"][int(p) & 0x7FFFFFFF]) for p in want[2][0][:want[1][0]] if int(p) >> 31]
                        assert min(minus) < border <= max(minus) and any(int(p) >> 31 == 0 for p in want[2][0][:want[1][0]])
                assert h.spaced_stats()["spaced_cut_genes"] == (4 if slice_rows else 0)
            finally:
                h.close()
    finally:
        arena.close()


@pytest.mark.gpu
def test_gpu_calls_out_of_order_and_error_codes(engine, case):
    from cropsr_amd import baseedit, coding
    from cropsr_amd import search as srch
    L = nat.lib()
    arena = engine.arena([b"ACGTTGCAAGGCCTTAGGACCA" * 60])
    try:
        h = sel.ArenaSelect(arena, [0, 100], [50, 900])

        def status(fn):
            with pytest.raises(nat.CropsrHipError) as e:
                fn()
            return e.value.status, str(e.value)

        assert status(h.fetch_spaced)[0] == nat.CRP_ERR_STATE                              # nothing has run
        st, text = status(lambda: h.run_spaced(sel.Params(5), 20))
        assert st == nat.CRP_ERR_STATE and "guide length 20" in text                         # no scan yet
        arena.scan_score_device(19)
        assert status(lambda: h.run_spaced(sel.Params(5), 20))[0] == nat.CRP_ERR_STATE      # a scan at another length
        n_plus, n_minus = arena.scan_score_device(20)
        st, text = status(lambda: h.run_spaced(sel.Params(5, require_cds=True), 20))
        assert st == nat.CRP_ERR_STATE and "crp_select_set_flags" in text
        h.set_flags(np.ones(3, np.uint8))
        st, text = status(lambda: h.run_spaced(sel.Params(5, require_cds=True), 20))
        assert st == nat.CRP_ERR_STATE and "crp_annotate_lookup" in text
        pattern, gp, M, scheme = srch.check_specificity(20, 3)
        handle = srch.ArenaSelfSearch(arena, pattern, gp, 3, M)
        try:
            st, text = status(lambda: h.run_spaced(sel.Params(5), 20, handle))
            assert st == nat.CRP_ERR_STATE and "joined" in text
        finally:
            handle.close()
        from cropsr_amd import properties
        h.set_property_limits(properties.Limits(0, 20, None, None, None))
        st, text = status(lambda: h.run_spaced(sel.Params(5), 20))
        assert st == nat.CRP_ERR_STATE and "crp_guide_properties" in text
        h.set_property_limits(None)
        for k in (0, 65):
            p = nat.SelectParams(0.0, 0, 0, k, 0, 0)
            assert L.crp_select_run_spaced(h._h, ctypes.byref(p), 20, None) == nat.CRP_ERR_INVALID
        p = nat.SelectParams(0.0, 0, 0, 5, 0, 0)
        assert L.crp_select_run_spaced(h._h, ctypes.byref(p), 1 << 31, None) == nat.CRP_ERR_INVALID
        assert L.crp_select_run_spaced(h._h, ctypes.byref(p), 0xFFFFFFFF, None) == nat.CRP_ERR_INVALID
        assert b"minimum distance" in L.crp_last_error(h._ctx)
        assert L.crp_select_run_spaced(None, ctypes.byref(p), 20, None) == nat.CRP_ERR_INVALID
        assert L.crp_select_run_spaced(h._h, None, 20, None) == nat.CRP_ERR_INVALID
        with pytest.raises(ValueError):
            h.run_spaced(sel.Params(5), -1)
        # limits whose item kernels own a predicate per gene and row
        for set_, clear, word in ((lambda: h.set_coding_limits(coding.Limits(0, 100, 0)), lambda: h.set_coding_limits(None), "coding limits"),
                                  (lambda: h.set_edit_limits(None, baseedit.Limits(0, 100, 20)), lambda: h.set_edit_limits(None, None), "edit limits"),
                                  (lambda: h.set_splice_limits(None, "cbe", baseedit.SpliceLimits(0, 100, 20, "any")),
                                   lambda: h.set_splice_limits(None, "cbe", None), "splice limits"),
                                  (lambda: h.set_family_limits(sel.FamilyLimits(2)), lambda: h.set_family_limits(None), "family limits")):
            set_()
            st, text = status(lambda: h.run_spaced(sel.Params(5), 20))
            assert st == nat.CRP_ERR_INVALID and word in text
            clear()
        assert status(h.fetch_spaced)[0] == nat.CRP_ERR_STATE                              # a failed run leaves nothing to fetch
        out = np.zeros(9)
        assert L.crp_select_spaced_stats(h._h, out.ctypes.data_as(nat.f64p), 10) == nat.CRP_ERR_INVALID
        assert L.crp_select_spaced_stats(None, out.ctypes.data_as(nat.f64p), 9) == nat.CRP_ERR_INVALID
        tables = None
        for D in (0, 20, (1 << 31) - 1):
            h.run_spaced(sel.Params(64), D)
            if tables is None:
                tables = dict(zip(("pos_plus", "_", "score_plus", "pos_minus", "__", "score_minus"), arena.fetch(n_plus, n_minus)))
            _same(h.fetch_spaced(), sp.spaced_numpy(tables, [0, 100], [50, 900], 64, D))
        assert L.crp_select_fetch_spaced(h._h, None, None, None) == nat.CRP_OK            # any pointer may be NULL
        # a handle without genes
        empty = sel.ArenaSelect(arena, [], [])
        empty.run_spaced(sel.Params(5), 20)
        assert all(x.size == 0 for x in empty.fetch_spaced()[:2])
        empty.close()
        h.close()
    finally:
        arena.close()


@pytest.mark.gpu
def test_gpu_genome_level_call_with_coding(engine, oracle, tmp_path):
    """Genome.scan_score(select=Request(coding=True, min_spacing=20)) on the genes of tests/select_coding_cases.py: the rows are
    the spaced picks, and their coding fields are select_coding_reference's on those rows."""
    import select_coding_cases as coding_cases
    import select_coding_reference as cref
    c = coding_cases.build(oracle)
    gff_path = str(tmp_path / "genes.gff")
    with open(gff_path, "w") as f:
        f.write(c["gff"])
    genes, models = ref.gff_genes(c["gff"]), cref.model_numpy(c["gff"])
    g = engine.genome(c["contigs"], max_words=600)
    try:
        request = annotate.Request(annotate.Annotation(gff_path), c["names"], 0)
        S = g.scan_score(20, select=sel.Request(sel.Params(5), request, coding=True, min_spacing=20)).selection
        tables, entries, _ = ts._host_arena(c)
        lo, hi, gene = ref.layout(genes, entries, 0)
        layout_rows = cref.layout_rows(c["gff"], entries, 0)
        positions = cref.positions_numpy(tables, models, layout_rows)
        n_in, plain_pass, _ = ref.select_numpy(tables, lo, hi, 5)
        n_pass, n_spaced, picked = sp.spaced_numpy(tables, lo, hi, 5, 20)
        assert np.array_equal(n_pass, plain_pass)
        assert np.array_equal(S.n_pass[gene.astype(np.int64)], n_pass) and np.array_equal(S.n_in[gene.astype(np.int64)], n_in)
        r, col = np.nonzero(picked != NONE)
        order = np.lexsort((col, gene[r]))  # the Selection lists the genes in file order
        r, col = r[order], col[order]
        n_plus = len(tables["pos_plus"])
        t = np.where(picked[r, col] >> 31 != 0, (picked[r, col] & 0x7FFFFFFF).astype(np.int64) + n_plus, picked[r, col].astype(np.int64))
        assert S.rows.size == r.size > 100 and np.array_equal(S.rows["gene"], gene[r]) and np.array_equal(S.rows["rank"], col + 1)
        cut = np.where(S.rows["strand"] == b"-", S.rows["position"], S.rows["position"] - 3)
        want_cut = np.concatenate([tables["pos_plus"].astype(np.int64) - 3, tables["pos_minus"].astype(np.int64)])[t]
        offs = np.array([e[3] for e in entries])
        assert np.array_equal(cut + offs[S.rows["contig"]], want_cut)
        assert np.array_equal(S.cds_offset, positions[0][r, t]) and np.array_equal(S.transcripts_cut, positions[1][r, t])
        assert np.array_equal(S.cds_length, [models[int(x)]["length"] for x in gene[r]])
        assert np.array_equal(S.transcripts, [models[int(x)]["n_tx"] for x in gene[r]])
        assert (S.cds_offset == cref.NOT_INSIDE).any() and (S.cds_offset != cref.NOT_INSIDE).any()
        assert S.stats["spaced_items"] > 0 and S.stats["spaced_launches"] >= 3 and S.stats["coding_eval_ms"] > 0
        # not the plain selection's rows, and the same counts
        plain = g.scan_score(20, select=sel.Request(sel.Params(5), request, coding=True)).selection
        assert plain.rows.tobytes() != S.rows.tobytes() and np.array_equal(plain.n_pass, S.n_pass) and "spaced_items" not in plain.stats
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_command_line_end_to_end(case, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    out_csv = str(tmp_path / "out.csv")
    argv = ["-f", case["fasta_path"], "-g", case["gff_path"], "-o", out_csv, "--cas9", "--seed", "11", "--each-contig-once",
            "--select", "5", "--select-min-score", "0.3", "--select-min-spacing", "40", "--bench-json", str(tmp_path / "bench.json")]
    cli.run(cli.build_parser().parse_args(argv), out=io.StringIO())
    main, got = ts._read(out_csv), ts._read(out_csv + ".selected.csv")
    assert got[0] == ["gene", "rank", "passing"] + main[0][1:]
    want = _expected_file_rows(case, main, 5, 40, 0.3)
    assert len(got) - 1 == len(want) and len(want) > 100
    for g, w in zip(got[1:], want):
        assert g[:11] == w[:11] and abs(float(g[11]) - float(w[11])) < 1e-15 and g[12:] == w[12:], (g, w)
    with open(tmp_path / "bench.json") as f:
        stage = json.load(f)["select"]
    assert stage["items"] > 0 and stage["spaced_items"] > 0 and stage["spaced_launches"] >= 3 and "spaced_key_ms" in stage


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["straddle", "top"])
def test_gpu_high_positions(engine, oracle, placement):
    """A gene's rows on either side of 2^30 (straddle) and within 2^20 of 2^31 (top), behind the filler contig of
    tests/high_position_cases.py: the distance arithmetic and the tie word cut << 1 | strand at the top of their range."""
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
        for slice_rows in (None, 64):
            h = sel.ArenaSelect(genome.arenas[0], lo, hi)
            try:
                if slice_rows:
                    h.set_limits(slice_rows)
                for K, D in ((5, 20), (64, 20), (64, (1 << 31) - 1), (33, 0)):
                    h.run_spaced(sel.Params(K), D)
                    want = sp.spaced_numpy(tables, lo, hi, K, D)
                    _same(h.fetch_spaced(), want, "%s K %d D %d" % (placement, K, D))
                    if D == 20 and K == 64 and placement == "straddle":  # picks on both sides of 2^30
                        cuts = [_cut(tables, p) for p in want[2][k][:want[1][k]]]
                        assert min(cuts) < hp.TWO30 <= max(cuts)
            finally:
                h.close()
    finally:
        genome.close()
