"""--select: the best K guides of every gene (cropsr_amd/select.py, csrc/crp_select.hip).  The definition is restated
twice in tests/select_reference.py; the genome and its genes come from tests/select_cases.py."""
import csv
import ctypes
import io
import os

import numpy as np
import pytest

from conftest import OracleBackend

import select_cases as cases
import select_reference as ref
from cropsr_amd import _native as nat
from cropsr_amd import annotate, cli, rows
from cropsr_amd import search as srch
from cropsr_amd import select as sel

KS = (1, 5, 64)
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    c = cases.build(oracle)
    d = tmp_path_factory.mktemp("select")
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
    """The tables of one arena from the oracle's per-contig hits and the texts' arena offsets."""
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


def _synthetic_columns(tables, rng, n_strings):
    """Specificity columns and label-set ids with every kind of row: unjoined, perfect copies, large sums, no feature."""
    spec, cds = {}, {}
    for s in ("plus", "minus"):
        n = len(tables["pos_" + s])
        counts = rng.integers(0, 3, (n, 4)).astype(np.uint32)
        sums = rng.integers(0, 1 << 33, n).astype(np.uint64)
        un = rng.random(n) < 0.1
        counts[un], sums[un] = NONE, np.uint64(0xFFFFFFFFFFFFFFFF)
        spec["counts_" + s], spec["sum_" + s] = counts, sums
        feat = rng.integers(0, n_strings, n).astype(np.uint32)
        feat[rng.random(n) < 0.3] = NONE
        cds["feat_" + s] = feat
    cds["flags"] = (rng.random(n_strings) < 0.5).astype(np.uint8)
    return spec, cds


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("n_in", "n_pass", "sel")):
        assert np.array_equal(np.asarray(g, np.uint32), np.asarray(w, np.uint32)), (what, name)


# ---------------------------------------------------------------------------------------------- without a GPU
def test_numpy_statement_equals_the_plain_loop(case):
    tables, entries, _ = _host_arena(case)
    lo, hi, _ = ref.layout(case["genes"], entries, 0)
    rng = np.random.default_rng(5)
    spec, cds = _synthetic_columns(tables, rng, 9)
    spec.update(max_mm0=1, max_hit_sum=1 << 32)
    # (the loop visits every row for every gene: a spread of the genes is enough for it)
    pick = np.arange(0, len(lo), 3)
    for K in (1, 5):
        _same(ref.select_numpy(tables, lo[pick], hi[pick], K), ref.select_loop(tables, lo[pick], hi[pick], K), "plain K=%d" % K)
    _same(ref.select_numpy(tables, lo[pick], hi[pick], 64, 0.55, spec, cds), ref.select_loop(tables, lo[pick], hi[pick], 64, 0.55, spec, cds),
          "all thresholds")
    n_in, n_pass, picked = ref.select_numpy(tables, lo, hi, 5, 0.55, spec, cds)
    assert (n_pass <= n_in).all() and n_pass.max() > 5 and 0 < n_pass.min() + 1
    assert ((picked != NONE).sum(axis=1) == np.minimum(n_pass, 5)).all()


def test_native_genes_and_labels(case):
    labels, seqids, start, end = case["annotation"].genes()
    want = case["genes"]
    assert labels == [g[3] for g in want] and seqids == [g[0] for g in want]
    assert start.tolist() == [g[1] for g in want] and end.tolist() == [g[2] for g in want]
    assert labels == ["gene:" + i for i in case["ids"]]  # odd lines passed over, Name / Parent / "." labels
    assert case["annotation"].n_genes == len(want)


def test_gene_label_drops_the_annotation_info_suffix(tmp_path):
    gff, info = tmp_path / "a.gff", tmp_path / "a.txt"
    gff.write_text("c\tx\tgene\t5\t50\t.\t+\t.\tID=g1.v2;Name=g1\n")
    info.write_text("#pacId\tlocusName\ttranscriptName\tpeptideName\tPfam\tPanther\tKOG\tKEGG/ec\tKO\tGO\tBest-hit-arabi-name\tarabi-symbol\t"
                    "arabi-defline\n1\tg1\tt\tp\t\t\t\t\t\t\tAT1G01010.1\tNAC1\ta defline\n")
    ann = annotate.Annotation(str(gff), str(info))
    assert ann.strings[0] == "gene:g1.v2|AT1G01010.1|a defline"
    assert ann.genes()[0] == ["gene:g1.v2"]


@pytest.mark.parametrize("dec", [0, 1])
def test_native_gene_layout_equals_the_restated_mapping(case, dec):
    ann = case["annotation"]
    _, entries, _ = _host_arena(case)
    # whole contigs, a contig the GFF does not name, and pieces of contigs with a start offset (one of them empty)
    pieces = [("c0", 0, 10000, 64), ("c0", 9872, 20128, 10240), ("nameless", 0, 500, 40000), ("c1", 2500, 0, 41000),
              ("c1", 2500, 1200, 41088), ("c2", 23000, 1000, 43000)]
    for ent in (entries, pieces):
        got = ann.gene_layout(ent, dec)
        want = ref.layout(case["genes"], ent, dec)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    lo, hi, gene = ann.gene_layout(entries, dec)
    ids = [case["ids"][int(g)] for g in gene]
    for none in ("backwards", "unknown_seqid", "beyond_end"):
        assert none not in ids
    k = ids.index("clipped_left")
    assert lo[k] == 64 and hi[k] == 64 + 250 + dec - 1  # coordinate 0 lies before the text
    k = ids.index("last_rows")
    assert hi[k] == entries[3][3] + len(case["contigs"][3]) - 1  # cut at the contig's last character
    # the capacity protocol of crp_annotation_track, and its order check
    n = ctypes.c_uint64()
    e = ann._entries(entries)
    small = np.zeros(3, np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.uint64)
    st = nat.lib().crp_annotation_gene_layout(ann._h, e.ctypes.data_as(nat.u64p), len(entries), dec, small[0].ctypes.data_as(nat.u32p),
                                              small[1].ctypes.data_as(nat.u32p), small[2].ctypes.data_as(nat.u64p), 3, ctypes.byref(n))
    assert st == nat.CRP_ERR_CAPACITY and n.value == len(lo)
    e2 = np.ascontiguousarray(e[::-1])
    assert nat.lib().crp_annotation_gene_layout(ann._h, e2.ctypes.data_as(nat.u64p), len(entries), dec, None, None, None, 0,
                                                ctypes.byref(n)) == nat.CRP_ERR_INVALID


def test_cds_flags_follow_the_strings(case):
    ann = case["annotation"]
    strings = [ann.strings[k] for k in range(len(ann.strings))]
    flags = ann.cds_flags()
    assert np.array_equal(flags, ref.cds_flags(strings))
    assert 0 < flags.sum() < flags.size


def test_specificity_threshold_to_hit_sum():
    spec = lambda h: float(srch.specificity(np.uint64(h)))
    assert sel.max_hit_sum_for(1.0) == 0
    assert sel.max_hit_sum_for(0) == sel.max_hit_sum_for(-3.5) == 0xFFFFFFFFFFFFFFFF
    for h in (1, 7, 1 << 30, (1 << 30) + 12345, 3 << 40):
        S = spec(h)  # a representable value: h itself still passes, the next sum that prints another value does not
        got = sel.max_hit_sum_for(S)
        assert got >= h and spec(got) >= S and spec(got + 1) < S
        up, down = np.nextafter(S, 2.0), np.nextafter(S, 0.0)
        above, below = sel.max_hit_sum_for(up), sel.max_hit_sum_for(down)
        assert spec(above) >= up and spec(above + 1) < up and above < h + 1 and above <= got
        assert spec(below) >= down and spec(below + 1) < down and below >= got
    with pytest.raises(ValueError):
        sel.max_hit_sum_for(1.0000001)
    p = sel.Params(5, min_specificity=0.5, max_perfect=0)
    assert (p.max_mm0, p.max_hit_sum, p.needs_specificity) == (0, 1 << 30, True)
    assert not sel.Params(5, min_specificity=0).needs_specificity
    for bad in (0, 65, -1):
        with pytest.raises(ValueError):
            sel.Params(bad)


# ---------------------------------------------------------------------------------------------- the command line
class SelectingOracleBackend(OracleBackend):
    """OracleBackend plus the `select` keyword: the selection by the numpy statement over one host arena."""

    def scan(self, strings, l, offtarget=False, annotation=None, specificity=None, select=None):
        out = OracleBackend.scan(self, strings, l, offtarget=offtarget, annotation=annotation)
        if select is None:
            return out
        assert specificity is None  # (the oracle has no self search)
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
        out = sel.HitList(out)
        out.selection = sel.assemble(req.annotation.genes()[0], select.params.k, [part])
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


def _expected_selection_rows(case, main_rows, K, min_score=0.0, require_cds=False):
    """The selection file from the main CSV's own rows and the numpy statement."""
    tables, entries, offsets = _host_arena(case)
    lo, hi, gene = ref.layout(case["genes"], entries, 0)
    cds = None
    if require_cds:
        from oracle import annotate_oracle
        ann = case["annotation"]
        feats = [annotate_oracle.host_join(ann, n, 0, 0, h, 20, len(t)) for n, t, h in zip(case["names"], case["contigs"], case["hits"])]
        cds = dict(feat_plus=np.concatenate([f[0] for f in feats]), feat_minus=np.concatenate([f[1] for f in feats]),
                   flags=ref.cds_flags([ann.strings[k] for k in range(len(ann.strings))]))
    n_in, n_pass, picked = ref.select_numpy(tables, lo, hi, K, min_score, None, cds)
    # main CSV rows by (chromosome, end_pos, strand)
    by_key = {(r[4], r[6], r[8]): r for r in main_rows[1:] if len(r) >= 12}
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
            main = by_key[(case["names"][c], str(end), "-" if minus else "+")]
            want.append((int(g), rank, [case["genes"][int(g)][3], str(rank + 1), str(int(n_pass[row_of_layout]))] + main[1:]))
    return [w[2] for w in sorted(want, key=lambda w: w[:2])]  # genes in GFF order


def test_cli_selection_file_over_the_oracle(case, oracle, tmp_path, monkeypatch, manifest):
    plain, _ = _run(case, tmp_path, monkeypatch, [], OracleBackend(oracle), "plain.csv")
    out, stdout = _run(case, tmp_path, monkeypatch, ["--select", "5", "--select-min-score", "0.3"], SelectingOracleBackend(oracle))
    with open(plain, "rb") as a, open(out, "rb") as b:
        assert a.read() == b.read()  # the main table is what it was
    main = _read(out)
    got = _read(out + ".selected.csv")
    assert got[0] == ["gene", "rank", "passing"] + rows.HEADER[1:]
    want = _expected_selection_rows(case, main, 5, 0.3)
    # (the main table's last rows of a batch are re-scored in the reference's BLAS tail order: compare the score as a number)
    assert len(got) - 1 == len(want) and len(want) > 100
    for g, w in zip(got[1:], want):
        assert g[:11] == w[:11] and abs(float(g[11]) - float(w[11])) < 1e-15 and g[12:] == w[12:], (g, w)
    genes_in_file = [r[0] for r in got[1:]]
    assert "gene:backwards" not in genes_in_file and "gene:whole_c1" in genes_in_file


def test_cli_default_output_is_unchanged_and_golden(oracle, tmp_path, monkeypatch, manifest):
    """Without the flags the main CSV is byte for byte the golden one (md5_libm)."""
    import hashlib
    from conftest import golden_fasta_path, run_cli
    data, _ = run_cli(tmp_path, monkeypatch, golden_fasta_path("sample", tmp_path), OracleBackend(oracle), manifest["seed"])
    assert hashlib.md5(data).hexdigest() == manifest["cases"]["sample"]["md5_libm"]


def test_cli_select_cds_and_select_only(case, oracle, tmp_path, monkeypatch):
    out, _ = _run(case, tmp_path, monkeypatch, ["--select", "3", "--select-cds", "--select-only", "--select-output", str(tmp_path / "s.csv")],
                  SelectingOracleBackend(oracle))
    assert not os.path.exists(out)  # --select-only: no main table
    got = _read(str(tmp_path / "s.csv"))
    main_path, _ = _run(case, tmp_path, monkeypatch, [], OracleBackend(oracle), "main.csv")
    want = _expected_selection_rows(case, _read(main_path), 3, 0.0, require_cds=True)
    assert len(got) - 1 == len(want) > 20
    for g, w in zip(got[1:], want):
        assert g[:11] == w[:11] and g[12] == "" and g[13:] == w[13:]  # (no --annotate: `features` stays empty)
    assert "gene:no_cds" not in [r[0] for r in got[1:]]


REFUSALS = [
    (["--select", "5"], "needs -g", True),
    (["--select", "0"], "1..64", False),
    (["--select", "65"], "1..64", False),
    (["--select", "5", "-l", "19"], "-l 20", False),
    (["--select", "5", "--select-max-perfect", "0"], "--specificity", False),
    (["--select", "5", "--select-min-specificity", "0.5"], "--specificity", False),
    (["--select-min-score", "0.5"], "belongs to --select", False),
    (["--select-cds"], "belongs to --select", False),
    (["--select-only"], "belongs to --select", False),
    (["--select-output", "x.csv"], "belongs to --select", False),
    (["--select", "5", "--gpus", "2"], "one GPU", False),
    (["--select", "5", "--devices", "0,1"], "one GPU", False),
    (["--select", "5", "--specificity", "--select-min-specificity", "1.5"], "above 1", False),
]


@pytest.mark.parametrize("extra,text,no_gff", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_cli_refusals_come_before_any_side_effect(case, oracle, tmp_path, monkeypatch, extra, text, no_gff):
    monkeypatch.chdir(tmp_path)
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9"] + ([] if no_gff else ["-g", case["gff_path"]]) + extra
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=SelectingOracleBackend(oracle), out=io.StringIO())
    assert "--select" in str(e.value.code) and text in str(e.value.code)
    assert os.listdir(tmp_path) == []


def test_cli_refuses_a_launchers_ranks(case, oracle, tmp_path, monkeypatch):
    class Group:
        world, rank, local_rank = 2, 0, 0
    monkeypatch.chdir(tmp_path)
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9", "-g", case["gff_path"], "--select", "5"]
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=SelectingOracleBackend(oracle), out=io.StringIO(), group=Group())
    assert "--select" in str(e.value.code) and "2 ranks" in str(e.value.code)
    assert os.listdir(tmp_path) == []


# ---------------------------------------------------------------------------------------------- on the GPU
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def _scanned(engine, case, max_words):
    """A genome with its tables, annotation ids and joined specificity columns (M = 3) resident, and per arena the
    reference's view of the same: tables from the oracle's hits, genes by the restated layout."""
    g = engine.genome(case["contigs"], max_words=max_words)
    request = annotate.Request(case["annotation"], case["names"], 0)
    hits = g.scan_score(20)
    feats = g.annotate(request, [(h.n_plus, h.n_minus) for h in hits.per_arena])
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
        arenas.append(dict(tables=tables, lo=lo, hi=hi, gene=gene, ids=[case["ids"][int(x)] for x in gene],
                           spec=dict(counts_plus=cp, sum_plus=sp, counts_minus=cm, sum_minus=sm),
                           cds=dict(feat_plus=feats[a][0], feat_minus=feats[a][1], flags=case["annotation"].cds_flags())))
    return dict(genome=g, request=request, handles=handles, arenas=arenas, cache={})


@pytest.fixture(scope="module", params=[1, 3], ids=["one-arena", "three-arenas"])
def scanned(request, engine, case):
    s = _scanned(engine, case, None if request.param == 1 else 600)
    assert len(s["genome"].arenas) == request.param
    yield s
    for h in s["handles"]:
        h.close()
    s["genome"].close()


def _reference(s, a, K, min_score=0.0, spec=None, cds=False):
    """select_numpy for arena a, computed once per set of arguments."""
    key = (a, K, min_score, None if spec is None else tuple(sorted(spec.items())), cds)
    if key not in s["cache"]:
        A = s["arenas"][a]
        s["cache"][key] = ref.select_numpy(A["tables"], A["lo"], A["hi"], K, min_score, None if spec is None else dict(A["spec"], **spec),
                                           A["cds"] if cds else None)
    return s["cache"][key]


def _device(s, a, K, slice_rows, min_score=0.0, spec=None, cds=False):
    params = sel.Params(K, min_score, require_cds=cds)
    if spec is not None:
        params.max_mm0, params.max_hit_sum = spec["max_mm0"], spec["max_hit_sum"]
    req = sel.Request(params, s["request"], slice_rows)
    lo, hi, gene, n_in, n_pass, picked, stats = sel.select_arena(s["genome"], a, req, s["handles"][a] if spec is not None else None)
    A = s["arenas"][a]
    assert np.array_equal(lo, A["lo"]) and np.array_equal(hi, A["hi"]) and np.array_equal(gene, A["gene"])
    return (n_in, n_pass, picked), stats


def _run_lengths(A):
    """Rows per strand inside every gene's range (scored or not: the kernel's runs)."""
    t = A["tables"]
    cp, cm = t["pos_plus"].astype(np.int64) - 3, t["pos_minus"].astype(np.int64)
    n_p = np.searchsorted(cp, A["hi"].astype(np.int64), "right") - np.searchsorted(cp, A["lo"].astype(np.int64), "left")
    n_m = np.searchsorted(cm, A["hi"].astype(np.int64), "right") - np.searchsorted(cm, A["lo"].astype(np.int64), "left")
    return n_p, n_m


@pytest.mark.gpu
def test_gpu_the_genome_contains_the_cases(scanned, case):
    """On the reference's own rows: every run length, edge and tie the other GPU tests rely on is really there."""
    s = scanned
    sizes_p, sizes_m, ids = set(), set(), []
    for A in s["arenas"]:
        n_p, n_m = _run_lengths(A)
        sizes_p.update(int(n) for i, n in zip(A["ids"], n_p) if i.startswith("p_run"))
        sizes_m.update(int(n) for i, n in zip(A["ids"], n_m) if i.startswith("m_run"))
        ids += A["ids"]
        by = {i: k for k, i in enumerate(A["ids"])}
        t = A["tables"]
        if "plus_only" in by:
            assert (n_p[by["plus_only"]], n_m[by["plus_only"]]) == (1, 0)
        if "first_rows" in by:  # its runs begin at row 0 of both tables
            k = by["first_rows"]
            assert t["pos_plus"][0] - 3 >= A["lo"][k] and t["pos_minus"][0] >= A["lo"][k] and n_p[k] > 0 and n_m[k] > 0
        if "last_rows" in by:  # ... and end at the tables' last rows, unscored ones (the contig end cuts their window) among them
            k = by["last_rows"]
            assert t["pos_plus"][-1] - 3 <= A["hi"][k] and t["pos_minus"][-1] <= A["hi"][k] and n_m[k] > 0
            assert (t["score_plus"][-n_p[k]:] == -1.0).any() or (t["score_minus"][-n_m[k]:] == -1.0).any()
        if "whole_c1" in by:
            assert n_p[by["whole_c1"]] > 1000
        if "repeat" in by:  # at least 65 rows of one score on each strand
            k = by["repeat"]
            for strand, cut in (("plus", t["pos_plus"].astype(np.int64) - 3), ("minus", t["pos_minus"].astype(np.int64))):
                inside = (cut >= A["lo"][k]) & (cut <= A["hi"][k]) & (t["score_" + strand] != -1.0)
                _, counts = np.unique(t["score_" + strand][inside].view(np.uint64), return_counts=True)
                assert counts.max() >= 65
        if "palindrome" in by:  # a '+' row and a '-' row with one cut site and one score
            k = by["palindrome"]
            n_in, n_pass, picked = _reference(s, s["arenas"].index(A), 1)
            assert n_in[k] == 2 and picked[k][0] >> 31 == 0
            r = int(picked[k][0])
            j = int(np.searchsorted(t["pos_minus"], t["pos_plus"][r] - 3))
            assert t["pos_minus"][j] == t["pos_plus"][r] - 3 and t["score_minus"][j].view(np.uint64) == t["score_plus"][r].view(np.uint64)
        if "n_run" in by:  # sentinel rows of the join inside a gene
            k = by["n_run"]
            cut = t["pos_plus"].astype(np.int64) - 3
            inside = (cut >= A["lo"][k]) & (cut <= A["hi"][k]) & (t["score_plus"] != -1.0)
            assert (A["spec"]["counts_plus"][inside][:, 0] == NONE).any()
    assert sizes_p == set(cases.RUN_SIZES) and sizes_m == set(cases.RUN_SIZES)
    for i in ("nested", "duplicate", "overlapping", "outer", "no_cds", "clipped_left"):
        assert i in ids
    assert ids.count("nested") == 2
    for i in ("backwards", "unknown_seqid", "beyond_end"):
        assert i not in ids


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
@pytest.mark.parametrize("K", KS)
def test_gpu_selection_equals_the_reference(scanned, K, slice_rows):
    s = scanned
    for a in range(len(s["arenas"])):
        got, stats = _device(s, a, K, slice_rows)
        _same(got, _reference(s, a, K), "arena %d" % a)
        n_p, n_m = _run_lengths(s["arenas"][a])
        long_genes = int(((n_p + n_m) > (slice_rows or 65536)).sum())
        assert stats["merged_genes"] == long_genes  # at 64 every gene longer than 64 rows goes through the merge
        assert stats["rows_in_runs"] == int((n_p + n_m).sum()) and stats["launches"] >= 1
        if slice_rows == 64 and len(s["arenas"]) == 1:
            assert long_genes > 10


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
def test_gpu_thresholds(scanned, slice_rows):
    s = scanned
    for a, A in enumerate(s["arenas"]):
        # nothing passes
        got, _ = _device(s, a, 5, slice_rows, min_score=2.0)
        assert (got[1] == 0).all() and (got[2] == NONE).all() and np.array_equal(got[0], _reference(s, a, 5)[0])
        # exactly K pass in the arena's largest gene: min_score = its K-th best score, where the next one is lower
        n_in, _, _ = _reference(s, a, 5)
        if n_in.max() < 100:
            continue
        g = int(n_in.argmax())
        t = A["tables"]
        scores = np.concatenate([t["score_plus"][(t["pos_plus"].astype(np.int64) - 3 >= A["lo"][g]) & (t["pos_plus"].astype(np.int64) - 3 <= A["hi"][g])],
                                 t["score_minus"][(t["pos_minus"] >= A["lo"][g]) & (t["pos_minus"] <= A["hi"][g])]])
        scores = np.sort(scores[scores != -1.0])[::-1]
        K = next(k for k in range(5, 60) if scores[k - 1] > scores[k])
        want = _reference(s, a, K, float(scores[K - 1]))
        assert want[1][g] == K
        got, _ = _device(s, a, K, slice_rows, min_score=float(scores[K - 1]))
        _same(got, want, "exactly K")


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
@pytest.mark.parametrize("K", KS)
def test_gpu_specificity_columns_and_cds(scanned, K, slice_rows):
    s = scanned
    for a in range(len(s["arenas"])):
        for spec in (dict(max_mm0=NONE, max_hit_sum=0xFFFFFFFFFFFFFFFF),  # only "joined"
                     dict(max_mm0=0, max_hit_sum=sel.max_hit_sum_for(0.5))):
            got, stats = _device(s, a, K, slice_rows, 0.2, spec, cds=False)
            want = _reference(s, a, K, 0.2, spec)
            _same(got, want, "spec arena %d" % a)
            assert stats["bytes_per_row"] == 24
        got, _ = _device(s, a, K, slice_rows, 0.0, dict(max_mm0=2, max_hit_sum=1 << 34), cds=True)
        want = _reference(s, a, K, 0.0, dict(max_mm0=2, max_hit_sum=1 << 34), cds=True)
        _same(got, want, "cds arena %d" % a)
        by = {i: k for k, i in enumerate(s["arenas"][a]["ids"])}
        if "no_cds" in by:
            assert want[0][by["no_cds"]] > 0 and want[1][by["no_cds"]] == 0
        if "n_run" in by:  # the unjoined rows are in the gene and never pass
            plain = _reference(s, a, K)
            joined_only = _reference(s, a, K, 0.0, dict(max_mm0=NONE, max_hit_sum=0xFFFFFFFFFFFFFFFF))
            assert joined_only[1][by["n_run"]] < plain[1][by["n_run"]]


@pytest.mark.gpu
def test_gpu_genome_level_call(engine, case):
    """Genome.scan_score(select=...): after the annotation look-up, between the join and the closing of its handles."""
    g = engine.genome(case["contigs"], max_words=600)
    try:
        request = annotate.Request(case["annotation"], case["names"], 0)
        params = sel.Params(5, 0.2, max_perfect=0, min_specificity=0.5, require_cds=True)
        hits = g.scan_score(20, specificity=dict(max_mm=3), select=sel.Request(params, request))
        S = hits.selection
        assert S.labels == [x[3] for x in case["genes"]] and S.counts.shape == (S.rows.size, 4)
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
            n_in, n_pass, picked = ref.select_numpy(tables, lo, hi, 5, 0.2, spec, dict(feat_plus=fp, feat_minus=fm, flags=case["annotation"].cds_flags()))
            parts.append(dict(offsets=arena.offsets, lengths=arena.lengths, group=group, gene=gene, n_in=n_in, n_pass=n_pass, sel=picked,
                              counts_plus=spec["counts_plus"], sum_plus=spec["sum_plus"], counts_minus=spec["counts_minus"],
                              sum_minus=spec["sum_minus"], **tables))
        W = sel.assemble(S.labels, 5, parts)
        assert np.array_equal(S.n_in, W.n_in) and np.array_equal(S.n_pass, W.n_pass) and S.n_pass.sum() > 50
        assert S.rows.tobytes() == W.rows.tobytes() and np.array_equal(S.counts, W.counts) and np.array_equal(S.hit_sum, W.hit_sum)
        # a selected row is what the contig's own table says at that index
        for r in S.rows[:50]:
            hc = hits.contig(int(r["contig"]))
            strand = "plus" if r["strand"] == b"+" else "minus"
            assert hc["pos_" + strand][r["index"]] == r["position"] and hc["score_" + strand][r["index"]] == r["score"]
        with pytest.raises(ValueError):
            g.scan_score(20, select=sel.Request(params, request))  # the specificity thresholds without the join
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_calls_out_of_order(engine, case):
    L = nat.lib()
    arena = engine.arena([b"ACGTTGCAAGGCCTTAGGACCA" * 60])
    try:
        with pytest.raises(nat.CropsrHipError) as e:
            sel.ArenaSelect(arena, [5], [4])
        assert e.value.status == nat.CRP_ERR_INVALID
        h = sel.ArenaSelect(arena, [0, 100], [50, 900])

        def status(fn):
            with pytest.raises(nat.CropsrHipError) as e:
                fn()
            return e.value.status, str(e.value)

        assert status(h.fetch)[0] == nat.CRP_ERR_STATE                       # nothing has run
        st, text = status(lambda: h.run(sel.Params(5)))
        assert st == nat.CRP_ERR_STATE and "guide length 20" in text          # no scan yet
        arena.scan_score_device(19)
        assert status(lambda: h.run(sel.Params(5)))[0] == nat.CRP_ERR_STATE   # a scan at another length
        n_plus, n_minus = arena.scan_score_device(20)
        st, text = status(lambda: h.run(sel.Params(5, require_cds=True)))
        assert st == nat.CRP_ERR_STATE and "crp_select_set_flags" in text
        h.set_flags(np.ones(3, np.uint8))
        st, text = status(lambda: h.run(sel.Params(5, require_cds=True)))
        assert st == nat.CRP_ERR_STATE and "crp_annotate_lookup" in text
        pattern, gp, M, scheme = srch.check_specificity(20, 3)
        handle = srch.ArenaSelfSearch(arena, pattern, gp, 3, M)
        try:
            st, text = status(lambda: h.run(sel.Params(5), handle))
            assert st == nat.CRP_ERR_STATE and "joined" in text
        finally:
            handle.close()
        for k in (0, 65):
            p = nat.SelectParams(0.0, 0, 0, k, 0, 0)
            assert L.crp_select_run(h._h, ctypes.byref(p), None) == nat.CRP_ERR_INVALID
        assert L.crp_select_set_limits(h._h, 63) == nat.CRP_ERR_INVALID
        assert status(h.fetch)[0] == nat.CRP_ERR_STATE                       # a failed run leaves nothing to fetch
        h.run(sel.Params(64))
        n_in, n_pass, picked = h.fetch()
        tables = dict(zip(("pos_plus", "_", "score_plus", "pos_minus", "__", "score_minus"), arena.fetch(n_plus, n_minus)))
        _same((n_in, n_pass, picked), ref.select_numpy(tables, [0, 100], [50, 900], 64))
        h.close()
    finally:
        arena.close()


@pytest.mark.gpu
def test_gpu_command_line_end_to_end(case, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    out_csv = str(tmp_path / "out.csv")
    argv = ["-f", case["fasta_path"], "-g", case["gff_path"], "-o", out_csv, "--cas9", "--seed", "11", "--each-contig-once", "--specificity",
            "--annotate", "--select", "5", "--select-min-score", "0.2", "--select-max-perfect", "0", "--select-min-specificity", "0.5",
            "--select-cds", "--bench-json", str(tmp_path / "bench.json")]
    cli.run(cli.build_parser().parse_args(argv), out=io.StringIO())
    main, got = _read(out_csv), _read(out_csv + ".selected.csv")
    assert got[0] == ["gene", "rank", "passing"] + main[0][1:] and main[0][-1] == "specificity"
    by_key = {(r[4], r[6], r[8]): r for r in main[1:] if len(r) == len(main[0])}
    assert len(got) > 50
    seen = {}
    for r in got[1:]:
        m = by_key[(r[6], r[8], r[10])]
        assert r[3:11] == m[1:9] and abs(float(r[11]) - float(m[9])) < 1e-15 and r[12:] == m[10:]
        assert float(r[11]) >= 0.2 and "CDS:" in r[12] and r[-6] == "0" and float(r[-1]) >= 0.5
        seen.setdefault(r[0], []).append((int(r[1]), float(r[11])))
    for gene, picked in seen.items():
        assert [k for k, _ in picked][:5] == list(range(1, min(5, len(picked)) + 1)) or gene == "gene:nested"
    import json
    with open(tmp_path / "bench.json") as f:
        assert json.load(f)["select"]["items"] > 0
