"""--splice-edit / --select-splice: guides with which a base editor destroys a splice site (cropsr_amd/baseedit.py, DESIGN.md
section 22).  Without a GPU: the three restatements against each other, crp_splice.h under sanitizers, the editor and the
limits, the selection statements, the command line over an oracle backend.  On the GPU: the evaluation kernel and the
selection with splice limits -- alone and as the alternative to the stop limits -- against the reference, exactly."""
import csv
import ctypes
import io
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import OracleBackend

import base_edit_reference as eref
import select_coding_cases as coding_cases
import select_coding_reference as cref
import select_reference as sref
import select_scale_cases as scale
import splice_edit_cases as cases
import splice_edit_reference as xref
from cropsr_amd import _native as nat
from cropsr_amd import annotate, baseedit, cli
from cropsr_amd import select as sel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
NO_SITE = baseedit.NO_SITE
KS = (1, 5, 64)
ZOO_ENTRIES = [("s", 0, 400, 64), ("other", 0, 300, 576), ("s", 25, 100, 1024), ("s", 45, 200, 1280)]  # whole contigs; pieces that begin inside an exon, inside an intron
NAMES = ("targets", "donors", "acceptors", "donor_off", "acceptor_off")


@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    c = cases.build(oracle)
    d = tmp_path_factory.mktemp("splice_edit")
    c["gff_path"] = str(d / "genes.gff")
    with open(c["gff_path"], "w") as f:
        f.write(c["gff"])
    c["fasta_path"] = str(d / "genome.fa")
    with open(c["fasta_path"], "w") as f:  # one line per contig: read unformatted (dec = 0)
        f.write("".join(">%s\n%s\n" % (n, t.decode()) for n, t in zip(c["names"], c["contigs"]))[:-1])
    c["annotation"] = annotate.Annotation(c["gff_path"])
    c["genes"] = sref.gff_genes(c["gff"])
    c["models"] = cref.model_numpy(c["gff"])
    return c


def _arena_tables(hits, offsets):
    cat = lambda key, dt, add: np.concatenate([h[key].astype(dt) + (dt(o) if add else dt(0)) for h, o in zip(hits, offsets)])
    return dict(pos_plus=cat("pos_plus", np.uint32, True), score_plus=cat("score_plus", np.float64, False),
                pos_minus=cat("pos_minus", np.uint32, True), score_minus=cat("score_minus", np.float64, False))


def _host_offsets(texts):
    """Offsets of an arena laid out like the device's: 64-aligned texts, one separator word between them."""
    offsets, off = [], 64
    for t in texts:
        offsets.append(off)
        off += ((len(t) + 63) // 64 + 1) * 64
    return offsets


def _position_member(tables, lo, hi):
    """Boolean (genes, rows of both tables): the row's cut site lies in the gene -- scored or not, so that the rows whose
    30 letters hold an N or run past a contig's end are evaluated too."""
    pos, strand = eref.rows_of(tables)
    cut = pos - np.where(strand == 0, 3, 0)
    return (cut[None, :] >= np.asarray(lo, np.int64)[:, None]) & (cut[None, :] <= np.asarray(hi, np.int64)[:, None])


def _view(case, texts, names, starts, offsets, hits):
    """The reference's view of one arena: tables, genes, layout rows, the letters, membership."""
    tables = _arena_tables(hits, offsets)
    entries = [(n, a, len(t), o) for n, a, t, o in zip(names, starts, texts, offsets)]
    lo, hi, gene = sref.layout(case["genes"], entries, 0)
    rows = cref.layout_rows(case["gff"], entries, 0)
    return dict(tables=tables, entries=entries, lo=lo, hi=hi, gene=gene, rows=rows, arena=eref.make_arena(texts, offsets),
                ids=[case["ids"][int(x)] for x in gene], member=cref.membership(tables, lo, hi), everyone=_position_member(tables, lo, hi),
                score=np.concatenate([tables["score_plus"], tables["score_minus"]]), outcomes={}, stops={})


def _outcomes(case, A, window, editor):
    """xref.outcomes over the rows whose cut site is in the gene, by the masks: computed once per arena, window and editor."""
    if (window, editor) not in A["outcomes"]:
        A["outcomes"][window, editor] = xref.outcomes(A["tables"], A["everyone"], case["models"], A["rows"], A["arena"], window, editor)
    return A["outcomes"][window, editor]


def _stops(case, A, window):
    if window not in A["stops"]:
        A["stops"][window] = eref.outcomes(A["tables"], A["everyone"], case["models"], A["rows"], A["arena"], window)
    return A["stops"][window]


def _scored(A, per_gene):
    """The outcomes of the rows IN the gene (scored rows only), as select_numpy takes them."""
    ok = A["score"] != -1.0
    return [tuple(v[ok[o[0]]] for v in o) for o in per_gene]


def _check_planted(case, A, offset_of):
    """Every planted construct gives, on the reference's rows, what it was planted for."""
    pos, strand = eref.rows_of(A["tables"])
    seen = 0
    for p in case["planted"]:
        if p["gene"] not in A["ids"] or p["contig"] not in offset_of:
            continue
        g = A["ids"].index(p["gene"])
        o = _outcomes(case, A, cases.WINDOW, p["editor"])[g]
        hit = np.flatnonzero((pos[o[0]] == p["pos"] + offset_of[p["contig"]]) & (strand[o[0]] == int(p["minus"])))
        assert hit.size == 1, p
        assert tuple(int(v[hit[0]]) for v in o[1:]) == tuple(p[key] for key in NAMES), p
        seen += 1
    return seen


# ---------------------------------------------------------------------------------------------- without a GPU
def _agree(gff, texts_by_name, entries, windows_all):
    """The three statements at every row position of every text for every gene: returns (rows compared, sites destroyed, rows
    with a donor and an acceptor)."""
    loop_models, np_models = cref.model_loop(gff), cref.model_numpy(gff)
    texts = [texts_by_name[n][a:a + ln] for n, a, ln, _ in entries]
    arena = eref.make_arena(texts, [e[3] for e in entries])
    n = n_sites = n_both = 0
    for row in cref.layout_rows(gff, entries, 0):
        g, _, lo, hi = row
        m = np_models[g]
        index_of = eref._index(m, row) if m["model"] else None
        for w, window in enumerate(xref.WINDOWS):
            for pos in range(lo - 30, hi + 31, 1 if window in windows_all else 5):
                for minus in (False, True):
                    for editor in xref.EDITORS:
                        a = xref.outcome_loop(loop_models[g], row, arena, pos + w % 5, minus, window, editor)
                        b = xref.outcome_masks(m, row, arena, pos + w % 5, minus, window, editor)
                        c = baseedit.splice_outcome(arena, pos + w % 5, minus, baseedit.Window(*window), baseedit.Editor(editor), index_of, m["length"],
                                                    m["strand"] == "-")
                        assert a == b == c, (g, row, pos, minus, window, editor, a, b, c)
                        n += 1
                        n_sites += a[1] + a[2]
                        n_both += bool(a[1] and a[2])
    return n, n_sites, n_both


def _with_sites(text, gff, seqid, rng):
    """text with canonical site letters (and a few near misses) written at the edges of the GFF's CDS rows on seqid."""
    text = bytearray(text)
    for typ, seq, a, b, strand, _ in cref.gff_rows(gff):
        if typ != "CDS" or seq != seqid or not 3 <= a <= b <= len(text) - 2:
            continue
        opens, closes = ((b"CT", b"AC") if strand == "-" else (b"GT", b"AG"))
        if rng.integers(4):
            text[b:b + 2] = opens if rng.integers(6) else b"GC"
        if rng.integers(4):
            text[a - 3:a - 1] = closes if rng.integers(6) else b"aN"
    return bytes(text)


def test_three_statements_agree_on_the_gff_zoo():
    """The string statement, the masks and baseedit.splice_outcome over section 20's GFF zoo with random letters and site
    letters at the exons' edges: whole contigs, a piece that begins inside an exon and one that begins inside an intron, both
    gene strands, both row strands, both editors, every window."""
    total = np.zeros(3, np.int64)
    for name in sorted(coding_cases.ZOO):
        rng = np.random.default_rng(len(name))
        alpha = np.frombuffer(b"ACGTACGTACGTacgtN", dtype=np.uint8)
        gff = coding_cases.ZOO[name]
        texts = {n: _with_sites(rng.choice(alpha, ln).tobytes(), gff, n, rng) for n, ln in coding_cases.ZOO_CONTIGS.items()}
        got = _agree(gff, texts, ZOO_ENTRIES, ((4, 8),))
        print(name, "rows", got[0], "sites", got[1], "both", got[2])
        assert got[0] > 1000
        total += got
    assert total[1] > 300, total


@pytest.mark.parametrize("seed", range(6))
def test_three_statements_agree_on_random_exon_structures(seed):
    text, gff = cases.random_case(seed)
    n, n_sites, n_both = _agree(gff, {"s": text}, [("s", 0, len(text), 64), ("s", 100, 300, 1024)], ((4, 8),))
    print("rows", n, "sites", n_sites, "both", n_both)
    assert n > 5000 and n_sites > 60 and n_both > 0


def test_pieces_begin_inside_an_exon_and_inside_an_intron():
    """The zoo's pieces are what the agreement test says they are: `plain` has an exon at the indices 19 .. 39 and an intron behind
    it, and the pieces start at 25 and at 45."""
    rows = [r for r in cref.gff_rows(coding_cases.ZOO["plain"]) if r[0] == "CDS"]
    assert (rows[0][2], rows[0][3], rows[1][2]) == (20, 40, 60)
    assert ZOO_ENTRIES[2][1] == 25 and ZOO_ENTRIES[3][1] == 45


def test_editor_and_limits_are_checked():
    assert baseedit.Editor().name == "cbe" and baseedit.Editor("ABE").code == 1 and baseedit.Editor(baseedit.Editor("abe")) == baseedit.Editor("abe")
    assert baseedit.Editor("cbe").edit(False) == ("C", "T") and baseedit.Editor("cbe").edit(True) == ("G", "A")
    assert baseedit.Editor("abe").edit(False) == ("A", "G") and baseedit.Editor("abe").edit(True) == ("T", "C")
    for bad in ("", "gbe", None, 1, "cbe "):
        with pytest.raises(ValueError):
            baseedit.Editor(bad)
    assert baseedit.SpliceLimits().astuple() == (0, 100, 20, 3) and baseedit.SpliceLimits(5, 65, 2, "donor").astuple() == (5, 65, 2, 1)
    assert baseedit.SpliceLimits(kinds="acceptor").astuple()[3] == 2
    for bad in ((-1, 100, 20), (0, 101, 20), (66, 65, 20), (0, 100, 21), (0, 100, -1), (0.5, 100, 20), (0, 100, True), (0, 100, 20, "both"),
                (0, 100, 20, None), (0, 100, 20, 3), ("5", 100, 20)):
        with pytest.raises(ValueError):
            baseedit.SpliceLimits(*bad)
    targets = np.array([1, 1, 1, 2, 1, 1, 1])
    donor = np.array([15, 12, NO_SITE, 30, 198, NO_SITE, NO_SITE], np.uint32)
    acceptor = np.array([NO_SITE, 195, 195, 30, NO_SITE, NO_SITE, 12], np.uint32)
    L = np.full(7, 300)
    for kinds, want in (("any", [True, True, True, False, False, False, False]), ("donor", [True, False, False, False, False, False, False]),
                        ("acceptor", [False, True, True, False, False, False, False])):
        lim = baseedit.SpliceLimits(5, 65, 1, kinds)
        assert lim.passes(targets, donor, acceptor, L).tolist() == want
        assert want == [xref.passes((5, 65, 1, kinds), (t, 0, 0, d, a), 300) for t, d, a in zip(targets, donor, acceptor)]
        assert xref.passes_numpy((5, 65, 1, kinds), (targets, None, None, donor, acceptor), 300).tolist() == want
    big = np.array([4294967100], np.uint32)  # 100 off needs its 64 bits
    none = np.array([NO_SITE], np.uint32)
    assert baseedit.SpliceLimits(99, 100).passes([1], big, none, [0xFFFFFFFF]).tolist() == [True]
    assert baseedit.SpliceLimits(0, 98).passes([1], none, big, [0xFFFFFFFF]).tolist() == [False]
    assert baseedit.splice_fields(3, 1, 1, 30, 150, 300) == (3, 2, "10.0", "50.0") and baseedit.splice_fields(2, 0, 0, NO_SITE, NO_SITE, 300) == (2, 0, "", "")
    assert baseedit.splice_fields(1, 0, 1, NO_SITE, 15, 300) == (1, 1, "", "5.0")
    assert baseedit.SPLICE_HEADER == ["splice_targets", "splice_sites", "donor_percent", "acceptor_percent"]
    from cropsr_amd import coding
    for more in (dict(pairs=sel.PairParams(1)), dict(coding_limits=coding.Limits())):
        with pytest.raises(ValueError):
            sel.Request(sel.Params(1), None, splice_limits=baseedit.SpliceLimits(), **more)
    with pytest.raises(ValueError):
        sel.Request(sel.Params(1), None, editor="abe", edit_limits=baseedit.Limits())
    with pytest.raises(ValueError):
        sel.Request(sel.Params(1), None, editor="dbe")
    r = sel.Request(sel.Params(1), None, splice_limits=baseedit.SpliceLimits())
    assert r.splice and not r.edit and r.editor == baseedit.Editor("cbe") and r.splice_window.astuple() == (4, 8)
    r = sel.Request(sel.Params(1), None, editor="abe", edit_window=baseedit.Window(1, 20))
    assert r.splice and not r.edit and r.splice_limits is None and r.splice_window.astuple() == (1, 20)
    r = sel.Request(sel.Params(1), None, splice_limits=baseedit.SpliceLimits(), edit_limits=baseedit.Limits())
    assert r.splice and r.edit
    r = sel.Request(sel.Params(1), None)
    assert not r.splice and r.editor is None and not r.edit


def test_baseedit_splice_outcome_is_the_definition(case):
    """baseedit.splice_outcome, the package's own general statement, on the planted constructs; and the constructs are there."""
    offsets = _host_offsets(case["contigs"])
    A = _view(case, case["contigs"], case["names"], [0] * 4, offsets, case["hits"])
    assert _check_planted(case, A, dict(enumerate(offsets))) == len(case["planted"])
    for p in case["planted"]:
        g = A["ids"].index(p["gene"])
        m = case["models"][A["rows"][g][0]]
        got = baseedit.splice_outcome(A["arena"], p["pos"] + offsets[p["contig"]], p["minus"], baseedit.Window(*cases.WINDOW), baseedit.Editor(p["editor"]),
                                      eref._index(m, A["rows"][g]) if m["model"] else None, m["length"], m["strand"] == "-")
        assert got == tuple(p[key] for key in NAMES), p
    hit = [p for p in case["planted"] if p["donors"] or p["acceptors"]]
    assert len(hit) > 20 and len(case["planted"]) - len(hit) > 30


def test_selection_statements_agree_on_the_case_genome(case):
    """select_numpy (masks) against select_loop (string statement) over the 80 kb genome: splice limits, and stop-or-splice."""
    A = _view(case, case["contigs"], case["names"], [0] * 4, _host_offsets(case["contigs"]), case["hits"])
    loop_models = cref.model_loop(case["gff"])
    ok = A["score"] >= 0.2
    for K, limits, window, editor, use_ok, stop in ((5, (5, 65, 20, "any"), (4, 8), "cbe", False, None), (1, (0, 100, 1, "donor"), (4, 8), "abe", True, None),
                                                    (64, (0, 100, 20, "acceptor"), (1, 20), "abe", False, None),
                                                    (5, (5, 65, 2, "any"), (4, 8), "cbe", False, (0, 100, 2))):
        per_gene = _scored(A, _outcomes(case, A, window, editor))
        stops = None if stop is None else (_scored(A, _stops(case, A, window)), stop)
        got = xref.select_numpy(A["tables"], A["member"], case["models"], A["rows"], K, per_gene, limits, ok if use_ok else None, stops)
        want = xref.select_loop(A["tables"], A["lo"], A["hi"], loop_models, A["rows"], A["arena"], window, editor, K, limits, ok if use_ok else None, stop)
        for g, w, name in zip(got, want, ("n_in", "n_pass", "sel")):
            assert np.array_equal(g, w), (K, limits, name)
        assert got[1].any() and (got[1] < got[0]).any()
        if stop is not None:  # the union is more than either part
            alone = xref.select_numpy(A["tables"], A["member"], case["models"], A["rows"], K, per_gene, limits)
            only_stop = eref.select_numpy(A["tables"], A["member"], case["models"], A["rows"], K, stops[0], stop)
            assert (got[1] >= alone[1]).all() and (got[1] >= only_stop[1]).all() and (got[1] > alone[1]).any() and (got[1] > only_stop[1]).any()


def test_splice_driver_under_sanitizers(tmp_path):
    """tests/native/splice_driver.cpp: crp_splice.h over hand-made planes and step functions against a brute-force loop, under
    ASan + UBSan."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "splice_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "cropsr_amd", "csrc"), os.path.join(ROOT, "tests", "native", "splice_driver.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout + run.stderr


# ---------------------------------------------------------------------------------------------- the command line, over the oracle
class SpliceOracleBackend(OracleBackend):
    """OracleBackend plus the `select` keyword with base editing of both kinds: the selection by the numpy statement over one
    host arena, the outcomes of the selected rows by the masks (and the stop fields by base_edit_reference's closed form)."""

    def __init__(self, orc, case):
        OracleBackend.__init__(self, orc)
        self.case = case
        self.requests = []

    def scan(self, strings, l, offtarget=False, annotation=None, specificity=None, select=None):
        out = OracleBackend.scan(self, strings, l, offtarget=offtarget, annotation=annotation)
        if select is None:
            return out
        self.requests.append(select)
        texts = [bytes(s) for s in strings]
        offsets = _host_offsets(texts)
        A = _view(self.case, texts, self.case["names"], [0] * len(texts), offsets, out)
        req = select.annotation
        lo, hi, gene = req.gene_layout([(k, o, len(t)) for k, (t, o) in enumerate(zip(texts, offsets))])
        assert [r[0] for r in A["rows"]] == gene.tolist()
        models, K = self.case["models"], select.params.k
        ok = A["score"] >= select.params.min_score
        window = (select.splice_window if select.splice else select.edit_window).astuple() if (select.splice or select.edit) else cases.WINDOW
        editor = select.editor.name if select.splice else "cbe"
        per_gene = _scored(A, _outcomes(self.case, A, window, editor))
        stops = _scored(A, _stops(self.case, A, window))
        stop = None if select.edit_limits is None else select.edit_limits.astuple()
        if select.splice and select.splice_limits is not None:
            limits = select.splice_limits.astuple()[:3] + (select.splice_limits.kinds,)
            n_in, n_pass, picked = xref.select_numpy(A["tables"], A["member"], models, A["rows"], K, per_gene, limits, ok, None if stop is None else (stops, stop))
        else:
            n_in, n_pass, picked = eref.select_numpy(A["tables"], A["member"], models, A["rows"], K, stops, stop, ok)
        part = dict(offsets=np.array(offsets, np.uint64), lengths=np.array([len(t) for t in texts], np.uint64), group=list(range(len(texts))),
                    gene=gene, n_in=n_in, n_pass=n_pass, sel=picked, **A["tables"])
        n_plus = len(A["tables"]["pos_plus"])
        length = np.array([models[r[0]]["length"] for r in A["rows"]], np.uint32)

        def of_picked(per, fill):
            cols = [np.full(picked.shape, f, np.uint32) for f in fill]
            for g, o in enumerate(per):
                where = {int(x): j for j, x in enumerate(o[0])}
                for k, packed in enumerate(picked[g]):
                    if packed != NONE:
                        j = where[(int(packed) & 0x7FFFFFFF) + (n_plus if int(packed) >> 31 else 0)]
                        for col, v in zip(cols, o[1:]):
                            col[g, k] = v[j]
            return cols

        if select.edit:
            part["edit"] = dict(zip(("targets", "stops", "stop_off"), of_picked(stops, (0, 0, eref.NO_STOP))), length=length)
        if select.splice:
            part["splice"] = dict(zip(NAMES, of_picked(per_gene, (0, 0, 0, NO_SITE, NO_SITE))), length=length)
        out = sel.HitList(out)
        out.selection = sel.assemble(req.annotation.genes()[0], K, [part], stats=dict(splice_select_ms=0.0, splice_eval_ms=0.0, editor=editor)
                                     if select.splice else None)
        return out


def _run(case, tmp_path, monkeypatch, extra, backend, name="out.csv"):
    monkeypatch.chdir(tmp_path)
    out_csv = str(tmp_path / name)
    argv = ["-f", case["fasta_path"], "-g", case["gff_path"], "-o", out_csv, "--cas9", "--seed", "11", "--each-contig-once"] + list(extra)
    buf = io.StringIO()
    cli.run(cli.build_parser().parse_args(argv), **({} if backend is None else dict(backend=backend)), out=buf)
    return out_csv, buf.getvalue()


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def _expected_fields(case, got_rows, limits, min_score, editor, window=cases.WINDOW, stop=None, K=5):
    """Per row of a selection file (gene label, end_pos, strand -> the table row): the four fields by the string statement, and
    the set of (gene, chromosome, end_pos, strand) the selection must consist of."""
    from decimal import ROUND_HALF_UP, Decimal
    offsets = _host_offsets(case["contigs"])
    A = _view(case, case["contigs"], case["names"], [0] * 4, offsets, case["hits"])
    models = cref.model_loop(case["gff"])
    n_in, n_pass, picked = xref.select_loop(A["tables"], A["lo"], A["hi"], models, A["rows"], A["arena"], window, editor, K, limits, A["score"] >= min_score, stop)
    label_row = {case["genes"][int(g)][3]: r for r, g in enumerate(A["gene"])}
    offset_of = dict(zip(case["names"], offsets))
    want_rows = set()
    for r in range(len(A["rows"])):
        for packed in picked[r]:
            if packed != NONE:
                minus, t = int(packed) >> 31, int(packed) & 0x7FFFFFFF
                pos = int(A["tables"]["pos_minus" if minus else "pos_plus"][t])
                k = max(i for i, o in enumerate(offsets) if o <= pos)
                want_rows.add((case["genes"][int(A["gene"][r])][3], case["names"][k], str(pos - offsets[k] + (3 if minus else 0)), "-" if minus else "+"))
    pct = lambda off, L: "" if off == NO_SITE else str((Decimal(100 * off) / Decimal(L)).quantize(Decimal("0.1"), rounding=ROUND_HALF_UP))
    fields = []
    for g in got_rows:
        r = label_row[g[0]]
        end, minus = int(g[8]) + offset_of[g[6]], g[10] == "-"  # (gene, rank, passing, then the main table's fields without its first)
        m = models[A["rows"][r][0]]
        o = xref.outcome_loop(m, A["rows"][r], A["arena"], end - 3 if minus else end, minus, window, editor)  # end_pos: i, or j + 3
        fields.append([str(o[0]), str(o[1] + o[2]), pct(o[3], m["length"]), pct(o[4], m["length"])])
    return fields, want_rows, n_pass, label_row


def test_cli_fields_and_filter_over_the_oracle(case, oracle, tmp_path, monkeypatch):
    from cropsr_amd import rows as rows_mod
    backend = SpliceOracleBackend(oracle, case)
    base = ["--select", "5", "--select-min-score", "0.2"]
    plain, _ = _run(case, tmp_path, monkeypatch, base, backend, "plain.csv")
    assert backend.requests[-1].splice is False and backend.requests[-1].editor is None
    with_fields, _ = _run(case, tmp_path, monkeypatch, base + ["--splice-edit"], backend, "fields.csv")
    last = backend.requests[-1]
    assert last.splice and not last.edit and last.splice_limits is None and last.editor.name == "cbe" and last.splice_window.astuple() == (4, 8)
    bench = str(tmp_path / "bench.json")
    filtered, _ = _run(case, tmp_path, monkeypatch, base + ["--select-splice", "--select-splice-min", "5", "--select-splice-max", "65",
                                                            "--select-max-edit-targets", "2", "--bench-json", bench], backend, "filtered.csv")
    last = backend.requests[-1]
    assert last.splice_limits.astuple() == (5, 65, 2, 3) and last.edit_limits is None and not last.edit
    abe, _ = _run(case, tmp_path, monkeypatch, base + ["--base-editor", "abe", "--select-splice", "acceptor", "--base-edit-window", "1-20"], backend, "abe.csv")
    last = backend.requests[-1]
    assert last.splice_limits.astuple() == (0, 100, 20, 2) and last.editor.name == "abe" and last.splice_window.astuple() == (1, 20) and not last.edit
    both, _ = _run(case, tmp_path, monkeypatch, base + ["--select-splice", "donor", "--select-stop-max", "65", "--select-max-edit-targets", "3"], backend, "both.csv")
    last = backend.requests[-1]
    assert last.splice_limits.astuple() == (0, 100, 3, 1) and last.edit_limits.astuple() == (0, 65, 3) and last.edit
    for path in (with_fields, filtered, abe, both):  # the main table is what it was
        with open(plain, "rb") as a, open(path, "rb") as b:
            assert a.read() == b.read()
    # without the new options: the header and the fields of before; with --splice-edit: the same file with four more fields
    old, new = _read(plain + ".selected.csv"), _read(with_fields + ".selected.csv")
    assert old[0] == ["gene", "rank", "passing"] + rows_mod.HEADER[1:] and new[0] == old[0] + baseedit.SPLICE_HEADER
    assert [r[:-4] for r in new] == old and len(old) > 60
    buf = io.StringIO()
    csv.writer(buf).writerows([r[:-4] for r in new])
    with open(plain + ".selected.csv", newline="") as f:
        assert f.read() == buf.getvalue()  # byte for byte
    fields, want_rows, _, _ = _expected_fields(case, new[1:], None, 0.2, "cbe")
    assert [r[-4:] for r in new[1:]] == fields
    assert any(f[2] != "" for f in fields) and any(f[3] != "" for f in fields) and any(f[2] == "" and f[3] == "" for f in fields)
    assert set((r[0], r[6], r[8], r[10]) for r in new[1:]) == want_rows
    # the filtered selection: the reference's rows, every one with a destroyed site inside the limits
    got = _read(filtered + ".selected.csv")
    fields, want_rows, n_pass, label_row = _expected_fields(case, got[1:], (5, 65, 2, "any"), 0.2, "cbe")
    assert got[0] == new[0] and [r[-4:] for r in got[1:]] == fields and 10 < len(got) < len(new)
    assert set((r[0], r[6], r[8], r[10]) for r in got[1:]) == want_rows
    for r in got[1:]:
        assert int(r[2]) == n_pass[label_row[r[0]]] and int(r[-3]) >= 1 and 1 <= int(r[-4]) <= 2
        assert any(v != "" and 5.0 <= float(v) <= 65.0 for v in r[-2:])
    assert not any(r[0].startswith("gene:no_cds") or r[0].startswith("gene:no_strand") for r in got[1:])
    got = _read(abe + ".selected.csv")
    fields, want_rows, _, _ = _expected_fields(case, got[1:], (0, 100, 20, "acceptor"), 0.2, "abe", (1, 20))
    assert [r[-4:] for r in got[1:]] == fields and set((r[0], r[6], r[8], r[10]) for r in got[1:]) == want_rows and len(got) > 10
    assert all(r[-1] != "" for r in got[1:]) and got[0] == new[0]
    # stop or splice: both groups of fields, section 21's first; the rows of the union
    got = _read(both + ".selected.csv")
    assert got[0] == old[0] + baseedit.HEADER + baseedit.SPLICE_HEADER
    fields, want_rows, _, _ = _expected_fields(case, got[1:], (0, 100, 3, "donor"), 0.2, "cbe", stop=(0, 65, 3))
    assert [r[-4:] for r in got[1:]] == fields and set((r[0], r[6], r[8], r[10]) for r in got[1:]) == want_rows
    assert any(r[-2] != "" for r in got[1:]) and any(r[-2] == "" and r[-5] != "" for r in got[1:])  # by the donor, and by the stop alone
    with open(bench) as f:
        stage = json.load(f)["select"]
    assert stage["editor"] == "cbe" and "splice_select_ms" in stage and "splice_eval_ms" in stage


SPLICE_REFUSALS = [
    (["--base-editor", "abe"], "belongs to --select", False),
    (["--splice-edit"], "belongs to --select", False),
    (["--select-splice"], "belongs to --select", False),
    (["--select-splice", "donor"], "belongs to --select", False),
    (["--select-splice-min", "5"], "belongs to --select", False),
    (["--select-splice-max", "65"], "belongs to --select", False),
    (["--select", "5", "--splice-edit"], "needs -g", True),
    (["--select", "5", "--select-splice"], "needs -g", True),
    (["--select", "5", "--base-editor", "gbe"], "cbe or abe", False),
    (["--select", "5", "--base-editor", ""], "cbe or abe", False),
    (["--select", "5", "--select-splice", "both"], "donor, acceptor or any", False),
    (["--select", "5", "--select-splice", "5"], "donor, acceptor or any", False),
    (["--select", "5", "--select-splice-min", "101"], "0..100", False),
    (["--select", "5", "--select-splice-max", "-1"], "0..100", False),
    (["--select", "5", "--select-splice-max", "6.5"], "0..100", False),
    (["--select", "5", "--select-splice-min", "half"], "0..100", False),
    (["--select", "5", "--select-splice-min", "66", "--select-splice-max", "65"], "lies above", False),
    (["--select", "5", "--select-splice", "--select-max-edit-targets", "21"], "0..20", False),
    (["--select", "5", "--select-splice", "--base-edit-window", "8-4"], "--base-edit-window", False),
    (["--select", "5", "--base-editor", "abe", "--base-edit"], "adenine editor", False),
    (["--select", "5", "--base-editor", "abe", "--select-stop"], "adenine editor", False),
    (["--select", "5", "--base-editor", "abe", "--select-stop-min", "5"], "adenine editor", False),
    (["--select", "5", "--base-editor", "abe", "--select-stop-max", "65"], "adenine editor", False),
    (["--select", "5", "--base-editor", "abe", "--select-max-edit-targets", "2"], "adenine editor", False),
    (["--select", "5", "--base-editor", "abe", "--select-splice", "--select-stop"], "adenine editor", False),
    (["--select", "5", "--select-splice", "--select-coding-min", "5"], "--select-coding-min", False),
    (["--select", "5", "--select-splice-min", "5", "--select-coding-max", "65"], "--select-coding-max", False),
    (["--select", "5", "--select-splice-max", "65", "--select-transcripts", "100"], "--select-transcripts", False),
    (["--select", "5", "--select-splice", "--select-pairs", "3"], "--select-pairs", False),
    (["--select", "5", "--select-splice-min", "5", "--select-pairs", "3"], "--select-pairs", False),
    (["--select", "5", "--select-splice-max", "65", "--select-pairs", "3"], "--select-pairs", False),
    (["--select", "5", "--splice-edit", "--gpus", "2"], "one GPU", False),
    (["--select", "5", "--select-splice", "-l", "21"], "-l 20", False),
]


@pytest.mark.parametrize("extra,text,no_gff", SPLICE_REFUSALS, ids=[" ".join(r[0]) for r in SPLICE_REFUSALS])
def test_cli_refusals_come_before_any_side_effect(case, oracle, tmp_path, monkeypatch, extra, text, no_gff):
    monkeypatch.chdir(tmp_path)
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9"] + ([] if no_gff else ["-g", case["gff_path"]]) + extra
    backend = SpliceOracleBackend(oracle, case)
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=backend, out=io.StringIO())
    assert "--select" in str(e.value.code) and text in str(e.value.code)
    assert os.listdir(tmp_path) == [] and not backend.requests


# ---------------------------------------------------------------------------------------------- on the GPU
LIMITS = ((5, 65, 20, "any"), (0, 100, 20, "any"), (0, 100, 20, "donor"), (0, 100, 20, "acceptor"), (0, 100, 0, "any"), (0, 100, 1, "any"),
          (40, 60, 20, "any"), (0, 0, 20, "any"))


@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def _scanned(engine, case, max_words):
    """A genome with its tables, annotation ids, property and repair columns resident, and per arena the reference's view."""
    from cropsr_amd import properties, repair
    g = engine.genome(case["contigs"], max_words=max_words)
    request = annotate.Request(case["annotation"], case["names"], 0)
    hits = g.scan_score(20)
    counts = [(h.n_plus, h.n_minus) for h in hits.per_arena]
    feats = g.annotate(request, counts)
    props = g.guide_properties(counts)
    repairs = g.repair_scores(counts, 30)
    flags = case["annotation"].cds_flags()
    arenas = []
    for a, (arena, group) in enumerate(zip(g.arenas, g.groups)):
        A = _view(case, [case["contigs"][k] for k in group], [case["names"][k] for k in group], [0] * len(group), [int(o) for o in arena.offsets],
                  [case["hits"][k] for k in group])
        got = hits.per_arena[a]
        for key in A["tables"]:  # (the scan itself is pinned elsewhere; here it is the ground the selection stands on)
            assert np.array_equal(A["tables"][key].view(np.uint8), getattr(got, key).view(np.uint8)), key
        got_lo, got_hi, got_gene = request.gene_layout(sel.arena_layout(g, a))
        assert np.array_equal(got_lo, A["lo"]) and np.array_equal(got_hi, A["hi"]) and np.array_equal(got_gene, A["gene"])
        ids = np.concatenate([feats[a][0], feats[a][1]]).astype(np.int64)
        packed, rep = np.concatenate([props[a][0], props[a][1]]), np.concatenate([repairs[a][0], repairs[a][1]])
        A.update(model=request.coding_layout(sel.arena_layout(g, a)), flags=flags, group=list(group), offset_of={k: int(o) for k, o in zip(group, arena.offsets)},
                 ok_cds=(ids != NONE) & (np.concatenate([flags, [0]])[np.where(ids == NONE, flags.size, ids)] != 0),
                 ok_props=lambda lim, packed=packed: properties.Limits(**lim).passes(packed),
                 ok_repair=lambda lim, rep=rep: repair.Limits(*lim).passes(rep))
        arenas.append(A)
    return dict(genome=g, request=request, arenas=arenas, cache={}, models=case["models"], case=case)


@pytest.fixture(scope="module", params=[1, 3], ids=["one-arena", "three-arenas"])
def scanned(request, engine, case):
    s = _scanned(engine, case, None if request.param == 1 else 600)
    assert len(s["genome"].arenas) == request.param
    yield s
    s["genome"].close()


def _ok(A, min_score=0.0, cds=False, props=None, rep=None):
    ok = A["score"] >= np.float64(min_score)
    if cds:
        ok = ok & A["ok_cds"]
    if props is not None:
        ok = ok & A["ok_props"](props)
    if rep is not None:
        ok = ok & A["ok_repair"](rep)
    return ok


def _reference(s, a, K, limits, window=cases.WINDOW, editor="cbe", stop=None, **more):
    key = (a, K, limits, window, editor, stop, tuple(sorted((k, str(v)) for k, v in more.items())))
    if key not in s["cache"]:
        A = s["arenas"][a]
        stops = None if stop is None else (_scored(A, _stops(s["case"], A, window)), stop)
        s["cache"][key] = xref.select_numpy(A["tables"], A["member"], s["models"], A["rows"], K, _scored(A, _outcomes(s["case"], A, window, editor)), limits,
                                            _ok(A, **more), stops)
    return s["cache"][key]


def _device(s, a, K, slice_rows, limits, window=cases.WINDOW, editor="cbe", stop=None, min_score=0.0, cds=False, props=None, rep=None):
    from cropsr_amd import properties, repair
    A = s["arenas"][a]
    h = sel.ArenaSelect(s["genome"].arenas[a], A["lo"], A["hi"])
    try:
        if cds:
            h.set_flags(A["flags"])
        if slice_rows:
            h.set_limits(slice_rows)
        if props is not None:
            h.set_property_limits(properties.Limits(**props))
        if rep is not None:
            h.set_repair_limits(repair.Limits(*rep))
        h.set_coding(A["model"])
        if stop is not None:
            h.set_edit_limits(baseedit.Window(*window), baseedit.Limits(*stop))
        h.set_splice_limits(baseedit.Window(*window), editor, None if limits is None else baseedit.SpliceLimits(*limits))
        h.run(sel.Params(K, min_score, require_cds=cds))
        return h.fetch(), h.stats(), h.splice_stats()
    finally:
        h.close()


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("n_in", "n_pass", "sel")):
        print(what, name, "differing genes:", int((np.asarray(g) != np.asarray(w)).reshape(len(g), -1).any(axis=1).sum()))
        assert np.array_equal(np.asarray(g, np.uint32), np.asarray(w, np.uint32)), (what, name)


@pytest.mark.gpu
def test_gpu_the_genome_contains_the_cases(scanned, case):
    """On the reference's rows, before the device is looked at: every planted construct gives what it was planted for, the
    genome holds the step counts and the natural variety the other tests stand on, and under the limits used some genes have
    no passing row, some exactly K and some more than K."""
    seen = sum(_check_planted(case, A, A["offset_of"]) for A in scanned["arenas"])
    assert seen == len(case["planted"]) == 66
    what = " | ".join(p["what"] for p in case["planted"])
    for text in ("a GC donor", "the AT of an AT-AC", "the AC of an AT-AC", "an N in a site", "lower-case letters in a site", "before P's first exon",
                 "behind P's last exon", "without CDS", "strand is none", "a 3-letter intron", "a 2-letter intron", "a 1-letter intron", "P's first intron",
                 "P's last intron", "another transcript only", "two introns under one guide", "nested in the intron", "inside its intron",
                 "past the end of contig 0", "past the end of contig 3", "a donor behind 15 of 300", "a donor behind 195 of 300"):
        assert text in what, text
    # the table of the definition: per gene strand and site, the two (editor, row) that destroy it do so at either edge of the
    # window and not from just outside it; the other two (editor, row) do not
    for gene in "+-":
        for kind, letters in (("donor", "GT" if gene == "+" else "AC"), ("acceptor", "AG" if gene == "+" else "CT")):
            mine = [p for p in case["planted"] if p["what"].startswith("%s gene %s %s" % (gene, kind, letters))]
            assert len(mine) == 10
            edge = [p for p in mine if "window's" in p["what"]]
            assert len(edge) == 4 and all(p[kind + "s"] == 1 and p[kind + "_off"] == 31 and p["targets"] >= 1 for p in edge)
            assert sum("partner outside" in p["what"] for p in edge) == 2
            assert sorted((p["editor"], p["minus"]) for p in edge) == sorted([cases.EDITS[c] for c in letters] * 2)
            assert all(p["donors"] == p["acceptors"] == 0 for p in mine if p not in edge)
            assert sorted((p["editor"], p["minus"]) for p in mine if "no letter of it" in p["what"]) == sorted(
                set((e, r) for e in ("cbe", "abe") for r in (False, True)) - set(cases.EDITS[c] for c in letters))
    steps = {}
    for A in scanned["arenas"]:
        first = A["model"]["first"].astype(np.int64)
        steps.update({ident: int(first[r + 1] - first[r]) for r, ident in enumerate(A["ids"])})
        info = A["model"]["info"]
        assert ((info >> 17 & 1) == [int(case["models"][row[0]]["model"]) for row in A["rows"]]).all()
    assert steps["steps0"] == 0 and steps["steps2"] == 2 and steps["steps64"] == 64 and steps["steps65"] == 65
    assert case["models"][case["ids"].index("steps0")]["model"] and not case["models"][[i for i, x in enumerate(case["ids"]) if x.startswith("no_cds")][0]]["model"]
    two = [A for A in scanned["arenas"] if "two_introns" in A["ids"]][0]
    o = _outcomes(case, two, (1, 20), "cbe")[two["ids"].index("two_introns")]
    assert ((o[2] == 2) & (o[3] == 2) & (o[4] == 31) & (o[5] == 31)).any()  # two donors and two acceptors from one guide under the window 1-20
    # natural variety: destroyed sites of both kinds under both editors beyond the planted ones, rows without any
    for editor in xref.EDITORS:
        per = [o for A in scanned["arenas"] for o in _outcomes(case, A, cases.WINDOW, editor)]
        donors, acceptors = np.concatenate([o[2] for o in per]), np.concatenate([o[3] for o in per])
        assert donors.size > 3000 and (donors > 0).sum() > 40 and (acceptors > 0).sum() > 40 and ((donors == 0) & (acceptors == 0)).sum() > 1000
    for K in KS:  # nothing, exactly K, more than K
        n_pass = np.concatenate([_reference(scanned, a, K, (0, 100, 20, "any"), (1, 20))[1] for a in range(len(scanned["arenas"]))])
        assert (n_pass == 0).any() and (n_pass > K).any() == (K < 64) and ((n_pass == K).any() or K == 64), (K, np.bincount(n_pass))
    assert (np.concatenate([_reference(scanned, a, 1, (5, 65, 20, "any"))[1] for a in range(len(scanned["arenas"]))]) == 1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("editor", xref.EDITORS)
@pytest.mark.parametrize("window", xref.WINDOWS, ids=["%d-%d" % w for w in xref.WINDOWS])
def test_gpu_eval_of_every_gene_row_pair(scanned, case, window, editor):
    """The five outcomes of the evaluation kernel for EVERY (gene, row whose cut site is in the gene) pair, exactly; it needs no
    limits and no run."""
    n = n_sites = 0
    for a, A in enumerate(scanned["arenas"]):
        per_gene = _outcomes(case, A, window, editor)
        g = np.concatenate([np.full(o[0].size, r, np.uint32) for r, o in enumerate(per_gene)])
        t, want = np.concatenate([o[0] for o in per_gene]), [np.concatenate([o[j] for o in per_gene]) for j in range(1, 6)]
        n_plus = len(A["tables"]["pos_plus"])
        packed = np.where(t < n_plus, t, (t - n_plus) | (1 << 31)).astype(np.uint32)
        h = sel.ArenaSelect(scanned["genome"].arenas[a], A["lo"], A["hi"])
        try:
            h.set_coding(A["model"])
            got = h.splice_eval(baseedit.Window(*window), editor, g, packed)
            st = h.splice_stats()
            assert st["splice_eval_ms"] > 0 and st["splice_window"] == window[1] - window[0] + 1
            for name, x, w in zip(NAMES, got, want):
                print("arena", a, "window", window, editor, "pairs", g.size, name, "differs:", int((x != w).sum()))
            for x, w in zip(got, want):
                assert np.array_equal(x, w)
            assert h.splice_eval(None, editor, [], [])[0].size == 0
            if window == cases.WINDOW:  # NULL is the default window
                assert all(np.array_equal(x, w) for x, w in zip(h.splice_eval(None, baseedit.Editor(editor), g, packed), want))
        finally:
            h.close()
        n, n_sites = n + g.size, n_sites + int(((want[1] > 0) | (want[2] > 0)).sum())
    assert n > 3000 and n_sites > 8 * min(window[1] - window[0] + 1, 10)


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
@pytest.mark.parametrize("K", KS)
def test_gpu_selection_equals_the_reference(scanned, K, slice_rows):
    """sel, n_in, n_pass with splice limits against the reference, exactly: every value of kinds, max_targets 0 and 1, both
    editors, the widest window."""
    merged = 0
    for a in range(len(scanned["arenas"])):
        for editor in xref.EDITORS:
            for limits in LIMITS:
                got, stats, splice = _device(scanned, a, K, slice_rows, limits, editor=editor)
                _same(got, _reference(scanned, a, K, limits, editor=editor), "arena %d K %d %s limits %s" % (a, K, editor, limits))
                assert splice["splice_select_ms"] > 0 and splice["splice_window"] == 5
                merged += stats["merged_genes"]
            for limits in ((5, 65, 20, "any"), (0, 100, 20, "donor")):  # the widest window: many genes with more than K passing rows
                _same(_device(scanned, a, K, slice_rows, limits, (1, 20), editor)[0], _reference(scanned, a, K, limits, (1, 20), editor),
                      "arena %d K %d %s wide %s" % (a, K, editor, limits))
        got, _, splice = _device(scanned, a, K, slice_rows, None)  # limits cleared: the plain selection, and nothing of the splice kernel
        assert splice["splice_select_ms"] == 0
        A = scanned["arenas"][a]
        _same(got, xref.select_numpy(A["tables"], A["member"], scanned["models"], A["rows"], K, _scored(A, _outcomes(scanned["case"], A, cases.WINDOW, "cbe"))),
              "no limits")
    passing = np.concatenate([_reference(scanned, a, K, (0, 100, 20, "any"))[1] for a in range(len(scanned["arenas"]))])
    assert passing.sum() > 60 and (merged >= 1) == (slice_rows == 64)
    for kinds in ("donor", "acceptor"):  # each kind alone passes less than both, and something
        one = np.concatenate([_reference(scanned, a, K, (0, 100, 20, kinds))[1] for a in range(len(scanned["arenas"]))])
        assert 0 < one.sum() < passing.sum()
    for most in (0, 1):
        few = np.concatenate([_reference(scanned, a, K, (0, 100, most, "any"))[1] for a in range(len(scanned["arenas"]))])
        assert (few.sum() == 0) == (most == 0) and few.sum() < passing.sum()


@pytest.mark.gpu
def test_gpu_more_genes_than_one_launch(engine, case):
    """The splice kernel behind the driver's launch loop (crp_select_run hands every launch `d_items + first`): the arena's
    genes of few steps tiled to more than 2^20 (tests/select_scale_cases.py), with the tiled model, under limits that pass a
    row and fail a row of some gene.  At the default slices the second launch begins at gene 2^20; at slices of 64 a cut
    gene's pieces lie on both sides of every launch boundary (the list begins where boundary_start says, for both slicings).
    n_in, n_pass and sel whole, against the reference taken through the tiling."""
    s = _scanned(engine, case, None)
    try:
        A, K, limits = s["arenas"][0], 5, (0, 100, 20, "any")
        want, plain = _reference(s, 0, K, limits), _reference(s, 0, K, None)
        base = scale.few_steps(A["model"])
        assert ((0 < want[1][base]) & (want[1][base] < plain[1][base])).any()  # the limits pass a row and fail a row of some gene
        total = A["everyone"].sum(axis=1)  # the rows of a gene's two runs, scored or not
        assert total[base].max() > 64  # runs that the slices of 64 cut
        ids = scale.tiling(base, scale.G, scale.boundary_start(total, base, 64))
        assert scale.straddles(total[ids], 64)
        model = scale.tile_model(A["model"], ids)
        for slice_rows in (None, 64):
            cut = scale.host_cut(total[ids], slice_rows or 65536)
            h = sel.ArenaSelect(s["genome"].arenas[0], A["lo"][ids], A["hi"][ids])
            try:
                if slice_rows:
                    h.set_limits(slice_rows)
                h.set_coding(model)
                h.set_splice_limits(baseedit.Window(*cases.WINDOW), "cbe", baseedit.SpliceLimits(*limits))
                h.run(sel.Params(K))
                got, stats, splice = h.fetch(), h.stats(), h.splice_stats()
            finally:
                h.close()
            _same(got, [np.asarray(w)[ids] for w in want], "slices %r" % slice_rows)
            assert stats["items"] == cut["items"] and stats["launches"] == -(-cut["items"] // scale.MAX_ITEMS) >= 2
            assert stats["merged_genes"] == cut["cut_genes"] and splice["splice_select_ms"] > 0
            if slice_rows is None:
                assert stats["items"] == scale.G and stats["launches"] == 2
            else:
                assert stats["items"] > scale.G and cut["cut_genes"] > 0
    finally:
        s["genome"].close()


@pytest.mark.gpu
def test_gpu_limits_with_equality_nothing_and_exactly_k(scanned):
    """exact300 holds two guides whose donors lie behind 5 % and 65 % of L_P = 300 exactly; limits that pass nothing; limits that
    pass exactly K; the other windows."""
    A = [A for A in scanned["arenas"] if "exact300" in A["ids"]][0]
    a, r = scanned["arenas"].index(A), A["ids"].index("exact300")
    assert scanned["models"][A["rows"][r][0]]["length"] == 300
    for limits, n in (((5, 65, 20, "any"), 2), ((6, 65, 20, "any"), 1), ((5, 64, 20, "any"), 1), ((6, 64, 20, "any"), 0), ((5, 5, 20, "donor"), 1),
                      ((65, 65, 20, "donor"), 1), ((5, 65, 0, "any"), 0), ((5, 65, 20, "acceptor"), 0)):
        got = _device(scanned, a, 2, None, limits)[0]
        _same(got, _reference(scanned, a, 2, limits), "equality %s" % (limits,))
        assert got[1][r] == n and (got[2][r] != NONE).sum() == n, limits   # (with (5, 65) exactly K = 2 pass)
    for b in range(len(scanned["arenas"])):
        got = _device(scanned, b, 5, None, (100, 100, 20, "any"))[0]
        assert not got[1].any() and (got[2] == NONE).all() and np.array_equal(got[0], scanned["arenas"][b]["member"].sum(axis=1))
        for window in ((1, 20), (1, 1), (20, 20), (13, 17)):
            for editor in xref.EDITORS:
                _same(_device(scanned, b, 5, 64, (5, 65, 3, "any"), window, editor)[0], _reference(scanned, b, 5, (5, 65, 3, "any"), window, editor),
                      "window %s %s" % (window, editor))


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
def test_gpu_stop_or_splice_is_the_union(scanned, slice_rows):
    """Edit limits and splice limits on one handle: a row passes by either test under its own limits."""
    more = 0
    for a in range(len(scanned["arenas"])):
        for K, limits, stop, window in ((5, (5, 65, 20, "any"), (5, 65, 20), (4, 8)), (1, (0, 100, 1, "donor"), (0, 100, 2), (4, 8)),
                                        (64, (40, 100, 20, "acceptor"), (0, 50, 20), (1, 20)), (5, (100, 100, 20, "any"), (0, 100, 20), (13, 17))):
            got = _device(scanned, a, K, slice_rows, limits, window, "cbe", stop)[0]
            want = _reference(scanned, a, K, limits, window, "cbe", stop)
            _same(got, want, "arena %d K %d %s or %s" % (a, K, limits, stop))
            A = scanned["arenas"][a]
            only_stop = eref.select_numpy(A["tables"], A["member"], scanned["models"], A["rows"], K, _scored(A, _stops(scanned["case"], A, window)), stop)
            only_splice = _reference(scanned, a, K, limits, window)
            assert (want[1] >= only_stop[1]).all() and (want[1] >= only_splice[1]).all()
            more += int((want[1] > only_stop[1]).sum() > 0 and (want[1] > only_splice[1]).sum() > 0)
    assert more >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
def test_gpu_combined_with_the_other_limits(scanned, slice_rows):
    props = dict(gc_min=5, gc_max=15, max_run=5, max_t_run=4, max_stem=None)
    fewer = 0
    for a in range(len(scanned["arenas"])):
        for more in (dict(min_score=0.3), dict(cds=True), dict(props=props), dict(rep=(200, 50)),
                     dict(min_score=0.1, cds=True, props=props, rep=(100, 40))):
            for editor in xref.EDITORS:
                got = _device(scanned, a, 5, slice_rows, (0, 100, 20, "any"), (1, 20), editor, **more)[0]
                want = _reference(scanned, a, 5, (0, 100, 20, "any"), (1, 20), editor, **more)
                _same(got, want, "arena %d %s %s" % (a, editor, more))
                fewer += int((want[1] < _reference(scanned, a, 5, (0, 100, 20, "any"), (1, 20), editor)[1]).sum())
    assert fewer > 10


def _pieces(case):
    """Two texts that are PIECES of contigs, each beginning inside the intron of a planted gene whose guide destroys the
    intron's END site (the start site's exon is cut off): on p0 ('+' gene: the acceptor) and on p2 ('-' gene: the donor).
    Returns (texts, (name, start, length))."""
    cuts = []
    for k, text in ((0, "+ gene acceptor AG: G of a - row at the window's first"), (2, "- gene donor AC: A of a + row at the window's first")):
        first = [p for p in case["planted"] if p["what"].startswith(text)][0]
        assert first["donors"] + first["acceptors"] == 1
        m = case["models"][case["ids"].index(first["gene"])]
        cuts.append((case["names"][k], int(m["transcripts"][0][1][0]) - 1 + 36, 5000))  # (dec = 0: index = coordinate - 1) 35 letters of the intron cut off, 25 left
    return [case["contigs"][case["names"].index(n)][a:a + ln] for n, a, ln in cuts], cuts


@pytest.mark.gpu
def test_gpu_a_piece_that_starts_inside_an_intron(engine, case, oracle):
    """Texts that begin inside an intron: the row's steps open with cum > 0 where the next exon begins, the intron's end site is
    found from that step alone, and the offset counts from P's first coding letter all the same."""
    texts, cuts = _pieces(case)
    arena = engine.arena(texts)
    try:
        n_plus, n_minus = arena.scan_score_device(20)
        offsets = [int(o) for o in arena.offsets]
        A = _view(case, texts, [c[0] for c in cuts], [c[1] for c in cuts], offsets, [oracle.scan_score(t, 20) for t in texts])
        cols = arena.fetch(n_plus, n_minus)
        for key, got in zip(("pos_plus", "score_plus", "pos_minus", "score_minus"), (cols[0], cols[2], cols[3], cols[5])):
            assert np.array_equal(A["tables"][key].view(np.uint8), got.view(np.uint8)), key
        lo, hi, gene = case["annotation"].gene_layout(A["entries"], 0)
        assert np.array_equal(lo, A["lo"]) and np.array_equal(hi, A["hi"]) and np.array_equal(gene, A["gene"])
        model = case["annotation"].coding_layout(A["entries"], 0)
        for base, editor in zip(offsets, ("cbe", "abe")):  # non-vacuous: the first step of the row is the exon behind the intron, 31 letters counted
            r = int(np.flatnonzero(A["lo"] == base)[0])
            k = int(model["first"][r])
            assert model["at"][k] == base + 25 and model["cum"][k] == 31 and model["word"][k] & (1 << 17)
            o = _outcomes(case, A, cases.WINDOW, editor)[r]
            assert ((o[2] + o[3] == 1) & ((o[4] == 31) | (o[5] == 31))).any(), base
        h = sel.ArenaSelect(arena, lo, hi)
        try:
            h.set_coding(model)
            for editor in xref.EDITORS:
                per_gene = _outcomes(case, A, cases.WINDOW, editor)
                g = np.concatenate([np.full(o[0].size, r, np.uint32) for r, o in enumerate(per_gene)])
                t = np.concatenate([o[0] for o in per_gene])
                packed = np.where(t < n_plus, t, (t - n_plus) | (1 << 31)).astype(np.uint32)
                got = h.splice_eval(baseedit.Window(*cases.WINDOW), editor, g, packed)
                for j, x in enumerate(got):
                    assert np.array_equal(x, np.concatenate([o[j + 1] for o in per_gene])), (editor, j)
                assert g.size > 30
                for limits in ((5, 65, 20, "any"), (0, 100, 1, "any")):
                    h.set_splice_limits(None, editor, baseedit.SpliceLimits(*limits))
                    h.run(sel.Params(5))
                    want = xref.select_numpy(A["tables"], A["member"], case["models"], A["rows"], 5, _scored(A, per_gene), limits)
                    _same(h.fetch(), want, "pieces %s %s" % (editor, limits))
                    assert want[1].any()
        finally:
            h.close()
    finally:
        arena.close()


@pytest.mark.gpu
def test_gpu_calls_out_of_order(scanned, engine, case):
    """Each call returns its code and launches nothing; tables of another guide length are refused."""
    from cropsr_amd import coding
    A = scanned["arenas"][0]
    arena = scanned["genome"].arenas[0]
    L = nat.lib()
    h = sel.ArenaSelect(arena, A["lo"], A["hi"])

    def status(fn):
        with pytest.raises(nat.CropsrHipError) as e:
            fn()
        return e.value.status, str(e.value)

    try:
        h.set_splice_limits(None, "cbe", baseedit.SpliceLimits(5, 65))
        st, text = status(lambda: h.run(sel.Params(5)))
        assert st == nat.CRP_ERR_STATE and "crp_select_set_coding" in text        # limits without a model
        st, text = status(lambda: h.splice_eval(None, "cbe", [0], [0]))
        assert st == nat.CRP_ERR_STATE and "crp_select_set_coding" in text        # eval without a model
        lim = nat.SelectSpliceLimits(0, 100, 20, 3)
        for win in ((0, 8), (9, 8), (4, 21)):
            w = nat.SelectEditWindow(*win)
            assert L.crp_select_set_splice_limits(h._h, ctypes.byref(w), 0, ctypes.byref(lim)) == nat.CRP_ERR_INVALID
            assert b"window" in L.crp_last_error(h._ctx)
        assert L.crp_select_set_splice_limits(h._h, None, 2, ctypes.byref(lim)) == nat.CRP_ERR_INVALID and b"editor" in L.crp_last_error(h._ctx)
        for bad in ((66, 65, 20, 3), (0, 101, 20, 3)):
            c = nat.SelectSpliceLimits(*bad)
            assert L.crp_select_set_splice_limits(h._h, None, 0, ctypes.byref(c)) == nat.CRP_ERR_INVALID
            assert b"percentages" in L.crp_last_error(h._ctx)
        for bad in ((0, 100, 20, 0), (0, 100, 20, 4)):
            c = nat.SelectSpliceLimits(*bad)
            assert L.crp_select_set_splice_limits(h._h, None, 1, ctypes.byref(c)) == nat.CRP_ERR_INVALID
            assert b"kinds" in L.crp_last_error(h._ctx)
        h.set_coding(A["model"])
        h.run(sel.Params(5))                                                      # a refused setting changed nothing
        _same(h.fetch(), _reference(scanned, 0, 5, (5, 65, 20, "any")), "after the refusals")
        out = np.zeros(2, np.uint32)
        ptr = out.ctypes.data_as(nat.u32p)
        w = nat.SelectEditWindow(4, 21)
        assert L.crp_select_splice_eval(h._h, ctypes.byref(w), 0, ptr, ptr, 1, ptr, ptr) == nat.CRP_ERR_INVALID
        assert L.crp_select_splice_eval(h._h, None, 7, ptr, ptr, 1, ptr, ptr) == nat.CRP_ERR_INVALID and b"editor" in L.crp_last_error(h._ctx)
        n_plus, n_minus = len(A["tables"]["pos_plus"]), len(A["tables"]["pos_minus"])
        for g, packed in ((len(A["lo"]), 0), (0, n_plus), (0, n_minus | 1 << 31), (0xFFFFFFFF, 0)):
            st, text = status(lambda: h.splice_eval(None, "abe", [0, g], [0, packed]))
            assert st == nat.CRP_ERR_INVALID and "query 1" in text                # out of range: refused on the host
        st, text = status(lambda: h.run_pairs(sel.Params(5), sel.PairParams(5)))
        assert st == nat.CRP_ERR_UNSUPPORTED and "splice limits" in text          # pairs with splice limits
        h.set_coding_limits(coding.Limits(5, 65))
        st, text = status(lambda: h.run(sel.Params(5)))
        assert st == nat.CRP_ERR_UNSUPPORTED and "coding limits" in text          # both predicates at once
        h.set_coding_limits(None)
        h.set_splice_limits(None, "abe", baseedit.SpliceLimits(5, 65))
        h.set_edit_limits(None, baseedit.Limits())
        st, text = status(lambda: h.run(sel.Params(5)))
        assert st == nat.CRP_ERR_UNSUPPORTED and "adenine" in text                # ABE next to edit limits
        h.set_edit_limits(None, None)
        h.run(sel.Params(5))                                                      # ABE alone runs
        _same(h.fetch(), _reference(scanned, 0, 5, (5, 65, 20, "any"), editor="abe"), "abe after the refusal")
        h.set_splice_limits(None, "cbe", None)
        h.run_pairs(sel.Params(5), sel.PairParams(5))                             # and without limits the pairs run
        h.set_splice_limits(None, "cbe", baseedit.SpliceLimits(5, 65))
        h.set_coding(None)
        assert status(lambda: h.run(sel.Params(5)))[0] == nat.CRP_ERR_STATE       # model cleared
        assert status(lambda: h.splice_eval(None, "cbe", [0], [0]))[0] == nat.CRP_ERR_STATE
    finally:
        h.close()
    # tables from a scan at another guide length
    other = engine.arena([case["contigs"][1]])
    try:
        other.scan_score_device(21)
        entries = [(case["names"][1], 0, len(case["contigs"][1]), int(other.offsets[0]))]
        lo, hi, _ = case["annotation"].gene_layout(entries, 0)
        h = sel.ArenaSelect(other, lo, hi)
        try:
            h.set_coding(case["annotation"].coding_layout(entries, 0))
            h.set_splice_limits(None, "cbe", baseedit.SpliceLimits())
            st, text = status(lambda: h.run(sel.Params(5)))
            assert st == nat.CRP_ERR_STATE and "guide length 20" in text
            st, text = status(lambda: h.splice_eval(None, "cbe", [0], [0]))
            assert st == nat.CRP_ERR_STATE and "guide length 20" in text
        finally:
            h.close()
    finally:
        other.close()


@pytest.mark.gpu
def test_gpu_genome_level_call(engine, case):
    """Genome.scan_score(select=...) with splice editing: the Selection's fields against the reference, three arenas."""
    g = engine.genome(case["contigs"], max_words=600)
    try:
        request = annotate.Request(case["annotation"], case["names"], 0)
        A = _view(case, case["contigs"], case["names"], [0] * 4, _host_offsets(case["contigs"]), case["hits"])
        n_plus = len(A["tables"]["pos_plus"])
        for limits, window, editor in ((None, (4, 8), "cbe"), ((5, 65, 2, "any"), (4, 8), "abe"), ((0, 100, 20, "donor"), (1, 20), "cbe")):
            req = sel.Request(sel.Params(5), request, edit_window=baseedit.Window(*window), editor=editor,
                              splice_limits=None if limits is None else baseedit.SpliceLimits(*limits))
            s = g.scan_score(20, select=req).selection
            assert (s.stats["splice_select_ms"] > 0) == (limits is not None) and s.stats["splice_eval_ms"] > 0 and s.stats["editor"] == editor
            assert s.stats["splice_window"] == window[1] - window[0] + 1 and s.edit_targets is None
            per_gene = _scored(A, _outcomes(case, A, window, editor))
            n_in, n_pass, picked = xref.select_numpy(A["tables"], A["member"], case["models"], A["rows"], 5, per_gene, limits)
            gene = A["gene"]
            assert np.array_equal(s.n_pass[gene.astype(np.int64)], n_pass) and np.array_equal(s.n_in[gene.astype(np.int64)], n_in)
            r, c = np.nonzero(picked != NONE)
            order = np.lexsort((c, gene[r]))  # the Selection lists the genes in file order
            r, c = r[order], c[order]
            t = np.where(picked[r, c] >> 31 != 0, (picked[r, c] & 0x7FFFFFFF).astype(np.int64) + n_plus, picked[r, c].astype(np.int64))
            want = np.array([[int(v[list(per_gene[gr][0]).index(tr)]) for v in per_gene[gr][1:]] for gr, tr in zip(r.tolist(), t.tolist())], np.uint32)
            assert s.rows.size == r.size and np.array_equal(s.rows["gene"], gene[r]) and np.array_equal(s.rows["rank"], c + 1)
            for j, got in enumerate((s.splice_targets, s.donors, s.acceptors, s.donor_offset, s.acceptor_offset)):
                assert np.array_equal(got, want[:, j]), NAMES[j]
            assert np.array_equal(s.cds_length, [case["models"][int(x)]["length"] for x in gene[r]])
            if limits is not None:
                assert ((s.donor_offset != NO_SITE) | (s.acceptor_offset != NO_SITE)).all() and (s.splice_targets <= limits[2]).all() and s.rows.size > 20
            else:
                assert (s.donor_offset == NO_SITE).any() and (s.donor_offset != NO_SITE).any() and (s.acceptor_offset != NO_SITE).any()
        plain = g.scan_score(20, select=sel.Request(sel.Params(5), request)).selection
        assert plain.splice_targets is None and plain.cds_length is None and "splice_select_ms" not in plain.stats
        # stop or splice, with both groups of fields
        both = g.scan_score(20, select=sel.Request(sel.Params(5), request, splice_limits=baseedit.SpliceLimits(5, 65), edit_limits=baseedit.Limits(5, 65))).selection
        stops = _scored(A, _stops(case, A, cases.WINDOW))
        want = xref.select_numpy(A["tables"], A["member"], case["models"], A["rows"], 5, _scored(A, _outcomes(case, A, cases.WINDOW, "cbe")), (5, 65, 20, "any"),
                                 None, (stops, (5, 65, 20)))
        assert np.array_equal(both.n_pass[A["gene"].astype(np.int64)], want[1]) and both.rows.size == int((want[2] != NONE).sum())
        assert both.stop_offset is not None and ((both.stop_offset != eref.NO_STOP) | (both.donor_offset != NO_SITE) | (both.acceptor_offset != NO_SITE)).all()
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_command_line_end_to_end(case, tmp_path, monkeypatch):
    out_csv, _ = _run(case, tmp_path, monkeypatch, ["--select", "5", "--select-min-score", "0.2", "--base-editor", "abe", "--select-splice",
                                                    "--select-splice-min", "5", "--select-splice-max", "65", "--select-max-edit-targets", "3",
                                                    "--bench-json", str(tmp_path / "bench.json")], None)
    got = _read(out_csv + ".selected.csv")
    fields, want_rows, n_pass, label_row = _expected_fields(case, got[1:], (5, 65, 3, "any"), 0.2, "abe")
    assert got[0][-4:] == baseedit.SPLICE_HEADER and [r[-4:] for r in got[1:]] == fields and len(got) > 10
    assert "edit_targets" not in got[0] and set((r[0], r[6], r[8], r[10]) for r in got[1:]) == want_rows
    with open(tmp_path / "bench.json") as f:
        stage = json.load(f)["select"]
    assert stage["splice_select_ms"] > 0 and stage["splice_eval_ms"] > 0 and stage["splice_window"] == 5 and stage["editor"] == "abe"
