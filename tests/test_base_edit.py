"""--base-edit / --select-stop: guides with which a cytosine base editor writes a stop codon (cropsr_amd/baseedit.py, DESIGN.md
section 21).  Without a GPU: the three restatements against each other, crp_edit.h under sanitizers, the limits, the
selection statements, the command line over an oracle backend.  On the GPU: the evaluation kernel and the selection with
edit limits against the reference, exactly."""
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

import base_edit_cases as cases
import base_edit_reference as eref
import select_coding_cases as coding_cases
import select_coding_reference as cref
import select_reference as sref
import select_scale_cases as scale
from cropsr_amd import _native as nat
from cropsr_amd import annotate, baseedit, cli
from cropsr_amd import select as sel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
NO_STOP = baseedit.NO_STOP
KS = (1, 5, 64)
ZOO_ENTRIES = [("s", 0, 400, 64), ("other", 0, 300, 576), ("s", 25, 100, 1024)]  # whole contigs, and a piece that begins inside an exon


@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    c = cases.build(oracle)
    d = tmp_path_factory.mktemp("base_edit")
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
                score=np.concatenate([tables["score_plus"], tables["score_minus"]]), outcomes={})


def _outcomes(case, A, window):
    """eref.outcomes over the rows whose cut site is in the gene, by the closed form: computed once per arena and window."""
    if window not in A["outcomes"]:
        A["outcomes"][window] = eref.outcomes(A["tables"], A["everyone"], case["models"], A["rows"], A["arena"], window)
    return A["outcomes"][window]


def _scored(A, per_gene):
    """The outcomes of the rows IN the gene (scored rows only), as select_numpy takes them."""
    ok = A["score"] != -1.0
    return [tuple(v[ok[at]] for v in (at, t, s, o)) for at, t, s, o in per_gene]


def _check_planted(case, A, offset_of):
    """Every planted construct gives, on the reference's rows, what it was planted for."""
    per_gene = _outcomes(case, A, cases.WINDOW)
    pos, strand = eref.rows_of(A["tables"])
    seen = 0
    for p in case["planted"]:
        if p["gene"] not in A["ids"] or p["contig"] not in offset_of:
            continue
        g = A["ids"].index(p["gene"])
        at, targets, stops, off = per_gene[g]
        hit = np.flatnonzero((pos[at] == p["pos"] + offset_of[p["contig"]]) & (strand[at] == int(p["minus"])))
        assert hit.size == 1, p
        assert (int(targets[hit[0]]), int(stops[hit[0]]), int(off[hit[0]])) == (p["targets"], p["stops"], p["stop_off"]), p
        seen += 1
    return seen


# ---------------------------------------------------------------------------------------------- without a GPU
def _agree(gff, texts_by_name, entries, windows_all):
    """The three statements at every row position of every text for every gene: returns (rows compared, stops seen)."""
    loop_models, np_models = cref.model_loop(gff), cref.model_numpy(gff)
    texts = [texts_by_name[n][a:a + ln] for n, a, ln, _ in entries]
    arena = eref.make_arena(texts, [e[3] for e in entries])
    n = n_stops = 0
    for row in cref.layout_rows(gff, entries, 0):
        g, _, lo, hi = row
        for w, window in enumerate(eref.WINDOWS):
            for pos in range(lo - 30, hi + 31, 1 if window in windows_all else 5):
                for minus in (False, True):
                    a = eref.outcome_loop(loop_models[g], row, arena, pos + w % 5, minus, window)
                    b = eref.outcome_closed(np_models[g], row, arena, pos + w % 5, minus, window)
                    c = eref.outcome_subset(np_models[g], row, arena, pos + w % 5, minus, window)
                    assert a == b == c, (g, row, pos, minus, window, a, b, c)
                    n += 1
                    n_stops += a[1]
    return n, n_stops


@pytest.mark.parametrize("name", sorted(coding_cases.ZOO))
def test_three_statements_agree_on_the_gff_zoo(name):
    """The string statement, the closed form and the subset form over section 20's GFF zoo with random letters: whole contigs
    and a piece that begins inside an exon, both gene strands, both row strands, every window."""
    rng = np.random.default_rng(len(name))
    alpha = np.frombuffer(b"ACGTACGTACGTacgtN", dtype=np.uint8)
    texts = {n: rng.choice(alpha, ln).tobytes() for n, ln in coding_cases.ZOO_CONTIGS.items()}
    n, n_stops = _agree(coding_cases.ZOO[name], texts, ZOO_ENTRIES, ((4, 8),))
    print("rows", n, "stops", n_stops)
    assert n > 1000


@pytest.mark.parametrize("seed", range(6))
def test_three_statements_agree_on_random_exon_structures(seed):
    text, gff = cases.random_case(seed)
    n, n_stops = _agree(gff, {"s": text}, [("s", 0, len(text), 64), ("s", 100, 300, 1024)], ((4, 8), (1, 20)))
    print("rows", n, "stops", n_stops)
    assert n > 5000 and n_stops > 20


def test_baseedit_outcome_is_the_definition(case):
    """baseedit.outcome, the package's own general statement, against the closed form on the planted constructs."""
    offsets = _host_offsets(case["contigs"])
    A = _view(case, case["contigs"], case["names"], [0] * 4, offsets, case["hits"])
    assert _check_planted(case, A, dict(enumerate(offsets))) == len(case["planted"])
    index_of = {}
    for p in case["planted"]:
        g = A["ids"].index(p["gene"])
        m = case["models"][A["rows"][g][0]]
        if g not in index_of:
            index_of[g] = eref._index(m, A["rows"][g]) if m["model"] else None
        got = baseedit.outcome(A["arena"], p["pos"] + offsets[p["contig"]], p["minus"], baseedit.Window(*cases.WINDOW), index_of[g], m["length"],
                               m["strand"] == "-")
        assert got == (p["targets"], p["stops"], p["stop_off"]), p
    assert sum(p["stops"] > 0 for p in case["planted"]) > 40 and sum(p["stops"] == 0 for p in case["planted"]) > 40
    assert max(p["stops"] for p in case["planted"]) == 2


def test_window_and_limits_are_checked():
    assert baseedit.Window().astuple() == (4, 8) and len(baseedit.Window(1, 20)) == 20 and baseedit.Window.parse("13-17").astuple() == (13, 17)
    for bad in ((0, 5), (5, 4), (1, 21), (4.5, 8), (True, 8)):
        with pytest.raises(ValueError):
            baseedit.Window(*bad)
    for bad in ("4", "4-", "a-b", "4-8-9", "-4-8", "8-4", "0-3", "4:8", ""):
        with pytest.raises(ValueError):
            baseedit.Window.parse(bad)
    assert baseedit.Window(4, 8).positions(100, False) == [83, 84, 85, 86, 87] and baseedit.Window(4, 8).positions(100, True) == [115, 116, 117, 118, 119]
    assert baseedit.Limits().astuple() == (0, 100, 20)
    for bad in ((-1, 100, 20), (0, 101, 20), (66, 65, 20), (0, 100, 21), (0, 100, -1), (0.5, 100, 20), (0, 100, True)):
        with pytest.raises(ValueError):
            baseedit.Limits(*bad)
    lim = baseedit.Limits(5, 65, 1)
    targets, off, L = np.array([1, 1, 1, 2, 1, 1]), np.array([15, 12, 195, 30, 198, NO_STOP], np.uint32), np.full(6, 300)
    assert lim.passes(targets, off, L).tolist() == [True, False, True, False, False, False]
    assert lim.passes(targets, off, L).tolist() == [eref.passes((5, 65, 1), t, o, 300) for t, o in zip(targets, off)]
    big = np.array([4294967100], np.uint32)  # 100 off needs its 64 bits
    assert baseedit.Limits(99, 100).passes([1], big, [0xFFFFFFFF]).tolist() == [True] and baseedit.Limits(0, 98).passes([1], big, [0xFFFFFFFF]).tolist() == [False]
    assert baseedit.fields(3, 1, 30, 300) == (3, 1, 11, "10.0") and baseedit.fields(2, 0, NO_STOP, 300) == (2, 0, "", "")
    with pytest.raises(ValueError):
        sel.Request(sel.Params(1), None, edit_limits=baseedit.Limits(), pairs=sel.PairParams(1))
    with pytest.raises(ValueError):
        from cropsr_amd import coding
        sel.Request(sel.Params(1), None, edit_limits=baseedit.Limits(), coding_limits=coding.Limits())
    r = sel.Request(sel.Params(1), None, edit_limits=baseedit.Limits())
    assert r.edit and r.edit_window.astuple() == (4, 8) and not sel.Request(sel.Params(1), None).edit


def test_selection_statements_agree_on_the_case_genome(case):
    """select_numpy (closed form) against select_loop (string statement) over the 80 kb genome."""
    A = _view(case, case["contigs"], case["names"], [0] * 4, _host_offsets(case["contigs"]), case["hits"])
    loop_models = cref.model_loop(case["gff"])
    ok = A["score"] >= 0.2
    for K, limits, window, use_ok in ((5, (5, 65, 20), (4, 8), False), (1, (0, 100, 1), (4, 8), True), (64, (0, 100, 20), (1, 20), False)):
        per_gene = _scored(A, _outcomes(case, A, window))
        got = eref.select_numpy(A["tables"], A["member"], case["models"], A["rows"], K, per_gene, limits, ok if use_ok else None)
        want = eref.select_loop(A["tables"], A["lo"], A["hi"], loop_models, A["rows"], A["arena"], window, K, limits, ok if use_ok else None)
        for g, w, name in zip(got, want, ("n_in", "n_pass", "sel")):
            assert np.array_equal(g, w), (K, limits, name)
        assert got[1].any() and (got[1] < got[0]).any()


def test_edit_driver_under_sanitizers(tmp_path):
    """tests/native/edit_driver.cpp: crp_edit.h over hand-made planes and step functions against a brute-force loop, under
    ASan + UBSan."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "edit_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "cropsr_amd", "csrc"), os.path.join(ROOT, "tests", "native", "edit_driver.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout + run.stderr


# ---------------------------------------------------------------------------------------------- the command line, over the oracle
class EditOracleBackend(OracleBackend):
    """OracleBackend plus the `select` keyword with base editing: the selection by the numpy statement over one host arena,
    the outcomes of the selected rows by the closed form."""

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
        window = select.edit_window.astuple() if select.edit else cases.WINDOW
        per_gene = _scored(A, _outcomes(self.case, A, window))
        limits = None if select.edit_limits is None else select.edit_limits.astuple()
        ok = A["score"] >= select.params.min_score
        n_in, n_pass, picked = eref.select_numpy(A["tables"], A["member"], self.case["models"], A["rows"], select.params.k, per_gene, limits, ok)
        part = dict(offsets=np.array(offsets, np.uint64), lengths=np.array([len(t) for t in texts], np.uint64), group=list(range(len(texts))),
                    gene=gene, n_in=n_in, n_pass=n_pass, sel=picked, **A["tables"])
        if select.edit:
            n_plus = len(A["tables"]["pos_plus"])
            shape = picked.shape
            targets, stops, off = np.zeros(shape, np.uint32), np.zeros(shape, np.uint32), np.full(shape, NO_STOP, np.uint32)
            for g, (at, t, s, o) in enumerate(per_gene):
                where = {int(x): j for j, x in enumerate(at)}
                for k, packed in enumerate(picked[g]):
                    if packed != NONE:
                        j = where[(int(packed) & 0x7FFFFFFF) + (n_plus if int(packed) >> 31 else 0)]
                        targets[g, k], stops[g, k], off[g, k] = t[j], s[j], o[j]
            part["edit"] = dict(targets=targets, stops=stops, stop_off=off,
                                length=np.array([self.case["models"][r[0]]["length"] for r in A["rows"]], np.uint32))
        out = sel.HitList(out)
        out.selection = sel.assemble(req.annotation.genes()[0], select.params.k, [part])
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


def _expected_fields(case, got_rows, limits, min_score, window=cases.WINDOW):
    """Per row of a selection file (gene label, end_pos, strand -> the table row): the four fields by the string statement, and
    the set of (gene, chromosome, end_pos, strand) the selection must consist of."""
    from decimal import ROUND_HALF_UP, Decimal
    offsets = _host_offsets(case["contigs"])
    A = _view(case, case["contigs"], case["names"], [0] * 4, offsets, case["hits"])
    models = cref.model_loop(case["gff"])
    n_in, n_pass, picked = eref.select_loop(A["tables"], A["lo"], A["hi"], models, A["rows"], A["arena"], window, 5, limits, A["score"] >= min_score)
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
    fields = []
    for g in got_rows:
        r = label_row[g[0]]
        end, minus = int(g[8]) + offset_of[g[6]], g[10] == "-"  # (gene, rank, passing, then the main table's fields without its first)
        m = models[A["rows"][r][0]]
        targets, stops, off = eref.outcome_loop(m, A["rows"][r], A["arena"], end - 3 if minus else end, minus, window)  # end_pos: i, or j + 3
        if off == NO_STOP:
            fields.append([str(targets), str(stops), "", ""])
        else:
            pct = (Decimal(100 * off) / Decimal(m["length"])).quantize(Decimal("0.1"), rounding=ROUND_HALF_UP)
            fields.append([str(targets), str(stops), str(off // 3 + 1), str(pct)])
    return fields, want_rows, n_pass, label_row


def test_cli_fields_and_filter_over_the_oracle(case, oracle, tmp_path, monkeypatch):
    from cropsr_amd import rows as rows_mod
    backend = EditOracleBackend(oracle, case)
    base = ["--select", "5", "--select-min-score", "0.2"]
    plain, plain_out = _run(case, tmp_path, monkeypatch, base, backend, "plain.csv")
    assert backend.requests[-1].edit is False and backend.requests[-1].edit_limits is None
    with_fields, fields_out = _run(case, tmp_path, monkeypatch, base + ["--base-edit"], backend, "fields.csv")
    assert backend.requests[-1].edit is True and backend.requests[-1].edit_limits is None and backend.requests[-1].edit_window.astuple() == (4, 8)
    bench = str(tmp_path / "bench.json")
    filtered, _ = _run(case, tmp_path, monkeypatch, base + ["--select-stop-min", "5", "--select-stop-max", "65", "--select-max-edit-targets", "2",
                                                            "--bench-json", bench], backend, "filtered.csv")
    assert backend.requests[-1].edit_limits.astuple() == (5, 65, 2)
    wide, _ = _run(case, tmp_path, monkeypatch, base + ["--select-stop", "--base-edit-window", "1-20"], backend, "wide.csv")
    assert backend.requests[-1].edit_limits.astuple() == (0, 100, 20) and backend.requests[-1].edit_window.astuple() == (1, 20)
    for path in (with_fields, filtered, wide):  # the main table is what it was
        with open(plain, "rb") as a, open(path, "rb") as b:
            assert a.read() == b.read()
    # without the new options: the header and the fields of before; with --base-edit: the same file with four more fields
    old, new = _read(plain + ".selected.csv"), _read(with_fields + ".selected.csv")
    assert old[0] == ["gene", "rank", "passing"] + rows_mod.HEADER[1:] and new[0] == old[0] + baseedit.HEADER
    assert [r[:-4] for r in new] == old and len(old) > 60
    buf = io.StringIO()
    csv.writer(buf).writerows([r[:-4] for r in new])
    with open(plain + ".selected.csv", newline="") as f:
        assert f.read() == buf.getvalue()  # byte for byte
    fields, want_rows, _, _ = _expected_fields(case, new[1:], None, 0.2)
    assert [r[-4:] for r in new[1:]] == fields
    assert any(f[2] == "" for f in fields) and any(f[2] != "" for f in fields)
    assert set((r[0], r[6], r[8], r[10]) for r in new[1:]) == want_rows
    # the filtered selection: the reference's rows, every one with a stop inside the limits
    got = _read(filtered + ".selected.csv")
    fields, want_rows, n_pass, label_row = _expected_fields(case, got[1:], (5, 65, 2), 0.2)
    assert got[0] == new[0] and [r[-4:] for r in got[1:]] == fields and 10 < len(got) < len(new)
    assert set((r[0], r[6], r[8], r[10]) for r in got[1:]) == want_rows
    for r in got[1:]:
        assert int(r[2]) == n_pass[label_row[r[0]]] and 5.0 <= float(r[-1]) <= 65.0 and int(r[-3]) >= 1 and 1 <= int(r[-4]) <= 2
    assert "gene:no_cds" not in [r[0] for r in got[1:]] and "gene:no_strand" not in [r[0] for r in got[1:]]
    got = _read(wide + ".selected.csv")
    fields, want_rows, _, _ = _expected_fields(case, got[1:], (0, 100, 20), 0.2, (1, 20))
    assert [r[-4:] for r in got[1:]] == fields and set((r[0], r[6], r[8], r[10]) for r in got[1:]) == want_rows and len(got) > 10
    with open(bench) as f:
        assert "select" in json.load(f)


EDIT_REFUSALS = [
    (["--base-edit"], "belongs to --select", False),
    (["--base-edit-window", "4-8"], "belongs to --select", False),
    (["--select-stop"], "belongs to --select", False),
    (["--select-stop-min", "5"], "belongs to --select", False),
    (["--select-stop-max", "65"], "belongs to --select", False),
    (["--select-max-edit-targets", "2"], "belongs to --select", False),
    (["--select", "5", "--base-edit"], "needs -g", True),
    (["--select", "5", "--select-stop"], "needs -g", True),
    (["--select", "5", "--base-edit-window", "8-4"], "--base-edit-window", False),
    (["--select", "5", "--base-edit-window", "0-8"], "--base-edit-window", False),
    (["--select", "5", "--base-edit-window", "4-21"], "--base-edit-window", False),
    (["--select", "5", "--base-edit-window", "4"], "LO-HI", False),
    (["--select", "5", "--base-edit-window", "a-b"], "LO-HI", False),
    (["--select", "5", "--select-stop-min", "101"], "0..100", False),
    (["--select", "5", "--select-stop-max", "-1"], "0..100", False),
    (["--select", "5", "--select-stop-max", "6.5"], "0..100", False),
    (["--select", "5", "--select-stop-min", "half"], "0..100", False),
    (["--select", "5", "--select-stop-min", "66", "--select-stop-max", "65"], "lies above", False),
    (["--select", "5", "--select-max-edit-targets", "21"], "0..20", False),
    (["--select", "5", "--select-max-edit-targets", "-1"], "0..20", False),
    (["--select", "5", "--select-max-edit-targets", "two"], "0..20", False),
    (["--select", "5", "--select-stop", "--select-coding-min", "5"], "--select-coding-min", False),
    (["--select", "5", "--select-stop-min", "5", "--select-coding-max", "65"], "--select-coding-max", False),
    (["--select", "5", "--select-stop-max", "65", "--select-transcripts", "100"], "--select-transcripts", False),
    (["--select", "5", "--select-max-edit-targets", "2", "--select-coding-min", "5"], "--select-coding-min", False),
    (["--select", "5", "--select-stop", "--select-pairs", "3"], "--select-pairs", False),
    (["--select", "5", "--select-stop-min", "5", "--select-pairs", "3"], "--select-pairs", False),
    (["--select", "5", "--select-stop-max", "65", "--select-pairs", "3"], "--select-pairs", False),
    (["--select", "5", "--select-max-edit-targets", "2", "--select-pairs", "3"], "--select-pairs", False),
    (["--select", "5", "--base-edit", "--gpus", "2"], "one GPU", False),
    (["--select", "5", "--base-edit", "-l", "21"], "-l 20", False),
]


@pytest.mark.parametrize("extra,text,no_gff", EDIT_REFUSALS, ids=[" ".join(r[0]) for r in EDIT_REFUSALS])
def test_cli_refusals_come_before_any_side_effect(case, oracle, tmp_path, monkeypatch, extra, text, no_gff):
    monkeypatch.chdir(tmp_path)
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9"] + ([] if no_gff else ["-g", case["gff_path"]]) + extra
    backend = EditOracleBackend(oracle, case)
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=backend, out=io.StringIO())
    assert "--select" in str(e.value.code) and text in str(e.value.code)
    assert os.listdir(tmp_path) == [] and not backend.requests


# ---------------------------------------------------------------------------------------------- on the GPU
LIMITS = ((5, 65, 20), (0, 100, 20), (0, 100, 0), (0, 100, 1), (40, 60, 20), (0, 0, 20))


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


def _reference(s, a, K, limits, window=cases.WINDOW, **more):
    key = (a, K, limits, window, tuple(sorted((k, str(v)) for k, v in more.items())))
    if key not in s["cache"]:
        A = s["arenas"][a]
        s["cache"][key] = eref.select_numpy(A["tables"], A["member"], s["models"], A["rows"], K, _scored(A, _outcomes(s["case"], A, window)), limits,
                                            _ok(A, **more))
    return s["cache"][key]


def _device(s, a, K, slice_rows, limits, window=cases.WINDOW, min_score=0.0, cds=False, props=None, rep=None):
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
        h.set_edit_limits(baseedit.Window(*window), None if limits is None else baseedit.Limits(*limits))
        h.run(sel.Params(K, min_score, require_cds=cds))
        return h.fetch(), h.stats(), h.edit_stats()
    finally:
        h.close()


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("n_in", "n_pass", "sel")):
        print(what, name, "differing genes:", int((np.asarray(g) != np.asarray(w)).reshape(len(g), -1).any(axis=1).sum()))
        assert np.array_equal(np.asarray(g, np.uint32), np.asarray(w, np.uint32)), (what, name)


@pytest.mark.gpu
def test_gpu_the_genome_contains_the_cases(scanned, case):
    """On the reference's rows, before the device is looked at: every planted construct gives what it was planted for, and
    the genome holds the step counts and the natural variety the other tests stand on."""
    seen = sum(_check_planted(case, A, A["offset_of"]) for A in scanned["arenas"])
    assert seen == len(case["planted"]) == 122
    what = " | ".join(p["what"] for p in case["planted"])
    for text in ("split by an intron", "first three letters of an exon", "last three letters of an exon", "P's first codon", "P's last codon",
                 "L_P = 1 mod 3", "L_P = 2 mod 3", "original TAG", "without targets", "an N inside", "lower-case", "two stops", "without CDS",
                 "strand is none", "nested in the intron", "antisense", "row in its intron", "past the end of contig 0", "past the end of contig 3",
                 "a stop at 15 of 300", "a stop at 195 of 300"):
        assert text in what, text
    for codon in ("CAA", "CAG", "CGA", "TGG"):
        for gene in "+-":
            for row in "+-":
                mine = [p for p in case["planted"] if p["what"].startswith("%s %s gene %s row" % (codon, gene, row))]
                makes = (codon == "TGG") != (gene == row)  # the edit reads C -> T where the strands agree, G -> A where they do not
                assert len(mine) == 6 and any(p["stops"] for p in mine) == makes and not all(p["stops"] for p in mine), (codon, gene, row)
    tgg = [p for p in case["planted"] if p["what"].startswith("TGG + gene - row")]
    assert sorted((p["targets"], p["stops"]) for p in tgg) == [(0, 0), (1, 1), (1, 1), (2, 1), (2, 1), (2, 1)]  # third only, second only, both
    steps = {}
    for A in scanned["arenas"]:
        first = A["model"]["first"].astype(np.int64)
        steps.update({ident: int(first[r + 1] - first[r]) for r, ident in enumerate(A["ids"])})
        info = A["model"]["info"]
        assert ((info >> 17 & 1) == [int(case["models"][row[0]]["model"]) for row in A["rows"]]).all()
    assert steps["steps0"] == 0 and steps["steps2"] == 2 and steps["steps64"] == 64 and steps["steps65"] == 65
    assert case["models"][case["ids"].index("steps0")]["model"] and not case["models"][case["ids"].index("no_cds")]["model"]
    is_it = lambda ident: ident.startswith("two_stops_") and not ident.startswith("two_stops_ga")
    three = [A for A in scanned["arenas"] if any(is_it(i) for i in A["ids"])][0]
    g = [i for i, ident in enumerate(three["ids"]) if is_it(ident)][0]
    assert _outcomes(case, three, (1, 20))[g][2].max() == 3  # three stops from one guide under the window 1-20
    # natural variety: rows with and without stops on both strands of rows and genes, stops beyond the planted ones
    total = np.concatenate([o[2] for A in scanned["arenas"] for o in _outcomes(case, A, cases.WINDOW)])
    assert total.size > 3000 and (total > 0).sum() > 120 and (total == 0).sum() > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("window", eref.WINDOWS, ids=["%d-%d" % w for w in eref.WINDOWS])
def test_gpu_eval_of_every_gene_row_pair(scanned, case, window):
    """targets, stops and stop_off of the evaluation kernel for EVERY (gene, row whose cut site is in the gene) pair, exactly; it
    needs no limits and no run."""
    n = n_stops = 0
    for a, A in enumerate(scanned["arenas"]):
        per_gene = _outcomes(case, A, window)
        g = np.concatenate([np.full(o[0].size, r, np.uint32) for r, o in enumerate(per_gene)])
        t, want = np.concatenate([o[0] for o in per_gene]), [np.concatenate([o[j] for o in per_gene]) for j in (1, 2, 3)]
        n_plus = len(A["tables"]["pos_plus"])
        packed = np.where(t < n_plus, t, (t - n_plus) | (1 << 31)).astype(np.uint32)
        h = sel.ArenaSelect(scanned["genome"].arenas[a], A["lo"], A["hi"])
        try:
            h.set_coding(A["model"])
            got = h.edit_eval(baseedit.Window(*window), g, packed)
            st = h.edit_stats()
            assert st["edit_eval_ms"] > 0 and st["edit_targets_window"] == window[1] - window[0] + 1
            for name, x, w in zip(("targets", "stops", "stop_off"), got, want):
                print("arena", a, "window", window, "pairs", g.size, name, "differs:", int((x != w).sum()))
            for x, w in zip(got, want):
                assert np.array_equal(x, w)
            assert h.edit_eval(None, [], [])[0].size == 0
            if window == cases.WINDOW:  # NULL is the default window
                assert all(np.array_equal(x, w) for x, w in zip(h.edit_eval(None, g, packed), want))
        finally:
            h.close()
        n, n_stops = n + g.size, n_stops + int((want[1] > 0).sum())
    assert n > 3000 and n_stops > 15 * min(window[1] - window[0] + 1, 10)


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
@pytest.mark.parametrize("K", KS)
def test_gpu_selection_equals_the_reference(scanned, K, slice_rows):
    """sel, n_in, n_pass with edit limits against the reference, exactly."""
    merged = 0
    for a in range(len(scanned["arenas"])):
        for limits in LIMITS:
            got, stats, edit = _device(scanned, a, K, slice_rows, limits)
            want = _reference(scanned, a, K, limits)
            _same(got, want, "arena %d K %d limits %s" % (a, K, limits))
            assert edit["edit_select_ms"] > 0 and edit["edit_targets_window"] == 5
            merged += stats["merged_genes"]
        for limits in ((5, 65, 20), (0, 100, 20)):  # the widest window: many genes with more than K passing rows
            _same(_device(scanned, a, K, slice_rows, limits, (1, 20))[0], _reference(scanned, a, K, limits, (1, 20)), "arena %d K %d wide %s" % (a, K, limits))
        got, _, edit = _device(scanned, a, K, slice_rows, None)  # limits cleared: the plain selection, and nothing of the edit kernel
        assert edit["edit_select_ms"] == 0
        _same(got, eref.select_numpy(scanned["arenas"][a]["tables"], scanned["arenas"][a]["member"], scanned["models"], scanned["arenas"][a]["rows"], K,
                                     _scored(scanned["arenas"][a], _outcomes(scanned["case"], scanned["arenas"][a], cases.WINDOW))), "no limits")
    passing = np.concatenate([_reference(scanned, a, K, (0, 100, 20))[1] for a in range(len(scanned["arenas"]))])
    assert passing.sum() > 120 and (merged >= 1) == (slice_rows == 64)


@pytest.mark.gpu
def test_gpu_more_genes_than_one_launch(engine, case):
    """The edit kernel behind the driver's launch loop (crp_select_run hands every launch `d_items + first`): the arena's genes
    of few steps tiled to more than 2^20 (tests/select_scale_cases.py), with the tiled model, under limits that pass a row and
    fail a row of some gene.  At the default slices the second launch begins at gene 2^20; at slices of 64 a cut gene's pieces
    lie on both sides of every launch boundary (the list begins where boundary_start says, for both slicings).  n_in, n_pass
    and sel whole, against the reference taken through the tiling."""
    s = _scanned(engine, case, None)
    try:
        A, K, limits = s["arenas"][0], 5, (5, 65, 20)
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
                h.set_edit_limits(baseedit.Window(*cases.WINDOW), baseedit.Limits(*limits))
                h.run(sel.Params(K))
                got, stats, edit = h.fetch(), h.stats(), h.edit_stats()
            finally:
                h.close()
            _same(got, [np.asarray(w)[ids] for w in want], "slices %r" % slice_rows)
            assert stats["items"] == cut["items"] and stats["launches"] == -(-cut["items"] // scale.MAX_ITEMS) >= 2
            assert stats["merged_genes"] == cut["cut_genes"] and edit["edit_select_ms"] > 0
            if slice_rows is None:
                assert stats["items"] == scale.G and stats["launches"] == 2
            else:
                assert stats["items"] > scale.G and cut["cut_genes"] > 0
    finally:
        s["genome"].close()


@pytest.mark.gpu
def test_gpu_limits_with_equality_nothing_and_exactly_k(scanned):
    """exact300 holds two guides whose stops lie at 5 % and at 65 % of L_P = 300 exactly; limits that pass nothing; limits that
    pass exactly K; the other windows."""
    A = [A for A in scanned["arenas"] if "exact300" in A["ids"]][0]
    a, r = scanned["arenas"].index(A), A["ids"].index("exact300")
    assert scanned["models"][A["rows"][r][0]]["length"] == 300
    for limits, n in (((5, 65, 20), 2), ((6, 65, 20), 1), ((5, 64, 20), 1), ((6, 64, 20), 0), ((5, 5, 20), 1), ((65, 65, 20), 1), ((5, 65, 0), 0)):
        got = _device(scanned, a, 2, None, limits)[0]
        _same(got, _reference(scanned, a, 2, limits), "equality %s" % (limits,))
        assert got[1][r] == n and (got[2][r] != NONE).sum() == n, limits   # (with (5, 65) exactly K = 2 pass)
    for b in range(len(scanned["arenas"])):
        got = _device(scanned, b, 5, None, (100, 100, 20))[0]
        assert not got[1].any() and (got[2] == NONE).all() and np.array_equal(got[0], scanned["arenas"][b]["member"].sum(axis=1))
        for window in ((1, 20), (1, 1), (20, 20), (13, 17)):
            _same(_device(scanned, b, 5, 64, (5, 65, 3), window)[0], _reference(scanned, b, 5, (5, 65, 3), window), "window %s" % (window,))


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
def test_gpu_combined_with_the_other_limits(scanned, slice_rows):
    props = dict(gc_min=7, gc_max=14, max_run=4, max_t_run=3, max_stem=None)
    fewer = 0
    for a in range(len(scanned["arenas"])):
        for more in (dict(min_score=0.3), dict(cds=True), dict(props=props), dict(rep=(200, 50)),
                     dict(min_score=0.2, cds=True, props=props, rep=(100, 40))):
            got = _device(scanned, a, 5, slice_rows, (0, 100, 20), **more)[0]
            want = _reference(scanned, a, 5, (0, 100, 20), **more)
            _same(got, want, "arena %d %s" % (a, more))
            fewer += int((want[1] < _reference(scanned, a, 5, (0, 100, 20))[1]).sum())
        assert _reference(scanned, a, 5, (0, 100, 20), min_score=0.2, cds=True, props=props, rep=(100, 40))[1].any() or a > 0
    assert fewer > 10


def _pieces(case):
    """Two texts that are PIECES of contigs, each beginning inside an exon: 21 letters into the exon of a planted gene whose
    guide writes a stop, on e0 ('+' gene) and on e2 ('-' gene).  Returns (texts, (name, start, length))."""
    cuts = []
    for k, which in ((0, 2), (2, 38)):  # (guides on the '+' table: the piece keeps their PAM)
        first = [p for p in case["planted"] if p["contig"] == k][which]
        assert first["stops"] == 1
        m = case["models"][case["ids"].index(first["gene"])]
        cuts.append((case["names"][k], int(m["transcripts"][0][0][0]) - 1 + 21, 5000))  # (dec = 0: index = coordinate - 1)
    return [case["contigs"][case["names"].index(n)][a:a + ln] for n, a, ln in cuts], cuts


@pytest.mark.gpu
def test_gpu_a_piece_that_starts_inside_an_exon(engine, case, oracle):
    """Texts that begin inside an exon: the row's steps open at the text's first letter with cum > 0, and the frame counts
    from P's first coding letter all the same."""
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
        for base in offsets:  # non-vacuous: a row whose steps open at the text's first letter with 21 letters counted, and a stop found there
            r = int(np.flatnonzero(A["lo"] == base)[0])
            k = int(model["first"][r])
            assert model["at"][k] == base and model["cum"][k] == 21 and model["word"][k] == 1 << 17
            assert (_outcomes(case, A, cases.WINDOW)[r][2] > 0).any(), base
        h = sel.ArenaSelect(arena, lo, hi)
        try:
            h.set_coding(model)
            per_gene = _outcomes(case, A, cases.WINDOW)
            g = np.concatenate([np.full(o[0].size, r, np.uint32) for r, o in enumerate(per_gene)])
            t = np.concatenate([o[0] for o in per_gene])
            packed = np.where(t < n_plus, t, (t - n_plus) | (1 << 31)).astype(np.uint32)
            got = h.edit_eval(baseedit.Window(*cases.WINDOW), g, packed)
            for j, x in enumerate(got):
                assert np.array_equal(x, np.concatenate([o[j + 1] for o in per_gene])), j
            assert g.size > 30
            for limits in ((5, 65, 20), (0, 100, 1)):
                h.set_edit_limits(None, baseedit.Limits(*limits))
                h.run(sel.Params(5))
                want = eref.select_numpy(A["tables"], A["member"], case["models"], A["rows"], 5, _scored(A, per_gene), limits)
                _same(h.fetch(), want, "pieces %s" % (limits,))
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
        h.set_edit_limits(None, baseedit.Limits(5, 65))
        st, text = status(lambda: h.run(sel.Params(5)))
        assert st == nat.CRP_ERR_STATE and "crp_select_set_coding" in text        # limits without a model
        st, text = status(lambda: h.edit_eval(None, [0], [0]))
        assert st == nat.CRP_ERR_STATE and "crp_select_set_coding" in text        # eval without a model
        for win in ((0, 8), (9, 8), (4, 21)):
            w, lim = nat.SelectEditWindow(*win), nat.SelectEditLimits(0, 100, 20)
            assert L.crp_select_set_edit_limits(h._h, ctypes.byref(w), ctypes.byref(lim)) == nat.CRP_ERR_INVALID
            assert b"window" in L.crp_last_error(h._ctx)
        for lim in ((66, 65, 20), (0, 101, 20)):
            c = nat.SelectEditLimits(*lim)
            assert L.crp_select_set_edit_limits(h._h, None, ctypes.byref(c)) == nat.CRP_ERR_INVALID
            assert b"percentages" in L.crp_last_error(h._ctx)
        h.set_coding(A["model"])
        h.run(sel.Params(5))                                                      # a refused setting changed nothing
        _same(h.fetch(), _reference(scanned, 0, 5, (5, 65, 20)), "after the refusals")
        w = nat.SelectEditWindow(4, 21)
        out = np.zeros(2, np.uint32)
        assert L.crp_select_edit_eval(h._h, ctypes.byref(w), out.ctypes.data_as(nat.u32p), out.ctypes.data_as(nat.u32p), 1, out.ctypes.data_as(nat.u32p),
                                      out.ctypes.data_as(nat.u32p)) == nat.CRP_ERR_INVALID
        n_plus, n_minus = len(A["tables"]["pos_plus"]), len(A["tables"]["pos_minus"])
        for g, packed in ((len(A["lo"]), 0), (0, n_plus), (0, n_minus | 1 << 31), (0xFFFFFFFF, 0)):
            st, text = status(lambda: h.edit_eval(None, [0, g], [0, packed]))
            assert st == nat.CRP_ERR_INVALID and "query 1" in text                # out of range: refused on the host
        st, text = status(lambda: h.run_pairs(sel.Params(5), sel.PairParams(5)))
        assert st == nat.CRP_ERR_UNSUPPORTED and "edit limits" in text            # pairs with edit limits
        h.set_coding_limits(coding.Limits(5, 65))
        st, text = status(lambda: h.run(sel.Params(5)))
        assert st == nat.CRP_ERR_UNSUPPORTED and "coding limits" in text          # both predicates at once
        h.set_edit_limits(None, None)
        h.run(sel.Params(5))                                                      # the coding selection alone runs
        h.set_coding_limits(None)
        h.run_pairs(sel.Params(5), sel.PairParams(5))                             # and without limits the pairs run
        h.set_edit_limits(None, baseedit.Limits(5, 65))
        h.set_coding(None)
        assert status(lambda: h.run(sel.Params(5)))[0] == nat.CRP_ERR_STATE       # model cleared
        assert status(lambda: h.edit_eval(None, [0], [0]))[0] == nat.CRP_ERR_STATE
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
            h.set_edit_limits(None, baseedit.Limits())
            st, text = status(lambda: h.run(sel.Params(5)))
            assert st == nat.CRP_ERR_STATE and "guide length 20" in text
            st, text = status(lambda: h.edit_eval(None, [0], [0]))
            assert st == nat.CRP_ERR_STATE and "guide length 20" in text
        finally:
            h.close()
    finally:
        other.close()


@pytest.mark.gpu
def test_gpu_genome_level_call(engine, case):
    """Genome.scan_score(select=...) with base editing: the Selection's fields against the reference, three arenas."""
    g = engine.genome(case["contigs"], max_words=600)
    try:
        request = annotate.Request(case["annotation"], case["names"], 0)
        A = _view(case, case["contigs"], case["names"], [0] * 4, _host_offsets(case["contigs"]), case["hits"])
        n_plus = len(A["tables"]["pos_plus"])
        for limits, window in ((None, (4, 8)), ((5, 65, 2), (4, 8)), ((0, 100, 20), (1, 20))):
            req = sel.Request(sel.Params(5), request, edit_window=baseedit.Window(*window), edit_limits=None if limits is None else baseedit.Limits(*limits))
            s = g.scan_score(20, select=req).selection
            assert (s.stats["edit_select_ms"] > 0) == (limits is not None) and s.stats["edit_eval_ms"] > 0
            assert s.stats["edit_targets_window"] == window[1] - window[0] + 1
            per_gene = _scored(A, _outcomes(case, A, window))
            n_in, n_pass, picked = eref.select_numpy(A["tables"], A["member"], case["models"], A["rows"], 5, per_gene, limits)
            gene = A["gene"]
            assert np.array_equal(s.n_pass[gene.astype(np.int64)], n_pass) and np.array_equal(s.n_in[gene.astype(np.int64)], n_in)
            r, c = np.nonzero(picked != NONE)
            order = np.lexsort((c, gene[r]))  # the Selection lists the genes in file order
            r, c = r[order], c[order]
            t = np.where(picked[r, c] >> 31 != 0, (picked[r, c] & 0x7FFFFFFF).astype(np.int64) + n_plus, picked[r, c].astype(np.int64))
            want = np.array([[int(v[list(per_gene[gr][0]).index(tr)]) for v in per_gene[gr][1:]] for gr, tr in zip(r.tolist(), t.tolist())], np.uint32)
            assert s.rows.size == r.size and np.array_equal(s.rows["gene"], gene[r]) and np.array_equal(s.rows["rank"], c + 1)
            assert np.array_equal(s.edit_targets, want[:, 0]) and np.array_equal(s.stop_codons, want[:, 1]) and np.array_equal(s.stop_offset, want[:, 2])
            assert np.array_equal(s.cds_length, [case["models"][int(x)]["length"] for x in gene[r]])
            if limits is not None:
                assert (s.stop_offset != NO_STOP).all() and (s.stop_codons >= 1).all() and (s.edit_targets <= limits[2]).all() and s.rows.size > 50
            else:
                assert (s.stop_offset == NO_STOP).any() and (s.stop_offset != NO_STOP).any()
        plain = g.scan_score(20, select=sel.Request(sel.Params(5), request)).selection
        assert plain.edit_targets is None and plain.cds_length is None and "edit_select_ms" not in plain.stats
        # the fields beside a pair selection (no limits): both parts arrive, each what it is alone
        both = g.scan_score(20, select=sel.Request(sel.Params(5), request, edit_window=baseedit.Window(), pairs=sel.PairParams(3))).selection
        pairs_alone = g.scan_score(20, select=sel.Request(sel.Params(5), request, pairs=sel.PairParams(3))).selection
        fields_alone = g.scan_score(20, select=sel.Request(sel.Params(5), request, edit_window=baseedit.Window())).selection
        assert both.pairs.size > 20 and np.array_equal(both.pairs, pairs_alone.pairs) and np.array_equal(both.rows, fields_alone.rows)
        assert np.array_equal(both.stop_offset, fields_alone.stop_offset) and pairs_alone.stop_offset is None
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_command_line_end_to_end(case, tmp_path, monkeypatch):
    out_csv, _ = _run(case, tmp_path, monkeypatch, ["--select", "5", "--select-min-score", "0.2", "--select-stop", "--select-stop-min", "5",
                                                    "--select-stop-max", "65", "--select-max-edit-targets", "2",
                                                    "--bench-json", str(tmp_path / "bench.json")], None)
    got = _read(out_csv + ".selected.csv")
    fields, want_rows, n_pass, label_row = _expected_fields(case, got[1:], (5, 65, 2), 0.2)
    assert got[0][-4:] == baseedit.HEADER and [r[-4:] for r in got[1:]] == fields and len(got) > 10
    assert set((r[0], r[6], r[8], r[10]) for r in got[1:]) == want_rows
    with open(tmp_path / "bench.json") as f:
        stage = json.load(f)["select"]
    assert stage["edit_select_ms"] > 0 and stage["edit_eval_ms"] > 0 and stage["edit_targets_window"] == 5
