"""--properties: GC, runs, poly-T and hairpin stem per hit (cropsr_amd/properties.py, csrc/crp_properties.hip).  The
definition is restated twice in tests/guide_properties_reference.py; the genomes come from tests/guide_properties_cases.py,
the genes of the selection tests from tests/select_cases.py."""
import csv
import ctypes
import io
import json
import os

import numpy as np
import pytest

from conftest import OracleBackend

import guide_properties_cases as cases
import guide_properties_reference as ref
import select_cases
import select_reference as sref
from cropsr_amd import _native as nat
from cropsr_amd import annotate, cli, properties, rows
from cropsr_amd import search as srch
from cropsr_amd import select as sel

NONE = 0xFFFFFFFF
EVERYTHING = (0, 255, 255, 255, 255)
NOTHING = (21, 255, 255, 255, 255)  # more C and G than a guide of 20 letters has


@pytest.fixture(scope="module")
def genome():
    """The case genome, and per guide length the kept positions and the reference's columns (numpy statement), per contig."""
    texts = cases.contigs()
    cache = {}

    def at(l):
        if l not in cache:
            per = []
            for t in texts:
                plus, minus = cases.kept(t, l)
                per.append(dict(pos_plus=plus, pos_minus=minus, props_plus=ref.column_numpy(t, plus, False, l),
                                props_minus=ref.column_numpy(t, minus, True, l)))
            cache[l] = per
        return cache[l]

    return dict(texts=texts, at=at)


def _w(text):
    return [ref.BASE.get(ch) for ch in text]


# ---------------------------------------------------------------------------------------------- without a GPU
def test_hand_built_windows():
    # the diagonal form of stem: arm GCAT, loop of 3 / 4 / 2
    assert ref.stem_by_definition(_w("GCATAAAATGC")) == ref.stem_by_diagonals(_w("GCATAAAATGC")) == 4
    assert ref.stem_by_definition(_w("GCATAAAAATGC")) == 4
    assert ref.stem_by_definition(_w("GCATAAATGC")) == 3          # loop of 2: the innermost pair does not count
    assert ref.stem_by_definition(_w("GCATATGC")) == 2            # no loop at all: a palindrome, q - p >= 4 leaves two pairs
    assert ref.stem_by_definition(_w("GCATNAAATGC")) == 4 and ref.stem_by_definition(_w("GCNTAAAATGC")) == 2  # (the N ends the stem after two pairs)
    assert ref.stem_by_definition(_w("GGGAAATTT")) == 1            # G-T is no pair (no wobble): only A3-T8 / A4-T8 / A3-T7 alone
    assert ref.stem_by_definition(_w("A")) == ref.stem_by_definition(_w("ATAT")) == 0 and ref.stem_by_definition(_w("ACCCT")) == 1
    for l in (20, 32, 33, 50):
        d = cases.designed(l)
        assert ref.stem_by_definition(_w(d["hairpin"].decode())) == (l - 3) // 2
        assert ref.stem_by_definition(_w(d["hairpin_loop2"].decode())) in ((l - 2) // 2 - 1, (l - 3) // 2)  # never (l - 2) // 2
        if "palindrome" in d:
            assert ref.stem_by_definition(_w(d["palindrome"].decode())) == (l - 4) // 2
            rc = cases.revcomp(d["hairpin"])
            assert ref.stem_by_definition(_w(rc.decode())) == (l - 3) // 2  # unchanged under reverse complement
    # t_run's strand rule: T on '+', A on '-'
    w = _w("TTTTTAACGAAA")
    assert ref.window_loop(w, False) == (2, 5, 5, ref.stem_by_definition(w)) and ref.window_loop(w, True)[2] == 3
    assert ref.window_loop(_w("T" * 20), False)[1:3] == (20, 20) and ref.window_loop(_w("T" * 20), True)[1:3] == (20, 0)
    assert ref.window_loop(_w("A" * 20), True)[2] == 20 and ref.window_loop(_w("A" * 20), False)[2] == 0
    # non-bases end runs; a window without a base
    assert ref.window_loop(_w("GGNGGGRGG"), False)[:2] == (7, 3) and ref.window_loop(_w("NNNN"), False) == (0, 0, 0, 0)
    assert ref.window_loop(_w("TTNTT"), False)[2] == 2
    # lower case, U and Z: case is ignored, U is A, Z and u are no bases
    assert ref.window_loop(_w("ggccAUauT"), False) == (4, 3, 1, 1)  # GGCCAAA.T: run AAA, the one pair A4-T8
    assert ref.window_loop(_w("AUUa"), True)[1:3] == (4, 4) and ref.window_loop(_w("AZA"), False)[1] == 1 and ref.window_loop(_w("AuA"), False)[1] == 1
    # void tails: a '-' window the end of the string cuts, a '+' window is never cut
    text = b"ACGTACGTCCATTTT"
    assert ref.window(text, 8, True, 6) == ["T", "T", "T", "T", None, None] and ref.window(text, 8, False, 4) == ["A", "C", "G", "T"]
    assert ref.column_loop(text, [8], True, 6)[0] == ref.pack((0, 4, 0, 0))
    assert np.array_equal(ref.column_numpy(text, [8], True, 6), ref.column_loop(text, [8], True, 6))
    # the packing, and the command line's percentages as counts
    g = properties.unpack(np.array([ref.pack((11, 3, 2, 4))], np.uint32))
    assert [int(v[0]) for v in g] == [11, 3, 2, 4] and properties.pack(11, 3, 2, 4) == ref.pack((11, 3, 2, 4))
    assert properties.gc_count_bounds(40, 70, 20) == (8, 14) and properties.gc_count_bounds(41, 69, 20) == (9, 13)
    assert properties.gc_count_bounds(33, 67, 33) == (11, 22) and properties.gc_count_bounds(None, None, 20) == (0, 255)
    assert properties.gc_count_bounds(0, 100, 50) == (0, 50) and properties.gc_count_bounds(1, 99, 50) == (1, 49)


def test_diagonal_form_and_numpy_equal_the_definition_on_random_windows():
    rng = np.random.default_rng(8)
    letters = np.frombuffer(b"ACGTACGTACGTacgtNRUuZ", dtype=np.uint8)
    for trial in range(400):
        l = int(rng.integers(1, 51))
        n = int(rng.integers(l + 3, l + 30))
        text = rng.choice(letters[:12] if trial % 3 else letters, n).tobytes()
        if trial % 7 == 0:  # self-complementary stretches: long stems
            half = rng.choice(letters[:4], n // 2).tobytes()
            text = (half + b"AT"[:n % 2] + cases.revcomp(half))[:n]
        minus = bool(trial & 1)
        pos = int(rng.integers(0, n - 2)) if minus else int(rng.integers(l, n))  # '-' windows may run past the end
        w = ref.window(text, pos, minus, l)
        assert ref.stem_by_definition(w) == ref.stem_by_diagonals(w) <= max(0, (l - 3) // 2), (text, pos, minus, l)
        assert ref.column_numpy(text, [pos], minus, l)[0] == ref.pack(ref.window_loop(w, minus)), (text, pos, minus, l)


def test_loop_equals_numpy_on_the_case_genome(genome):
    for l in cases.LENGTHS:
        for t, per in zip(genome["texts"], genome["at"](l)):
            for minus, s in ((False, "plus"), (True, "minus")):
                pos = per["pos_" + s]
                pick = np.unique(np.concatenate([np.arange(0, pos.size, 211 if l > 20 else 97), np.arange(min(12, pos.size)),
                                                 np.arange(max(0, pos.size - 12), pos.size)]))
                assert np.array_equal(ref.column_loop(t, pos[pick], minus, l), per["props_" + s][pick]), (l, s)


def test_the_case_genome_contains_the_cases(genome):
    texts = genome["texts"]
    offsets, off = [], 64
    for t in texts:  # one arena: 64-aligned texts, one separator word between them
        offsets.append(off)
        off += ((len(t) + 63) // 64 + 1) * 64
    for l in cases.LENGTHS:
        per = genome["at"](l)
        bits = {s: set() for s in ("plus", "minus")}
        for t, o, h in zip(texts, offsets, per):
            bits["plus"].update(((h["pos_plus"].astype(np.int64) + o - l) & 63).tolist())
            bits["minus"].update(((h["pos_minus"].astype(np.int64) + o + 3) & 63).tolist())
            cut = h["pos_minus"].astype(np.int64) + 3 + l - len(t)
            assert {k for k in (1, 5, 10) if k <= l} <= set(cut.tolist()) and cut.max() <= 10  # cut by the end of EVERY contig
        for s in bits:  # windows that start at bit 0 (one word), 44 / 45 (the last one-word and the first straddling start at l = 20), 63, 14
            assert {0, 14, 44, 45, 63} <= bits[s]
        assert int(per[0]["pos_plus"][0]) - l == 5
        text0, h0 = texts[0], per[0]
        gc, run, t_run, stem = properties.unpack(h0["props_plus"])
        gcm, runm, t_runm, stemm = properties.unpack(h0["props_minus"])
        for name, w in cases.designed(l).items():
            i = text0.index(w + b"AGG") + l
            r = int(np.searchsorted(h0["pos_plus"], i))
            assert h0["pos_plus"][r] == i, (l, name)
            j = text0.index(b"CCT" + (w if name == "no_base" else cases.revcomp(w)))
            m = int(np.searchsorted(h0["pos_minus"], j))
            assert h0["pos_minus"][m] == j, (l, name)
            if name == "poly_t":    # '+' window all T: l; '-' window all A (its spacer all T): l
                assert (t_run[r], run[r], gc[r]) == (l, l, 0) and t_runm[m] == l
            if name == "poly_a":    # '+' window all A: 0; '-' window all T (its spacer all A): 0
                assert (t_run[r], run[r]) == (0, l) and (t_runm[m], runm[m]) == (0, l)
            if name == "no_base":
                assert h0["props_plus"][r] == 0 and h0["props_minus"][m] == 0
            if name == "hairpin":
                assert stem[r] == stemm[m] == (l - 3) // 2
            if name == "hairpin_loop2":
                assert stem[r] == stemm[m] < (l - 2) // 2
            if name == "palindrome":
                assert stem[r] == stemm[m] == (l - 4) // 2
        # N runs, single IUPAC letters, soft-masked stretches inside windows
        inside = lambda a, b: ((h0["pos_plus"].astype(np.int64) - l < b) & (h0["pos_plus"].astype(np.int64) > a)).any()
        if l >= 20:
            assert inside(10000, 10012) and inside(11200, 11400) and sum(inside(10500 + 37 * k, 10501 + 37 * k) for k in range(13)) >= 5
    for n_rows in cases.TABLE_ROWS:
        for l in cases.LENGTHS:
            plus, minus = cases.kept(cases.exact_table(n_rows), l)
            assert plus.size == n_rows and minus.size == 0


def _hits_with_props(oracle, text, l, rng, with_spec):
    h = oracle.scan_score(text, l)
    h["props_plus"], h["props_minus"] = ref.column_numpy(text, h["pos_plus"], False, l), ref.column_numpy(text, h["pos_minus"], True, l)
    if with_spec:
        for s in ("plus", "minus"):
            n = h["pos_" + s].size
            h["self_counts_" + s] = rng.integers(0, 5, (n, 4)).astype(np.uint32)
            h["self_sum_" + s] = rng.integers(0, 1 << 40, n).astype(np.uint64)
    return h


def _texts(rng):
    acgt = np.frombuffer(b"ACGTACGTACGTacgN", dtype=np.uint8)
    texts = [bytearray(b"'" + rng.choice(acgt, n).tobytes() + b"'),") for n in (1500, 40, 700)]
    texts[0][-15:-13] = b"CC"  # a '-' hit whose long_sequence the end of the string cuts: an 11-field row
    texts[1] = b"ATATATATAT" + b"ATATTATAATATTAATATAT" + b"TGG"  # one hit, its long_sequence cut: a contig of 11-field rows only
    return [bytes(t) for t in texts]


@pytest.mark.parametrize("with_spec", [False, True])
def test_python_and_native_writers_give_the_same_bytes(oracle, tmp_path, with_spec):
    rng = np.random.default_rng(12)
    texts = _texts(rng)
    backend = OracleBackend(oracle)
    blocks = [_hits_with_props(oracle, t, 20, rng, with_spec) for t in texts]
    paths = {}
    for kind in ("python", "native"):
        path = str(tmp_path / (kind + ".csv"))
        rows.write_header(path, specificity=3 if with_spec else None, properties=True)
        np.random.seed(99)
        ds = rows.Dataset() if kind == "python" else rows.NativeDataset(n_threads=3)
        for k, (t, h) in enumerate(zip(texts, blocks)):
            name = "('c%d'," % k
            ds.append(rows.ContigRows(name, t.decode("latin-1"), h, 20) if kind == "python" else rows.ContigTable(name, t, h, 20))
            if kind == "python":
                rows.write_pass(path, ds, backend.rescore)
            else:
                rows.write_pass_native(path, ds, backend.rescore)
        paths[kind] = path
    a, b = open(paths["python"], "rb").read(), open(paths["native"], "rb").read()
    assert a == b
    table = list(csv.reader(io.StringIO(a.decode("latin-1"), newline="")))
    assert table[0] == rows.HEADER + (rows.SPECIFICITY_HEADER(3) if with_spec else []) + properties.HEADER
    assert rows.PROPERTIES_HEADER == properties.HEADER == ["guide_gc", "guide_run", "guide_t_run", "guide_stem"]
    h0 = blocks[0]
    col = np.concatenate([h0["props_plus"], h0["props_minus"]])
    n0, widths = col.size, set()
    for r in range(n0):  # the first pass holds contig 0's rows alone; the fields come last, after the specificity fields
        widths.add(len(table[1 + r]))
        assert table[1 + r][-4:] == [str(int(v[r])) for v in properties.unpack(col)], r
    base = 6 if with_spec else 0
    assert widths == {11 + base + 4, 12 + base + 4}  # the 11-field rows get the columns too
    n1 = blocks[1]["pos_plus"].size + blocks[1]["pos_minus"].size
    assert n1 >= 1 and all(len(table[1 + n0 + n0 + r]) == 11 + base + 4 for r in range(n1))


def test_write_segments_props_with_null_columns_is_write_segments_cols(oracle, tmp_path):
    rng = np.random.default_rng(3)
    texts = _texts(rng)[::2]
    np.random.seed(4)
    ds = rows.NativeDataset(n_threads=2)
    for k, t in enumerate(texts):
        ds.append(rows.ContigTable("('c%d'," % k, t, _hits_with_props(oracle, t, 20, rng, True), 20))
    segs, keep = [], []
    ds.chunk_segments(segs, keep, 0, len(ds), None, 0, OracleBackend(oracle).rescore, ids_rev=rows.draw_ids(len(ds), reverse=True))
    assert len(segs) == 2 and all(getattr(g, "props", None) and getattr(g, "extra", None) is not None for g in segs)
    arr = (nat.RowSegment * 2)(*segs)
    ext = (nat.RowExtra * 2)(*[g.extra for g in segs])
    L_ = nat.lib()
    P = lambda x: ctypes.cast(x, ctypes.c_void_p)

    def write(name, call):
        path = tmp_path / name
        with open(path, "wb") as f:
            n = ctypes.c_uint64()
            nat.check(call(f.fileno(), ctypes.byref(n)), name)
        data = path.read_bytes()
        assert len(data) == n.value > 0
        return data

    for e in (None, P(ext)):
        cols = write("cols", lambda fd, n: L_.crp_write_segments_cols(fd, 20, P(arr), e, 2, n, 2))
        null = write("null", lambda fd, n: L_.crp_write_segments_props(fd, 20, P(arr), e, None, 2, n, 2))
        nulls = (ctypes.c_void_p * 2)(None, None)
        none = write("none", lambda fd, n: L_.crp_write_segments_props(fd, 20, P(arr), e, P(nulls), 2, n, 2))
        assert cols == null == none
    plain = write("plain", lambda fd, n: L_.crp_write_segments(fd, 20, P(arr), 2, n, 2))
    assert plain == write("plain2", lambda fd, n: L_.crp_write_segments_props(fd, 20, P(arr), None, None, 2, n, 2))
    # one segment with the column, one without: the second's bytes are the plain call's
    mixed_ptrs = (ctypes.c_void_p * 2)(segs[0].props, None)
    mixed = write("mixed", lambda fd, n: L_.crp_write_segments_props(fd, 20, P(arr), None, P(mixed_ptrs), 2, n, 2))
    one = (nat.RowSegment * 1)(segs[1])
    tail = write("tail", lambda fd, n: L_.crp_write_segments(fd, 20, P(one), 1, n, 2))
    assert mixed.endswith(tail) and len(mixed) > len(plain)
    with open(tmp_path / "all", "wb") as f:
        assert rows.write_segments(f.fileno(), segs, 20, 2) > len(mixed)


def test_library_declares_the_abi():
    text = open(os.path.join(os.path.dirname(nat.__file__), "..", "include", "cropsr_hip.h")).read()
    assert "#define CRP_ABI_VERSION 6" in text
    for name in ("crp_guide_properties", "crp_guide_properties_stats", "crp_select_set_property_limits", "crp_write_segments_props"):
        assert hasattr(nat.lib(), name) and name in nat.SIGNATURES and name + "(" in text
    assert ctypes.sizeof(nat.SelectPropertyLimits) == 20 and ctypes.sizeof(nat.SelectParams) == 32 and ctypes.sizeof(nat.RowExtra) == 24
    assert "properties" in nat.KINDS


# ---------------------------------------------------------------------------------------------- the selection's reference
@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    """tests/select_cases.py's genome and genes, with the reference's property columns of every contig."""
    c = select_cases.build(oracle)
    d = tmp_path_factory.mktemp("props")
    c["gff_path"] = str(d / "genes.gff")
    with open(c["gff_path"], "w") as f:
        f.write(c["gff"])
    c["fasta_path"] = str(d / "genome.fa")
    with open(c["fasta_path"], "w") as f:  # one line per contig: read unformatted (dec = 0)
        f.write("".join(">%s\n%s\n" % (n, t.decode()) for n, t in zip(c["names"], c["contigs"]))[:-1])
    c["annotation"] = annotate.Annotation(c["gff_path"])
    c["genes"] = sref.gff_genes(c["gff"])
    c["props"] = [dict(props_plus=ref.column_numpy(t, h["pos_plus"], False, 20), props_minus=ref.column_numpy(t, h["pos_minus"], True, 20))
                  for t, h in zip(c["contigs"], c["hits"])]
    return c


def _arena_tables(hits, props, offsets):
    cat = lambda src, key, dt, add: np.concatenate([h[key].astype(dt) + (dt(o) if add else dt(0)) for h, o in zip(src, offsets)])
    tables = dict(pos_plus=cat(hits, "pos_plus", np.uint32, True), score_plus=cat(hits, "score_plus", np.float64, False),
                  pos_minus=cat(hits, "pos_minus", np.uint32, True), score_minus=cat(hits, "score_minus", np.float64, False))
    return tables, dict(props_plus=cat(props, "props_plus", np.uint32, False), props_minus=cat(props, "props_minus", np.uint32, False))


def _host_arena(texts, names, hits, props):
    offsets, off = [], 64
    for t in texts:
        offsets.append(off)
        off += ((len(t) + 63) // 64 + 1) * 64
    tables, cols = _arena_tables(hits, props, offsets)
    return tables, cols, [(n, 0, len(t), o) for n, t, o in zip(names, texts, offsets)], offsets


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("n_in", "n_pass", "sel")):
        assert np.array_equal(np.asarray(g, np.uint32), np.asarray(w, np.uint32)), (what, name)


def test_selection_numpy_statement_equals_the_plain_loop(case):
    tables, cols, entries, _ = _host_arena(case["contigs"], case["names"], case["hits"], case["props"])
    lo, hi, _ = sref.layout(case["genes"], entries, 0)
    pick = np.arange(0, len(lo), 4)
    rng = np.random.default_rng(5)
    cds = {}
    for s in ("plus", "minus"):
        feat = rng.integers(0, 9, len(tables["pos_" + s])).astype(np.uint32)
        feat[rng.random(feat.size) < 0.3] = NONE
        cds["feat_" + s] = feat
    cds["flags"] = (rng.random(9) < 0.5).astype(np.uint8)
    for limits, with_cds in (((8, 14, 255, 3, 4), False), ((0, 12, 3, 255, 255), True), (EVERYTHING, False), (NOTHING, False)):
        args = (tables, lo[pick], hi[pick], 5, 0.3, None, cds if with_cds else None, cols, limits)
        got = ref.select_numpy(*args)
        _same(got, ref.select_loop(*args), str(limits))
        if limits == EVERYTHING:
            _same(got, sref.select_numpy(tables, lo[pick], hi[pick], 5, 0.3))
        if limits == NOTHING:
            assert got[1].sum() == 0 and got[0].sum() > 0
    full = ref.select_numpy(tables, lo, hi, 5, 0.0, None, None, cols, (8, 14, 255, 3, 4))
    plain = sref.select_numpy(tables, lo, hi, 5)
    assert np.array_equal(full[0], plain[0]) and (full[1] <= plain[1]).all() and 0 < full[1].sum() < plain[1].sum()


# ---------------------------------------------------------------------------------------------- the command line
class PropertiesOracleBackend(OracleBackend):
    """OracleBackend plus the `properties` and `select` keywords: the columns by the numpy statement, the selection with
    its property limits by the extended numpy statement over one host arena."""

    def scan(self, strings, l, offtarget=False, annotation=None, specificity=None, select=None, properties=False):
        out = OracleBackend.scan(self, strings, l, offtarget=offtarget, annotation=annotation)
        assert specificity is None  # (the oracle has no self search)
        texts = [bytes(s) for s in strings]
        props = [dict(props_plus=ref.column_numpy(t, h["pos_plus"], False, l), props_minus=ref.column_numpy(t, h["pos_minus"], True, l))
                 for t, h in zip(texts, out)]
        self.ran_properties = bool(properties) or (select is not None and select.property_limits is not None)
        if select is not None:
            tables, cols, _, offsets = _host_arena(texts, list(range(len(texts))), out, props)
            req = select.annotation
            lo, hi, gene = req.gene_layout([(k, o, len(t)) for k, (t, o) in enumerate(zip(texts, offsets))])
            limits = None if select.property_limits is None else select.property_limits.astuple()
            n_in, n_pass, picked = ref.select_numpy(tables, lo, hi, select.params.k, select.params.min_score, None, None, cols, limits)
            part = dict(offsets=np.array(offsets, np.uint64), lengths=np.array([len(t) for t in texts], np.uint64), group=list(range(len(texts))),
                        gene=gene, n_in=n_in, n_pass=n_pass, sel=picked, **tables)
            selection = sel.assemble(req.annotation.genes()[0], select.params.k, [part])
        if properties:
            for h, p in zip(out, props):
                h.update(p)
        if select is not None:
            out = sel.HitList(out)
            out.selection = selection
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


CLI_FLAGS = ["--properties", "--select", "5", "--select-gc-min", "40", "--select-gc-max", "70", "--select-max-t-run", "3", "--select-max-stem", "4"]
CLI_LIMITS = (8, 14, 255, 3, 4)


def _check_cli_output(case, main, got, n_extra=0):
    """main / got: the rows of the main table and of the selection file of a run with CLI_FLAGS, against the reference."""
    assert main[0][-4:] == properties.HEADER and got[0] == ["gene", "rank", "passing"] + main[0][1:]
    tables, cols, entries, _ = _host_arena(case["contigs"], case["names"], case["hits"], case["props"])
    lo, hi, gene = sref.layout(case["genes"], entries, 0)
    n_in, n_pass, picked = ref.select_numpy(tables, lo, hi, 5, 0.0, None, None, cols, CLI_LIMITS)
    # every main row carries the reference's values: rows by (chromosome, end_pos, strand)
    by_key = {(r[4], r[6], r[8] if len(r) == len(main[0]) else r[7]): r for r in main[1:]}  # (an 11-field row has no cutsite field)
    n_checked = 0
    for name, h, p in zip(case["names"], case["hits"], case["props"]):
        for s, sign, end_of in (("plus", "+", 0), ("minus", "-", 3)):
            vals = properties.unpack(p["props_" + s])
            for r in range(0, h["pos_" + s].size, 7):
                row = by_key[(name, str(int(h["pos_" + s][r]) + end_of), sign)]
                assert row[-4:] == [str(int(v[r])) for v in vals]
                n_checked += 1
    assert n_checked > 1000
    # the selection file: the rows the extended reference picks, gene after gene
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
            m = by_key[(case["names"][c], str(end), "-" if minus else "+")]
            want.append((int(g), rank, [case["genes"][int(g)][3], str(rank + 1), str(int(n_pass[row_of_layout]))] + m[1:]))
    want = [w[2] for w in sorted(want, key=lambda w: w[:2])]
    assert len(got) - 1 == len(want) > 100
    for g, w in zip(got[1:], want):
        assert g[:11] == w[:11] and abs(float(g[11]) - float(w[11])) < 1e-15 and g[12:] == w[12:], (g, w)
        gc, run, t_run, stem = (int(v) for v in g[-4:])
        assert 8 <= gc <= 14 and t_run <= 3 and stem <= 4
    assert sref.select_numpy(tables, lo, hi, 5)[1].sum() > n_pass.sum() > 0  # the limits did filter


def test_cli_over_the_oracle(case, oracle, tmp_path, monkeypatch):
    backend = PropertiesOracleBackend(oracle)
    out, _ = _run(case, tmp_path, monkeypatch, CLI_FLAGS + ["--bench-json", str(tmp_path / "b.json")], backend)
    _check_cli_output(case, _read(out), _read(out + ".selected.csv"))
    # the filters alone run the kernel and leave the main table what it was; --properties alone adds the columns only
    plain, plain_stdout = _run(case, tmp_path, monkeypatch, [], OracleBackend(oracle), "plain.csv")
    filt, filt_stdout = _run(case, tmp_path, monkeypatch, CLI_FLAGS[1:], backend, "filt.csv")
    assert backend.ran_properties and open(plain, "rb").read() == open(filt, "rb").read() and plain_stdout == filt_stdout
    assert _read(filt + ".selected.csv")[0] == ["gene", "rank", "passing"] + rows.HEADER[1:]
    assert [r[:-4] for r in _read(out + ".selected.csv")[1:]] == _read(filt + ".selected.csv")[1:]
    cols, _ = _run(case, tmp_path, monkeypatch, ["--properties"], backend, "cols.csv")
    assert [r[:-4] for r in _read(cols)] == _read(plain) and not os.path.exists(cols + ".selected.csv")


def test_cli_default_output_is_unchanged_and_golden(oracle, tmp_path, monkeypatch, manifest):
    """Without the flags the main CSV is byte for byte the golden one (md5_libm)."""
    import hashlib
    from conftest import golden_fasta_path, run_cli
    data, _ = run_cli(tmp_path, monkeypatch, golden_fasta_path("sample", tmp_path), OracleBackend(oracle), manifest["seed"])
    assert hashlib.md5(data).hexdigest() == manifest["cases"]["sample"]["md5_libm"]


REFUSALS = [
    (["--properties", "-l", "0"], "--properties", "1..50"),
    (["--properties", "-l", "51"], "--properties", "1..50"),
    (["--properties", "-l", "-3"], "--properties", "1..50"),
    (["--select-gc-min", "40"], "--select", "belongs to --select"),
    (["--select-gc-max", "70"], "--select", "belongs to --select"),
    (["--select-max-run", "4"], "--select", "belongs to --select"),
    (["--select-max-t-run", "3"], "--select", "belongs to --select"),
    (["--select-max-stem", "4"], "--select", "belongs to --select"),
    (["--properties", "--select-max-stem", "4"], "--select", "belongs to --select"),
    (["--select", "5", "--select-gc-min", "101"], "--select", "0..100"),
    (["--select", "5", "--select-gc-max", "-1"], "--select", "0..100"),
    (["--select", "5", "--select-max-run", "-1"], "--select", "number of letters"),
    (["--properties", "--gpus", "2"], "--properties", "one GPU"),
    (["--properties", "--devices", "0,1"], "--properties", "one GPU"),
    (["--select", "5", "--select-max-t-run", "3", "--gpus", "2"], "--select", "one GPU"),
    (["--select", "5", "--select-gc-min", "40", "--devices", "0,1"], "--select", "one GPU"),
]


@pytest.mark.parametrize("extra,flag,text", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_cli_refusals_come_before_any_side_effect(case, oracle, tmp_path, monkeypatch, extra, flag, text):
    monkeypatch.chdir(tmp_path)
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9", "-g", case["gff_path"]] + extra
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=PropertiesOracleBackend(oracle), out=io.StringIO())
    assert flag in str(e.value.code) and text in str(e.value.code)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra,flag", [(["--properties"], "--properties"), (["--select", "5", "--select-max-stem", "4"], "--select")])
def test_cli_refuses_a_launchers_ranks(case, oracle, tmp_path, monkeypatch, extra, flag):
    class Group:
        world, rank, local_rank = 2, 0, 0
    monkeypatch.chdir(tmp_path)
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9", "-g", case["gff_path"]] + extra
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=PropertiesOracleBackend(oracle), out=io.StringIO(), group=Group())
    assert flag in str(e.value.code) and "2 ranks" in str(e.value.code)
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
@pytest.mark.parametrize("l", cases.LENGTHS)
def test_gpu_columns_equal_the_reference(engine, genome, l, n_arenas):
    g = engine.genome(genome["texts"], max_words=None if n_arenas == 1 else 600)
    try:
        assert len(g.arenas) == n_arenas
        hits = g.scan_score(l, properties=True)
        assert len(hits.properties) == len(genome["texts"]) and g.properties_stats["rows"] == hits.n_plus + hits.n_minus
        for k, want in enumerate(genome["at"](l)):
            got = hits.contig(k)
            for key in ("pos_plus", "pos_minus"):  # (the scan itself is pinned elsewhere; here it is the ground the column stands on)
                assert np.array_equal(got[key], want[key]), (k, key)
            for s, key in enumerate(("props_plus", "props_minus")):
                bad = np.flatnonzero(got[key] != want[key])
                assert bad.size == 0, (k, key, bad[:5], got[key][bad[:5]], want[key][bad[:5]])
                assert hits.properties[k][s] is not None and np.array_equal(hits.properties[k][s], want[key])
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", cases.TABLE_ROWS)
def test_gpu_exact_tables_and_an_empty_strand(engine, n_rows):
    text = cases.exact_table(n_rows)
    arena = engine.arena([text])
    try:
        for l in cases.LENGTHS:
            n_plus, n_minus = arena.scan_score_device(l)
            assert (n_plus, n_minus) == (n_rows, 0)
            pp, pm = arena.guide_properties(n_plus, n_minus)
            pos = arena.fetch(n_plus, n_minus)[0].astype(np.int64) - int(arena.offsets[0])
            assert pm.size == 0 and np.array_equal(pp, ref.column_numpy(text, pos, False, l)), l
            st = arena.guide_properties_stats()
            assert st["rows"] == n_rows and st["guide_len"] == l and st["kernel_ms"] > 0
    finally:
        arena.close()


@pytest.mark.gpu
def test_gpu_calls_out_of_order(engine):
    L = nat.lib()
    text = b"ACGTTGCAAGGCCTTAGGACCA" * 60
    arena = engine.arena([text])
    try:
        def status(fn):
            with pytest.raises(nat.CropsrHipError) as e:
                fn()
            return e.value.status, str(e.value)

        assert status(lambda: arena.guide_properties(0, 0))[0] == nat.CRP_ERR_STATE  # no tables
        assert status(arena.guide_properties_stats)[0] == nat.CRP_ERR_STATE
        n_plus, n_minus = arena.scan_score_device(0)
        st, msg = status(lambda: arena.guide_properties(n_plus, n_minus))
        assert st == nat.CRP_ERR_INVALID and "guide length 0" in msg
        assert L.crp_guide_properties(None, None, None) == nat.CRP_ERR_INVALID
        n_plus, n_minus = arena.scan_score_device(20)
        h = sel.ArenaSelect(arena, [0, 100], [50, 900])
        limits = properties.Limits(gc_min=8, gc_max=14, max_t_run=3)
        h.set_property_limits(limits)
        st, msg = status(lambda: h.run(sel.Params(5)))
        assert st == nat.CRP_ERR_STATE and "crp_guide_properties" in msg  # limits without a column
        assert arena.guide_properties(n_plus, n_minus, fetch=False) is None  # NULL pointers: the column stays on the device
        pp, pm = arena.guide_properties(n_plus, n_minus)
        cols = arena.fetch(n_plus, n_minus)
        off = int(arena.offsets[0])
        assert np.array_equal(pp, ref.column_numpy(text, cols[0].astype(np.int64) - off, False, 20))
        assert np.array_equal(pm, ref.column_numpy(text, cols[3].astype(np.int64) - off, True, 20))
        tables = dict(pos_plus=cols[0], score_plus=cols[2], pos_minus=cols[3], score_minus=cols[5])
        h.run(sel.Params(5))
        _same(h.fetch(), ref.select_numpy(tables, [0, 100], [50, 900], 5, 0.0, None, None, dict(props_plus=pp, props_minus=pm), limits.astuple()))
        assert h.stats()["bytes_per_row"] == 16
        arena.scan_score_device(20)  # a re-scan: the column belongs to the earlier tables
        st, msg = status(lambda: h.run(sel.Params(5)))
        assert st == nat.CRP_ERR_STATE and "crp_guide_properties" in msg
        h.set_property_limits(None)  # cleared: the plain selection again
        h.run(sel.Params(5))
        _same(h.fetch(), sref.select_numpy(tables, [0, 100], [50, 900], 5))
        assert h.stats()["bytes_per_row"] == 12
        h.close()
    finally:
        arena.close()


@pytest.fixture(scope="module", params=[1, 3], ids=["one-arena", "three-arenas"])
def scanned(request, engine, case):
    """select_cases' genome with tables, annotation ids, property column and joined specificity columns resident, and per
    arena the reference's view of the same."""
    g = engine.genome(case["contigs"], max_words=None if request.param == 1 else 600)
    assert len(g.arenas) == request.param
    areq = annotate.Request(case["annotation"], case["names"], 0)
    hits = g.scan_score(20)
    feats = g.annotate(areq, [(h.n_plus, h.n_minus) for h in hits.per_arena])
    dev_props = g.guide_properties([(h.n_plus, h.n_minus) for h in hits.per_arena])
    pattern, gp, M, scheme = srch.check_specificity(20, 3)
    handles = []
    srch._self_handles(g, pattern, gp, srch.SPECIFICITY_PAM_LEN, M, scheme, None, None, handles)
    srch._self_compare_all(handles, M)
    arenas = []
    for a, (arena, group) in enumerate(zip(g.arenas, g.groups)):
        tables, cols = _arena_tables([case["hits"][k] for k in group], [case["props"][k] for k in group], [int(o) for o in arena.offsets])
        for key in tables:
            assert np.array_equal(tables[key].view(np.uint8), getattr(hits.per_arena[a], key).view(np.uint8)), key
        assert np.array_equal(dev_props[a][0], cols["props_plus"]) and np.array_equal(dev_props[a][1], cols["props_minus"])
        entries = [(case["names"][k], 0, int(arena.lengths[j]), int(arena.offsets[j])) for j, k in enumerate(group)]
        lo, hi, gene = sref.layout(case["genes"], entries, 0)
        cp, sp, cm, sm = handles[a].join_hits(20)
        arenas.append(dict(tables=tables, props=cols, lo=lo, hi=hi, gene=gene, spec=dict(counts_plus=cp, sum_plus=sp, counts_minus=cm, sum_minus=sm),
                           cds=dict(feat_plus=feats[a][0], feat_minus=feats[a][1], flags=case["annotation"].cds_flags())))
    yield dict(genome=g, request=areq, handles=handles, arenas=arenas)
    for h in handles:
        h.close()
    g.close()


def _device(s, a, K, slice_rows, limits, min_score=0.0, spec=None, cds=False):
    params = sel.Params(K, min_score, require_cds=cds)
    if spec is not None:
        params.max_mm0, params.max_hit_sum = spec["max_mm0"], spec["max_hit_sum"]
    req = sel.Request(params, s["request"], slice_rows, *limits)
    _, _, _, n_in, n_pass, picked, stats = sel.select_arena(s["genome"], a, req, s["handles"][a] if spec is not None else None)
    return (n_in, n_pass, picked), stats


def _exactly_k(A, K):
    """Limits under which exactly K rows of the arena's largest gene pass, found by search over the reference's columns."""
    plain = sref.select_numpy(A["tables"], A["lo"], A["hi"], 1)
    g = int(plain[0].argmax())
    t = A["tables"]
    vals = []
    for s, back in (("plus", 3), ("minus", 0)):
        cut = t["pos_" + s].astype(np.int64) - back
        inside = (cut >= A["lo"][g]) & (cut <= A["hi"][g]) & (t["score_" + s] != -1.0)
        vals.append(np.stack([v[inside].astype(np.int64) for v in properties.unpack(A["props"]["props_" + s])], axis=1))
    v = np.concatenate(vals)
    if v.shape[0] < K:
        return None, g
    for gc_lo in range(0, 21):
        for gc_hi in range(gc_lo, 21):
            m_gc = (v[:, 0] >= gc_lo) & (v[:, 0] <= gc_hi)
            if m_gc.sum() < K:
                continue
            for max_run in (255, 5, 4, 3, 2):
                for max_t in (255, 3, 2, 1, 0):
                    for max_stem in (255, 5, 4, 3, 2):
                        if int((m_gc & (v[:, 1] <= max_run) & (v[:, 2] <= max_t) & (v[:, 3] <= max_stem)).sum()) == K:
                            return (gc_lo, gc_hi, max_run, max_t, max_stem), g
    return None, g


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
@pytest.mark.parametrize("K", (1, 5, 64))
def test_gpu_selection_with_limits_equals_the_reference(scanned, K, slice_rows):
    s = scanned
    exact = 0
    for a, A in enumerate(s["arenas"]):
        args = (A["tables"], A["lo"], A["hi"], K, 0.0, None, None, A["props"])
        for limits in ((8, 14, 255, 3, 4), (0, 10, 3, 255, 2), NOTHING, EVERYTHING):
            got, stats = _device(s, a, K, slice_rows, limits)
            want = ref.select_numpy(*args, limits)
            _same(got, want, "arena %d %r" % (a, limits))
            assert stats["bytes_per_row"] == 16
            if limits == NOTHING:
                assert (got[1] == 0).all() and (got[2] == NONE).all() and got[0].sum() > 0
            if limits == EVERYTHING:
                _same(got, sref.select_numpy(A["tables"], A["lo"], A["hi"], K))
        limits, g = _exactly_k(A, K)
        if limits is not None:
            got, _ = _device(s, a, K, slice_rows, limits)
            _same(got, ref.select_numpy(*args, limits), "exactly K")
            assert got[1][g] == K and (got[2][g] != NONE).all()
            exact += 1
    assert exact >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
def test_gpu_limits_with_joined_columns_and_cds(scanned, slice_rows):
    s = scanned
    spec = dict(max_mm0=2, max_hit_sum=1 << 34)
    limits = (6, 15, 4, 3, 5)
    total = 0
    for a, A in enumerate(s["arenas"]):
        got, stats = _device(s, a, 5, slice_rows, limits, 0.2, spec, cds=True)
        want = ref.select_numpy(A["tables"], A["lo"], A["hi"], 5, 0.2, dict(A["spec"], **spec), A["cds"], A["props"], limits)
        _same(got, want, "arena %d" % a)
        assert stats["bytes_per_row"] == 32
        without = sref.select_numpy(A["tables"], A["lo"], A["hi"], 5, 0.2, dict(A["spec"], **spec), A["cds"])
        assert (want[1] <= without[1]).all()
        total += int(without[1].sum() - want[1].sum())
    assert total > 0


@pytest.mark.gpu
def test_gpu_genome_level_call_runs_the_kernel_before_the_selection(engine, case):
    g = engine.genome(case["contigs"], max_words=600)
    try:
        areq = annotate.Request(case["annotation"], case["names"], 0)
        req = sel.Request(sel.Params(5, 0.2, max_perfect=0, min_specificity=0.5), areq, None, 8, 14, None, 3, 4)
        hits = g.scan_score(20, specificity=dict(max_mm=3), select=req)  # the limits alone run the kernel; nothing is fetched
        assert hits.properties is None and "props_plus" not in hits.contig(0) and g.properties_stats["rows"] == hits.n_plus + hits.n_minus
        with_cols = g.scan_score(20, specificity=dict(max_mm=3), select=req, properties=True)
        S, T = hits.selection, with_cols.selection
        assert S.rows.tobytes() == T.rows.tobytes() and np.array_equal(S.n_pass, T.n_pass) and 0 < S.n_pass.sum()
        for k in range(len(case["contigs"])):
            assert np.array_equal(with_cols.contig(k)["props_plus"], case["props"][k]["props_plus"])
            assert np.array_equal(with_cols.properties[k][1], case["props"][k]["props_minus"])
        loose = g.scan_score(20, specificity=dict(max_mm=3), select=sel.Request(sel.Params(5, 0.2, max_perfect=0, min_specificity=0.5), areq))
        assert loose.selection.n_pass.sum() > S.n_pass.sum()
        for r in S.rows:  # every selected row keeps the limits
            p = case["props"][int(r["contig"])]["props_plus" if r["strand"] == b"+" else "props_minus"][int(r["index"])]
            assert ref.limits_pass(np.array([p]), (8, 14, 255, 3, 4))[0]
        with pytest.raises(ValueError):
            g.scan_score(0, properties=True)
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_command_line_end_to_end(case, tmp_path, monkeypatch):
    out, _ = _run(case, tmp_path, monkeypatch, CLI_FLAGS + ["--bench-json", str(tmp_path / "bench.json")], None)
    _check_cli_output(case, _read(out), _read(out + ".selected.csv"))
    with open(tmp_path / "bench.json") as f:
        stage = json.load(f)["properties"]
    assert stage["kernel_ms"] > 0 and stage["rows"] == sum(h["pos_plus"].size + h["pos_minus"].size for h in case["hits"])
