"""--specificity: the self search's rows joined onto the guide table (search.specificity_columns, crp_search_self_join_hits,
crp_write_segments_cols; DESIGN.md section 15, CSV join).  Without a GPU: the join in numpy on the oracle's hits and the
CPU references' rows, the two CSV writers byte for byte, the command line's refusals and the whole command line over the
oracle.  On the GPU: the joined columns against that numpy join, exactly, on the small genome of specificity_join_cases
(one arena and several), at 2 * 10^5 hits, and the command line end to end."""
import csv
import ctypes
import io
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, OracleBackend, run_cli

import specificity_join_cases as cases
from cropsr_amd import _native as nat
from cropsr_amd import cli, fasta, rows
from cropsr_amd import search as srch

L = cases.L
SCORES = ["none", "hsu2013", "pair"]


def _ref_score(kind, l=L):
    return {"none": None, "hsu2013": "hsu2013", "pair": cases.pair_table(l)}[kind]


def _lib_score(kind, l=L):
    if kind == "pair":
        pair, offs, pam = cases.pair_table(l)
        return srch.PairTable(pair, offs, pam)
    return _ref_score(kind, l)


@pytest.fixture(scope="module")
def small():
    """The small genome, the oracle's hits of it and, per (M, score), the references' rows: computed once, never changed."""
    from oracle import oracle as orc
    orc.lib()
    contigs, guides = cases.genome()
    hits = [orc.scan_score(c, L) for c in contigs]
    cache = {}

    def table(M, kind):
        if (M, kind) not in cache:
            cache[(M, kind)] = cases.rows(contigs, L, M, "NRG", _ref_score(kind))
        return cache[(M, kind)]

    return dict(contigs=contigs, guides=guides, hits=hits, table=table)


def _same_columns(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for key in ("self_counts_plus", "self_counts_minus", "self_sum_plus", "self_sum_minus"):
            assert g[key].dtype == w[key].dtype and g[key].shape == w[key].shape, (k, key, g[key].shape, w[key].shape)
            assert (g[key] == w[key]).all(), (k, key)


# ------------------------------------------------------------------ the join in numpy (CPU)
def test_small_genome_carries_every_case(small):
    hits, table = small["hits"], small["table"](3, "hsu2013")
    cols = cases.join(hits, table, L, 3)
    W = cases.WHERE

    def row_of(strand, where):
        k, p = where
        at = np.nonzero(hits[k]["pos_" + strand] == p)[0]
        return None if at.size == 0 else (cols[k]["self_counts_" + strand][at[0]], int(cols[k]["self_sum_" + strand][at[0]]))

    def joined(r):
        return r is not None and (r[0] != cases.NO_COUNT).all() and r[1] != cases.NO_SUM

    def sentinel(r):
        return r is not None and (r[0] == cases.NO_COUNT).all() and r[1] == cases.NO_SUM

    assert joined(row_of("plus", W["plus_first_kept"])) and int(hits[0]["pos_plus"][0]) == 25
    assert row_of("plus", W["plus_not_kept"]) is None and (0, 4, 0) in table  # a guide site of the search that owns no row
    n0, n1 = len(small["contigs"][0]), len(small["contigs"][1])
    assert joined(row_of("minus", (0, n0 - 23)))      # the window ends with the contig
    assert sentinel(row_of("minus", (0, n0 - 22)))    # cut by 1: kept by the reference, no site
    assert sentinel(row_of("minus", (1, n1 - 13)))    # cut by 10
    assert int(hits[1]["pos_minus"][-1]) == n1 - 13
    assert sentinel(row_of("plus", W["plus_n_in_guide"])) and sentinel(row_of("minus", W["minus_n_in_guide"]))
    for name in ("plus_straddles_word", "plus_at_word_start"):
        assert joined(row_of("plus", W[name])) and (W[name][1] - L) % 64 in (63, 0)
    for name in ("minus_before_word", "minus_at_word_start"):
        assert joined(row_of("minus", W[name])) and W[name][1] % 64 in (63, 0)
    # the NAG copy is a candidate only, the lower-case gg copy a guide site; neither is a hit, both count for the proper copy
    k, p = W["nag_copy"]
    assert (k, p, 0) not in table and p + L not in hits[k]["pos_plus"].tolist()
    k, p = W["lower_gg_copy"]
    assert (k, p, 0) in table and p + L not in hits[k]["pos_plus"].tolist()
    proper = row_of("plus", W["proper_copy"])
    assert joined(proper) and proper[0][0] >= 5  # g1 exactly: twice on '-' of contig 0, NAG, gg, '-' of contig 2
    without_nag = cases.rows(small["contigs"], L, 3, "NGG", "hsu2013")
    assert without_nag[(1, 500, 0)][0][0] == proper[0][0] - 1
    # planted near copies: rows with hits at 1..3 mismatches, and sums
    n_joined = sum(int((c["self_sum_plus"] != cases.NO_SUM).sum() + (c["self_sum_minus"] != cases.NO_SUM).sum()) for c in cols)
    n_rows = sum(h["pos_plus"].size + h["pos_minus"].size for h in hits)
    assert 500 < n_joined < n_rows
    assert sum(int(c["self_counts_plus"][c["self_sum_plus"] != cases.NO_SUM][:, 1:].sum()) for c in cols) >= 10


def test_fast_join_is_the_join(small):
    for kind in ("none", "hsu2013"):
        table = small["table"](3, kind)
        keys = sorted(table)
        sites = np.array([(k, p, b"-" if s else b"+") for k, p, s in keys], dtype=srch.SELF_SITE_DTYPE)
        counts = np.array([table[key][0] for key in keys], dtype=np.uint32)
        sums = None if kind == "none" else np.array([table[key][1] for key in keys], dtype=np.uint64)
        _same_columns(cases.join_fast(small["hits"], sites, counts, sums, L), cases.join(small["hits"], table, L, 3))


# ------------------------------------------------------------------ the two writers (CPU)
SPECIAL_SUMS = [0, 1, 1 << 30, 1 << 62]


def _synthetic_hits(orc, text, with_ot, rng, M=3):
    """The oracle's hits of `text` with made-up joined columns: joined and unjoined rows mixed, the special sums among them."""
    h = orc.scan_score(text, L)
    for name in ("plus", "minus"):
        n = h["pos_" + name].size
        counts = rng.integers(0, 5000, (n, M + 1)).astype(np.uint32)
        sums = rng.integers(0, 1 << 40, n).astype(np.uint64)
        sums[:len(SPECIAL_SUMS)] = SPECIAL_SUMS[:n]
        un = rng.random(n) < 0.3
        un[:len(SPECIAL_SUMS)] = False
        if n > len(SPECIAL_SUMS):
            un[-1] = True  # (the last '-' row is the contig end's 11-field row)
        counts[un], sums[un] = cases.NO_COUNT, cases.NO_SUM
        h["self_counts_" + name], h["self_sum_" + name] = counts, sums
        if with_ot:
            ot = rng.integers(0, 900, (n, 4)).astype(np.uint32)
            ot[rng.random(n) < 0.2] = 0xFFFFFFFF
            h["ot_" + name] = ot
    return h


@pytest.mark.parametrize("with_ot", [False, True])
def test_python_and_native_writers_give_the_same_bytes(oracle, tmp_path, with_ot):
    rng = np.random.default_rng(12)
    acgt = np.frombuffer(b"ACGTACGTACGTacgN", dtype=np.uint8)
    texts = [bytearray(b"'" + rng.choice(acgt, n).tobytes() + b"'),") for n in (1500, 40, 700)]
    texts[0][-15:-13] = b"CC"  # a '-' hit whose long_sequence the end of the string cuts: an 11-field row
    texts[1] = b"ATATATATAT" + b"ATATTATAATATTAATATAT" + b"TGG"  # one hit, its long_sequence cut: a contig of 11-field rows only
    texts = [bytes(t) for t in texts]
    backend = OracleBackend(oracle)
    blocks = [_synthetic_hits(oracle, t, with_ot, rng) for t in texts]
    assert any(b["pos_plus"].size + b["pos_minus"].size > 0 for b in blocks)
    paths = {}
    for kind in ("python", "native"):
        path = str(tmp_path / (kind + ".csv"))
        rows.write_header(path, offtarget=with_ot, specificity=3)
        np.random.seed(99)
        ds = rows.Dataset() if kind == "python" else rows.NativeDataset(n_threads=3)
        for k, (t, h) in enumerate(zip(texts, blocks)):
            name = "('c%d'," % k
            ds.append(rows.ContigRows(name, t.decode("latin-1"), h, L) if kind == "python" else rows.ContigTable(name, t, h, L))
            if kind == "python":  # a pass per contig, the dataset growing (CROPSR.py:407)
                rows.write_pass(path, ds, backend.rescore)
            else:
                rows.write_pass_native(path, ds, backend.rescore)
        paths[kind] = path
    a, b = open(paths["python"], "rb").read(), open(paths["native"], "rb").read()
    assert a == b
    table = list(csv.reader(io.StringIO(a.decode("latin-1"), newline="")))
    assert table[0] == rows.HEADER + (rows.OFFTARGET_HEADER if with_ot else []) + ["self_mm0", "self_mm1", "self_mm2", "self_mm3",
                                                                                   "self_hit_sum", "specificity"]
    assert rows.SPECIFICITY_HEADER(0) == ["self_mm0", "self_hit_sum", "specificity"]
    # the first pass holds contig 0's rows alone: every added field against the columns
    h0 = blocks[0]
    n_plus, n0 = h0["pos_plus"].size, h0["pos_plus"].size + h0["pos_minus"].size
    widths = set()
    for r in range(n0):
        row = table[1 + r]
        widths.add(len(row))
        assert row[-6:] == cases.expected_fields(h0, n_plus, r), r
        if with_ot:
            name, i = ("plus", r) if r < n_plus else ("minus", r - n_plus)
            assert row[-10:-6] == ["-1" if v == 0xFFFFFFFF else str(v) for v in h0["ot_" + name][i].tolist()]
    base = 4 if with_ot else 0
    assert widths == {11 + base + 6, 12 + base + 6}  # the 11-field rows get the columns too
    first = [table[1 + r][-2:] for r in range(4)]
    assert first == [["0", "1.0"], ["1", repr(1.0 / (1.0 + 2.0 ** -30))], ["1073741824", "0.5"],
                     ["4611686018427387904", repr(1.0 / (1.0 + 2.0 ** 32))]]
    assert any(row[-6:] == ["-1"] * 6 for row in table[1:1 + n0])
    # contig 1: 11-field rows only
    n1 = blocks[1]["pos_plus"].size + blocks[1]["pos_minus"].size
    assert n1 >= 1 and all(len(table[1 + n0 + n0 + r]) == 11 + base + 6 for r in range(n1))


def _segments_of(oracle, texts, rng, with_ot):
    """RowSegment entries (and what keeps their arrays alive) of one chunk over several contigs with joined columns."""
    ds = rows.NativeDataset(n_threads=2)
    for k, t in enumerate(texts):
        ds.append(rows.ContigTable("('c%d'," % k, t, _synthetic_hits(oracle, t, with_ot, rng), L))
    segs, keep = [], []
    ids = rows.draw_ids(len(ds), reverse=True)
    ds.chunk_segments(segs, keep, 0, len(ds), None, 0, OracleBackend(oracle).rescore, ids_rev=ids)
    return segs, keep, ds


def test_write_segments_cols_without_extras_is_write_segments(oracle, tmp_path):
    rng = np.random.default_rng(3)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    texts = [b"'" + rng.choice(acgt, n).tobytes() + b"')," for n in (900, 333)]
    np.random.seed(4)
    segs, keep, ds = _segments_of(oracle, texts, rng, True)
    assert len(segs) == 2 and all(getattr(g, "extra", None) is not None for g in segs)
    arr = (nat.RowSegment * len(segs))(*segs)
    L_ = nat.lib()

    def write(name, call):
        path = tmp_path / name
        with open(path, "wb") as f:
            n = ctypes.c_uint64()
            nat.check(call(f.fileno(), ctypes.byref(n)), name)
        data = path.read_bytes()
        assert len(data) == n.value > 0
        return data

    plain = write("plain", lambda fd, n: L_.crp_write_segments(fd, L, ctypes.cast(arr, ctypes.c_void_p), len(segs), n, 2))
    null = write("null", lambda fd, n: L_.crp_write_segments_cols(fd, L, ctypes.cast(arr, ctypes.c_void_p), None, len(segs), n, 2))
    empty = (nat.RowExtra * len(segs))()  # entries whose self_counts is NULL
    none = write("none", lambda fd, n: L_.crp_write_segments_cols(fd, L, ctypes.cast(arr, ctypes.c_void_p),
                                                                     ctypes.cast(empty, ctypes.c_void_p), len(segs), n, 2))
    assert plain == null == none
    # one segment with the columns, one without: the second's bytes are the plain call's
    mixed_ext = (nat.RowExtra * len(segs))(segs[0].extra, nat.RowExtra())
    mixed = write("mixed", lambda fd, n: L_.crp_write_segments_cols(fd, L, ctypes.cast(arr, ctypes.c_void_p),
                                                                       ctypes.cast(mixed_ext, ctypes.c_void_p), len(segs), n, 2))
    one = (nat.RowSegment * 1)(segs[1])
    tail = write("tail", lambda fd, n: L_.crp_write_segments(fd, L, ctypes.cast(one, ctypes.c_void_p), 1, n, 2))
    assert mixed.endswith(tail) and mixed != plain and len(mixed) > len(plain)
    with open(tmp_path / "all", "wb") as f:
        assert rows.write_segments(f.fileno(), segs, L, 2) > len(mixed)
    bad = (nat.RowExtra * len(segs))(nat.RowExtra(segs[0].extra.self_counts, 0, None), nat.RowExtra())
    with open(tmp_path / "bad", "wb") as f:
        assert L_.crp_write_segments_cols(f.fileno(), L, ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(bad, ctypes.c_void_p), len(segs),
                                          None, 2) == nat.CRP_ERR_INVALID


def test_library_declares_the_join_abi():
    with open(os.path.join(ROOT, "include", "cropsr_hip.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    assert ("int crp_search_self_join_hits(crp_search_self *self, int guide_len, uint32_t *counts_plus, uint64_t *hit_sum_plus, "
            "uint32_t *counts_minus, uint64_t *hit_sum_minus);") in header
    assert ("int crp_search_self_join_device(crp_search_self *self, void **counts_plus, void **hit_sum_plus, void **counts_minus, "
            "void **hit_sum_minus);") in header
    assert ("typedef struct crp_row_extra { const uint32_t *self_counts; int n_counts; const uint64_t *self_hit_sum; } crp_row_extra;"
            in header)
    assert ("int crp_write_segments_cols(int fd, int guide_len, const crp_row_segment *segs, const crp_row_extra *extras, uint64_t n_segs, "
            "uint64_t *bytes_written, int n_threads);") in header
    L_ = nat.lib()
    for name in ("crp_search_self_join_hits", "crp_search_self_join_device", "crp_write_segments_cols"):
        assert hasattr(L_, name) and name in nat.SIGNATURES
    assert nat.SIGNATURES["crp_search_self_join_hits"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, nat.u32p, nat.u64p, nat.u32p,
                                                                          nat.u64p])
    assert L_.crp_abi_version() == 6 == nat.ABI_VERSION
    assert ctypes.sizeof(nat.RowExtra) == 24 and ctypes.sizeof(nat.RowSegment) == 13 * 8


# ------------------------------------------------------------------ the command line (CPU)
class JoinBackend(OracleBackend):
    """The oracle backend plus --specificity by the numpy join of the CPU references."""

    def scan(self, strings, l, offtarget=False, annotation=None, specificity=None):
        out = super().scan(strings, l, offtarget=offtarget, annotation=annotation)
        self.asked = specificity
        if specificity is not None:
            texts = [bytes(s) for s in strings]
            score = specificity["score"]
            if isinstance(score, srch.PairTable):
                score = (np.asarray(score.pair), tuple(score.pam_offsets), score.pam)
            table = cases.rows(texts, l, specificity["max_mm"], specificity["candidate_pam"], score)
            self.columns = cases.join(out, table, l, specificity["max_mm"])
            for h, cols in zip(out, self.columns):
                h.update(cols)
        return out


def _fasta(tmp_path, contigs):
    fa = tmp_path / "small.fa"
    with open(fa, "wb") as f:
        for k, c in enumerate(contigs):
            f.write(b">c%d\n" % k)
            for i in range(0, len(c), 60):
                f.write(c[i:i + 60] + b"\n")
    return str(fa)


def _parse(data):
    return list(csv.reader(io.StringIO(data.decode("latin-1"), newline="")))


def _check_added_fields(table, plain, hits, columns, n_added, first=12):
    """Rows of an --each-contig-once CSV: the first fields are the plain run's, the last n_added the joined columns'."""
    at = 1
    for h, cols in zip(hits, columns):
        n_plus, n = h["pos_plus"].size, h["pos_plus"].size + h["pos_minus"].size
        for r in range(n):
            row, was = table[at + r], plain[at + r]
            assert row[:len(was)] == was and len(row) == len(was) + n_added
            assert row[-n_added:] == cases.expected_fields(cols, n_plus, r)[-n_added:], (at, r)
        at += n
    assert at == len(table) == len(plain)


def test_cli_over_the_oracle(small, oracle, tmp_path, monkeypatch):
    fa = _fasta(tmp_path, small["contigs"])
    seed = 5
    runs = {}
    for name, extra in (("plain", ()), ("native", ("--specificity",)), ("python", ("--specificity", "--csv-writer", "python")),
                        ("ot", ("--specificity", "--offtarget", "--specificity-mismatches", "2", "--specificity-pam", "NGG")),
                        ("ot_plain", ("--offtarget",))):
        d = tmp_path / name
        d.mkdir()
        backend = JoinBackend(oracle)
        data, _ = run_cli(d, monkeypatch, fa, backend, seed, extra=("--each-contig-once",) + extra)
        runs[name] = (data, backend)
    assert runs["native"][0] == runs["python"][0] != runs["plain"][0]
    assert runs["native"][1].asked == dict(max_mm=3, candidate_pam="NRG", score="hsu2013") and runs["plain"][1].asked is None
    plain, table = _parse(runs["plain"][0]), _parse(runs["native"][0])
    assert table[0] == plain[0] + rows.SPECIFICITY_HEADER(3)
    texts = [bytes(v) for _, v in fasta.table_from_bytes(open(fa, "rb").read())]
    hits = [oracle.scan_score(t, L) for t in texts]
    _check_added_fields(table, plain, hits, runs["native"][1].columns, 6)
    # with --offtarget: the off-target fields first, then the join's
    ot, ot_plain = _parse(runs["ot"][0]), _parse(runs["ot_plain"][0])
    assert ot[0] == rows.HEADER + rows.OFFTARGET_HEADER + rows.SPECIFICITY_HEADER(2)
    _check_added_fields(ot, ot_plain, hits, runs["ot"][1].columns, 5)
    # the reference's accumulating passes: both writers, the same bytes
    acc = {}
    for kind in ("native", "python"):
        d = tmp_path / ("acc_" + kind)
        d.mkdir()
        acc[kind], _ = run_cli(d, monkeypatch, fa, JoinBackend(oracle), seed, extra=("--specificity", "--csv-writer", kind))
    assert acc["native"] == acc["python"] and len(acc["native"]) > len(runs["native"][0])


class _NeverBackend:
    def scan(self, *a, **kw):
        raise AssertionError("the run was not refused before the scan")

    rescore = scan


def _refused(tmp_path, monkeypatch, extra, backend=None):
    out = tmp_path / "refused.csv"
    monkeypatch.chdir(tmp_path)
    argv = ["-f", os.path.join(GOLDEN, "probe_multi.fa"), "-g", os.path.join(GOLDEN, "sample_head.gff"), "-o", str(out), "--cas9"] + list(extra)
    args = cli.build_parser().parse_args(argv)
    with pytest.raises(SystemExit) as e:
        cli.run(args, backend=backend or _NeverBackend(), out=io.StringIO())
    assert isinstance(e.value.code, str) and e.value.code.startswith("cropsr_amd: ")
    return e.value.code, out


def test_cli_refusals(tmp_path, monkeypatch):
    w19 = tmp_path / "w19.txt"
    w19.write_text(" ".join(["0.5"] * 19))
    bad = tmp_path / "bad.txt"
    bad.write_text("0.5 x")
    cases_ = [(["--specificity", "-l", "30"], "-l 30"),                                    # l + 3 > 32
              (["--specificity", "-l", "3", "--specificity-weights", str(w19)], "too short"),  # l < M + 1
              (["--specificity", "--specificity-mismatches", "5"], "0..4"),
              (["--specificity", "--specificity-mismatches", "-1"], "0..4"),
              (["--specificity", "-l", "19"], "Hsu 2013"),                                   # hsu2013 needs l = 20
              (["--specificity", "-l", "21"], "Hsu 2013"),
              (["--specificity", "-l", "21", "--specificity-weights", str(w19)], "19 weights"),
              (["--specificity", "--specificity-weights", str(bad)], "weights file"),
              (["--specificity", "--specificity-weights", str(tmp_path / "missing.txt")], "missing.txt"),
              (["--specificity", "--specificity-table", str(bad)], "pair table"),
              (["--specificity", "--specificity-pam", "NAG"], "accepts"),                    # does not contain NGG
              (["--specificity", "--specificity-pam", "NXG"], "letters outside"),
              (["--specificity", "--specificity-pam", "NNGG"], "3 letters"),
              (["--specificity", "--devices", "0,1"], "one GPU"),
              (["--specificity", "--gpus", "2"], "one GPU"),
              (["--specificity", "--specificity-weights", str(w19), "--specificity-table", str(bad)], "give one of them"),
              (["--specificity-mismatches", "2"], "belongs to --specificity"),
              (["--specificity-pam", "NGG"], "belongs to --specificity")]
    for extra, word in cases_:
        msg, out = _refused(tmp_path, monkeypatch, extra)
        assert word in msg, (extra, msg)
        assert not out.exists() and not (tmp_path / "time.txt").exists(), extra
    # --gpus N is refused before any rank is started
    with pytest.raises(SystemExit) as e:
        cli.main(["-f", os.path.join(GOLDEN, "probe_multi.fa"), "-o", str(tmp_path / "r.csv"), "--cas9", "--specificity", "--gpus", "2"])
    assert "one GPU" in str(e.value.code) and not (tmp_path / "r.csv").exists()
    # -l 19 with 19 weights, and -l 29 (T = 32), pass the checks
    for extra in (["-l", "19", "--specificity-weights", str(w19)], ["-l", "29", "--specificity-table", "x"]):
        args = cli.build_parser().parse_args(["-f", "x", "--cas9", "--specificity"] + extra)
        if "x" in extra:
            with pytest.raises(SystemExit) as e:
                cli.specificity_request(args)
            assert "-l 29" not in str(e.value.code) and "x" in str(e.value.code)
        else:
            assert cli.specificity_request(args)["score"] == [0.5] * 19

    # a handle that does not fit the device memory it may take: reported with the bytes it needs
    class Full(_NeverBackend):
        def scan(self, *a, **kw):
            raise srch.SelfCapacityError(123456789, None)

    msg, _ = _refused(tmp_path, monkeypatch, ["--specificity"], backend=Full())
    assert "123456789 bytes" in msg and "--specificity" in msg


def test_specificity_columns_refuses_before_the_genome():
    E = srch.SearchInputError
    for kw in (dict(guide_len=30), dict(guide_len=3, score=[0.5] * 3), dict(guide_len=20, max_mm=5), dict(guide_len=19),
               dict(guide_len=20, candidate_pam="NAG"), dict(guide_len=20, candidate_pam="RG"), dict(guide_len=0)):
        with pytest.raises(E):
            srch.specificity_columns(None, **kw)
    assert srch.check_specificity(20)[:3] == ("N" * 20 + "NRG", "N" * 20 + "NGG", 3)
    assert srch.check_specificity(29, 4, "NGG", None) == ("N" * 29 + "NGG", "N" * 29 + "NGG", 4, None)


# ------------------------------------------------------------------ the library (GPU)
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def _scan(g, contigs, small_hits=None):
    hits = g.scan_score(L)
    got = [hits.contig(k) for k in range(len(contigs))]
    if small_hits is not None:  # the tables the join works on are the oracle's
        for a, b in zip(got, small_hits):
            assert (a["pos_plus"] == b["pos_plus"]).all() and (a["pos_minus"] == b["pos_minus"]).all()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SCORES)
@pytest.mark.parametrize("M", [0, 3, 4])
def test_gpu_join_equals_the_numpy_join(engine, small, M, kind):
    g = engine.genome(small["contigs"])
    try:
        assert len(g.arenas) == 1
        _scan(g, small["contigs"], small["hits"])
        got = g.specificity_columns(L, max_mm=M, score=_lib_score(kind))
        _same_columns(got, cases.join(small["hits"], small["table"](M, kind), L, M))
        assert got.stats["join_ms"] > 0
        if kind == "none":
            assert all((c["self_sum_plus"] == cases.NO_SUM).all() and (c["self_sum_minus"] == cases.NO_SUM).all() for c in got)
        # through scan_score: the columns travel with the contig's rows
        h = g.scan_score(L, specificity=dict(max_mm=M, score=_lib_score(kind))).contig(1)
        assert (h["self_counts_minus"] == got[1]["self_counts_minus"]).all() and (h["self_sum_plus"] == got[1]["self_sum_plus"]).all()
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_join_does_not_depend_on_the_cut(engine, small):
    one = engine.genome(small["contigs"])
    many = engine.genome(small["contigs"], max_words=50)
    try:
        assert len(one.arenas) == 1 and len(many.arenas) == 3
        for kind, M in (("hsu2013", 3), ("pair", 4), ("none", 3)):
            want = cases.join(small["hits"], small["table"](M, kind), L, M)
            for g in (one, many):
                _scan(g, small["contigs"], small["hits"])
                _same_columns(g.specificity_columns(L, max_mm=M, score=_lib_score(kind)), want)
    finally:
        one.close()
        many.close()


@pytest.mark.gpu
def test_gpu_join_abi(engine, small):
    """The C ABI's refusals and states, the device columns and the ninth stats value."""
    Lb = nat.lib()
    g = engine.genome(small["contigs"])
    h23 = h22 = h5 = None
    try:
        a = g.arenas[0]
        h23 = srch.ArenaSelfSearch(a, "N" * 20 + "NRG", "N" * 20 + "NGG", 3, 3)
        h22 = srch.ArenaSelfSearch(a, "N" * 19 + "NRG", "N" * 19 + "NGG", 3, 3)
        h5 = srch.ArenaSelfSearch(a, "TTTV" + "N" * 19, "TTTV" + "N" * 19, 4, 3)
        p = [ctypes.c_void_p() for _ in range(4)]
        assert Lb.crp_search_self_join_device(h23._h, *[ctypes.byref(x) for x in p]) == nat.CRP_ERR_STATE
        ctx = engine._ctx

        def refused(h, l, word):
            st = Lb.crp_search_self_join_hits(h._h, l, None, None, None, None)
            assert st == nat.CRP_ERR_INVALID and word in Lb.crp_last_error(ctx).decode(), (l, Lb.crp_last_error(ctx))

        refused(h23, 20, "no hit tables")      # nothing scanned yet
        a.scan_score_device(19)
        refused(h23, 20, "no hit tables")      # tables of another guide length
        refused(h23, 19, "guide_len + 3")
        refused(h5, 20, "PAM")
        n_plus, n_minus = a.scan_score_device(20)
        refused(h22, 20, "guide_len + 3")
        refused(h22, 19, "no hit tables")
        srch._self_compare_all([h23], 3)
        cp, sp, cm, sm = h23.join_hits(20)     # unscored: counts only
        want = cases.join(small["hits"], small["table"](3, "none"), L, 3)
        assert (cp == np.concatenate([w["self_counts_plus"] for w in want])).all()
        assert (cm == np.concatenate([w["self_counts_minus"] for w in want])).all()
        assert (sp == cases.NO_SUM).all() and (sm == cases.NO_SUM).all() and cp.shape == (n_plus, 4)
        dev = h23.join_device()
        assert all(dev) and len(set(dev)) == 4
        assert h23.join_hits(20, fetch=False) is None and h23.join_device() == dev  # (the columns are kept, not reallocated)
        out = np.zeros(10, dtype=np.float64)
        assert Lb.crp_search_self_stats(h23._h, out.ctypes.data_as(nat.f64p), 9) == nat.CRP_OK and out[8] > 0 and out[9] == 0
        eight = np.zeros(9, dtype=np.float64)
        assert Lb.crp_search_self_stats(h23._h, eight.ctypes.data_as(nat.f64p), 8) == nat.CRP_OK and eight[8] == 0 and eight[2] == out[2]
        assert Lb.crp_search_self_stats(h23._h, out.ctypes.data_as(nat.f64p), 10) == nat.CRP_ERR_INVALID
        a.scan_score_device(20)                 # a new scan: the same join again, the same columns
        again = h23.join_hits(20)
        assert (again[0] == cp).all() and (again[2] == cm).all()
    finally:
        for h in (h23, h22, h5):
            if h is not None:
                h.close()
        g.close()


@pytest.mark.gpu
def test_gpu_join_of_two_hundred_thousand_hits(engine):
    """A 2.4 Mb genome with a second copy carrying substitutions: the joined columns against the numpy join of the engine's
    own hits with search_self's own rows -- the look-up across many workgroups."""
    rng = np.random.default_rng(78)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    first = rng.choice(acgt, 1_200_000)
    second = first.copy()
    at = np.nonzero(rng.random(second.size) < 0.03)[0]
    second[at] = rng.choice(acgt, at.size)
    n_run = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), 30_001)
    contigs = [first.tobytes(), second.tobytes(), n_run.tobytes()]
    g = engine.genome(contigs)
    try:
        res = g.search_self("N" * 20 + "NRG", 3, 3, guide_pattern="N" * 20 + "NGG", score="hsu2013")
        hits = _scan(g, contigs)
        n_hits = sum(h["pos_plus"].size + h["pos_minus"].size for h in hits)
        assert n_hits > 200_000
        got = g.specificity_columns(L, max_mm=3, score="hsu2013")
        want = cases.join_fast(hits, res.sites, res.counts, res.hit_sum, L)
        _same_columns(got, want)
        joined = sum(int((w["self_sum_plus"] != cases.NO_SUM).sum() + (w["self_sum_minus"] != cases.NO_SUM).sum()) for w in want)
        assert n_hits - 20_000 < joined < n_hits  # the N contig's and the contig ends' hits are the unjoined ones
        assert sum(int(w["self_counts_plus"][w["self_sum_plus"] != cases.NO_SUM][:, 1:].sum()) for w in want) > 5000
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_cli_end_to_end(small, oracle, tmp_path, monkeypatch):
    fa = _fasta(tmp_path, small["contigs"])
    gff = tmp_path / "small.gff"
    gff.write_text("##gff-version 3\nc0\tt\tgene\t100\t2000\t.\t+\t.\tID=g1\nc1\tt\tgene\t50\t900\t.\t-\t.\tID=g2\n"
                   "c1\tt\tCDS\t400\t700\t.\t-\t0\tID=g2.cds\n")
    seed = 5
    texts = [bytes(v) for _, v in fasta.table_from_bytes(open(fa, "rb").read())]
    hits = [oracle.scan_score(t, L) for t in texts]
    want3 = cases.join(hits, cases.rows(texts, L, 3, "NRG", "hsu2013"), L, 3)

    def run(name, extra):
        d = tmp_path / name
        d.mkdir()
        return run_cli(d, monkeypatch, fa, None, seed, extra=("-g", str(gff), "--each-contig-once") + tuple(extra))[0]

    plain = run("plain", ())
    native = run("native", ("--specificity",))
    python = run("python", ("--specificity", "--csv-writer", "python"))
    assert native == python
    p, t = _parse(plain), _parse(native)
    assert t[0] == p[0] + rows.SPECIFICITY_HEADER(3) and all(len(r) in (11, 12) for r in p[1:])
    _check_added_fields(t, p, hits, want3, 6)  # the first 12 (or 11) fields are the plain run's, byte for byte
    assert [",".join(r) for r in p] == [",".join(r[:len(q)]) for r, q in zip(t, p)]
    # the union of the opt-in columns, in the documented order: features inside the row, off-target, then the join's
    pair, offs, pam = cases.pair_table(L)
    tab = tmp_path / "table.txt"
    lines = ["pam-offsets 1 2"] + ["pam %s%s %r" % ("ACGT"[i // 4], "ACGT"[i % 4], float(v)) for i, v in enumerate(pam)]
    lines += ["pair %d %s %s %r" % (gq, "ACGT"[a], "ACGT"[b], float(pair[gq, a, b])) for gq in range(L) for a in range(4) for b in range(4) if a != b]
    tab.write_text("\n".join(lines) + "\n")
    both_plain = run("both_plain", ("--offtarget", "--annotate"))
    both = run("both", ("--specificity", "--offtarget", "--annotate", "--specificity-mismatches", "4", "--specificity-table", str(tab)))
    bp, bt = _parse(both_plain), _parse(both)
    assert bt[0] == rows.HEADER + rows.OFFTARGET_HEADER + rows.SPECIFICITY_HEADER(4)
    want4 = cases.join(hits, cases.rows(texts, L, 4, "NRG", (pair, offs, pam)), L, 4)
    _check_added_fields(bt, bp, hits, want4, 7)
    assert any(r[10] for r in bt[1:] if len(r) == 12 + 4 + 7)  # annotated rows among them
    assert python != plain
