"""cropsr_amd/hitcols.py: the one list of per-hit columns, and its users.  The helpers are compared with the expressions the
callers used to spell out per column (arr[a:b], arr[mask], np.concatenate), over the oracle's tables; a column the code has
never heard of must travel through every place that slices, filters or stitches hit tables; the CSV header and the tuple
path's rows are pinned to literals recorded before the list existed; and the native writer must give the tuple path's
bytes for every combination of the opt-in columns."""
import csv
import io
import itertools

import numpy as np
import pytest

from conftest import OracleBackend

from cropsr_amd import cli, hitcols, parallel, rows

STEMS = ("pos", "score", "pre", "ot", "feat", "self_counts", "self_sum", "props")
M = 3
U, US = rows.UNJOINED_COUNT, rows.UNJOINED_SUM


def _text(rng, n, letters=b"ACGTGGCCacgtN"):
    return b"'" + rng.choice(np.frombuffer(letters, dtype=np.uint8), n).tobytes() + b"'),"


def _all_columns(oracle, texts, rng, width=M + 1):
    """The oracle's hits of every text with all eight columns: ot from the oracle's seed scan, the others random, with
    not-a-site and unjoined rows among them."""
    per = [oracle.scan_score(t, 20) for t in texts]
    for h, ot in zip(per, oracle.offtarget_genome(texts, 20)):
        for s in hitcols.STRANDS:
            n = h["pos_" + s].size
            h["ot_" + s] = ot["ot_" + s].reshape(n, 4)
            h["feat_" + s] = rng.integers(0, 9, n).astype(np.uint32)
            h["self_counts_" + s] = rng.integers(0, 5, (n, width)).astype(np.uint32)
            h["self_sum_" + s] = rng.integers(0, 1 << 40, n).astype(np.uint64)
            h["props_" + s] = rng.integers(0, 1 << 32, n).astype(np.uint32)
            h["ot_" + s][::5] = 0xFFFFFFFF
            h["self_counts_" + s][::7], h["self_sum_" + s][::7] = U, US
    return per


@pytest.fixture(scope="module")
def arena(oracle):
    """Three contigs laid out like a device arena (64-aligned, a separator word between them): the second is empty, the
    third has no '-' hit.  dict(texts, offsets, per (hit dicts per contig), table (the arena's columns), cuts)."""
    rng = np.random.default_rng(20)
    texts = [_text(rng, 800), b"", _text(rng, 300, b"AGTGGagtN")]
    per = _all_columns(oracle, texts, rng)
    assert per[0]["pos_minus"].size > 20 and per[0]["pos_plus"].size > 20 and per[1]["pos_plus"].size == 0 and per[2]["pos_plus"].size > 20 and per[2]["pos_minus"].size == 0
    offsets, off = [], 64
    for t in texts:
        offsets.append(off)
        off += ((len(t) + 63) // 64 + 1) * 64
    table, cuts = {}, {}
    for s in hitcols.STRANDS:
        for stem in STEMS:
            key = "%s_%s" % (stem, s)
            table[key] = np.concatenate([h[key] + np.uint32(o) if stem == "pos" else h[key] for h, o in zip(per, offsets)])
        cuts[s] = np.concatenate([[0], np.cumsum([h["pos_" + s].size for h in per])])
    return dict(texts=texts, offsets=offsets, per=per, table=table, cuts=cuts)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all()


def test_the_list_names_the_columns():
    assert tuple(c.stem for c in hitcols.COLUMNS) == STEMS
    assert [c.stem for c in hitcols.COLUMNS if c.always] == ["pos", "score"]
    assert [c.stem for c in hitcols.csv_columns()] == ["ot", "self_counts", "self_sum", "props"]
    assert hitcols.keys(["ot", "feat"]) == ("ot_plus", "ot_minus", "feat_plus", "feat_minus") and len(hitcols.keys()) == 16


def test_helpers_equal_the_expressions_written_out(arena):
    table, cuts, spec = arena["table"], arena["cuts"], {c.stem: c for c in hitcols.COLUMNS}
    rng = np.random.default_rng(21)
    slices = []
    for k, off in enumerate(arena["offsets"]):
        (a, b), (c, d) = cuts["plus"][k:k + 2], cuts["minus"][k:k + 2]
        got = hitcols.take(table, slice(a, b), slice(c, d), origin=off)
        view = hitcols.take(table, slice(a, b), slice(c, d))
        slices.append(got)
        assert set(got) == set(hitcols.keys(STEMS)) == set(view)
        for stem in STEMS:
            for s, (x, y) in zip(hitcols.STRANDS, ((a, b), (c, d))):
                key = "%s_%s" % (stem, s)
                want = table[key][x:y] - np.uint32(off) if stem == "pos" else table[key][x:y]
                assert _same(got[key], want) and _same(got[key], arena["per"][k][key]), (k, key)
                assert _same(view[key], table[key][x:y]) and (view[key].size == 0 or np.shares_memory(view[key], table[key])), (k, key)
                assert got[key].dtype == spec[stem].dtype
                assert got[key].shape[1:] == {"ot": (4,), "self_counts": (M + 1,)}.get(stem, ()), (k, key)  # (0, 4) and (0, M + 1) too
        # rows by mask and by index
        mp, mm = rng.random(b - a) < 0.5, rng.random(d - c) < 0.5
        masked, indexed = hitcols.take(got, mp, mm), hitcols.take(got, np.flatnonzero(mp), np.flatnonzero(mm))
        for key in hitcols.keys(STEMS):
            want = got[key][mp if key.endswith("_plus") else mm]
            assert _same(masked[key], want) and _same(indexed[key], want), (k, key)
    assert slices[1]["ot_plus"].shape == (0, 4) and slices[2]["self_counts_minus"].shape == (0, M + 1)
    # contig after contig is the table again (positions local to their contig)
    whole = hitcols.concat(slices)
    for key in hitcols.keys(STEMS):
        want = np.concatenate([s[key] for s in slices])
        assert _same(whole[key], want), key
        if not key.startswith("pos_"):
            assert _same(whole[key], table[key]), key
    # '+' rows, then '-' rows
    for k, h in enumerate(slices):
        for stem in STEMS:
            want = np.ascontiguousarray(np.concatenate([h[stem + "_plus"], h[stem + "_minus"]]))
            got = hitcols.both(h, stem)
            assert _same(got, want) and got.flags.c_contiguous, (k, stem)
    assert hitcols.both({"pos_plus": table["pos_plus"]}, "ot") is None
    # absent stays absent, None stays None; without parts the always-present columns exist
    part = hitcols.take(dict(pos_plus=table["pos_plus"], pos_minus=table["pos_minus"], pre_plus=None, pre_minus=None), slice(0, 3), slice(0, 0))
    assert set(part) == {"pos_plus", "pos_minus", "pre_plus", "pre_minus"} and part["pre_plus"] is None and part["pos_plus"].size == 3
    empty = hitcols.concat([])
    assert set(empty) == {"pos_plus", "pos_minus", "score_plus", "score_minus"}
    assert empty["pos_plus"].dtype == np.uint32 and empty["score_minus"].dtype == np.float64 and empty["pos_plus"].shape == (0,)


def _zz(pos, strand):
    """The unknown column's value of a hit: a function of its contig position and strand, so that it can be checked row for
    row wherever the row ends up."""
    return np.asarray(pos).astype(np.uint32) * np.uint32(7) + np.uint32(strand == "minus")


def _check_zz(hits, what, shift=0):
    for s in hitcols.STRANDS:
        assert hits["zz_" + s].dtype == np.uint32 and hits["zz_" + s].size == hits["pos_" + s].size, (what, s)
        assert (hits["zz_" + s] == _zz(hits["pos_" + s].astype(np.int64) + shift, s)).all(), (what, s)


def test_an_unknown_column_travels(arena, oracle, monkeypatch):
    from cropsr_amd import engine, node
    monkeypatch.setattr(hitcols, "COLUMNS", hitcols.COLUMNS + [hitcols.Column("zz", np.uint32)])
    table, offsets, texts = arena["table"], arena["offsets"], arena["texts"]
    zz = {"zz_" + s: _zz(table["pos_" + s], s) for s in hitcols.STRANDS}  # (of the ARENA position)
    n_rows = 0
    # engine.Hits over host arrays
    h = engine.Hits(np.array(offsets, np.uint64), np.array([len(t) for t in texts], np.uint64), 20,
                    [table[k] for k in ("pos_plus", "pre_plus", "score_plus", "pos_minus", "pre_minus", "score_minus")])
    assert h.zz_plus is None and "zz_plus" not in h.contig(0)
    h.zz_plus, h.zz_minus = zz["zz_plus"], zz["zz_minus"]
    for k, off in enumerate(offsets):
        got = h.contig(k)
        _check_zz(got, ("Hits", k), off)
        assert (got["pos_plus"] == arena["per"][k]["pos_plus"]).all() and (got["pos_minus"] == arena["per"][k]["pos_minus"]).all()
        n_rows += got["zz_plus"].size + got["zz_minus"].size
        # parallel.slice_piece: the same rows out of an arena's column dict
        _check_zz(parallel.slice_piece(dict(table, **zz), off, len(texts[k])), ("slice_piece", k), off)
    assert n_rows == table["pos_plus"].size + table["pos_minus"].size
    # node.NodeHits: one table, contig after contig, positions local to the contig
    local = hitcols.concat(arena["per"])
    nh = node.NodeHits([(p["pos_plus"].size, p["pos_minus"].size) for p in arena["per"]],
                       [local[k] for k in ("pos_plus", "score_plus", "pos_minus", "score_minus")], 20)
    assert "zz_minus" not in nh.contig(0)
    nh.zz_plus, nh.zz_minus = _zz(local["pos_plus"], "plus"), _zz(local["pos_minus"], "minus")
    for k in range(len(texts)):
        got = nh.contig(k)
        _check_zz(got, ("NodeHits", k))
        assert (got["pos_plus"] == arena["per"][k]["pos_plus"]).all() and (got["pos_minus"] == arena["per"][k]["pos_minus"]).all()
    # parallel.stitch_pieces: a contig cut into three pieces with halos
    rng = np.random.default_rng(22)
    text = _text(rng, 1000)
    pieces = []
    for start, end in ((0, 300), (300, 650), (650, len(text))):
        view, shift = parallel.piece_view(text, start, end)
        ph = oracle.scan_score(view, 20)
        for s in hitcols.STRANDS:
            ph["zz_" + s] = _zz(ph["pos_" + s].astype(np.int64) - shift + start, s)
        pieces.append((start, end, shift, ph))
    assert sum(p[3]["pos_plus"].size for p in pieces) > oracle.scan_score(text, 20)["pos_plus"].size  # (the halos hold hits)
    got, want = parallel.stitch_pieces(pieces), oracle.scan_score(text, 20)
    _check_zz(got, "stitch_pieces")
    for key in want:
        assert _same(got[key], want[key]), key
    # cli.refilter_hits at -l 60, over the scan at the clamped length
    short = _text(rng, 260)
    scan = oracle.scan_score(short, cli.device_guide_length(60))
    for s in hitcols.STRANDS:
        scan["zz_" + s] = _zz(scan["pos_" + s], s)
    got = cli.refilter_hits(scan, len(short), 60)
    _check_zz(got, "refilter_hits")
    want_plus, want_minus = oracle.scan(short, 60)
    assert (got["pos_plus"] == want_plus).all() and (got["pos_minus"] == want_minus).all()
    assert 0 < want_plus.size + want_minus.size < scan["pos_plus"].size + scan["pos_minus"].size  # (the literal filter drops rows)


# rows.extra_header and ContigRows.row of the three rows below for every combination of (offtarget, specificity M, properties),
# as they were before the column list existed: a scored '+' row, an 11-field '+' row that is not a site and unjoined, a '-' row.
ROW_TEXT = "ACGTTGCAAGGCCTTAGGATCCGATTACAGGCCATTGGCACGTAACCGGTTAGCATGGAC"
BASE_ROWS = [("ID0", "cas9", "CUGUAAUCGGAUCCUAAGGC", "AUGGCCUGUAAUCGGAUCCUAAGGCCUUGC", "chr1", 10, 30, 27, "+", 0.25, "", "completed"),
             ("ID1", "cas9", "CCAUGCUAACCGGUUACGUG", "GUCCAUGCUAACCGGUUACGUGCCAAU", "chr1", 38, 58, "+", -1, "", "completed"),
             ("ID2", "cas9", "UUAGGAUCCGAUUACAGGCC", "AGGCCUUAGGAUCCGAUUACAGGCCAUUGG", "chr1", 33, 13, 10, "-", 0.5, "", "completed")]
EXPECTED = {
    (False, None, False): ([], [(), (), ()]),
    (False, None, True): (["guide_gc", "guide_run", "guide_t_run", "guide_stem"], [(10, 2, 3, 4), (0, 0, 0, 0), (20, 3, 2, 1)]),
    (False, 0, False): (["self_mm0", "self_hit_sum", "specificity"], [(1, 12345, 0.999988502955), (-1, -1, -1), (2, 1073741824, 0.5)]),
    (False, 0, True): (["self_mm0", "self_hit_sum", "specificity", "guide_gc", "guide_run", "guide_t_run", "guide_stem"],
                       [(1, 12345, 0.999988502955, 10, 2, 3, 4), (-1, -1, -1, 0, 0, 0, 0), (2, 1073741824, 0.5, 20, 3, 2, 1)]),
    (False, 3, False): (["self_mm0", "self_mm1", "self_mm2", "self_mm3", "self_hit_sum", "specificity"],
                        [(1, 0, 2, 5, 12345, 0.999988502955), (-1, -1, -1, -1, -1, -1), (2, 1, -1, 0, 1073741824, 0.5)]),
    (False, 3, True): (["self_mm0", "self_mm1", "self_mm2", "self_mm3", "self_hit_sum", "specificity", "guide_gc", "guide_run", "guide_t_run",
                        "guide_stem"],
                       [(1, 0, 2, 5, 12345, 0.999988502955, 10, 2, 3, 4), (-1, -1, -1, -1, -1, -1, 0, 0, 0, 0),
                        (2, 1, -1, 0, 1073741824, 0.5, 20, 3, 2, 1)]),
    (True, None, False): (["offtarget_seed_mm0", "offtarget_seed_mm1", "offtarget_seed_mm2", "offtarget_seed_mm3"],
                          [(1, 2, 3, 4), (-1, -1, -1, -1), (0, 0, 7, -1)]),
    (True, None, True): (["offtarget_seed_mm0", "offtarget_seed_mm1", "offtarget_seed_mm2", "offtarget_seed_mm3", "guide_gc", "guide_run",
                          "guide_t_run", "guide_stem"],
                         [(1, 2, 3, 4, 10, 2, 3, 4), (-1, -1, -1, -1, 0, 0, 0, 0), (0, 0, 7, -1, 20, 3, 2, 1)]),
    (True, 0, False): (["offtarget_seed_mm0", "offtarget_seed_mm1", "offtarget_seed_mm2", "offtarget_seed_mm3", "self_mm0", "self_hit_sum",
                        "specificity"],
                       [(1, 2, 3, 4, 1, 12345, 0.999988502955), (-1, -1, -1, -1, -1, -1, -1), (0, 0, 7, -1, 2, 1073741824, 0.5)]),
    (True, 0, True): (["offtarget_seed_mm0", "offtarget_seed_mm1", "offtarget_seed_mm2", "offtarget_seed_mm3", "self_mm0", "self_hit_sum",
                       "specificity", "guide_gc", "guide_run", "guide_t_run", "guide_stem"],
                      [(1, 2, 3, 4, 1, 12345, 0.999988502955, 10, 2, 3, 4), (-1, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0),
                       (0, 0, 7, -1, 2, 1073741824, 0.5, 20, 3, 2, 1)]),
    (True, 3, False): (["offtarget_seed_mm0", "offtarget_seed_mm1", "offtarget_seed_mm2", "offtarget_seed_mm3", "self_mm0", "self_mm1",
                        "self_mm2", "self_mm3", "self_hit_sum", "specificity"],
                       [(1, 2, 3, 4, 1, 0, 2, 5, 12345, 0.999988502955), (-1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
                        (0, 0, 7, -1, 2, 1, -1, 0, 1073741824, 0.5)]),
    (True, 3, True): (["offtarget_seed_mm0", "offtarget_seed_mm1", "offtarget_seed_mm2", "offtarget_seed_mm3", "self_mm0", "self_mm1",
                       "self_mm2", "self_mm3", "self_hit_sum", "specificity", "guide_gc", "guide_run", "guide_t_run", "guide_stem"],
                      [(1, 2, 3, 4, 1, 0, 2, 5, 12345, 0.999988502955, 10, 2, 3, 4), (-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0),
                       (0, 0, 7, -1, 2, 1, -1, 0, 1073741824, 0.5, 20, 3, 2, 1)]),
}
COMBINATIONS = list(itertools.product((False, True), (None, 0, 3), (False, True)))


def _three_rows(ot, mm, props):
    h = dict(pos_plus=np.array([30, 58], np.uint32), score_plus=np.array([0.25, -1.0]), pos_minus=np.array([10], np.uint32),
             score_minus=np.array([0.5]))
    if ot:
        h["ot_plus"], h["ot_minus"] = np.array([[1, 2, 3, 4], [0xFFFFFFFF] * 4], np.uint32), np.array([[0, 0, 7, 0xFFFFFFFF]], np.uint32)
    if mm is not None:
        h["self_counts_plus"] = np.array([[1, 0, 2, 5][:mm + 1], [U] * (mm + 1)], np.uint32)
        h["self_counts_minus"] = np.array([[2, 1, U, 0][:mm + 1]], np.uint32)
        h["self_sum_plus"], h["self_sum_minus"] = np.array([12345, US], np.uint64), np.array([1 << 30], np.uint64)
    if props:
        h["props_plus"], h["props_minus"] = np.array([0x0403020A, 0], np.uint32), np.array([0x01020314], np.uint32)
    return h


@pytest.mark.parametrize("ot,mm,props", COMBINATIONS)
def test_header_and_rows_are_unchanged(ot, mm, props):
    assert set(EXPECTED) == set(COMBINATIONS)
    header, extra = EXPECTED[(ot, mm, props)]
    assert rows.extra_header(ot, mm, props) == header
    assert rows.extra_header(offtarget=ot, specificity=mm, properties=props) == header
    blk = rows.ContigRows(">chr1", ROW_TEXT, _three_rows(ot, mm, props), 20)
    for k in range(3):
        got = blk.row(k, "ID%d" % k)
        assert got == BASE_ROWS[k] + extra[k], k
        assert [type(v) for v in got] == [type(v) for v in BASE_ROWS[k] + extra[k]], k
        assert len(got) == (11 if k == 1 else 12) + len(header)


@pytest.fixture(scope="module")
def two_contigs(oracle):
    rng = np.random.default_rng(23)
    texts = [_text(rng, 2700), _text(rng, 2500)]
    texts[0] = texts[0][:-15] + b"CC" + texts[0][-13:]  # a '-' hit whose long_sequence the end of the string cuts: an 11-field row
    per = {mm: _all_columns(oracle, texts, np.random.default_rng(24), width=(mm or 0) + 1) for mm in (None, 0, 3)}
    assert all(250 <= h["pos_plus"].size + h["pos_minus"].size <= 450 for h in per[3])
    return texts, per


@pytest.mark.parametrize("ot,mm,props", COMBINATIONS)
def test_native_writer_equals_the_tuple_path(two_contigs, oracle, tmp_path, ot, mm, props):
    texts, per = two_contigs
    drop = ([] if ot else ["ot"]) + ([] if mm is not None else ["self_counts", "self_sum"]) + ([] if props else ["props"]) + ["feat", "pre"]
    hits = [{k: v for k, v in h.items() if k not in hitcols.keys(drop)} for h in per[mm]]
    backend = OracleBackend(oracle)
    name = lambda k: ">c%d" % k
    paths = {kind: str(tmp_path / (kind + ".csv")) for kind in ("python", "native")}
    for path in paths.values():
        rows.write_header(path, offtarget=ot, specificity=mm, properties=props)
    np.random.seed(99)
    ds = rows.Dataset()
    for k, (t, h) in enumerate(zip(texts, hits)):
        ds.append(rows.ContigRows(name(k), t.decode("latin-1"), h, 20))
        rows.write_pass(paths["python"], ds, backend.rescore)
    np.random.seed(99)
    passes = []
    for last in range(len(texts)):  # (the dataset is never cleared: pass k holds contigs 0..k)
        nds = rows.NativeDataset(n_threads=3)
        for k in range(last + 1):
            nds.append(rows.ContigTable(name(k), texts[k], hits[k], 20))
        passes.append((nds, rows.draw_ids(len(nds), reverse=True)))
    rows.write_passes_native(paths["native"], passes, backend.rescore)
    a, b = open(paths["python"], "rb").read(), open(paths["native"], "rb").read()
    assert a == b
    table = list(csv.reader(io.StringIO(a.decode("latin-1"), newline="")))
    n_extra = len(rows.extra_header(ot, mm, props))
    assert table[0] == rows.HEADER + rows.extra_header(ot, mm, props) and {len(r) for r in table[1:]} == {11 + n_extra, 12 + n_extra}
    assert len(table) - 1 == len(passes[0][0]) + len(passes[1][0])


@pytest.mark.gpu
def test_gpu_every_column_through_two_arenas(oracle, tmp_path):
    """Three contigs in two arenas, one scan with every opt-in step: each contig's hit dict carries all eight columns,
    bit-equal to its rows of the arena's table, of the joined columns and of hits.properties; and the CSV of those dicts
    is the same through the native writer and the tuple path.  (want_pre, so that `pre` is a column and not None.)"""
    import select_cases
    from cropsr_amd import Engine, annotate
    rng = np.random.default_rng(25)
    texts = [_text(rng, 200, b"AGTGGagtN"), _text(rng, 2000), _text(rng, 5000)]
    names = ["c2", "c1", "c0"]
    gff = tmp_path / "genes.gff"
    gff.write_text(select_cases.build(oracle)["gff"])
    ann = annotate.Annotation(str(gff))
    eng = Engine(0)
    try:
        g = eng.genome(texts, max_words=100)
        assert g.groups == [[0, 1], [2]]
        hits = g.scan_score(20, want_pre=True, offtarget=True, annotation=annotate.Request(ann, names, 0), specificity={}, properties=True)
        dicts = [hits.contig(k) for k in range(3)]
        assert dicts[0]["pos_minus"].size == 0 and dicts[0]["pos_plus"].size > 0  # an empty strand slice
        n_feat = 0
        for k, d in enumerate(dicts):
            a, j = g._where[k]
            whole, off = hits.per_arena[a], int(g.arenas[a].offsets[j])
            assert set(d) == set(hitcols.keys(STEMS)) and all(v is not None for v in d.values())
            for s, col in zip(hitcols.STRANDS, (0, 1)):
                pos = getattr(whole, "pos_" + s)
                lo, hi = np.searchsorted(pos, [off, off + len(texts[k])])
                assert hi - lo == d["pos_" + s].size and _same(d["pos_" + s], pos[lo:hi] - np.uint32(off))
                for stem in ("score", "pre", "ot", "feat", "props"):
                    assert _same(d["%s_%s" % (stem, s)], getattr(whole, "%s_%s" % (stem, s))[lo:hi]), (k, stem, s)
                for stem in ("self_counts", "self_sum"):
                    assert _same(d["%s_%s" % (stem, s)], hits.columns[k]["%s_%s" % (stem, s)]), (k, stem, s)
                assert _same(d["props_" + s], hits.properties[k][col])
                assert d["ot_" + s].shape == (hi - lo, 4) and d["self_counts_" + s].shape == (hi - lo, 4)
                n_feat += int((d["feat_" + s] != annotate.NO_FEATURE).sum())
            want = oracle.scan_score(texts[k], 20)
            assert all(_same(d[key], want[key]) for key in want), k
        assert n_feat > 100
        rescore = lambda seqs, order: eng.score_30mers(seqs, order)[1]
        paths = {kind: str(tmp_path / (kind + ".csv")) for kind in ("python", "native")}
        np.random.seed(5)
        ds = rows.Dataset()
        for k, d in enumerate(dicts):
            ds.append(rows.ContigRows(">" + names[k], texts[k].decode("latin-1"), d, 20, features=(ann.strings, hitcols.both(d, "feat"))))
            rows.write_pass(paths["python"], ds, rescore)
        np.random.seed(5)
        nds = rows.NativeDataset(n_threads=3)
        for k, d in enumerate(dicts):
            nds.append(rows.ContigTable(">" + names[k], texts[k], d, 20, features=(ann.strings, hitcols.both(d, "feat"))))
            rows.write_pass_native(paths["native"], nds, rescore)
        a, b = open(paths["python"], "rb").read(), open(paths["native"], "rb").read()
        assert a == b and a.count(b"\r\n") == 3 * len(ds.blocks[0].short) + 2 * len(ds.blocks[1].short) + len(ds.blocks[2].short)
        g.close()
    finally:
        ann.close()
        eng.close()
