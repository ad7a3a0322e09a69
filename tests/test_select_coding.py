"""--coding / --select-coding-*: where in the coding sequence a guide cuts (cropsr_amd/coding.py).
Without a GPU: the two restatements against each other, the native model and layout against them on a GFF zoo, the limits,
the command line over an oracle backend, crp_coding.h under sanitizers.  On the GPU: the selection with coding limits and
the evaluation kernel against the reference, exactly."""
import csv
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import OracleBackend

import select_coding_cases as cases
import select_coding_reference as cref
import select_reference as sref
import select_scale_cases as scale
from cropsr_amd import _native as nat
from cropsr_amd import annotate, cli, coding
from cropsr_amd import select as sel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
KS = (1, 5, 64)
ZOO_ENTRIES = [("s", 0, 400, 64), ("other", 0, 300, 576), ("s", 25, 100, 1024), ("nowhere", 0, 50, 1280), ("s", 130, 0, 1400)]


@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    c = cases.build(oracle)
    d = tmp_path_factory.mktemp("select_coding")
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


@pytest.fixture(scope="module")
def zoo(tmp_path_factory):
    d = tmp_path_factory.mktemp("coding_zoo")
    out = {}
    for name, text in cases.ZOO.items():
        path = str(d / (name + ".gff"))
        with open(path, "w") as f:
            f.write(text)
        out[name] = path
    return out


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
    return _arena_tables(case["hits"], offsets), entries


def _same_model(a, b, what):
    assert len(a) == len(b), what
    for g, (x, y) in enumerate(zip(a, b)):
        for key in ("strand", "model", "n_tx", "length", "primary"):
            assert x[key] == y[key], (what, g, key)
        for s, (start, end) in zip(x["transcripts"], y["transcripts"]):  # (x: sets of coordinates, y: merged segments)
            assert s == set(p for a0, b0 in zip(start.tolist(), end.tolist()) for p in range(a0, b0 + 1)), (what, g)


# ---------------------------------------------------------------------------------------------- without a GPU
@pytest.mark.parametrize("name", sorted(cases.ZOO))
def test_numpy_statement_equals_the_plain_loop_on_the_zoo(name):
    text = cases.ZOO[name]
    loop, vec = cref.model_loop(text), cref.model_numpy(text)
    _same_model(loop, vec, name)
    for dec in (0, 1):
        for row in cref.layout_rows(text, ZOO_ENTRIES, dec):
            c = np.arange(max(row[2] - 3, 0), row[3] + 5)
            off, cover = cref.position_numpy(vec[row[0]], row, c)
            want = [cref.position_loop(loop[row[0]], row, int(x)) for x in c]
            assert off.tolist() == [w[0] for w in want] and cover.tolist() == [w[1] for w in want], (name, dec, row)


def test_the_zoo_contains_what_it_is_for():
    m = {name: cref.model_loop(text) for name, text in cases.ZOO.items()}
    assert [g["n_tx"] for g in m["comma_parent"]] == [2, 1] and m["comma_parent"][0]["length"] == 21 + 111
    assert m["child_before_parent"][0]["length"] == 21 + 31 and m["child_before_parent"][0]["strand"] == "-"
    assert m["cds_off_the_gene"][0]["n_tx"] == 1 and m["implicit_and_explicit"][0]["n_tx"] == 3
    assert m["implicit_and_explicit"][0]["primary"] == 0  # three of one length: the mRNA row before the gene row wins
    assert [g["model"] for g in m["duplicate_ids"]] == [True, False] and m["duplicate_ids"][0]["n_tx"] == 2
    assert m["mrna_on_another_seqid"][0]["n_tx"] == 1 and m["mrna_on_another_seqid"][0]["length"] == 31
    assert m["transcript_type"][0]["length"] == 21
    assert [g["model"] for g in m["strand_dot"]] == [False] * 3
    assert [g["n_tx"] for g in m["transcript_without_cds"]] == [1, 0]
    assert m["overlapping_and_duplicate_cds"][0]["length"] == 41 + 9 and len(m["overlapping_and_duplicate_cds"][0]["transcripts"][0]) == 50
    assert [g["length"] for g in m["short_cds"]] == [3, 1]
    assert [g["model"] for g in m["start_after_end"]] == [True, False, True] and m["start_after_end"][0]["length"] == 31
    assert [(g["n_tx"], g["primary"]) for g in m["tie"]] == [(2, 0), (2, 0)]
    assert m["outside_gene_and_contig"][0]["length"] == 121 + 521
    assert [g["model"] for g in m["empty_values"]] == [False, False, True] and m["empty_values"][2]["length"] == 21 + 11
    assert m["odd_lines"][0]["length"] == 21  # the one CDS line that is whole and names its parent


@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("name", sorted(cases.ZOO))
def test_native_model_and_layout_equal_the_restatement(zoo, name, dec):
    text = cases.ZOO[name]
    an = annotate.Annotation(zoo[name])
    ref = cref.model_loop(text)
    strand, n_tx, length = an.gene_coding()
    assert [s.decode() for s in strand] == [g["strand"] for g in ref]
    assert n_tx.tolist() == [g["n_tx"] for g in ref] and length.tolist() == [g["length"] for g in ref]
    # the existing views do not see the new rows
    assert an.n_genes == len(ref) and an.n_cds == sum(1 for r in cref.gff_rows(text) if r[0] == "CDS")
    assert set(an.seq_index) == set(r[1] for r in cref.gff_rows(text) if r[0] in ("gene", "CDS"))
    lo, hi, gene = an.gene_layout(ZOO_ENTRIES, dec)
    model = an.coding_layout(ZOO_ENTRIES, dec)
    rows = cref.layout_rows(text, ZOO_ENTRIES, dec)
    want_lo, want_hi, want_gene = sref.layout(sref.gff_genes(text), ZOO_ENTRIES, dec)
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi) and np.array_equal(gene, want_gene)
    assert [r[0] for r in rows] == gene.tolist() and model["info"].size == len(rows)  # exactly gene_layout's rows
    assert model["first"][0] == 0 and model["first"][-1] == model["at"].size and (np.diff(model["first"].astype(np.int64)) >= 0).all()
    for r, row in enumerate(rows):
        m = ref[row[0]]
        assert int(model["info"][r]) == ((m["n_tx"] | (m["strand"] == "-") << 16 | 1 << 17) if m["model"] else 0), (name, r)
        assert int(model["length"][r]) == m["length"]
        a, b = int(model["first"][r]), int(model["first"][r + 1])
        at, word = model["at"][a:b].astype(np.int64), model["word"][a:b]
        assert (np.diff(at) > 0).all() and (np.diff(word.astype(np.int64)) != 0).all() and (b == a or word[-1] == 0)
        # every change point is an a, an a + 1 or a b + 1 of a merged segment, clipped to the text
        allowed = set()
        for T in cref.model_numpy(text)[row[0]]["transcripts"] if m["model"] else []:
            for s, e in zip((T[0] + row[1]).tolist(), (T[1] + row[1]).tolist()):
                s, e = max(s, row[2]), min(e, row[3])
                if s <= e:
                    allowed.update((s, s + 1, e + 1))
        assert set(at.tolist()) <= allowed, (name, r)
        c = np.arange(max(row[2] - 3, 0), row[3] + 5)
        off, cover = cref.steps_position(model, r, c)
        want = [cref.position_loop(m, row, int(x)) for x in c]
        assert off.tolist() == [w[0] for w in want] and cover.tolist() == [w[1] for w in want], (name, dec, r)
    an.close()


def test_a_piece_that_begins_inside_an_exon_starts_with_the_right_count(zoo):
    an = annotate.Annotation(zoo["plain"])
    model = an.coding_layout([("s", 25, 100, 1024)], 0)  # the text's first letter is coordinate 26, the 7th of the exon 20..40
    assert model["at"][0] == 1024 and model["cum"][0] == 6 and model["word"][0] == 1 << 17  # s[c] is coding, the cut is not inside
    assert model["at"][1] == 1025 and model["cum"][1] == 7 and model["word"][1] == (1 | 1 << 16 | 1 << 17)
    an.close()


def test_native_layout_capacity_protocol(zoo):
    an = annotate.Annotation(zoo["plain"])
    e = an._entries(ZOO_ENTRIES)
    L = nat.lib()
    n, m = ctypes.c_uint64(), ctypes.c_uint64()
    args = (an._h, e.ctypes.data_as(nat.u64p), e.shape[0], 0)
    assert L.crp_annotation_coding_layout(*args, None, None, None, 0, ctypes.byref(n), None, None, None, 0, ctypes.byref(m)) == nat.CRP_ERR_CAPACITY
    rows, steps = n.value, m.value
    assert rows == 2 and steps == 9 + 6  # the whole contig: three exons; the piece: two, the first one clipped
    info, length, first = np.zeros(rows, np.uint32), np.zeros(rows, np.uint32), np.zeros(rows, np.uint64)
    at, word, cum = (np.full(steps, 7, np.uint32) for _ in range(3))
    p32 = lambda x: x.ctypes.data_as(nat.u32p)
    st = L.crp_annotation_coding_layout(*args, p32(info), p32(length), first.ctypes.data_as(nat.u64p), rows, ctypes.byref(n), p32(at), p32(word),
                                        p32(cum), steps - 4, ctypes.byref(m))
    assert st == nat.CRP_ERR_CAPACITY and (n.value, m.value) == (rows, steps) and (at[steps - 4:] == 7).all()
    st = L.crp_annotation_coding_layout(*args, p32(info), p32(length), first.ctypes.data_as(nat.u64p), rows, ctypes.byref(n), p32(at), p32(word),
                                        p32(cum), steps, ctypes.byref(m))
    assert st == nat.CRP_OK and first.tolist() == [0, 9]
    assert L.crp_annotation_coding_layout(*args, None, None, None, 0, None, None, None, None, 0, ctypes.byref(m)) == nat.CRP_ERR_INVALID
    bad = e.copy()
    bad[1, 3] = 10  # texts out of order
    assert L.crp_annotation_coding_layout(an._h, bad.ctypes.data_as(nat.u64p), bad.shape[0], 0, None, None, None, 0, ctypes.byref(n), None, None,
                                          None, 0, ctypes.byref(m)) == nat.CRP_ERR_INVALID
    an.close()


def test_limits_are_checked():
    assert coding.Limits().astuple() == (0, 100, 0) and coding.Limits(5, 65, 50).astuple() == (5, 65, 50)
    for bad in (dict(min_pct=-1), dict(max_pct=101), dict(min_transcripts_pct=101), dict(min_pct=66, max_pct=65), dict(min_pct=1.5),
                dict(max_pct=True), dict(min_transcripts_pct=-3)):
        with pytest.raises(ValueError):
            coding.Limits(**bad)
    # exact integers: 100 off against pct L near 2^32
    lim = coding.Limits(50, 50, 0)
    got = lim.passes([True, True, True, False], [2147483600, 2147483601, coding.NOT_INSIDE, 2147483600], [1] * 4, [4294967200] * 4, [1] * 4)
    assert got.tolist() == [True, False, False, False]
    assert coding.Limits(0, 100, 50).passes([True, True], [5, 5], [1, 2], [10, 10], [3, 3]).tolist() == [False, True]
    assert [coding.percent(o, l) for o, l in ((1, 3), (1, 2000), (1999, 2000), (130, 200), (1, 8))] == ["33.3", "0.1", "100.0", "65.0", "12.5"]
    assert coding.fields(coding.NOT_INSIDE, 200, 0, 2) == ("", "", "", 0, 2) and coding.fields(130, 200, 1, 2) == (130, 200, "65.0", 1, 2)
    with pytest.raises(ValueError):
        sel.Request(sel.Params(1), None, coding_limits=coding.Limits(), pairs=sel.PairParams(1))


def test_selection_statements_agree_on_the_case_genome(case):
    """select_numpy against select_loop over the 80 kb genome, and the case genome holds what it was built for."""
    tables, entries = _host_arena(case)
    lo, hi, gene = sref.layout(case["genes"], entries, 0)
    rows = cref.layout_rows(case["gff"], entries, 0)
    loop_models = cref.model_loop(case["gff"])
    _same_model(loop_models, case["models"], "case")
    for K, limits in ((5, None), (5, (5, 65, 0)), (1, (0, 100, 100)), (64, (0, 0, 0))):
        got = cref.select_numpy(tables, lo, hi, case["models"], rows, K, limits)
        want = cref.select_loop(tables, lo, hi, loop_models, rows, K, limits)
        for g, w, name in zip(got, want, ("n_in", "n_pass", "sel")):
            assert np.array_equal(g, w), (K, limits, name)
        assert got[1].any() == (limits != (0, 0, 0))


def test_a_tiled_model_holds_the_base_rows(case):
    """select_scale_cases.tile_model over the case genome's host layout: every tiled row is its base row -- info, length,
    the step slices, and the (off, cover) they give --, and first is a running sum.  Twice: the list of the GPU test, more
    than 2^20 genes over the rows of few steps, and a short list over all rows, those of 129 and 257 steps among them."""
    tables, entries = _host_arena(case)
    request = annotate.Request(case["annotation"], case["names"], 0)
    model = request.coding_layout([(k, e[3], e[2]) for k, e in enumerate(entries)])
    base_first = model["first"].astype(np.int64)
    n_rows = model["info"].size
    lo, hi, _ = sref.layout(case["genes"], entries, 0)
    total = scale.rows_in(tables, lo.astype(np.int64), hi.astype(np.int64))
    few = scale.few_steps(model)
    assert n_rows == len(lo) and 10 < len(few) < n_rows and np.diff(base_first).max() >= 129 and (np.diff(base_first)[few] == 0).any()
    rng = np.random.default_rng(20)
    pos = np.concatenate([tables["pos_plus"].astype(np.int64) - 3, tables["pos_minus"].astype(np.int64) + 6])
    c = pos[rng.choice(pos.size, 64, replace=False)]  # the cut boundaries of 64 sampled table rows
    off = np.concatenate([cref.steps_position(model, b, c)[0] for b in few])
    assert (off != cref.NOT_INSIDE).any() and (off == cref.NOT_INSIDE).any()
    for base, n_genes in ((few, scale.G), (list(range(n_rows)), 5 * n_rows + 3)):
        start = scale.boundary_start(total, base, 64, n_genes) if n_genes == scale.G else 3
        ids = scale.tiling(base, n_genes, start)
        tiled = scale.tile_model(model, ids)
        print("tiled model: %d rows, %d steps, %.1f MB" % (ids.size, tiled["at"].size, sum(v.nbytes for v in tiled.values()) / 1e6))
        first = tiled["first"].astype(np.int64)
        assert first.size == n_genes + 1 and first[0] == 0 and first[-1] == tiled["at"].size == tiled["word"].size == tiled["cum"].size
        assert (np.diff(first) >= 0).all() and np.array_equal(np.diff(first), np.diff(base_first)[ids])
        assert np.array_equal(tiled["info"], model["info"][ids]) and np.array_equal(tiled["length"], model["length"][ids])
        assert tiled["first"].dtype == np.uint64 and all(tiled[key].dtype == model[key].dtype for key in ("info", "length", "at", "word", "cum"))
        # the step slices, by plain slicing: every base row at the list's start, on both sides of 2^20 and at its end
        n = len(base)
        where = set(range(min(2 * n, n_genes))) | set(range(n_genes - 2 * n, n_genes))
        if n_genes > scale.MAX_ITEMS:
            where |= set(range(scale.MAX_ITEMS - n, scale.MAX_ITEMS + n))
        seen = set()
        for g in sorted(where):
            b = int(ids[g])
            for key in ("at", "word", "cum"):
                assert np.array_equal(tiled[key][first[g]:first[g + 1]], model[key][base_first[b]:base_first[b + 1]]), (g, key)
            if (b, g > scale.MAX_ITEMS) not in seen:  # (the step function itself: once per base row and side of 2^20)
                seen.add((b, g > scale.MAX_ITEMS))
                got, want = cref.steps_position(tiled, g, c), cref.steps_position(model, b, c)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), g
        assert len(seen) == (2 if n_genes > scale.MAX_ITEMS else 1) * n
    # the list of the GPU test reaches a second launch, and at slices of 64 a cut gene lies across every launch boundary
    assert total[few].max() > 64
    ids = scale.tiling(few, scale.G, scale.boundary_start(total, few, 64))
    cut = scale.host_cut(total[ids], 64)
    assert cut["items"] > scale.G > scale.MAX_ITEMS and 0 < cut["cut_genes"] and scale.straddles(total[ids], 64)


def test_coding_driver_under_sanitizers(zoo, tmp_path):
    """tests/native/coding_driver.cpp: crp_coding.h over hand-made step functions against a brute-force count (L_P and off
    near 2^32), then the model builder and the layout over the zoo, its prefixes and garbage, under ASan + UBSan."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "coding_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "cropsr_amd", "csrc"), os.path.join(ROOT, "tests", "native", "coding_driver.cpp"),
           os.path.join(ROOT, "cropsr_amd", "csrc", "crp_annotation.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe] + [zoo[name] for name in sorted(zoo)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout + run.stderr


# ---------------------------------------------------------------------------------------------- on the GPU
LIMITS = ((5, 65, 0), (0, 100, 0), (0, 100, 100), (0, 100, 51), (0, 0, 0), (40, 60, 0), (65, 100, 50))


@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def _scanned(engine, case, max_words):
    """A genome with its tables, annotation ids and property column resident, and per arena the reference's view of the
    same: tables from the oracle's hits, genes by the restated layout, the coding position of every table row for every
    gene row (computed once and shared)."""
    from cropsr_amd import properties
    g = engine.genome(case["contigs"], max_words=max_words)
    request = annotate.Request(case["annotation"], case["names"], 0)
    hits = g.scan_score(20)
    counts = [(h.n_plus, h.n_minus) for h in hits.per_arena]
    feats = g.annotate(request, counts)
    props = g.guide_properties(counts)
    flags = case["annotation"].cds_flags()
    arenas = []
    for a, (arena, group) in enumerate(zip(g.arenas, g.groups)):
        tables = _arena_tables([case["hits"][k] for k in group], [int(o) for o in arena.offsets])
        got = hits.per_arena[a]
        for key in tables:  # (the scan itself is pinned elsewhere; here it is the ground the selection stands on)
            assert np.array_equal(tables[key].view(np.uint8), getattr(got, key).view(np.uint8)), key
        entries = [(case["names"][k], 0, int(arena.lengths[j]), int(arena.offsets[j])) for j, k in enumerate(group)]
        lo, hi, gene = sref.layout(case["genes"], entries, 0)
        rows = cref.layout_rows(case["gff"], entries, 0)
        model = request.coding_layout(sel.arena_layout(g, a))
        got_lo, got_hi, got_gene = request.gene_layout(sel.arena_layout(g, a))
        assert np.array_equal(got_lo, lo) and np.array_equal(got_hi, hi) and np.array_equal(got_gene, gene)
        ids = np.concatenate([feats[a][0], feats[a][1]]).astype(np.int64)
        packed = np.concatenate([props[a][0], props[a][1]])
        arenas.append(dict(tables=tables, lo=lo, hi=hi, gene=gene, rows=rows, model=model, ids=[case["ids"][int(x)] for x in gene],
                           positions=cref.positions_numpy(tables, case["models"], rows), member=cref.membership(tables, lo, hi),
                           score=np.concatenate([tables["score_plus"], tables["score_minus"]]), flags=flags,
                           ok_cds=(ids != NONE) & (np.concatenate([flags, [0]])[np.where(ids == NONE, flags.size, ids)] != 0),
                           ok_props=lambda lim, packed=packed: properties.Limits(**lim).passes(packed)))
    return dict(genome=g, request=request, arenas=arenas, cache={}, models=case["models"])


@pytest.fixture(scope="module", params=[1, 3], ids=["one-arena", "three-arenas"])
def scanned(request, engine, case):
    s = _scanned(engine, case, None if request.param == 1 else 600)
    assert len(s["genome"].arenas) == request.param
    yield s
    s["genome"].close()


def _ok(A, min_score=0.0, cds=False, props=None):
    ok = A["score"] >= np.float64(min_score)
    if cds:
        ok = ok & A["ok_cds"]
    if props is not None:
        ok = ok & A["ok_props"](props)
    return ok


def _reference(s, a, K, limits, min_score=0.0, cds=False, props=None):
    key = (a, K, limits, min_score, cds, None if props is None else tuple(sorted(props.items())))
    if key not in s["cache"]:
        A = s["arenas"][a]
        s["cache"][key] = cref.select_numpy(A["tables"], A["lo"], A["hi"], s["models"], A["rows"], K, limits, _ok(A, min_score, cds, props),
                                            positions=A["positions"])
    return s["cache"][key]


def _device(s, a, K, slice_rows, limits, min_score=0.0, cds=False, props=None):
    from cropsr_amd import properties
    A = s["arenas"][a]
    h = sel.ArenaSelect(s["genome"].arenas[a], A["lo"], A["hi"])
    try:
        if cds:
            h.set_flags(A["flags"])
        if slice_rows:
            h.set_limits(slice_rows)
        if props is not None:
            h.set_property_limits(properties.Limits(**props))
        h.set_coding(A["model"])
        h.set_coding_limits(None if limits is None else coding.Limits(*limits))
        h.run(sel.Params(K, min_score, require_cds=cds))
        return h.fetch(), h.stats(), h.coding_stats()
    finally:
        h.close()


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("n_in", "n_pass", "sel")):
        print(what, name, "differing genes:", int((np.asarray(g) != np.asarray(w)).reshape(len(g), -1).any(axis=1).sum()))
        assert np.array_equal(np.asarray(g, np.uint32), np.asarray(w, np.uint32)), (what, name)


def _gene_view(s, ident):
    """(arena dict, layout row) of a case gene."""
    for A in s["arenas"]:
        if ident in A["ids"]:
            return A, A["ids"].index(ident)
    raise AssertionError("no gene " + ident)


def _segments(s, A, r):
    """Arena letters (first, last) of the merged segments of the primary transcript of layout row r."""
    m = s["models"][A["rows"][r][0]]
    start, end = m["transcripts"][m["primary"]]
    return start + A["rows"][r][1], end + A["rows"][r][1]


def _boundaries(A):
    t = A["tables"]
    return np.concatenate([t["pos_plus"].astype(np.int64) - 3, t["pos_minus"].astype(np.int64) + 6])


@pytest.mark.gpu
def test_gpu_the_genome_contains_the_cases(scanned, case):
    """Every class of row the kernels can get wrong is present ON THE REFERENCE'S ROWS; nothing here looks at the device."""
    s = scanned
    inside_of = lambda A, r: A["member"][r] & (A["positions"][0][r] != cref.NOT_INSIDE)
    outside_of = lambda A, r: A["member"][r] & (A["positions"][0][r] == cref.NOT_INSIDE)
    # '+' and '-' genes with a cut at an exon's first letter, one letter in, at its last letter and one past it
    for ident, minus in (("edges_plus", False), ("edges_minus", True)):
        A, r = _gene_view(s, ident)
        assert bool(A["model"]["info"][r] >> 16 & 1) == minus
        a, b = _segments(s, A, r)
        c = _boundaries(A)[A["member"][r]]
        for name, edge in (("a", a), ("a + 1", a + 1), ("b", b), ("b + 1", b + 1)):
            assert np.isin(edge, c).any(), (ident, name)
        off = A["positions"][0][r][A["member"][r]]
        assert (off[np.isin(c, a)] == cref.NOT_INSIDE).all() and (off[np.isin(c, b + 1)] == cref.NOT_INSIDE).all()  # on an edge: not inside
        assert (off[np.isin(c, a + 1)] != cref.NOT_INSIDE).all() and (off[np.isin(c, b)] != cref.NOT_INSIDE).all()
    # one, three and many exons with rows inside and rows in the introns (or the flanks)
    for ident in ("one_exon", "three_exons", "steps129", "shared_first", "tie", "outer", "nested", "antisense", "clipped_left", "past_end"):
        A, r = _gene_view(s, ident)
        assert inside_of(A, r).any() and outside_of(A, r).any(), ident
    A, r = _gene_view(s, "three_exons")
    a, b = _segments(s, A, r)
    c = _boundaries(A)
    assert (A["member"][r] & (c > b[0] + 1) & (c < a[1])).any()  # a row in the first intron
    # two transcripts sharing only their first exon: rows in both, in the primary alone, in the other alone
    A, r = _gene_view(s, "shared_first")
    off, cover = A["positions"][0][r][A["member"][r]], A["positions"][1][r][A["member"][r]]
    assert ((cover == 2) & (off != cref.NOT_INSIDE)).any() and ((cover == 1) & (off != cref.NOT_INSIDE)).any()
    assert ((cover == 1) & (off == cref.NOT_INSIDE)).any() and (cover == 0).any()
    m = s["models"][A["rows"][r][0]]
    assert m["n_tx"] == 2 and m["primary"] == 1 and m["length"] == 151 + 301
    # the tie: equal lengths, the earlier row is primary although its CDS rows come later
    A, r = _gene_view(s, "tie")
    m = s["models"][A["rows"][r][0]]
    assert m["n_tx"] == 2 and m["primary"] == 0 and len(m["transcripts"][0][0]) == 2 and m["length"] == 200
    # nested and antisense genes: rows shared with `outer`, with other answers
    A, r_outer = _gene_view(s, "outer")
    r_nested, r_anti = A["ids"].index("nested"), A["ids"].index("antisense")
    both = inside_of(A, r_outer) & inside_of(A, r_anti)
    assert both.any() and (A["positions"][0][r_outer][both] != A["positions"][0][r_anti][both]).all()
    assert (inside_of(A, r_nested) & outside_of(A, r_outer)).any() and (outside_of(A, r_anti) & inside_of(A, r_outer)).any()
    # no model: rows, and nothing to be inside of
    for ident in ("no_cds", "no_strand"):
        A, r = _gene_view(s, ident)
        assert A["member"][r].sum() > 5 and A["model"]["info"][r] == 0 and A["model"]["first"][r] == A["model"]["first"][r + 1]
    # clipped at the text's start: the letter before the text counts; past the contig's end: the letters beyond count
    A, r = _gene_view(s, "clipped_left")
    at = np.flatnonzero(inside_of(A, r))
    assert (A["positions"][0][r][at] == _boundaries(A)[at] - A["rows"][r][2] + 1).all()
    A, r = _gene_view(s, "past_end")
    assert s["models"][A["rows"][r][0]]["length"] == 201 + 451 and (A["positions"][0][r][inside_of(A, r)] > 301).all()
    # the step counts
    steps = np.concatenate([np.diff(A["model"]["first"].astype(np.int64)) for A in s["arenas"]])
    assert set(cases.STEP_COUNTS) <= set(steps.tolist()), sorted(set(steps.tolist()))
    # limits hit with equality
    for ident, pct in (("exact_min", 5), ("exact_max", 65), ("exact_min_minus", 5), ("exact_max_minus", 65)):
        A, r = _gene_view(s, ident)
        off = A["positions"][0][r][inside_of(A, r)].astype(np.int64)
        assert A["model"]["length"][r] == 200 and (100 * off == pct * 200).any(), ident
        assert ((100 * off < 5 * 200) | (100 * off > 65 * 200)).any(), ident  # and rows that (5, 65) turns away
    # runs that the slices of 64 cut, and genes with more than K rows
    assert max(int(A["member"].sum(axis=1).max()) for A in s["arenas"]) > 3 * 64


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
@pytest.mark.parametrize("K", KS)
def test_gpu_selection_equals_the_reference(scanned, K, slice_rows):
    for a in range(len(scanned["arenas"])):
        for limits in LIMITS:
            want = _reference(scanned, a, K, limits)
            plain = _reference(scanned, a, K, None)
            if limits == (0, 0, 0):
                assert not want[1].any() and plain[1].any()  # limits that pass nothing
            elif len(scanned["arenas"]) == 1:
                assert want[1].any() and (want[1] < plain[1]).any(), limits
            got, stats, cstats = _device(scanned, a, K, slice_rows, limits)
            _same(got, want, "arena %d K %d limits %s" % (a, K, limits))
            assert cstats["coding_steps"] == scanned["arenas"][a]["model"]["at"].size and cstats["coding_select_ms"] > 0
            if slice_rows == 64 and len(scanned["arenas"]) == 1:
                assert stats["merged_genes"] > 0
        # the model without limits: the plain selection, by the plain kernel
        got, _, cstats = _device(scanned, a, K, slice_rows, None)
        _same(got, _reference(scanned, a, K, None), "arena %d K %d no limits" % (a, K))
        assert cstats["coding_select_ms"] == 0


@pytest.mark.gpu
def test_gpu_more_genes_than_one_launch(engine, case):
    """The coding kernel behind the driver's launch loop (crp_select_run hands every launch `d_items + first`): the arena's
    genes of few steps tiled to more than 2^20 (tests/select_scale_cases.py), with the tiled model, under limits that pass a
    row and fail a row of some gene.  At the default slices the second launch begins at gene 2^20; at slices of 64 a cut
    gene's pieces lie on both sides of every launch boundary (the list begins where boundary_start says, for both slicings).
    n_in, n_pass and sel whole, against the reference taken through the tiling."""
    s = _scanned(engine, case, None)
    try:
        A, K, limits = s["arenas"][0], 5, (5, 65, 0)
        want, plain = _reference(s, 0, K, limits), _reference(s, 0, K, None)
        base = scale.few_steps(A["model"])
        assert ((0 < want[1][base]) & (want[1][base] < plain[1][base])).any()  # the limits pass a row and fail a row of some gene
        total = scale.rows_in(A["tables"], A["lo"].astype(np.int64), A["hi"].astype(np.int64))
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
                h.set_coding_limits(coding.Limits(*limits))
                h.run(sel.Params(K))
                got, stats, cstats = h.fetch(), h.stats(), h.coding_stats()
            finally:
                h.close()
            _same(got, [np.asarray(w)[ids] for w in want], "slices %r" % slice_rows)
            assert stats["items"] == cut["items"] and stats["launches"] == -(-cut["items"] // scale.MAX_ITEMS) >= 2
            assert stats["merged_genes"] == cut["cut_genes"] and cstats["coding_select_ms"] > 0
            if slice_rows is None:
                assert stats["items"] == scale.G and stats["launches"] == 2
            else:
                assert stats["items"] > scale.G and cut["cut_genes"] > 0
    finally:
        s["genome"].close()


@pytest.mark.gpu
def test_gpu_limits_that_pass_exactly_k_and_equality(scanned):
    K = 5
    found = 0
    for a, A in enumerate(scanned["arenas"]):
        for limits in ((5, 65, 0), (5, 5, 0), (65, 65, 0), (5, 64, 0), (6, 65, 0), (0, 5, 0)):
            want = _reference(scanned, a, K, limits)
            found += int((want[1] == K).sum())
            got, _, _ = _device(scanned, a, K, 64, limits)
            _same(got, want, "arena %d limits %s" % (a, limits))
        # equality keeps the row: with (5, 5) resp. (65, 65) exactly the rows with 100 off = pct L_P pass
        for ident, limits in (("exact_min", (5, 5, 0)), ("exact_max", (65, 65, 0)), ("exact_min_minus", (5, 5, 0)), ("exact_max_minus", (65, 65, 0))):
            if ident in A["ids"]:
                r = A["ids"].index(ident)
                assert _reference(scanned, a, K, limits)[1][r] >= 1
                wider = _reference(scanned, a, K, (5, 65, 0))[1][r]
                assert _reference(scanned, a, K, (6, 65, 0) if limits[0] == 5 else (5, 64, 0))[1][r] < wider
    assert found > 0  # some gene has exactly K passing rows under one of these limits


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
def test_gpu_combined_with_the_other_limits(scanned, slice_rows):
    props = dict(gc_min=8, gc_max=13, max_run=4, max_t_run=3, max_stem=4)
    for a, A in enumerate(scanned["arenas"]):
        for more in (dict(min_score=0.3), dict(cds=True), dict(props=props), dict(min_score=0.2, cds=True, props=props)):
            want = _reference(scanned, a, 5, (5, 65, 0), **more)
            alone, without = _reference(scanned, a, 5, (5, 65, 0)), _reference(scanned, a, 5, None, **more)
            if len(scanned["arenas"]) == 1:  # each of the two halves of the predicate takes rows away
                assert want[1].any() and (want[1] < alone[1]).any() and (want[1] < without[1]).any(), more
            got, _, _ = _device(scanned, a, 5, slice_rows, (5, 65, 0), **more)
            _same(got, want, "arena %d %s" % (a, more))


@pytest.mark.gpu
def test_gpu_eval_of_every_gene_row_pair(scanned):
    """off and cover of the evaluation kernel for EVERY (gene, row in the gene) pair, exactly; it needs no limits and no run."""
    offs, covers = [], []
    for a, A in enumerate(scanned["arenas"]):
        g, t = np.nonzero(A["member"])
        n_plus = len(A["tables"]["pos_plus"])
        packed = np.where(t < n_plus, t, (t - n_plus) | (1 << 31)).astype(np.uint32)
        h = sel.ArenaSelect(scanned["genome"].arenas[a], A["lo"], A["hi"])
        try:
            h.set_coding(A["model"])
            off, cover = h.coding_eval(g.astype(np.uint32), packed)
            assert g.size > 100 and h.coding_stats()["coding_eval_ms"] > 0
            print("arena", a, "pairs", g.size, "off differs:", int((off != A["positions"][0][g, t]).sum()), "cover differs:",
                  int((cover != A["positions"][1][g, t]).sum()))
            assert np.array_equal(off, A["positions"][0][g, t]) and np.array_equal(cover, A["positions"][1][g, t])
            assert h.coding_eval([], [])[0].size == 0
            offs.append(off)
            covers.append(cover)
        finally:
            h.close()
    off, cover = np.concatenate(offs), np.concatenate(covers)
    assert off.size > 2000 and (off != cref.NOT_INSIDE).sum() > 500 and (off == cref.NOT_INSIDE).sum() > 500 and cover.max() == 2


def _pieces(case):
    """Three texts that are PIECES of contigs, each beginning inside an exon: 20 letters into the first exon of edges_plus
    (c0) and of edges_minus (c1), and 300 letters into the second exon of `outer` (c0), which the antisense gene overlaps.
    Returns (texts, entries without arena offsets: (name, start, length))."""
    first_exon = lambda ident: int(case["models"][case["ids"].index(ident)]["transcripts"][0][0][0]) - 1  # (dec = 0: index = coordinate - 1)
    cuts = (("c0", first_exon("edges_plus") + 20, 4000), ("c1", first_exon("edges_minus") + 20, 3000), ("c0", 15800, 1400))
    texts = [case["contigs"][case["names"].index(n)][a:a + ln] for n, a, ln in cuts]
    return texts, cuts


@pytest.mark.gpu
def test_gpu_genes_clipped_by_the_start_of_a_piece(engine, case, oracle):
    """Texts that begin inside an exon: the row's steps open at the text's first letter with cum > 0, grow on and the cut not
    inside.  sel, n_in, n_pass of the selection and off, cover of every (gene, row) pair, exactly."""
    texts, cuts = _pieces(case)
    arena = engine.arena(texts)
    try:
        n_plus, n_minus = arena.scan_score_device(20)
        offsets = [int(o) for o in arena.offsets]
        entries = [(n, a, ln, o) for (n, a, ln), o in zip(cuts, offsets)]
        tables = _arena_tables([oracle.scan_score(t, 20) for t in texts], offsets)
        cols = arena.fetch(n_plus, n_minus)
        for key, got in zip(("pos_plus", "score_plus", "pos_minus", "score_minus"), (cols[0], cols[2], cols[3], cols[5])):
            assert np.array_equal(tables[key].view(np.uint8), got.view(np.uint8)), key  # (the ground the selection stands on)
        lo, hi, gene = case["annotation"].gene_layout(entries, 0)
        want_lo, want_hi, want_gene = sref.layout(case["genes"], entries, 0)
        assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi) and np.array_equal(gene, want_gene)
        rows = cref.layout_rows(case["gff"], entries, 0)
        model = case["annotation"].coding_layout(entries, 0)
        ids = [case["ids"][int(g)] for g in gene]
        positions, member = cref.positions_numpy(tables, case["models"], rows), cref.membership(tables, lo, hi)
        c = np.concatenate([tables["pos_plus"].astype(np.int64) - 3, tables["pos_minus"].astype(np.int64) + 6])
        # non-vacuous, on the reference's rows: each clipped gene opens with the right count, and rows cut inside the clipped exon
        for ident, base, cum0 in (("edges_plus", offsets[0], 20), ("edges_minus", offsets[1], 20), ("outer", offsets[2], 501 + 300)):
            r = ids.index(ident)
            k = int(model["first"][r])
            assert model["at"][k] == base and model["cum"][k] == cum0 and model["word"][k] == 1 << 17, ident  # grow, not inside
            L = int(model["length"][r])
            seg_end = int(model["at"][k + 2])  # a, a + 1, b + 1 of the clipped exon
            inside = np.flatnonzero(member[r] & (c > base) & (c < seg_end))
            assert inside.size >= 3, ident
            before = cum0 + (c[inside] - base)
            assert np.array_equal(positions[0][r][inside], L - before if ident == "edges_minus" else before), ident
            assert not (member[r] & (c == base)).any() or (positions[0][r][member[r] & (c == base)] == cref.NOT_INSIDE).all()
        assert "antisense" in ids and (member[ids.index("antisense")] & member[ids.index("outer")]).any()
        h = sel.ArenaSelect(arena, lo, hi)
        try:
            h.set_coding(model)
            g, t = np.nonzero(member)
            packed = np.where(t < n_plus, t, (t - n_plus) | (1 << 31)).astype(np.uint32)
            off, cover = h.coding_eval(g.astype(np.uint32), packed)
            print("pieces: pairs", g.size, "off differs:", int((off != positions[0][g, t]).sum()), "cover differs:", int((cover != positions[1][g, t]).sum()))
            assert g.size > 300 and np.array_equal(off, positions[0][g, t]) and np.array_equal(cover, positions[1][g, t])
            for slice_rows in (0, 64):
                h.set_limits(slice_rows)
                for limits in (None, (5, 65, 0), (0, 100, 0), (0, 100, 100), (0, 20, 0)):
                    want = cref.select_numpy(tables, lo, hi, case["models"], rows, 5, limits, positions=positions)
                    if limits is not None:
                        assert want[1].any() and (want[1] < cref.select_numpy(tables, lo, hi, case["models"], rows, 5, None, positions=positions)[1]).any()
                    h.set_coding_limits(None if limits is None else coding.Limits(*limits))
                    h.run(sel.Params(5))
                    _same(h.fetch(), want, "pieces slices %d limits %s" % (slice_rows, limits))
        finally:
            h.close()
    finally:
        arena.close()


@pytest.mark.gpu
@pytest.mark.parametrize("minus", [False, True], ids=["plus", "minus"])
def test_gpu_a_row_of_one_step(scanned, minus):
    """The layout never makes a row of ONE step (a row returns to the zero word), but crp_select_set_coding takes any ascending
    model: a hand-made one pins the binary search's n = 1 edge in both kernels.  Every gene gets the single step `inside P,
    one transcript, growing` at the median boundary of its rows; before it nothing holds."""
    A = scanned["arenas"][0]
    G = len(A["lo"])
    c = _boundaries(A)
    L, cum0 = 0xFFFFFFF0, 7
    at = np.array([int(np.median(c[A["member"][r]])) if A["member"][r].any() else int(A["lo"][r]) for r in range(G)], np.uint32)
    model = dict(info=np.full(G, 1 | (1 << 16 if minus else 0) | 1 << 17, np.uint32), length=np.full(G, L, np.uint32),
                 first=np.arange(G + 1, dtype=np.uint64), at=at, word=np.full(G, 1 | 1 << 16 | 1 << 17, np.uint32), cum=np.full(G, cum0, np.uint32))
    g, t = np.nonzero(A["member"])
    n_plus = len(A["tables"]["pos_plus"])
    packed = np.where(t < n_plus, t, (t - n_plus) | (1 << 31)).astype(np.uint32)
    holds = c[t] >= at[g].astype(np.int64)
    before = cum0 + (c[t] - at[g].astype(np.int64))
    want_off = np.where(holds, L - before if minus else before, cref.NOT_INSIDE).astype(np.uint32)
    assert holds.sum() > 500 and (~holds).sum() > 500  # rows on both sides of the one change point
    h = sel.ArenaSelect(scanned["genome"].arenas[0], A["lo"], A["hi"])
    try:
        h.set_coding(model)
        off, cover = h.coding_eval(g.astype(np.uint32), packed)
        assert np.array_equal(off, want_off) and np.array_equal(cover, holds.astype(np.uint32))
        # the selection: with (0, 100, 0) exactly the rows at or after the step pass; 100 off needs its 64 bits here
        h.set_coding_limits(coding.Limits(0, 100, 0))
        h.run(sel.Params(5))
        n_in, n_pass, _ = h.fetch()
        assert np.array_equal(n_pass, np.bincount(g[holds], minlength=G)) and np.array_equal(n_in, A["member"].sum(axis=1))
        h.set_coding_limits(coding.Limits(0, 0, 0) if not minus else coding.Limits(100, 100, 0))
        h.run(sel.Params(5))
        assert not h.fetch()[1].any()
    finally:
        h.close()


@pytest.mark.gpu
def test_gpu_calls_out_of_order(scanned):
    A = scanned["arenas"][0]
    arena = scanned["genome"].arenas[0]
    L = nat.lib()
    h = sel.ArenaSelect(arena, A["lo"], A["hi"])

    def status(fn):
        with pytest.raises(nat.CropsrHipError) as e:
            fn()
        return e.value.status, str(e.value)

    try:
        h.set_coding_limits(coding.Limits(5, 65))
        st, text = status(lambda: h.run(sel.Params(5)))
        assert st == nat.CRP_ERR_STATE and "crp_select_set_coding" in text        # limits without a model
        st, text = status(lambda: h.coding_eval([0], [0]))
        assert st == nat.CRP_ERR_STATE and "crp_select_set_coding" in text        # eval without a model
        short = {k: (v[:-1] if k in ("info", "length", "first") else v) for k, v in A["model"].items()}
        st, text = status(lambda: h.set_coding(short))
        assert st == nat.CRP_ERR_INVALID and "rows" in text                       # a model of the wrong row count
        bad = dict(A["model"], first=A["model"]["first"].copy())
        bad["first"][-1] += 1
        assert status(lambda: h.set_coding(bad))[0] == nat.CRP_ERR_INVALID        # steps that the arrays do not hold
        bad = dict(A["model"], at=A["model"]["at"][::-1].copy())
        st, text = status(lambda: h.set_coding(bad))
        assert st == nat.CRP_ERR_INVALID and "ascend" in text
        assert status(lambda: h.run(sel.Params(5)))[0] == nat.CRP_ERR_STATE       # a refused model is no model
        for lim in ((66, 65, 0), (0, 101, 0), (0, 100, 101)):
            c = nat.SelectCodingLimits(*lim)
            assert L.crp_select_set_coding_limits(h._h, ctypes.byref(c)) == nat.CRP_ERR_INVALID
        h.set_coding(A["model"])
        st, text = status(lambda: h.run_pairs(sel.Params(5), sel.PairParams(5)))
        assert st == nat.CRP_ERR_UNSUPPORTED and "coding limits" in text          # pairs with coding limits
        n_plus, n_minus = len(A["tables"]["pos_plus"]), len(A["tables"]["pos_minus"])
        for g, packed in ((len(A["lo"]), 0), (0, n_plus), (0, n_minus | 1 << 31), (0xFFFFFFFF, 0)):
            st, text = status(lambda: h.coding_eval([0, g], [0, packed]))
            assert st == nat.CRP_ERR_INVALID and "query 1" in text                # out of range: refused on the host
        h.run(sel.Params(5))
        _same(h.fetch(), _reference(scanned, 0, 5, (5, 65, 0)), "after the refusals")
        h.set_coding_limits(None)
        h.run_pairs(sel.Params(5), sel.PairParams(5))                             # without limits the pairs run, model or not
        h.run(sel.Params(5))
        _same(h.fetch(), _reference(scanned, 0, 5, None), "limits cleared")
        h.set_coding(None)
        assert status(lambda: h.coding_eval([0], [0]))[0] == nat.CRP_ERR_STATE    # model cleared
        empty = sel.ArenaSelect(arena, [], [])
        try:
            empty.set_coding(None)                                                # clearing works on a handle without genes
            empty.set_coding(dict(info=[], length=[], first=[0], at=[], word=[], cum=[]))
            empty.set_coding_limits(coding.Limits(5, 65))
            empty.run(sel.Params(5))
            empty.set_coding(None)
            assert status(lambda: empty.run(sel.Params(5)))[0] == nat.CRP_ERR_STATE
        finally:
            empty.close()
    finally:
        h.close()


@pytest.mark.gpu
def test_gpu_genome_level_call(engine, case):
    """Genome.scan_score(select=...) with the coding position: the Selection's fields against the reference, three arenas."""
    g = engine.genome(case["contigs"], max_words=600)
    try:
        request = annotate.Request(case["annotation"], case["names"], 0)
        for limits in (None, (5, 65, 50)):
            req = sel.Request(sel.Params(5), request, coding=True, coding_limits=None if limits is None else coding.Limits(*limits))
            s = g.scan_score(20, select=req).selection
            assert s.stats["coding_steps"] > 500 and (s.stats["coding_select_ms"] > 0) == (limits is not None) and s.stats["coding_eval_ms"] > 0
            tables, entries = _host_arena(case)
            lo, hi, gene = sref.layout(case["genes"], entries, 0)
            rows = cref.layout_rows(case["gff"], entries, 0)
            positions = cref.positions_numpy(tables, case["models"], rows)
            n_in, n_pass, picked = cref.select_numpy(tables, lo, hi, case["models"], rows, 5, limits, positions=positions)
            assert np.array_equal(s.n_pass[gene.astype(np.int64)], n_pass) and np.array_equal(s.n_in[gene.astype(np.int64)], n_in)
            r, c = np.nonzero(picked != NONE)
            order = np.lexsort((c, gene[r]))  # the Selection lists the genes in file order
            r, c = r[order], c[order]
            n_plus = len(tables["pos_plus"])
            t = np.where(picked[r, c] >> 31 != 0, (picked[r, c] & 0x7FFFFFFF).astype(np.int64) + n_plus, picked[r, c].astype(np.int64))
            assert s.rows.size == r.size and np.array_equal(s.rows["gene"], gene[r]) and np.array_equal(s.rows["rank"], c + 1)
            assert np.array_equal(s.cds_offset, positions[0][r, t]) and np.array_equal(s.transcripts_cut, positions[1][r, t])
            assert np.array_equal(s.cds_length, [case["models"][int(x)]["length"] for x in gene[r]])
            assert np.array_equal(s.transcripts, [case["models"][int(x)]["n_tx"] for x in gene[r]])
            if limits is not None:
                assert (s.cds_offset != coding.NOT_INSIDE).all() and (2 * s.transcripts_cut >= s.transcripts).all()
            else:
                assert (s.cds_offset == coding.NOT_INSIDE).any() and (s.cds_offset != coding.NOT_INSIDE).any()
        plain = g.scan_score(20, select=sel.Request(sel.Params(5), request)).selection
        assert plain.cds_offset is None and "coding_steps" not in plain.stats
        # the fields beside a pair selection (no limits): both parts arrive, each what it is alone
        both = g.scan_score(20, select=sel.Request(sel.Params(5), request, coding=True, pairs=sel.PairParams(3))).selection
        pairs_alone = g.scan_score(20, select=sel.Request(sel.Params(5), request, pairs=sel.PairParams(3))).selection
        fields_alone = g.scan_score(20, select=sel.Request(sel.Params(5), request, coding=True)).selection
        assert both.pairs.size > 20 and np.array_equal(both.pairs, pairs_alone.pairs) and np.array_equal(both.n_pairs, pairs_alone.n_pairs)
        assert np.array_equal(both.rows, fields_alone.rows) and np.array_equal(both.cds_offset, fields_alone.cds_offset)
        assert np.array_equal(both.transcripts_cut, fields_alone.transcripts_cut) and pairs_alone.cds_offset is None
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------- the command line
class CodingOracleBackend(OracleBackend):
    """OracleBackend plus the `select` keyword with the coding position: the selection by the numpy statement over one host
    arena, the coding position of the selected rows by the restated definition."""

    def __init__(self, orc, gff_text):
        OracleBackend.__init__(self, orc)
        self.gff_text = gff_text
        self.requests = []

    def scan(self, strings, l, offtarget=False, annotation=None, specificity=None, select=None):
        out = OracleBackend.scan(self, strings, l, offtarget=offtarget, annotation=annotation)
        if select is None:
            return out
        self.requests.append(select)
        texts = [bytes(s) for s in strings]
        offsets, off = [], 64
        for t in texts:
            offsets.append(off)
            off += ((len(t) + 63) // 64 + 1) * 64
        tables = _arena_tables(out, offsets)
        req = select.annotation
        lo, hi, gene = req.gene_layout([(k, o, len(t)) for k, (t, o) in enumerate(zip(texts, offsets))])
        entries = [(req.names[k], req.starts[k], len(t), o) for k, (t, o) in enumerate(zip(texts, offsets))]
        rows, models = cref.layout_rows(self.gff_text, entries, req.dec), cref.model_numpy(self.gff_text)
        assert [r[0] for r in rows] == gene.tolist()
        positions = cref.positions_numpy(tables, models, rows)
        limits = None if select.coding_limits is None else select.coding_limits.astuple()
        ok = np.concatenate([tables["score_plus"], tables["score_minus"]]) >= select.params.min_score
        n_in, n_pass, picked = cref.select_numpy(tables, lo, hi, models, rows, select.params.k, limits, ok, positions=positions)
        part = dict(offsets=np.array(offsets, np.uint64), lengths=np.array([len(t) for t in texts], np.uint64), group=list(range(len(texts))),
                    gene=gene, n_in=n_in, n_pass=n_pass, sel=picked, **tables)
        if select.coding:
            n_plus = len(tables["pos_plus"])
            t = np.where(picked >> 31 != 0, (picked & 0x7FFFFFFF).astype(np.int64) + n_plus, picked.astype(np.int64))
            t[picked == NONE] = 0
            g = np.arange(len(rows))[:, None]
            part["coding"] = dict(off=np.where(picked == NONE, NONE, positions[0][g, t]), cover=np.where(picked == NONE, 0, positions[1][g, t]),
                                  length=np.array([models[r[0]]["length"] for r in rows], np.uint32),
                                  n_tx=np.array([models[r[0]]["n_tx"] for r in rows], np.uint32))
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


def _expected_fields(case, got_rows, limits, min_score):
    """Per row of a selection file (gene label, end_pos, strand -> the table row): the five fields by the loop statement, and
    the set of (gene, chromosome, end_pos, strand) the selection must consist of."""
    from decimal import ROUND_HALF_UP, Decimal
    tables, entries = _host_arena(case)
    lo, hi, gene = sref.layout(case["genes"], entries, 0)
    rows = cref.layout_rows(case["gff"], entries, 0)
    models = cref.model_loop(case["gff"])
    n_in, n_pass, picked = cref.select_loop(tables, lo, hi, models, rows, 5, limits,
                                            np.concatenate([tables["score_plus"], tables["score_minus"]]) >= min_score)
    label_row = {case["genes"][int(g)][3]: r for r, g in enumerate(gene)}
    offset_of = {n: e[3] for n, e in zip(case["names"], entries)}
    want_rows = set()
    for r in range(len(rows)):
        for packed in picked[r]:
            if packed != NONE:
                minus, t = int(packed) >> 31, int(packed) & 0x7FFFFFFF
                pos = int(tables["pos_minus" if minus else "pos_plus"][t])
                k = max(i for i, e in enumerate(entries) if e[3] <= pos)
                want_rows.add((case["genes"][int(gene[r])][3], case["names"][k], str(pos - entries[k][3] + (3 if minus else 0)), "-" if minus else "+"))
    fields = []
    for g in got_rows:
        r = label_row[g[0]]
        end, minus = int(g[8]) + offset_of[g[6]], g[10] == "-"  # (gene, rank, passing, then the main table's fields without its first)
        c = end - 3 + 6 if minus else end - 3  # end_pos is i on the '+' strand and j + 3 on the '-' strand
        off, cover = cref.position_loop(models[rows[r][0]], rows[r], c)
        m = models[rows[r][0]]
        if off == cref.NOT_INSIDE:
            fields.append(["", "", "", str(cover), str(m["n_tx"])])
        else:
            pct = (Decimal(100 * off) / Decimal(m["length"])).quantize(Decimal("0.1"), rounding=ROUND_HALF_UP)
            fields.append([str(off), str(m["length"]), str(pct), str(cover), str(m["n_tx"])])
    return fields, want_rows, n_pass, label_row


def test_cli_coding_fields_and_filter_over_the_oracle(case, oracle, tmp_path, monkeypatch):
    from cropsr_amd import rows as rows_mod
    backend = CodingOracleBackend(oracle, case["gff"])
    plain, _ = _run(case, tmp_path, monkeypatch, ["--select", "5", "--select-min-score", "0.2"], backend, "plain.csv")
    assert backend.requests[-1].coding is False and backend.requests[-1].coding_limits is None
    with_fields, _ = _run(case, tmp_path, monkeypatch, ["--select", "5", "--select-min-score", "0.2", "--coding"], backend, "fields.csv")
    assert backend.requests[-1].coding is True and backend.requests[-1].coding_limits is None
    bench = str(tmp_path / "bench.json")
    filtered, _ = _run(case, tmp_path, monkeypatch, ["--select", "5", "--select-min-score", "0.2", "--select-coding-min", "5", "--select-coding-max", "65",
                                                     "--select-transcripts", "100", "--bench-json", bench], backend, "filtered.csv")
    assert backend.requests[-1].coding_limits.astuple() == (5, 65, 100)
    for path in (with_fields, filtered):  # the main table is what it was
        with open(plain, "rb") as a, open(path, "rb") as b:
            assert a.read() == b.read()
    # without the new options: the header and the fields of before; with --coding: the same file with five more fields
    old, new = _read(plain + ".selected.csv"), _read(with_fields + ".selected.csv")
    assert old[0] == ["gene", "rank", "passing"] + rows_mod.HEADER[1:] and new[0] == old[0] + coding.HEADER
    assert [r[:-5] for r in new] == old and len(old) > 60
    buf = io.StringIO()
    csv.writer(buf).writerows([r[:-5] for r in new])
    with open(plain + ".selected.csv", newline="") as f:
        assert f.read() == buf.getvalue()  # byte for byte
    fields, want_rows, _, _ = _expected_fields(case, new[1:], None, 0.2)
    assert [r[-5:] for r in new[1:]] == fields
    assert any(f[0] == "" for f in fields) and any(f[0] != "" for f in fields)
    assert set((r[0], r[6], r[8], r[10]) for r in new[1:]) == want_rows
    # the filtered selection: the reference's rows, every one inside and in every transcript
    got = _read(filtered + ".selected.csv")
    fields, want_rows, n_pass, label_row = _expected_fields(case, got[1:], (5, 65, 100), 0.2)
    assert got[0] == new[0] and [r[-5:] for r in got[1:]] == fields and 10 < len(got) < len(new)
    assert set((r[0], r[6], r[8], r[10]) for r in got[1:]) == want_rows
    for r in got[1:]:
        assert int(r[2]) == n_pass[label_row[r[0]]] and 5.0 <= float(r[-3]) <= 65.0 and r[-2] == r[-1]
    assert "gene:no_cds" not in [r[0] for r in got[1:]] and "gene:no_strand" not in [r[0] for r in got[1:]]
    assert any(r[-1] == "2" for r in got[1:])  # a gene of two transcripts, cut in both
    import json
    with open(bench) as f:
        assert "select" in json.load(f)


CODING_REFUSALS = [
    (["--coding"], "belongs to --select", False),
    (["--select-coding-min", "5"], "belongs to --select", False),
    (["--select-coding-max", "65"], "belongs to --select", False),
    (["--select-transcripts", "50"], "belongs to --select", False),
    (["--select", "5", "--coding"], "needs -g", True),
    (["--select", "5", "--select-coding-min", "5"], "needs -g", True),
    (["--select", "5", "--select-coding-min", "101"], "0..100", False),
    (["--select", "5", "--select-coding-max", "-1"], "0..100", False),
    (["--select", "5", "--select-coding-max", "6.5"], "0..100", False),
    (["--select", "5", "--select-transcripts", "200"], "0..100", False),
    (["--select", "5", "--select-transcripts", "half"], "0..100", False),
    (["--select", "5", "--select-coding-min", "66", "--select-coding-max", "65"], "lies above", False),
    (["--select", "5", "--select-coding-min", "5", "--select-pairs", "3"], "--select-pairs", False),
    (["--select", "5", "--select-coding-max", "65", "--select-pairs", "3"], "--select-pairs", False),
    (["--select", "5", "--select-transcripts", "100", "--select-pairs", "3"], "--select-pairs", False),
    (["--select", "5", "--coding", "--select-pairs", "3"], "--coding: the coding position", False),
    (["--select", "5", "--coding", "--gpus", "2"], "one GPU", False),
]


@pytest.mark.parametrize("extra,text,no_gff", CODING_REFUSALS, ids=[" ".join(r[0]) for r in CODING_REFUSALS])
def test_cli_refusals_come_before_any_side_effect(case, oracle, tmp_path, monkeypatch, extra, text, no_gff):
    monkeypatch.chdir(tmp_path)
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9"] + ([] if no_gff else ["-g", case["gff_path"]]) + extra
    backend = CodingOracleBackend(oracle, case["gff"])
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=backend, out=io.StringIO())
    assert "--select" in str(e.value.code) and text in str(e.value.code)
    assert os.listdir(tmp_path) == [] and not backend.requests


@pytest.mark.gpu
def test_gpu_command_line_end_to_end(case, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    out_csv = str(tmp_path / "out.csv")
    argv = ["-f", case["fasta_path"], "-g", case["gff_path"], "-o", out_csv, "--cas9", "--seed", "11", "--each-contig-once", "--select", "5",
            "--select-min-score", "0.2", "--select-coding-min", "5", "--select-coding-max", "65", "--select-transcripts", "100",
            "--bench-json", str(tmp_path / "bench.json")]
    cli.run(cli.build_parser().parse_args(argv), out=io.StringIO())
    got = _read(out_csv + ".selected.csv")
    fields, want_rows, n_pass, label_row = _expected_fields(case, got[1:], (5, 65, 100), 0.2)
    assert got[0][-5:] == coding.HEADER and [r[-5:] for r in got[1:]] == fields and len(got) > 10
    assert set((r[0], r[6], r[8], r[10]) for r in got[1:]) == want_rows
    import json
    with open(tmp_path / "bench.json") as f:
        stage = json.load(f)["select"]
    assert stage["coding_select_ms"] > 0 and stage["coding_eval_ms"] > 0 and stage["coding_steps"] > 500
