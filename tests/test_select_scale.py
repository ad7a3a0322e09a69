"""The selection's host driver past one launch, and one handle over many runs (cropsr_amd/csrc/crp_select.cpp; DESIGN.md
sections 16 and 19).

One launch covers at most 2^20 items, and as many merges; crp_select_run and crp_select_run_pairs loop over their items and
merges in chunks of that size and hand each launch `d_items + first`, `d_merge + first`, `d_pair_evals + first`.  The gene
lists of tests/select_scale_cases.py hold more than 2^20 genes over one 16 kb contig -- genes may overlap, and the list is a
cyclic tiling of 16 ranges --, so every one of the four loops takes a second trip, a gene's pieces lie in two launches, and
the reference costs 16 answers of tests/select_reference.py (tests/select_pairs_reference.py) and one `take`.  The CPU test
proves on the oracle's rows, with the host's cut restated, that the lists reach those paths; the GPU tests compare whole
arrays, bit for bit.  The second part keeps one handle through a sequence of runs -- a smaller K over the buffers of a
larger one, a pair run that rewrites the shared bounds, limits set and cleared, a rescan -- and compares every step with
the reference and with a fresh handle.

Out of scope: the coding, edit, splice and family kernels take the same `d_items + first` from the same loop, and feeding
them 2^20 genes needs a coding model or a family table for a million genes.  Their cut and merge paths are covered at small
size (tests/test_select_coding.py, test_base_edit.py, test_splice_edit.py, test_families.py); the launch loop is covered
here through the plain kernel."""
import numpy as np
import pytest

import select_pairs_reference as pref
import select_reference as ref
import select_scale_cases as cases
import guide_properties_reference as gpref
import repair_reference as rref
from cropsr_amd import _native as nat
from cropsr_amd import properties, repair
from cropsr_amd import select as sel

NONE = 0xFFFFFFFF
G, D, MAX_ITEMS = cases.G, cases.D, cases.MAX_ITEMS
ALL = list(range(D))
CUT = [j for j, n in enumerate(cases.ROWS) if n >= 65]             # list B: every gene is cut at slices of 64
PAIR_SMALL = [j for j, n in enumerate(cases.ROWS) if n <= 130]     # one item a gene at the default pair slices
PAIR_CUT = [j for j, n in enumerate(cases.ROWS) if 65 <= n <= 130]  # two or three items a gene at pair slices of 64
PAIR_WINDOW = (20, 120)


@pytest.fixture(scope="module")
def case(oracle):
    text = cases.contig()
    hits = oracle.scan_score(text, 20)
    lo, hi = cases.ranges(hits)
    return dict(contig=text, hits=hits, lo=lo, hi=hi, total=cases.rows_in(hits, lo, hi))


def _tables(hits, offset):
    return dict(pos_plus=hits["pos_plus"].astype(np.uint32) + np.uint32(offset), score_plus=hits["score_plus"].astype(np.float64),
                pos_minus=hits["pos_minus"].astype(np.uint32) + np.uint32(offset), score_minus=hits["score_minus"].astype(np.float64))


def _neighbours_differ(which, answers):
    """Cyclic neighbours of a tiling never share an answer: a result shifted by one gene cannot pass."""
    for a, b in zip(which, which[1:] + which[:1]):
        assert any(not np.array_equal(x[a], x[b]) for x in answers), (a, b)


# ---------------------------------------------------------------------------------------------- without a GPU
def test_the_lists_reach_a_second_launch(case):
    """On the oracle's rows, with the host's cut restated (select_scale_cases.host_cut): the lists need two or more item
    launches, put a gene's pieces across every launch boundary, and need two merge launches."""
    assert case["total"].tolist() == list(cases.ROWS) and G > MAX_ITEMS
    assert len(case["hits"]["pos_plus"]) > 900 and len(case["hits"]["pos_minus"]) > 900
    # list A at slices of 64: three launches, and at every boundary a gene that is cut in two by it
    start = cases.boundary_start(case["total"], ALL, 64)
    cut = cases.host_cut(case["total"][cases.tiling(ALL, G, start)], 64)
    assert cut["items"] > 2 * MAX_ITEMS and -(-cut["items"] // MAX_ITEMS) >= 3
    for b in range(MAX_ITEMS, cut["items"], MAX_ITEMS):
        g = int(np.searchsorted(cut["first_item"], b, "right") - 1)
        assert cut["pieces"][g] > 1 and cut["first_item"][g] < b < cut["first_item"][g] + cut["pieces"][g], (b, g)
        # its slots are consecutive from slot_first: they run across the boundary with its items
        assert cut["slot_first"][g] >= 0 and cut["slot_first"][g] + cut["pieces"][g] <= cut["slots"]
    assert cut["cut_genes"] < MAX_ITEMS  # (list A's merges fit one launch: list B is there for the merge loop)
    # the restated cut against a plain loop, on one cycle of the tiling
    items, slots = [], 0
    for g, n in enumerate(case["total"].tolist()):
        p = max(1, -(-n // 64))
        for c in range(p):
            items.append((g, slots + c if p > 1 else -1, min(n, 64 * c), min(n, 64 * (c + 1))))
        slots += p if p > 1 else 0
    one = cases.host_cut(case["total"], 64)
    assert (one["items"], one["slots"]) == (len(items), slots) and one["first_item"].tolist() == [
        next(i for i, it in enumerate(items) if it[0] == g) for g in range(D)]
    assert [int(s) for s in one["slot_first"]] == [next(it[1] for it in items if it[0] == g) for g in range(D)]
    # list A at the default slices: one item a gene, two launches; list B at 64: every gene is merged, two merge launches
    whole = cases.host_cut(case["total"][cases.tiling(ALL)], 65536)
    assert whole["items"] == G > MAX_ITEMS and whole["cut_genes"] == 0
    merged = cases.host_cut(case["total"][cases.tiling(CUT)], 64)
    assert merged["cut_genes"] == G > MAX_ITEMS and merged["items"] > 3 * MAX_ITEMS
    # the pair lists: one item a gene at the default pair slices (1024 rows), two or three at 64
    assert cases.host_cut(case["total"][cases.tiling(PAIR_SMALL)], 1024)["items"] == G
    pair_cut = cases.host_cut(case["total"][cases.tiling(PAIR_CUT)], 64)
    assert pair_cut["items"] >= 2 * G and pair_cut["cut_genes"] == G
    # the answers: neighbours in every tiling differ, and the empty range expects zeros and no row
    tables = _tables(case["hits"], 64)
    n_in, n_pass, picked = ref.select_numpy(tables, case["lo"] + 64, case["hi"] + 64, 1)
    for which in (ALL, CUT):
        _neighbours_differ(which, (n_in, picked[:, 0]))
    empty = cases.ROWS.index(0)
    assert n_in[empty] == 0 and n_pass[empty] == 0 and (picked[empty] == NONE).all()
    assert (n_in[[j for j in ALL if j != empty]] > 0).all()
    n_pass, n_pairs, pairs = pref.pairs_numpy(tables, case["lo"] + 64, case["hi"] + 64, 3, *PAIR_WINDOW)
    for which in (PAIR_SMALL, PAIR_CUT):
        _neighbours_differ(which, (n_pass, n_pairs, pairs[:, 0, 0]))
        assert (n_pairs[which] > 3).sum() >= 6 and n_pairs[empty] == 0 and (pairs[empty] == NONE).all()


# ---------------------------------------------------------------------------------------------- on the GPU
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def scanned(engine, case):
    """One arena, one scan, the tables fetched once: the scan is pinned elsewhere, here it is the ground the selection stands
    on.  The ranges are the oracle's, moved to the arena's offset."""
    arena = engine.arena([case["contig"]])
    n_plus, n_minus = arena.scan_score_device(20)
    cols = arena.fetch(n_plus, n_minus)
    tables = dict(pos_plus=cols[0], score_plus=cols[2], pos_minus=cols[3], score_minus=cols[5])
    off = int(arena.offsets[0])
    lo, hi = (case["lo"] + off).astype(np.uint32), (case["hi"] + off).astype(np.uint32)
    cuts = np.sort(np.concatenate([tables["pos_plus"].astype(np.int64) - 3, tables["pos_minus"].astype(np.int64)]))
    total = np.searchsorted(cuts, hi.astype(np.int64), "right") - np.searchsorted(cuts, lo.astype(np.int64), "left")
    assert total.tolist() == list(cases.ROWS)
    yield dict(arena=arena, tables=tables, lo=lo, hi=hi, total=total, counts=(n_plus, n_minus), cache={})
    arena.close()


def _reference(s, K, min_score=0.0):
    """select_numpy over the D ranges, once per set of arguments."""
    key = ("select", K, min_score)
    if key not in s["cache"]:
        s["cache"][key] = ref.select_numpy(s["tables"], s["lo"], s["hi"], K, min_score)
    return s["cache"][key]


def _pairs_reference(s, KP, min_score=0.0):
    key = ("pairs", KP, min_score)
    if key not in s["cache"]:
        s["cache"][key] = pref.pairs_numpy(s["tables"], s["lo"], s["hi"], KP, *PAIR_WINDOW, min_score=min_score)
    return s["cache"][key]


def _same(got, want, ids=None):
    """Whole arrays, bit for bit; ids: the tiling (the reference's rows are taken through it)."""
    assert len(got) == len(want) == 3
    for k, (g, w) in enumerate(zip(got, want)):
        w = np.asarray(w) if ids is None else np.asarray(w)[ids]
        assert g.shape == w.shape and np.array_equal(g, w.astype(g.dtype)), k


def _run(s, ids, K, slice_rows=None, min_score=0.0):
    """A fresh handle over the genes `ids`: (n_in, n_pass, sel), stats."""
    h = sel.ArenaSelect(s["arena"], s["lo"][ids], s["hi"][ids])
    try:
        if slice_rows:
            h.set_limits(slice_rows)
        h.run(sel.Params(K, min_score))
        return h.fetch(), h.stats()
    finally:
        h.close()


def _run_pairs(s, ids, KP, pair_slice_rows=None):
    h = sel.ArenaSelect(s["arena"], s["lo"][ids], s["hi"][ids])
    try:
        if pair_slice_rows:
            h.set_pair_limits(pair_slice_rows)
        h.run_pairs(sel.Params(5), sel.PairParams(KP, *PAIR_WINDOW))
        return h.fetch_pairs(), h.pairs_stats()
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 64])
def test_gpu_more_genes_than_one_launch(scanned, K):
    """List A at the default slices: one item a gene, the second launch begins at gene 2^20."""
    s = scanned
    ids = cases.tiling(ALL)
    got, stats = _run(s, ids, K)
    _same(got, _reference(s, K), ids)
    assert stats["items"] == G and stats["launches"] == 2 and stats["merged_genes"] == 0


@pytest.mark.gpu
def test_gpu_cut_genes_across_the_launch_boundaries(scanned):
    """List A at slices of 64: three launches, a gene's pieces and slots on both sides of each boundary."""
    s = scanned
    start = cases.boundary_start(s["total"], ALL, 64)
    ids = cases.tiling(ALL, G, start)
    cut = cases.host_cut(s["total"][ids], 64)
    got, stats = _run(s, ids, 5, 64)
    _same(got, _reference(s, 5), ids)
    assert stats["items"] == cut["items"] > 2 * MAX_ITEMS and stats["merged_genes"] == cut["cut_genes"]
    assert stats["launches"] == -(-cut["items"] // MAX_ITEMS) >= 3


@pytest.mark.gpu
def test_gpu_more_merges_than_one_launch(scanned):
    """List B at slices of 64 with a threshold at the median score: every gene is merged, the merge takes two launches."""
    s = scanned
    t = s["tables"]
    scores = np.concatenate([t["score_plus"], t["score_minus"]])
    median = float(np.median(scores[scores != -1.0]))
    ids = cases.tiling(CUT)
    want = _reference(s, 5, median)
    assert (want[1][CUT] < want[0][CUT]).all() and (want[1][CUT] >= 5).all()  # the threshold filters, and every list is full
    got, stats = _run(s, ids, 5, 64, median)
    _same(got, want, ids)
    assert stats["merged_genes"] == G > MAX_ITEMS and stats["items"] == cases.host_cut(s["total"][ids], 64)["items"]


@pytest.mark.gpu
def test_gpu_pairs_of_more_genes_than_one_launch(scanned):
    """The pair items, one a gene: the second launch begins at gene 2^20, with its own slice of the evaluation counts."""
    s = scanned
    ids = cases.tiling(PAIR_SMALL)
    want = _pairs_reference(s, 3)
    got, stats = _run_pairs(s, ids, 3)
    _same(got, want, ids)
    assert stats["items"] == G and stats["launches"] == 2
    assert stats["qualifying_pairs"] == float(want[1][ids].astype(np.float64).sum())


@pytest.mark.gpu
def test_gpu_pair_merges_of_more_genes_than_one_launch(scanned):
    """Pair slices of 64 over genes of 65 .. 130 rows: two or three items a gene, every gene merged, two merge launches."""
    s = scanned
    ids = cases.tiling(PAIR_CUT)
    cut = cases.host_cut(s["total"][ids], 64)
    want = _pairs_reference(s, 3)
    got, stats = _run_pairs(s, ids, 3, 64)
    _same(got, want, ids)
    assert stats["items"] == cut["items"] >= 2 * G and cut["cut_genes"] == G > MAX_ITEMS
    assert stats["launches"] == -(-cut["items"] // MAX_ITEMS) >= 3


# ---------------------------------------------------------------------------------------------- one handle, many runs
PROPERTY_LIMITS = properties.Limits(gc_min=7, gc_max=14, max_run=4, max_t_run=3, max_stem=5)
REPAIR_LIMITS = repair.Limits(min_mh=300, min_oof=55)


@pytest.mark.gpu
def test_gpu_one_handle_many_runs(scanned):
    """The handle's buffers only grow and its limits are set and cleared between runs: after every step the result is the
    reference's and a fresh handle's."""
    s = scanned
    arena, t, lo, hi = s["arena"], s["tables"], s["lo"], s["hi"]
    n_plus, n_minus = s["counts"]
    ids = np.arange(D)
    big = cases.ROWS.index(700)
    h = sel.ArenaSelect(arena, lo, hi)

    def step(K, slice_rows, min_score, want):
        h.set_limits(slice_rows)
        h.run(sel.Params(K, min_score))
        got = h.fetch()
        _same(got, want)
        _same(got, _run(s, ids, K, slice_rows, min_score)[0])
        return got

    def fresh_limited(K, slice_rows, prop=None, rep=None):
        f = sel.ArenaSelect(arena, lo, hi)
        try:
            f.set_limits(slice_rows)
            f.set_property_limits(prop)
            f.set_repair_limits(rep)
            f.run(sel.Params(K))
            return f.fetch()
        finally:
            f.close()

    try:
        # 1: the largest K over cut genes; 2: a smaller K and no slots over the buffers that run filled
        first = step(64, 64, 0.0, _reference(s, 64))
        assert h.stats()["merged_genes"] == int((s["total"] > 64).sum()) > 5
        step(1, 0, 0.0, _reference(s, 1))
        assert h.stats()["merged_genes"] == 0
        # 3: a threshold that leaves the largest gene fewer than K rows: the rest of its list is NONE, not the earlier run's rows
        inside = lambda pos, cut: (cut >= int(lo[big])) & (cut <= int(hi[big]))
        scores = np.concatenate([t["score_plus"][inside(t["pos_plus"], t["pos_plus"].astype(np.int64) - 3)],
                                 t["score_minus"][inside(t["pos_minus"], t["pos_minus"].astype(np.int64))]])
        high = float(np.sort(scores)[-3])
        want3 = _reference(s, 5, high)
        assert 0 < want3[1][big] < 5 and (want3[2][big] == NONE).any() and want3[0][big] > 600
        third = step(5, 64, high, want3)
        # 4: a pair run on the same handle rewrites the shared bounds; the selection's result stays fetchable
        h.set_pair_limits(64)
        h.run_pairs(sel.Params(1), sel.PairParams(5, *PAIR_WINDOW))
        want_pairs = _pairs_reference(s, 5)
        _same(h.fetch_pairs(), want_pairs)
        _same(h.fetch_pairs(), _run_pairs(s, ids, 5, 64)[0])
        assert want_pairs[1].max() > 5 and h.pairs_stats()["items"] > D
        _same(h.fetch(), third)
        # 5: the same selection again
        _same(step(5, 64, high, want3), third)
        # 6: property limits set and cleared, then repair limits
        pp, pm = arena.guide_properties(n_plus, n_minus)
        rp, rm = arena.repair_scores(n_plus, n_minus, 30)
        props, reps = dict(props_plus=pp, props_minus=pm), dict(repair_plus=rp, repair_minus=rm)
        plain = _reference(s, 5)
        want_prop = gpref.select_numpy(t, lo, hi, 5, 0.0, None, None, props, PROPERTY_LIMITS.astuple())
        want_rep = rref.select_numpy(t, lo, hi, 5, 0.0, None, None, reps, REPAIR_LIMITS.astuple())
        for want in (want_prop, want_rep):  # each limit takes rows away, and leaves some
            assert (want[1] <= plain[1]).all() and 0 < int(want[1].sum()) < int(plain[1].sum())
        h.set_property_limits(PROPERTY_LIMITS)
        h.run(sel.Params(5))
        _same(h.fetch(), want_prop)
        _same(h.fetch(), fresh_limited(5, 64, prop=PROPERTY_LIMITS))
        h.set_property_limits(None)
        step(5, 64, 0.0, plain)
        h.set_repair_limits(REPAIR_LIMITS)
        h.run(sel.Params(5))
        _same(h.fetch(), want_rep)
        _same(h.fetch(), fresh_limited(5, 64, rep=REPAIR_LIMITS))
        h.set_repair_limits(None)
        step(5, 64, 0.0, plain)
        # 7: a rescan: the tables are the same, the columns of the earlier tables are gone
        assert arena.scan_score_device(20) == (n_plus, n_minus)
        step(5, 64, 0.0, plain)
        h.set_property_limits(PROPERTY_LIMITS)
        with pytest.raises(nat.CropsrHipError) as e:
            h.run(sel.Params(5))
        assert e.value.status == nat.CRP_ERR_STATE and "crp_guide_properties" in str(e.value)
        arena.guide_properties(n_plus, n_minus, fetch=False)
        h.run(sel.Params(5))
        _same(h.fetch(), want_prop)
        h.set_property_limits(None)
        # 8: the first run once more
        _same(step(64, 64, 0.0, _reference(s, 64)), first)
    finally:
        h.close()
