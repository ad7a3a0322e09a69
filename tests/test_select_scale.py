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

The spaced selection (crp_select_run_spaced) has three such loops: over the whole genes (`d_spaced_items + first`), per round
over the pieces of the cut genes, which lie behind the whole ones (`d_spaced_items + n_whole + first`), and per round over the
cut genes (`d_spaced_merge + first`, with `first` also as the pick kernel's index into `picked`, which the host reads whole to
end the rounds).  The same lists, with the spaced driver's cut restated (select_scale_cases.spaced_cut), take each loop past
one launch, and a fourth list lets only its first genes pick in the late rounds, so that the exit depends on their entries of
`picked`; the reference is tests/select_spacing_reference.py over the 16 ranges and one `take`.

The other loops past one launch: the coding, edit, splice and family kernels get `d_items + first` from crp_select_run's
loop, each through its own call; tests/test_select_coding.py, test_base_edit.py, test_splice_edit.py and test_families.py
each tile their own genes to 2^20 + 4 099 (select_scale_cases.tile_model tiles the coding model) and compare with their own
reference.  crp_select_family_step's loop is in tests/test_family_sets.py, on select_scale_cases.late_list."""
import numpy as np
import pytest

import select_pairs_reference as pref
import select_reference as ref
import select_scale_cases as cases
import select_spacing_reference as sp
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
SPACING = 150  # the spaced selection's D > 0: at K = 5 some ranges end early and some fill K (proved on the reference below)
HEAD_SPACING = 300  # list C's D: cut ranges of at most 2, of 3 and of 4 picks at K = 5 (proved on the reference below)
HEAD_GENES = 4096   # list C's head: fewer genes than the second pick launch holds (G - 2^20)


def _picks_class(n_spaced, counts):
    """The cut ranges whose pick count at K = 5 is one of `counts`."""
    return [j for j in CUT if int(n_spaced[j]) in counts]


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
    # boundary_start looks a boundary up by its place in a cycle; on the whole lists: its start does, no smaller one does
    assert cases.straddles(case["total"][cases.tiling(ALL, G, start)], 64)
    assert not any(cases.straddles(case["total"][cases.tiling(ALL, G, s)], 64) for s in range(start))
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


def test_the_spaced_lists_reach_a_second_launch(case):
    """On the oracle's rows, with the spaced driver's cut restated (select_scale_cases.spaced_cut): the whole genes, the pieces
    and the cut genes each need a second launch under one of the lists, a cut gene's pieces lie on both sides of every
    boundary of the pieces list behind a non-zero n_whole, and at SPACING some ranges end early and some fill K."""
    total = case["total"]
    # list A at the default slices: every gene whole, two item launches
    whole = cases.spaced_cut(total[cases.tiling(ALL)], 65536)
    assert whole["n_whole"] == G > MAX_ITEMS and whole["n_cut"] == 0 and whole["n_pieces"] == 0
    # list A at slices of 64: whole genes in front of the pieces, three step launches, one pick launch
    start = cases.spaced_boundary_start(total, ALL, 64)
    ids = cases.tiling(ALL, G, start)
    cut = cases.spaced_cut(total[ids], 64)
    assert 0 < cut["n_whole"] < MAX_ITEMS and cut["n_whole"] == int((total[ids] <= 64).sum())
    assert cut["n_pieces"] > 2 * MAX_ITEMS and 0 < cut["n_cut"] < MAX_ITEMS and cut["n_whole"] + cut["n_cut"] == G
    for b in range(MAX_ITEMS, cut["n_pieces"], MAX_ITEMS):
        j = int(np.searchsorted(cut["piece_first"], b, "right") - 1)
        assert cut["piece_first"][j] < b < cut["piece_first"][j] + cut["pieces"][j], (b, j)
    # list B at slices of 64: every gene cut, two pick launches
    merged = cases.spaced_cut(total[cases.tiling(CUT)], 64)
    assert merged["n_cut"] == G > MAX_ITEMS and merged["n_whole"] == 0 and merged["n_pieces"] > 3 * MAX_ITEMS
    # the restated cut against a plain loop, on one cycle of the tiling
    n_whole, pieces, merges = 0, [], []
    for g, n in enumerate(total.tolist()):
        p = max(1, -(-n // 64))
        if p == 1:
            n_whole += 1
            continue
        merges.append((g, len(pieces), p))
        pieces += [(g, min(n, 64 * c), min(n, 64 * (c + 1))) for c in range(p)]
    one = cases.spaced_cut(total, 64)
    assert (one["n_whole"], one["n_pieces"], one["n_cut"]) == (n_whole, len(pieces), len(merges))
    assert list(zip(one["cut_genes"].tolist(), one["piece_first"].tolist(), one["pieces"].tolist())) == merges
    assert all(pieces[f][0] == g and pieces[f + p - 1][0] == g for g, f, p in merges)
    # the launch count, restated from the three loops; one launch each is test_select_spacing.py's identity 2 + 1 + 2 * rounds
    assert cases.spaced_launches(dict(n_whole=10, n_pieces=100, n_cut=7), 4) == 2 + 1 + 2 * 4
    assert cases.spaced_launches(cut, 5) == 2 + 1 + 5 * (3 + 1) and cases.spaced_launches(merged, 5) == 2 + 0 + 5 * (4 + 2)
    assert cases.spaced_launches(whole, 0) == 2 + 2
    # the answers at K = 5: SPACING ends at least three ranges early although K rows pass, and at least three fill K
    tables = _tables(case["hits"], 64)
    n_pass, n_spaced, picked = sp.spaced_numpy(tables, case["lo"] + 64, case["hi"] + 64, 5, SPACING)
    early, full = (n_spaced < 5) & (n_pass >= 5), n_spaced == 5
    print("SPACING", SPACING, "n_pass", n_pass.tolist(), "n_spaced", n_spaced.tolist())
    assert early.sum() >= 3 and full.sum() >= 3 and early[CUT].any() and full[CUT].any()
    # list C, for the host's exit over `picked`: at HEAD_SPACING the cut ranges fall into classes by their pick count, all with
    # K passing rows; the head's class outlasts the rest's, and the head fits below the genes of the second pick launch
    n_pass, n_spaced, picked = sp.spaced_numpy(tables, case["lo"] + 64, case["hi"] + 64, 5, HEAD_SPACING)
    print("HEAD_SPACING", HEAD_SPACING, "n_spaced", n_spaced.tolist())
    rest = _picks_class(n_spaced, (1, 2))
    assert len(rest) >= 2 and (n_pass[CUT] >= 5).all() and 0 < HEAD_GENES <= G - MAX_ITEMS
    for picks in (3, 4):
        head = _picks_class(n_spaced, (picks,))
        assert len(head) >= 2 and picks < 5
        ids = cases.head_list(head, rest, HEAD_GENES)
        assert ids.size == G and set(ids[:HEAD_GENES].tolist()) == set(head) and set(ids[HEAD_GENES:].tolist()) == set(rest)
        assert cases.spaced_cut(total[ids], 64)["n_cut"] == G
    # neighbours in every tiling differ in what the GPU tests compare.  The ranges overlap, and the ranges of 129 and of 130
    # rows share their best row: n_spaced and sel[:, 0] alone do not tell them apart at D = 0, n_pass and the whole row of sel do
    for K, D in ((5, 0), (5, SPACING), (1, 0), (1, SPACING)):
        n_pass, n_spaced, picked = sp.spaced_numpy(tables, case["lo"] + 64, case["hi"] + 64, K, D)
        for which in (ALL, CUT):
            _neighbours_differ(which, (n_pass, n_spaced, picked))


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


# ---------------------------------------------------------------------------------------------- the spaced selection
def _spaced_reference(s, K, D):
    """spaced_numpy over the D ranges, once per (K, D)."""
    key = ("spaced", K, D)
    if key not in s["cache"]:
        s["cache"][key] = sp.spaced_numpy(s["tables"], s["lo"], s["hi"], K, D)
    return s["cache"][key]


def _run_spaced(s, ids, K, D, slice_rows=None):
    h = sel.ArenaSelect(s["arena"], s["lo"][ids], s["hi"][ids])
    try:
        if slice_rows:
            h.set_limits(slice_rows)
        h.run_spaced(sel.Params(K), D)
        return h.fetch_spaced(), h.spaced_stats()
    finally:
        h.close()


def _spaced_stats_hold(stats, cut, want, ids, K):
    """The item and gene counts are the restated cut's, and the launches are those of the three loops: a cut gene is picked
    for in rounds 0 .. n_spaced - 1, and the loop ends behind the first round that picks nothing, or at K."""
    assert stats["spaced_items"] == cut["n_whole"] + cut["n_pieces"] and stats["spaced_cut_genes"] == cut["n_cut"]
    rounds = min(K, int(np.asarray(want[1])[ids][cut["cut_genes"]].max()) + 1) if cut["n_cut"] else 0
    assert stats["spaced_rounds"] == rounds
    assert stats["spaced_launches"] == cases.spaced_launches(cut, rounds)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [0, SPACING], ids=["D0", "spaced"])
@pytest.mark.parametrize("K", [1, 5])
def test_gpu_spaced_more_genes_than_one_launch(scanned, K, D):
    """List A at the default slices: every gene whole, the second item launch begins at gene 2^20."""
    s = scanned
    ids = cases.tiling(ALL)
    cut = cases.spaced_cut(s["total"][ids], 65536)
    want = _spaced_reference(s, K, D)
    got, stats = _run_spaced(s, ids, K, D)
    _same(got, want, ids)
    assert cut["n_whole"] == G and stats["spaced_launches"] == 2 + 2
    _spaced_stats_hold(stats, cut, want, ids, K)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [0, SPACING], ids=["D0", "spaced"])
def test_gpu_spaced_pieces_across_the_launch_boundaries(scanned, D):
    """List A at slices of 64: the pieces lie behind n_whole whole genes and take three step launches a round, a cut gene's
    pieces on both sides of each boundary; the cut genes take one pick launch."""
    s = scanned
    start = cases.spaced_boundary_start(s["total"], ALL, 64)
    ids = cases.tiling(ALL, G, start)
    cut = cases.spaced_cut(s["total"][ids], 64)
    want = _spaced_reference(s, 5, D)
    got, stats = _run_spaced(s, ids, 5, D, 64)
    _same(got, want, ids)
    assert 0 < cut["n_whole"] and cut["n_pieces"] > 2 * MAX_ITEMS and cut["n_cut"] < MAX_ITEMS
    _spaced_stats_hold(stats, cut, want, ids, 5)
    assert stats["spaced_launches"] == 2 + 1 + stats["spaced_rounds"] * (3 + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [0, SPACING], ids=["D0", "spaced"])
def test_gpu_spaced_more_cut_genes_than_one_launch(scanned, D):
    """List B at slices of 64: every gene is cut, two pick launches a round, and `picked` spans both."""
    s = scanned
    ids = cases.tiling(CUT)
    cut = cases.spaced_cut(s["total"][ids], 64)
    want = _spaced_reference(s, 5, D)
    got, stats = _run_spaced(s, ids, 5, D, 64)
    _same(got, want, ids)
    assert cut["n_cut"] == G > MAX_ITEMS and cut["n_whole"] == 0
    _spaced_stats_hold(stats, cut, want, ids, 5)
    assert stats["spaced_launches"] == 2 + stats["spaced_rounds"] * (-(-cut["n_pieces"] // MAX_ITEMS) + 2)


@pytest.mark.gpu
@pytest.mark.parametrize("picks", [3, 4])
def test_gpu_spaced_exit_reads_the_picks_of_both_launches(scanned, picks):
    """List C at slices of 64 and HEAD_SPACING: every gene is cut; the first HEAD_GENES genes tile the ranges of `picks` picks,
    all others the ranges of at most 2.  From round 2 on only the head picks, and its entries of `picked` are the first
    HEAD_GENES -- where a second pick launch that numbered its genes from 0 would write its own zeros.  The host's exit reads
    the whole array: the run takes picks + 1 rounds -- no fewer, which would also cost the head a pick, and no more."""
    s = scanned
    want = _spaced_reference(s, 5, HEAD_SPACING)
    head, rest = _picks_class(want[1], (picks,)), _picks_class(want[1], (1, 2))
    assert len(head) >= 2 and len(rest) >= 2
    ids = cases.head_list(head, rest, HEAD_GENES)
    cut = cases.spaced_cut(s["total"][ids], 64)
    got, stats = _run_spaced(s, ids, 5, HEAD_SPACING, 64)
    _same(got, want, ids)
    assert cut["n_cut"] == G and HEAD_GENES <= G - MAX_ITEMS
    _spaced_stats_hold(stats, cut, want, ids, 5)
    assert stats["spaced_rounds"] == picks + 1 <= 5


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
