"""The contig, gene ranges and gene lists of tests/test_select_scale.py: one random 16 kb contig, D gene ranges cut from
the oracle's own rows, and gene lists of more than 2^20 genes that tile those ranges cyclically -- range_id = (g + start)
% D --, so that a reference costs D answers and one `take`.  The lists exist to push the selection's host driver past one
launch (crp_select.cpp: at most 2^20 items and 2^20 merges a launch); the test checks on the reference's rows, before it
looks at the device, that they do.  The helpers below the ranges serve every module that takes a launch loop past 2^20 items:
the host's cut and the spaced driver's cut restated, tilings with a cut gene across the launch boundaries, a coding model
tiled with its genes, and lists that are not cyclic (late_list, head_list) where a loop's slip would hide behind a period."""
import numpy as np

SEED, LENGTH = 77, 16000
# total rows (both strands, scored or not: the kernel's runs) of the ranges: around one, two and three pieces of 64, a few
# pieces, many pieces; and none
ROWS = (0, 1, 2, 63, 64, 65, 66, 127, 128, 129, 130, 192, 193, 200, 321, 700)
D = len(ROWS)
MAX_ITEMS = 1 << 20           # crp::SELECT_MAX_ITEMS: items, and merges, of one launch
G = MAX_ITEMS + 4099          # genes of a big list: one launch and a bit, no multiple of anything
FIRST, STRIDE = 5, 71         # where the ranges begin among the sorted cut sites: they overlap, like genes do


def contig():
    rng = np.random.default_rng(SEED)
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), LENGTH).tobytes()


def cut_sites(hits):
    """Every row's cut site -- i - 3 of a '+' row, j of a '-' row --, scored or not, both strands merged, ascending."""
    return np.sort(np.concatenate([hits["pos_plus"].astype(np.int64) - 3, hits["pos_minus"].astype(np.int64)]))


def ranges(hits):
    """(lo, hi) int64 (D,), contig positions: range j holds exactly ROWS[j] rows.  Built like select_cases.runs(): from
    the k-th cut site to the (k + n - 1)-th, k moved on until the range's ends split no two rows that share a cut site."""
    cuts = cut_sites(hits)
    lo, hi = [], []
    for j, n in enumerate(ROWS):
        k = FIRST + STRIDE * j
        if n == 0:
            while cuts[k + 1] - cuts[k] < 2:
                k += 1
            lo.append(cuts[k] + 1)
            hi.append(cuts[k + 1] - 1)
            continue
        while cuts[k - 1] == cuts[k] or cuts[k + n - 1] == cuts[k + n]:
            k += 1
        lo.append(cuts[k])
        hi.append(cuts[k + n - 1])
    lo, hi = np.array(lo, np.int64), np.array(hi, np.int64)
    assert len(set(zip(lo.tolist(), hi.tolist()))) == D
    return lo, hi


def rows_in(hits, lo, hi):
    """Rows of both runs of every range, scored or not."""
    cuts = cut_sites(hits)
    return np.searchsorted(cuts, hi, "right") - np.searchsorted(cuts, lo, "left")


def tiling(which, n_genes=G, start=0):
    """range_id (n_genes,): the ranges `which` (indices into ROWS), over and over."""
    which = np.asarray(which, np.int64)
    return which[(np.arange(n_genes) + start) % which.size]


def host_cut(total, slice_rows):
    """The host's cut of a gene list (crp_select_run, crp_select_run_pairs), restated: total[g] rows of gene g ->
    dict(pieces (G,), first_item (G,): the gene's first item, items, cut_genes, slots, slot_first (G,): the first slot of a
    cut gene, -1 otherwise).  A gene is one piece per slice_rows rows, at least one; items are in gene order; only the genes
    of more than one piece take slots, consecutive ones."""
    total = np.asarray(total, np.int64)
    pieces = np.maximum(1, -(-total // slice_rows))
    first_item = np.cumsum(pieces) - pieces
    cut = pieces > 1
    slots = np.where(cut, pieces, 0)
    slot_first = np.where(cut, np.cumsum(slots) - slots, -1)
    return dict(pieces=pieces, first_item=first_item, items=int(pieces.sum()), cut_genes=int(cut.sum()), slots=int(slots.sum()),
                slot_first=slot_first)


def boundary_start(total_of_range, which, slice_rows, n_genes=G):
    """The smallest start offset of the tiling at which every launch boundary b = 2^20, 2 * 2^20, .. below the item count
    falls inside a cut gene -- first_item[g] < b < first_item[g] + pieces[g] --, so that one gene's pieces lie in two
    launches and its slots run across the boundary."""
    which = np.asarray(which, np.int64)
    pieces = np.maximum(1, -(-np.asarray(total_of_range, np.int64)[which] // slice_rows))
    n = which.size
    for start in range(n):
        # one cycle of tiling(which, ., start) holds the pieces rolled by start; a boundary is looked up by its place in a cycle
        rot = np.roll(pieces, -start)
        first, cycle = np.cumsum(rot) - rot, int(rot.sum())
        items = (n_genes // n) * cycle + int(rot[:n_genes % n].sum())
        r = np.arange(MAX_ITEMS, items, MAX_ITEMS) % cycle
        k = np.searchsorted(first, r, "right") - 1
        if r.size and (rot[k] > 1).all() and (first[k] < r).all():
            return start
    raise AssertionError("no start offset puts a cut gene across every launch boundary")


def straddles(total, slice_rows):
    """Whether every launch boundary below the item count of the gene list with total[g] rows a gene falls inside a cut gene:
    boundary_start's condition, on the whole list by host_cut."""
    cut = host_cut(total, slice_rows)
    bs = np.arange(MAX_ITEMS, cut["items"], MAX_ITEMS)
    g = np.searchsorted(cut["first_item"], bs, "right") - 1
    return bool(bs.size and (cut["pieces"][g] > 1).all() and (cut["first_item"][g] < bs).all())


def spaced_cut(total, slice_rows):
    """The spaced driver's cut (crp_select_run_spaced), restated: the genes of one piece and the pieces of the others go into
    two lists, each in gene order, and only a cut gene has a merge entry -> dict(n_whole, n_pieces, n_cut, cut_genes (n_cut,):
    the cut genes, piece_first (n_cut,): a cut gene's first piece in the pieces list, pieces (n_cut,): its piece count)."""
    total = np.asarray(total, np.int64)
    pieces = np.maximum(1, -(-total // slice_rows))
    cut = pieces > 1
    mine = pieces[cut]
    return dict(n_whole=int((~cut).sum()), n_pieces=int(mine.sum()), n_cut=int(cut.sum()), cut_genes=np.flatnonzero(cut),
                piece_first=np.cumsum(mine) - mine, pieces=mine)


def spaced_boundary_start(total_of_range, which, slice_rows, n_genes=G):
    """boundary_start over the pieces list of spaced_cut: the smallest start offset at which every launch boundary below
    n_pieces falls inside a cut gene's pieces."""
    for start in range(len(which)):
        cut = spaced_cut(np.asarray(total_of_range)[tiling(which, n_genes, start)], slice_rows)
        bs = np.arange(MAX_ITEMS, cut["n_pieces"], MAX_ITEMS)
        j = np.searchsorted(cut["piece_first"], bs, "right") - 1
        if bs.size and (cut["piece_first"][j] < bs).all() and (bs < cut["piece_first"][j] + cut["pieces"][j]).all():
            return start
    raise AssertionError("no start offset puts a cut gene's pieces across every launch boundary of the pieces list")


def spaced_launches(cut, rounds):
    """spaced_launches of a run of `rounds` rounds, from the driver's three loops: the two key launches, the whole genes'
    launches, and per round the step launches over the pieces and the pick launches over the cut genes."""
    per = lambda n: -(-n // MAX_ITEMS)
    return 2 + per(cut["n_whole"]) + rounds * (per(cut["n_pieces"]) + per(cut["n_cut"]))


FEW_STEPS = 16  # base rows of a tiled model have at most this many steps: a row of 257 would be tiled to 10^7 steps alone


def few_steps(model):
    """The rows of a coding model that tile_model's users take as base genes: those of at most FEW_STEPS steps."""
    return np.flatnonzero(np.diff(np.asarray(model["first"], np.int64)) <= FEW_STEPS).tolist()


def tile_model(model, ids):
    """The coding model of ArenaSelect.set_coding (info, length, first, at, word, cum) for the gene list ids: row g of the
    result is base row ids[g].  info and length are taken through ids; first is the running sum of the rows' step counts;
    at, word and cum are the base rows' step slices one behind the other, because the kernels read first[g] .. first[g + 1]."""
    ids = np.asarray(ids, np.int64)
    base_first = np.asarray(model["first"], np.int64)
    steps = np.diff(base_first)[ids]
    first = np.concatenate([[0], np.cumsum(steps)])
    # step k of the result lies in row g = the row it was repeated for: its source is base_first[ids[g]] + (k - first[g])
    source = np.repeat(base_first[:-1][ids] - first[:-1], steps) + np.arange(first[-1])
    out = {key: np.asarray(model[key])[ids] for key in ("info", "length")}
    out.update({key: np.asarray(model[key])[source] for key in ("at", "word", "cum")})
    out["first"] = first.astype(np.uint64)
    return out


def late_list(base_ids, late, n_genes=G, head=MAX_ITEMS + 64):
    """A gene list that is not cyclic: positions 0 .. head - 1 tile base_ids without the genes in `late`, the rest tiles all
    of base_ids, so that every gene of `late` occurs first at a position >= head > 2^20."""
    base_ids = [int(g) for g in base_ids]
    early = [g for g in base_ids if g not in set(int(x) for x in late)]
    assert early and n_genes > head > 0
    return np.concatenate([tiling(early, head), tiling(base_ids, n_genes - head)])


def head_list(head_ids, rest_ids, n_head, n_genes=G):
    """The opposite of late_list: positions 0 .. n_head - 1 tile head_ids, the rest tiles rest_ids."""
    assert 0 < n_head < n_genes
    return np.concatenate([tiling(head_ids, n_head), tiling(rest_ids, n_genes - n_head)])


def first_occurrence(ids, n_base):
    """(n_base,) the first position of every base gene in the list ids, -1 where it does not occur."""
    ids = np.asarray(ids, np.int64)
    out = np.full(n_base, -1, np.int64)
    where = np.arange(ids.size)[::-1]
    out[ids[::-1]] = where  # (the smallest position is written last)
    return out
