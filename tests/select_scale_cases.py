"""The contig, gene ranges and gene lists of tests/test_select_scale.py: one random 16 kb contig, D gene ranges cut from
the oracle's own rows, and gene lists of more than 2^20 genes that tile those ranges cyclically -- range_id = (g + start)
% D --, so that a reference costs D answers and one `take`.  The lists exist to push the selection's host driver past one
launch (crp_select.cpp: at most 2^20 items and 2^20 merges a launch); the test checks on the reference's rows, before it
looks at the device, that they do."""
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
    for start in range(len(which)):
        cut = host_cut(np.asarray(total_of_range)[tiling(which, n_genes, start)], slice_rows)
        bs = np.arange(MAX_ITEMS, cut["items"], MAX_ITEMS)
        g = np.searchsorted(cut["first_item"], bs, "right") - 1
        if bs.size and (cut["pieces"][g] > 1).all() and (cut["first_item"][g] < bs).all():
            return start
    raise AssertionError("no start offset puts a cut gene across every launch boundary")
