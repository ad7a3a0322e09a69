"""CPU reference of the greedy family sets (cropsr_amd/family_sets.py and DESIGN.md section 24 state the definition; it is
restated here).

  candidate  (gene g with family f, table row r) where r is in g and passes for g: the rows behind the selection's n_pass[g]
  cover      c(g, r) = (site_family[r] == f ? fam_cover[r] : 0) | 1 << member(g)
  greedy     covered = 0; for step 1 .. S: among f's candidates of every arena the largest gain = popcount(c & ~covered);
             ties to the higher score (its 64 bits), then the lower arena, then the smaller cut << 1 | strand of the arena
             position, then the smaller layout row.  No candidate or gain 0: stop.  Else record, covered |= c, and stop when
             covered == full_f = the low n_f bits.

An arena holds its contigs in genome order, so arena positions ascend with (contig, position): the references compare
(contig, cut << 1 | strand) and need no arena offsets.  Two candidates with one arena position lie in one contig, where layout
rows ascend with the gene's index in the GFF: the references compare the gene index.

Stated twice: `greedy_numpy` over arrays, `greedy_loop` over Python ints with the order written out as a chain of ifs.
"""
import numpy as np

NONE = 0xFFFFFFFF
FIELDS = ("family", "arena", "contig", "cut", "strand", "gene", "key", "cover", "position", "index")


def candidates(genes, gene_family, gene_member, passing, fam_ref, arena_of, key_of):
    """One tuple of FIELDS per candidate.  passing[g]: the passing rows of gene g as (contig, position, strand, the site's row
    in fam_ref, the row's index in its contig's strand table); key_of(contig, strand, index) -> the score's 64 bits."""
    out = []
    for g, rows in enumerate(passing):
        f = gene_family[g]
        if f == NONE:
            continue
        for kc, pos, strand, r, index in rows:
            assert kc == genes[g][1]
            cover = fam_ref["fam_cover"][r] if int(fam_ref["site_family"][r]) == f else 0
            cut = pos if strand else pos - 3
            out.append((f, arena_of[kc], kc, cut, strand, g, key_of(kc, strand, index), int(cover) | 1 << gene_member[g], pos, index))
    return out


def full_word(n):
    return (1 << n) - 1  # (Python ints: n = 64 is no special case here; it is on the device)


def _popcount(x):
    return bin(x).count("1")


# ---------------------------------------------------------------- numpy
def _popcount64(x):
    n = np.zeros(x.shape, np.int64)
    for b in range(64):
        n += ((x >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return n


def best_numpy(cands, covered):
    """Index into cands of the step's best candidate against `covered`, or None (no candidate, or gain 0)."""
    if not cands:
        return None
    col = lambda name, dt: np.array([c[FIELDS.index(name)] for c in cands], dtype=dt)
    gain = _popcount64(col("cover", np.uint64) & ~np.uint64(covered))
    key, tie = col("key", np.uint64), col("cut", np.int64) * 2 + col("strand", np.int64)
    order = np.lexsort((col("gene", np.int64), tie, col("contig", np.int64), col("arena", np.int64), np.iinfo(np.uint64).max - key, -gain))
    best = int(order[0])
    return best if gain[best] > 0 else None


def greedy_numpy(cands, sizes, S):
    return _greedy(cands, sizes, S, best_numpy)


# ---------------------------------------------------------------- the loop
def best_loop(cands, covered):
    best, best_gain = None, 0
    for i, c in enumerate(cands):
        _, arena, contig, cut, strand, gene, key, cover, _, _ = c
        gain = _popcount(cover & ~covered)
        if gain == 0:
            continue
        if best is None:
            take = True
        else:
            _, b_arena, b_contig, b_cut, b_strand, b_gene, b_key, _, _, _ = cands[best]
            if gain != best_gain:
                take = gain > best_gain
            elif key != b_key:
                take = key > b_key
            elif arena != b_arena:
                take = arena < b_arena
            elif contig != b_contig:
                take = contig < b_contig
            elif (cut << 1 | strand) != (b_cut << 1 | b_strand):
                take = (cut << 1 | strand) < (b_cut << 1 | b_strand)
            else:
                assert gene != b_gene  # (a total order: two candidates differ in something)
                take = gene < b_gene
        if take:
            best, best_gain = i, gain
    return best


def greedy_loop(cands, sizes, S):
    return _greedy(cands, sizes, S, best_loop)


def _greedy(cands, sizes, S, best_of):
    """(picks, complete): picks as dicts in family order, steps ascending -- the candidate's FIELDS, step, gain, covered after
    the step and tied (how many of the family's candidates had the pick's gain and key) --, complete per family."""
    picks, complete = [], []
    for f, n in enumerate(sizes):
        mine = [c for c in cands if c[0] == f]
        covered, full = 0, full_word(n)
        for step in range(1, S + 1):
            b = best_of(mine, covered)
            if b is None:
                break
            c = dict(zip(FIELDS, mine[b]))
            gain = _popcount(c["cover"] & ~covered)
            tied = sum(1 for o in mine if o[6] == c["key"] and _popcount(o[7] & ~covered) == gain)
            covered |= c["cover"]
            picks.append(dict(c, step=step, gain=gain, covered=covered, tied=tied))
            if covered == full:
                break
        complete.append(covered == full)
    return picks, complete


def arena_best(cands, sizes, covered, arena):
    """Per family the best candidate of one arena against covered[f] (a FIELDS dict with gain, or None): what one
    crp_select_family_step returns."""
    out = []
    for f in range(len(sizes)):
        mine = [c for c in cands if c[0] == f and c[1] == arena]
        b = best_loop(mine, covered[f])
        out.append(None if b is None else dict(zip(FIELDS, mine[b]), gain=_popcount(mine[b][7] & ~covered[f])))
    return out
