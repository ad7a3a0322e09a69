"""--family-sets S: the fewest guides that together cut every member of a gene family (DESIGN.md section 24;
csrc/crp_select_family_set.hip).

A polyploid's homeologs drift apart, and then no single guide cuts all of them: the per-gene selection with
`min_members="all"` comes back empty for such a family.  The question is which few guides TOGETHER cut every copy -- the
multiplex design problem.  It is a set cover, answered greedily here, on the columns the family selection already has in
HBM.

Definition (tests/family_set_reference.py restates it twice).  Take a families.FamilyTable and a select.Request whose
self-search handles carry the family join.  Family f has n_f known members; full_f is the word with the low n_f bits set
(all ones for n_f = 64).

  candidate  a pair (layout row g of an arena's crp_select handle, table row r) where g's gene has a family f != NONE and r
             is IN g and PASSES for g exactly as crp_select_run counts n_pass for g with the handle's limits in force:
             select.py's predicate, the property and repair limits, and the family limits where set.  The candidates of g
             are the rows behind n_pass[g].
  cover      c(g, r) = (site_family[r] == f ? fam_cover[r] : 0) | 1 << member(g).  The row cuts inside g, so g's own bit
             is always in c.  A row that an overlapping gene of another family owns covers g alone.  A row inside two
             overlapping members of one family is a candidate for each of them, with both bits set.  This is NOT the
             cover word of the family selection (crp_select_family_eval), which lacks the own-bit term.
  greedy set covered = 0.  For step t = 1 .. S: among f's candidates of EVERY arena take the one with the largest
             gain = popcount(c & ~covered); ties go to the higher score (its 64 bits, unsigned), then to the lower arena
             index, then to the smaller cut << 1 | strand (select.py's tie), then to the smaller layout row.  Stop before
             picking when there is no candidate or the best gain is 0.  Otherwise record the pick, covered |= c, and stop
             once covered == full_f: the family is then COMPLETE.  Integer arithmetic and a total order: the result is
             exact and does not depend on how the work is cut.
  steps      S = 1 .. 64.

Per pick the result carries family, step, gene, contig, position, strand, score and index (as select.ROW_DTYPE), gain, the
cover word c and covered after the step (select.FAMILY_SET_DTYPE); per family, whether it is complete.

Greedy, not optimal; one set per family and no alternatives; every member within the cover limit counts the same.

One step in one arena is two kernel launches (crp_select_family_step).  The merge over the arenas stays on the host on
purpose: homeologs lie on different chromosomes, hence in different arenas for a big genome, and a step's traffic is one
32-byte record per family and arena.
"""
import numpy as np


def full_words(sizes):
    """full_f per family: the low n_f bits set (n_f = 64: all ones, without a shift by 64)."""
    n = np.asarray(sizes, dtype=np.uint64)
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    return np.where(n >= 64, ones, (np.uint64(1) << np.minimum(n, np.uint64(63))) - np.uint64(1)).astype(np.uint64)


def merge_arenas(proposals):
    """(arena index per family, the winning records) of the arenas' proposals for one step (a list of arrays of
    _native.FAMILY_STEP_BEST_DTYPE, one per arena): larger gain, then higher key; a full tie stays with the lower arena."""
    best = proposals[0].copy()
    arena = np.zeros(best.size, np.int64)
    for a in range(1, len(proposals)):
        p = proposals[a]
        better = (p["gain"] > best["gain"]) | ((p["gain"] == best["gain"]) & (p["gain"] > 0) & (p["key"] > best["key"]))
        best[better] = p[better]
        arena[better] = a
    return arena, best


def family_sets(genome, request, handle_of, hits, flags=None):
    """The greedy sets of request.families over the resident tables of `genome` (engine.Genome) after its last scan at
    guide length 20, whose host copies `hits` (GenomeHits) holds.  handle_of(arena index) -> the arena's joined
    search.ArenaSelfSearch with the family join.  One ArenaSelect per arena stays open over all steps, so every arena's
    plan is built once.  Returns (picks select.FAMILY_SET_DTYPE -- families in table order, steps ascending --, complete
    bool per family, stats); stats["outside_mm0"] and stats["outside_hit_sum"] hold, pick by pick, what the guide hits outside
    the family of the gene it was picked for (crp_select_family_eval)."""
    from . import select as sel
    table, S = request.families, int(request.family_sets)
    F = len(table.names)
    full = full_words(table.size)
    covered = np.zeros(F, np.uint64)
    stats = dict(steps=0, step_ms=0.0, pick_ms=0.0, plan_builds=0.0, items=0.0, rows_in_runs=0.0, step_ms_per_step=[], pick_ms_per_step=[])
    opened, picks, where = [], [], []
    try:
        for a in range(len(genome.arenas)):
            lo, hi, gene = request.annotation.gene_layout(sel.arena_layout(genome, a))
            s = sel.ArenaSelect(genome.arenas[a], lo, hi)
            opened.append((s, np.asarray(gene, dtype=np.int64)))
            sel._set_row_limits(s, request, flags)
            sel._set_families(s, request, gene)
            g = np.asarray(gene, dtype=np.int64)
            s.set_family_members(table.gene_member[g] if g.size else np.zeros(0, np.uint32))
        for step in range(1, S + 1):
            if not F:
                break
            proposals = [s.family_step(request.params, handle_of(a), covered) for a, (s, _) in enumerate(opened)]
            one = [s.family_step_stats() for s, _ in opened]
            stats["step_ms_per_step"].append(sum(o["step_ms"] for o in one))
            stats["pick_ms_per_step"].append(sum(o["pick_ms"] for o in one))
            stats["steps"] = step
            arena, best = merge_arenas(proposals)
            took = np.nonzero(best["gain"] > 0)[0]
            if not took.size:
                break
            covered[took] |= best["cover"][took]
            part = np.empty(took.size, sel.FAMILY_SET_DTYPE)
            part["family"], part["step"] = took, step
            part["gain"], part["cover"], part["covered"] = best["gain"][took], best["cover"][took], covered[took]
            for a, (s, gene) in enumerate(opened):
                here = np.nonzero(arena[took] == a)[0]
                if not here.size:
                    continue
                h = hits.per_arena[a]
                packed = best["row"][took[here]]
                minus = (packed >> np.uint32(31)).astype(bool)
                row = (packed & np.uint32(0x7FFFFFFF)).astype(np.int64)
                offs = np.asarray(genome.arenas[a].offsets, dtype=np.int64)
                pos = sel._take(h.pos_plus, h.pos_minus, minus, row, np.int64)
                t = np.searchsorted(offs, pos, "right") - 1
                first_plus = np.searchsorted(np.asarray(h.pos_plus), offs.astype(np.uint32), "left")
                first_minus = np.searchsorted(np.asarray(h.pos_minus), offs.astype(np.uint32), "left")
                part["gene"][here] = gene[best["gene"][took[here]].astype(np.int64)]
                part["contig"][here] = np.asarray(genome.groups[a], dtype=np.uint32)[t]
                part["position"][here] = pos - offs[t]
                part["strand"][here] = np.where(minus, b"-", b"+")
                part["score"][here] = sel._take(h.score_plus, h.score_minus, minus, row, np.float64)
                part["index"][here] = row - np.where(minus, first_minus[t], first_plus[t])
            picks.append(part)
            where.append(np.stack([arena[took], best["gene"][took].astype(np.int64), best["row"][took].astype(np.int64)], axis=1))
        # what lies outside the family, for the picks: the family selection's values of (layout row, table row), from its kernel
        out = np.concatenate(picks) if picks else np.empty(0, sel.FAMILY_SET_DTYPE)
        where = np.concatenate(where) if where else np.empty((0, 3), np.int64)
        outside_mm0, outside_hit_sum = np.zeros(out.size, np.uint32), np.zeros(out.size, np.uint64)
        for a, (s, _) in enumerate(opened):
            here = np.nonzero(where[:, 0] == a)[0]
            if here.size:
                got = s.family_eval(handle_of(a), where[here, 1].astype(np.uint32), where[here, 2].astype(np.uint32))
                outside_mm0[here], outside_hit_sum[here] = got[0], got[1]
        for s, _ in opened:
            one = s.family_step_stats()
            stats["plan_builds"] += one["plan_builds"]
            stats["items"] += one["items"]
            stats["rows_in_runs"] += one["rows_in_runs"]
            stats["bytes_per_row"] = one["bytes_per_row"]
    finally:
        for s, _ in opened:
            s.close()
    stats["step_ms"], stats["pick_ms"] = sum(stats["step_ms_per_step"]), sum(stats["pick_ms_per_step"])
    order = np.lexsort((out["step"], out["family"]))
    stats["outside_mm0"], stats["outside_hit_sum"] = outside_mm0[order], outside_hit_sum[order]
    return out[order], covered == full, stats
