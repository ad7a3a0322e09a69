"""CPU reference of the self search (cropsr_amd/search.py and DESIGN.md section 15, Self search, state the definition).

Every guide site of the genome is a query against every candidate site; its row counts the candidates other than itself
by mismatches and sums their values.  Stated twice:

  search_self        row by row through the given-guides references (search_reference.search, or
                     search_score_reference.search with weights): the guide sites' queries, with 1 taken off counts[0]
  search_self_pairs  directly: all pairs of guide codes and candidate codes in numpy, the self pair removed by index
"""
import numpy as np

import search_reference as ref
import search_score_reference as sref


def _sorted_candidates(contigs, pattern):
    k, pos, strand, O = ref.candidates(contigs, pattern)
    order = np.lexsort((strand, pos, k))
    return k[order], pos[order], strand[order], O[order]


def guide_sites(contigs, pattern, pam_len, guide_pattern=None):
    """(candidates as (contig, position, strand, codes), sorted by contig, position, strand; bool mask: a guide site)."""
    k, pos, strand, O = _sorted_candidates(contigs, pattern)
    gpos = np.array(sref.guide_positions(pattern, pam_len), dtype=np.int64)
    T = len(pattern)
    ok = ref._allowed(guide_pattern or pattern)
    fits = ok[np.arange(T), O].all(axis=1) if O.size else np.zeros(0, bool)
    bases = (O[:, gpos] != 4).all(axis=1) if O.size else np.zeros(0, bool)
    return (k, pos, strand, O), fits & bases


def queries_of(O, pattern, pam_len):
    """The query of every window: its guide-region letters, N at the PAM positions."""
    gset = set(sref.guide_positions(pattern, pam_len))
    return ["".join("ACGT"[c] if p in gset else "N" for p, c in enumerate(row)) for row in O.tolist()]


def guide_letters(queries, pattern, pam_len):
    lo = min(sref.guide_positions(pattern, pam_len))
    return [q[lo:lo + len(pattern) - pam_len] for q in queries]


def search_self(contigs, pattern, max_mm, pam_len, guide_pattern=None, weights=None):
    """(sites [(contig, position, strand)], guides [G letters], counts (n, M + 1) int64, hit_sum [int] or None)."""
    (k, pos, strand, O), g = guide_sites(contigs, pattern, pam_len, guide_pattern)
    queries = queries_of(O[g], pattern, pam_len)
    if weights is None:
        counts, _ = ref.search(contigs, pattern, queries, max_mm)
        hit_sum = None
    else:
        factor, shape = sref.tables(weights)
        counts, _, hit_sum = sref.search(contigs, pattern, queries, max_mm, pam_len, factor, shape)
    counts = counts.astype(np.int64).reshape(len(queries), max_mm + 1)
    counts[:, 0] -= 1  # the site itself
    assert (counts >= 0).all()
    sites = list(zip(k[g].tolist(), pos[g].tolist(), strand[g].tolist()))
    return sites, guide_letters(queries, pattern, pam_len), counts, hit_sum


def search_self_pairs(contigs, pattern, max_mm, pam_len, guide_pattern=None, weights=None, rows=128):
    """The same result from all pairs at once."""
    (k, pos, strand, O), g = guide_sites(contigs, pattern, pam_len, guide_pattern)
    gpos = np.array(sref.guide_positions(pattern, pam_len), dtype=np.int64)
    C = O[:, gpos]                      # (c, G) codes in g order; 4 = not a base
    gi = np.nonzero(g)[0]
    w = np.uint64(1) << np.arange(gpos.size, dtype=np.uint64)
    counts = np.zeros((gi.size, max_mm + 1), dtype=np.int64)
    hit_sum = None if weights is None else []
    if weights is not None:
        factor, shape = sref.tables(weights)
    for r0 in range(0, gi.size, rows):
        idx = gi[r0:r0 + rows]
        mism = C[idx][:, None, :] != C[None, :, :]   # (r, c, G): a non-base never equals a guide's base
        mm = mism.sum(axis=2)
        mm[np.arange(idx.size), idx] = max_mm + 1    # the site itself
        for r in range(idx.size):
            sel = np.nonzero(mm[r] <= max_mm)[0]
            counts[r0 + r] = np.bincount(mm[r, sel], minlength=max_mm + 1)[:max_mm + 1]
            if weights is not None:
                masks = (mism[r, sel].astype(np.uint64) * w[None, :]).sum(axis=1, dtype=np.uint64)
                hit_sum.append(sum(int(v) for v in sref.values(masks, factor, shape).tolist()))
    sites = list(zip(k[g].tolist(), pos[g].tolist(), strand[g].tolist()))
    return sites, guide_letters(queries_of(O[g], pattern, pam_len), pattern, pam_len), counts, hit_sum


def format_rows(contig_names, sites, guides, counts, hit_sum):
    """The --self TSV, formatted independently of the package."""
    M1 = counts.shape[1]
    head = ["contig", "position", "strand", "guide"] + ["n%d" % k for k in range(M1)]
    lines = ["\t".join(head + ([] if hit_sum is None else ["hit_sum", "specificity"])) + "\n"]
    spec = None if hit_sum is None else sref.specificity(hit_sum)
    for i, ((k, pos, strand), guide) in enumerate(zip(sites, guides)):
        row = [contig_names[k], "%d" % pos, "+-"[strand], guide] + ["%d" % c for c in counts[i]]
        if hit_sum is not None:
            row += ["%.6f" % (int(hit_sum[i]) / float(sref.ONE)), "%.6f" % spec[i]]
        lines.append("\t".join(row) + "\n")
    return "".join(lines)
