"""CPU reference of the per-guide specificity score of the off-target search (cropsr_amd/search.py and DESIGN.md section 15
state the definition).

The guide region is the G = T - P pattern positions outside the PAM, numbered g = 0 .. G - 1 from the PAM-distal end.  A
scheme is factor[g] and shape[n][d].  A hit with mismatches at g1 < .. < gn (n >= 1) has

    h = factor[g1] * .. * factor[gn] * shape[n][gn - g1]      (float64, left to right)
    v = rint(h * 2^30)                                        (an integer; round to nearest even)

and a query's hit_sum is the sum of v over its sites with 1 .. M mismatches.  The definition is stated twice: `values`
in numpy over arrays of masks (bit g = a mismatch at g), and `value_loop` in plain Python in the shape CRISPOR gives the
MIT score (a list of consecutive distances, their mean, three factors), which also returns h without any table.
"""
import numpy as np

import search_reference as ref

SHIFT = 30
ONE = 1 << SHIFT
# Hsu et al. 2013, the 20 position weights, PAM-distal first
W_HSU = [0, 0, 0.014, 0, 0, 0.395, 0.317, 0, 0.389, 0.079, 0.445, 0.508, 0.613, 0.851, 0.732, 0.828, 0.615, 0.804, 0.685, 0.583]


def tables(weights):
    """(factor (G,), shape (9, 32)) of the Hsu form for G = len(weights) weights."""
    G = len(weights)
    factor = np.array([1.0 - float(w) for w in weights], dtype=np.float64)
    shape = np.zeros((9, 32), dtype=np.float64)
    for n in range(9):
        for d in range(32):
            if n == 0:
                shape[n, d] = 1.0
            elif n == 1:
                shape[n, d] = 1.0 / (n * n)
            elif n - 1 <= d <= G - 1:
                shape[n, d] = 1.0 / (((float(G - 1) - d / float(n - 1)) / float(G - 1)) * 4.0 + 1.0) / float(n * n)
    return factor, shape


def values(masks, factor, shape):
    """v (uint64) of every mask, vectorised: the product takes the positions in ascending g (a position without a
    mismatch multiplies by exactly 1)."""
    masks = np.asarray(masks, dtype=np.uint64)
    G = factor.size
    bits = ((masks[:, None] >> np.arange(G, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)  # (m, G)
    n = bits.sum(axis=1)
    h = np.ones(masks.size, dtype=np.float64)
    for g in range(G):
        h = h * np.where(bits[:, g], factor[g], 1.0)
    first = np.argmax(bits, axis=1)
    last = G - 1 - np.argmax(bits[:, ::-1], axis=1)
    d = np.where(n > 0, last - first, 0)
    h = h * shape[n, d]
    return np.where(n > 0, np.rint(h * float(ONE)).astype(np.uint64), np.uint64(0))


def value_loop(mask, weights, factor=None, shape=None):
    """One mask in plain Python, the way CRISPOR writes the MIT score: (v from the tables (None without them), h from
    the mean of the consecutive distances, no table)."""
    G = len(weights)
    positions = [g for g in range(G) if (mask >> g) & 1]
    n = len(positions)
    if n == 0:
        return 0, 1.0
    # the three factors of the publication
    score1 = 1.0
    for g in positions:
        score1 = score1 * (1.0 - float(weights[g]))
    dists = [b - a for a, b in zip(positions, positions[1:])]
    if n < 2:
        score2 = 1.0
    else:
        mean = sum(dists) / float(len(dists))
        score2 = 1.0 / (((float(G - 1) - mean) / float(G - 1)) * 4.0 + 1.0)
    score3 = 1.0 / (n * n)
    h_plain = score1 * score2 * score3
    v = None
    if factor is not None:
        h = 1.0
        for g in positions:
            h = h * float(factor[g])
        h = h * float(shape[n][positions[-1] - positions[0]])
        v = int(np.rint(np.float64(h) * float(ONE)))
    return v, h_plain


def guide_positions(pattern, pam_len):
    """The pattern position of g = 0 .. G - 1: the PAM is the pattern's last pam_len letters when everything before
    them is N, else its first."""
    T = len(pattern)
    if set(pattern[:T - pam_len]) <= {"N"}:
        return list(range(T - pam_len))
    assert set(pattern[pam_len:]) <= {"N"}
    return list(range(T - 1, pam_len - 1, -1))


def search(contigs, pattern, queries, max_mm, pam_len, factor, shape):
    """The scored search: (counts (Q, M + 1), sites as search_reference.search gives them plus "mask" (bit g) and
    "value", hit_sum (Q,) as Python ints)."""
    k, pos, strand, O = ref.candidates(contigs, pattern)
    order = np.lexsort((strand, pos, k))
    k, pos, strand, O = k[order], pos[order], strand[order], O[order]
    gpos = np.array(guide_positions(pattern, pam_len), dtype=np.int64)
    w = np.uint64(1) << np.arange(gpos.size, dtype=np.uint64)
    counts = np.zeros((len(queries), max_mm + 1), dtype=np.uint32)
    fields = ref.SITE_FIELDS + ("mask", "value")
    out = {f: [] for f in fields}
    hit_sum = []
    for q, query in enumerate(queries):
        qc = np.array([ref.CODE[ord(ch)] if ch in "ACGT" else 4 for ch in query.upper()], dtype=np.uint8)
        assert all(qc[p] == 4 for p in range(len(pattern)) if p not in set(gpos.tolist())), "a base at a PAM position"
        mism = (qc[None, :] != 4) & (O != qc[None, :])  # (m, T): a non-base (4) never equals a query base
        mm = mism.sum(axis=1)
        sel = np.nonzero(mm <= max_mm)[0]
        masks = (mism[sel][:, gpos].astype(np.uint64) * w[None, :]).sum(axis=1, dtype=np.uint64)
        v = values(masks, factor, shape)
        counts[q] = np.bincount(mm[sel], minlength=max_mm + 1)[:max_mm + 1]
        for f, col in zip(fields, (np.full(sel.size, q, dtype=np.int64), k[sel], pos[sel], strand[sel], mm[sel], masks, v)):
            out[f].append(col)
        hit_sum.append(sum(int(x) for x in v.tolist()))
    sites = {f: (np.concatenate(c) if c else np.zeros(0, np.int64)) for f, c in out.items()}
    return counts, sites, hit_sum


def specificity(hit_sum):
    return [1.0 / (1.0 + float(np.float64(np.uint64(s))) / float(ONE)) for s in hit_sum]


# ---------------------------------------------------------------- the two TSV files, formatted independently
def format_sites(names, queries, contig_names, site_rows, site_strings, values_):
    """site_rows: (query, contig, position, strand 0/1, mismatches) tuples; site_strings: the oriented windows as the
    unscored TSV prints them; values_: v per row."""
    lines = ["name\tquery\tcontig\tposition\tstrand\tmismatches\tsite\thit_score\n"]
    for (q, k, pos, strand, mm), site, v in zip(site_rows, site_strings, values_):
        score = "%.6f" % (int(v) / float(ONE)) if mm > 0 else ""
        lines.append("%s\t%s\t%s\t%d\t%s\t%d\t%s\t%s\n" % (names[q], queries[q], contig_names[k], pos, "+-"[strand], mm, site, score))
    return "".join(lines)


def format_counts(names, queries, counts, hit_sum):
    lines = ["name\tquery\t" + "\t".join("mm%d" % k for k in range(counts.shape[1])) + "\thit_sum\tspecificity\n"]
    spec = specificity(hit_sum)
    for q in range(len(queries)):
        lines.append("%s\t%s\t%s\t%.6f\t%.6f\n" % (names[q], queries[q], "\t".join(str(int(c)) for c in counts[q]),
                                                  int(hit_sum[q]) / float(ONE), spec[q]))
    return "".join(lines)
