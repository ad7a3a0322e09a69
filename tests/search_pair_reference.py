"""CPU reference of the pair-table hit score of the off-target search (cropsr_amd/search.py and DESIGN.md section 15, Pair
tables, state the definition): the CFD form, in which a mismatch costs by which query letter faces which site letter at
that position and the site's PAM letters weigh the whole hit.

`value_loop` is the definition as a plain Python loop over the letters of one query and one oriented site, with Python
floats (IEEE float64, one rounded multiply per step).  `search` finds the sites as search_reference does and scores each
hit with that loop.
"""
import numpy as np

import search_reference as ref

SHIFT = 30
ONE = 1 << SHIFT
LETTERS = "ACGT"


def guide_positions(pattern, pam_len):
    """(pattern positions of g = 0 .. G - 1, pattern position of the PAM's 5'-most letter)."""
    T = len(pattern)
    if set(pattern[:T - pam_len]) <= {"N"}:
        return list(range(T - pam_len)), T - pam_len
    assert set(pattern[pam_len:]) <= {"N"}
    return list(range(T - 1, pam_len - 1, -1)), 0


def value_loop(query, site, pattern, pam_len, pair, pam_offsets, pam):
    """v of one site.  query: T letters of ACGTN; site: the oriented window's T characters as the genome holds them after
    orientation (A, C, G, T, or anything else for a non-base); pair[g][a][b], pam_offsets and pam as the definition has
    them (pam: a flat sequence of 4^k values; ignored with no offsets)."""
    gpos, pam_at = guide_positions(pattern, pam_len)
    h = 1.0
    n = 0
    non_base = False
    for g, p in enumerate(gpos):  # g ascending
        a, b = query[p], site[p]
        if a == "N" or a == b:
            continue
        n += 1
        if b not in LETTERS:
            non_base = True
            continue
        h = h * float(pair[g][LETTERS.index(a)][LETTERS.index(b)])
    if n == 0 or non_base:
        return 0
    if len(pam_offsets):
        index = 0
        for o in pam_offsets:
            index = index * 4 + LETTERS.index(site[pam_at + o])
        h = h * float(pam[index])
    return int(np.rint(np.float64(h) * float(ONE)))


def search(contigs, pattern, queries, max_mm, pam_len, pair, pam_offsets, pam):
    """The scored search: (counts (Q, M + 1), sites as search_reference.search gives them plus "value", hit_sum (Q,) as
    Python ints)."""
    k, pos, strand, O = ref.candidates(contigs, pattern)
    order = np.lexsort((strand, pos, k))
    k, pos, strand, O = k[order], pos[order], strand[order], O[order]
    counts = np.zeros((len(queries), max_mm + 1), dtype=np.uint32)
    fields = ref.SITE_FIELDS + ("value",)
    out = {f: [] for f in fields}
    hit_sum = []
    for q, query in enumerate(queries):
        query = query.upper()
        qc = np.array([ref.CODE[ord(ch)] if ch in LETTERS else 4 for ch in query], dtype=np.uint8)
        mism = (qc[None, :] != 4) & (O != qc[None, :])
        mm = mism.sum(axis=1)
        sel = np.nonzero(mm <= max_mm)[0]
        v = []
        for i in sel.tolist():
            site = "".join("ACGT?"[c] for c in O[i].tolist())
            v.append(value_loop(query, site, pattern, pam_len, pair, pam_offsets, pam) if mm[i] else 0)
        counts[q] = np.bincount(mm[sel], minlength=max_mm + 1)[:max_mm + 1]
        for f, col in zip(fields, (np.full(sel.size, q, dtype=np.int64), k[sel], pos[sel], strand[sel], mm[sel], np.array(v, dtype=np.uint64))):
            out[f].append(col)
        hit_sum.append(sum(v))
    sites = {f: (np.concatenate(c) if c else np.zeros(0, np.int64)) for f, c in out.items()}
    return counts, sites, hit_sum


def random_table(rng, pattern, pam_len, pam_offsets):
    """(pair (G, 4, 4), pam (4^k,) or None): random, asymmetric, three decimals, with exact 0 and 1 entries among both."""
    G = len(pattern) - pam_len
    pair = np.round(rng.random((G, 4, 4)), 3)
    for g, a, b in ((1, 0, 1), (G // 2, 2, 3), (G - 1, 3, 0)):
        pair[g, a, b] = 0.0
    for g, a, b in ((0, 1, 0), (G // 2, 3, 2), (G - 1, 0, 3), (G - 2, 1, 2)):
        pair[g, a, b] = 1.0
    pam = None
    if len(pam_offsets):
        pam = np.round(rng.random(4 ** len(pam_offsets)), 3)
        pam[int(rng.integers(0, pam.size - 1))] = 0.0
        pam[-1] = 1.0
    return pair, pam
