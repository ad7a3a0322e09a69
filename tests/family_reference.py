"""CPU reference of the gene families of the self search (cropsr_amd/families.py and DESIGN.md section 23 state the
definition; it is restated here).

  family file  `gene<TAB>family` per line, `#` and blank lines skipped; a family's members are the GFF genes the file
               names, in GFF order (member j is the j-th); at most 64 of them.
  owner        a candidate site of a pattern of l guide letters and a 3-letter PAM on the 3' side cuts at p + l - 3 ('+',
               forward start p) or at j ('-', forward start j).  owner(c): the smallest gene index among the genes that
               have a family and whose range [lo, hi] on c's contig contains the cut; family(c): the owner's family.
  per guide site s with family F (compared and valued as the self search does, at its M):
    fam_counts[s][k]  candidates c != s with family(c) = F at exactly k mismatches (NAG sites of an NRG pattern count)
    fam_sum[s]        the sum of the hit values of those with 1 .. M mismatches
    fam_cover[s]      bit j: member j of F is owner(s), or a candidate c != s with owner(c) = member j is a guide site
                      and has at most C mismatches
  A guide site without a family has zeros and site_family NONE.

Stated twice: `family_rows` in numpy over the candidate list of search_self_reference, `family_rows_loop` over strings,
which knows nothing of the candidates' packing: it takes windows from the contig text, counts mismatches letter by letter
and finds owners by scanning the gene list.  `selection_values` is the per-(gene, row) part.
"""
import numpy as np

import search_pair_reference as pref
import search_reference as ref
import search_score_reference as sref
import search_self_reference as selfref

NONE = 0xFFFFFFFF


# ---------------------------------------------------------------- the family file and the table
def parse(text):
    pairs = {}
    for line in text.splitlines():
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        f = line.split("\t")
        if len(f) != 2:
            raise ValueError(line)
        gene, fam = f[0].strip(), f[1].strip()
        if pairs.setdefault(gene, fam) != fam:
            raise ValueError(line)
    return pairs


def table(pairs, idents):
    """(names, gene_family [id or NONE], gene_member, sizes, unknown) for the genes `idents` in GFF order."""
    names, gene_family, gene_member, sizes = [], [], [], []
    for ident in idents:
        fam = pairs.get(ident)
        if fam is None:
            gene_family.append(NONE)
            gene_member.append(0)
            continue
        if fam not in names:
            names.append(fam)
            sizes.append(0)
        f = names.index(fam)
        gene_family.append(f)
        gene_member.append(sizes[f])
        sizes[f] += 1
    if any(s > 64 for s in sizes):
        raise ValueError("more than 64 members")
    return names, gene_family, gene_member, sizes, sorted(set(pairs) - set(idents))


# ---------------------------------------------------------------- numpy
def owners(k, pos, strand, T, genes, gene_family):
    """owner gene index per candidate, -1 for none.  genes: [(ident, contig, lo, hi)], string indices, closed."""
    cut = np.where(strand == 0, pos + T - 6, pos)
    owner = np.full(k.size, -1, dtype=np.int64)
    for g in range(len(genes) - 1, -1, -1):  # (descending: the smallest index is written last)
        if gene_family[g] == NONE:
            continue
        _, kc, lo, hi = genes[g]
        owner[(k == kc) & (cut >= lo) & (cut <= hi)] = g
    return owner


def _masks(mism):
    w = np.uint64(1) << np.arange(mism.shape[1], dtype=np.uint64)
    return (mism.astype(np.uint64) * w[None, :]).sum(axis=1, dtype=np.uint64)


def _values(value, pattern, O, s, sel, mism):
    """Hit values of guide site s (a row of O) against the candidate rows `sel` with the (sel, G) mismatch matrix."""
    if value[0] == "weights":
        factor, shape = sref.tables(value[1])
        return [int(v) for v in sref.values(_masks(mism), factor, shape).tolist()]
    _, pair, offsets, pam = value
    gset = set(sref.guide_positions(pattern, 3))
    query = "".join("ACGT"[c] if p in gset else "N" for p, c in enumerate(O[s].tolist()))
    out = []
    for i, row in zip(sel.tolist(), mism):
        site = "".join("ACGT?"[c] for c in O[i].tolist())
        out.append(pref.value_loop(query, site, pattern, 3, pair, offsets, pam) if row.any() else 0)
    return out


def family_rows(contigs, pattern, max_mm, guide_pattern, genes, gene_family, gene_member, cover_mm=0, value=None):
    """dict over the guide sites in the order of search_self_reference (contig, position, strand): sites, site_family,
    site_gene (uint32, NONE), fam_counts (n, M + 1) int64, fam_sum (Python ints, None without value), fam_cover (Python
    ints), and over all candidates: cand (k, pos, strand), cand_owner, cand_guide.  value: None, ("weights", w) or
    ("pair", pair, offsets, pam)."""
    (k, pos, strand, O), g = selfref.guide_sites(contigs, pattern, 3, guide_pattern)
    T = len(pattern)
    owner = owners(k, pos, strand, T, genes, gene_family)
    fam = np.array([gene_family[o] if o >= 0 else NONE for o in owner.tolist()], dtype=np.int64)
    member = np.array([gene_member[o] if o >= 0 else 0 for o in owner.tolist()], dtype=np.int64)
    C = O[:, :T - 3]
    gi = np.nonzero(g)[0]
    counts = np.zeros((gi.size, max_mm + 1), dtype=np.int64)
    sums, cover = [0] * gi.size, [0] * gi.size
    by_family = {f: np.nonzero(fam == f)[0] for f in set(fam.tolist()) if f != NONE}
    for r, s in enumerate(gi.tolist()):
        if fam[s] == NONE:
            continue
        cand = by_family[int(fam[s])]
        cand = cand[cand != s]
        mism = C[cand] != C[s][None, :]  # a non-base (4) never equals a guide's base
        mm = mism.sum(axis=1)
        hit = mm <= max_mm
        counts[r] = np.bincount(mm[hit], minlength=max_mm + 1)[:max_mm + 1]
        if value is not None:
            sums[r] = sum(_values(value, pattern, O, s, cand[hit], mism[hit]))
        bits = 1 << int(member[s])
        for m in np.unique(member[cand[g[cand] & (mm <= cover_mm)]]).tolist():
            bits |= 1 << int(m)
        cover[r] = bits
    return dict(sites=list(zip(k[g].tolist(), pos[g].tolist(), strand[g].tolist())),
                site_family=np.where(fam[gi] == NONE, NONE, fam[gi]).astype(np.uint32),
                site_gene=np.where(owner[gi] < 0, NONE, owner[gi]).astype(np.uint32), fam_counts=counts,
                fam_sum=None if value is None else sums, fam_cover=cover, cand=(k, pos, strand), cand_owner=owner, cand_guide=g)


# ---------------------------------------------------------------- the loop over strings
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
_SETS = dict(ref.IUPAC_SETS, N="ACGT")


def _letter(ch):  # the arena alphabet: acgtACGT, U read as A; anything else is no base
    ch = ch.upper()
    return "A" if ch == "U" else ch if ch in "ACGT" else "?"


def _windows(contigs, pattern, guide_pattern):
    """[(contig, start, strand, oriented window, a guide site)] of every candidate, by contig, start, strand."""
    T, out = len(pattern), []
    for k, c in enumerate(contigs):
        text = "".join(_letter(ch) for ch in (c.decode("latin-1") if isinstance(c, bytes) else c))
        for p in range(len(text) - T + 1):
            fwd = text[p:p + T]
            for strand, w in ((0, fwd), (1, "".join(_COMP.get(ch, "?") for ch in reversed(fwd)))):
                if all(pl == "N" or ch in _SETS[pl] for pl, ch in zip(pattern, w)):
                    guide = all(pl == "N" or ch in _SETS[pl] for pl, ch in zip(guide_pattern, w)) and "?" not in w[:T - 3]
                    out.append((k, p, strand, w, guide))
    return out


def family_rows_loop(contigs, pattern, max_mm, guide_pattern, genes, gene_family, gene_member, cover_mm=0, weights=None):
    """family_rows for value None or ("weights", w), site by site: (sites, site_family, site_gene, fam_counts (lists),
    fam_sum, fam_cover)."""
    T = len(pattern)
    G = T - 3
    wins = _windows(contigs, pattern, guide_pattern)
    owner = []
    for k, p, strand, _, _ in wins:
        cut = p + G - 3 if strand == 0 else p
        o = -1
        for gidx, (_, kc, lo, hi) in enumerate(genes):
            if gene_family[gidx] != NONE and kc == k and lo <= cut <= hi:
                o = gidx
                break
        owner.append(o)
    members = {}
    for i, o in enumerate(owner):
        if o >= 0:
            members.setdefault(gene_family[o], []).append(i)
    if weights is not None:
        factor, shape = sref.tables(weights)
    sites, site_family, site_gene, counts, sums, cover = [], [], [], [], [], []
    for s, (k, p, strand, w, guide) in enumerate(wins):
        if not guide:
            continue
        sites.append((k, p, strand))
        row, total, bits = [0] * (max_mm + 1), 0, 0
        o = owner[s]
        if o >= 0:
            bits = 1 << gene_member[o]
            for c in members[gene_family[o]]:
                if c == s:
                    continue
                other = wins[c][3]
                mm = sum(a != b for a, b in zip(w[:G], other[:G]))  # letter by letter; a '?' equals no base of a guide
                if mm > max_mm:
                    continue
                mask = 0
                for gpos in range(G):
                    if w[gpos] != other[gpos]:
                        mask |= 1 << gpos
                row[mm] += 1
                if weights is not None and mm:
                    total += sref.value_loop(mask, weights, factor, shape)[0]
                if wins[c][4] and mm <= cover_mm:
                    bits |= 1 << gene_member[owner[c]]
        site_family.append(gene_family[o] if o >= 0 else NONE)
        site_gene.append(o if o >= 0 else NONE)
        counts.append(row)
        sums.append(total)
        cover.append(bits)
    return sites, site_family, site_gene, counts, (sums if weights is not None else None), cover


# ---------------------------------------------------------------- per (gene, row)
def selection_values(g, gene_family, sizes, row_family, counts0, hit_sum, fam_counts0, fam_sum, fam_cover):
    """(outside_mm0, outside_hit_sum, members_hit, family_size) of one table row for gene g."""
    f = gene_family[g]
    size = 1 if f == NONE else sizes[f]
    if f != NONE and row_family == f:
        return counts0 - fam_counts0, hit_sum - fam_sum, bin(fam_cover).count("1"), size
    return counts0, hit_sum, 1, size


def passes_family(values, min_members=None, max_perfect_outside=None, max_hit_sum_outside=None):
    """The family limits of one (gene, row): min_members an int or "all"."""
    mm0, hs, hit, size = values
    need = size if min_members == "all" else (min_members or 0)
    return ((max_perfect_outside is None or mm0 <= max_perfect_outside) and (max_hit_sum_outside is None or hs <= max_hit_sum_outside)
            and hit >= need)
