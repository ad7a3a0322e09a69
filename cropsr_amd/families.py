"""Gene families: homeolog-aware specificity of the self search (csrc/crp_search_family.hip).

Crop genomes are polyploid or full of recent duplications: almost every good guide of a gene has a perfect copy in the
gene's homeologs, and a knock-out is meant to cut them all.  The self search counts those copies as off-targets.  With
a family table the self search also says where a near copy lies, so that the copies inside the guide's own family can be
told from the ones outside.

Definitions (tests/family_reference.py restates them twice):

  family file  text, one `gene<TAB>family` pair per line; `#` lines and blank lines are skipped.  `gene` is the identifier
               the selection file prints after `gene:` (the gene's label without that prefix), `family` any token.  A
               family's members are the GFF genes the file names, in GFF file order: member j is the j-th of them.
               Refused: a gene named twice with different families, a line without exactly two fields, a family with
               more than 64 known members (the cover set is one 64-bit word per site).  Names the GFF does not hold are
               counted (FamilyTable.n_unknown), not fatal: orthogroup files cover more than one annotation.  A family of
               one known member is valid: its inside is the gene's own internal repeats.
  owner        a candidate site of a self-search handle whose pattern is l guide letters and a PAM of 3 on the 3' side
               cuts by the selection's rule: a '+' site with forward start p at p + l - 3, a '-' site with forward start
               j at j.  owner(c) is the smallest gene index, in GFF order, among the genes that belong to a family and
               whose clipped range [lo, hi] (Annotation.gene_layout) contains that cut site; NONE without one.
               family(c) is the owner's family.
  per guide site s with F = family(s) != NONE, candidates compared exactly as the self search compares them (the same
  masked words, the same hit value, the same scheme, the handle's own M):
    fam_counts[s][k], k = 0 .. M: the candidates c != s with family(c) = F and exactly k mismatches against s.  Candidates
               of every arena count, and the NAG sites of an NRG candidate pattern count as they do in `counts`.
    fam_sum[s]   the sum of the hit values of those with 1 .. M mismatches.
    fam_cover[s] 64 bits: bit j is set iff member j is owner(s), or some candidate c != s with owner(c) = member j is
               itself a guide site (it has a working NGG) and has at most C mismatches; C is the cover limit, 0 <= C <= M,
               default 0.
  A site that is not a guide site, or whose family is NONE, has all-zero counts, sum 0, cover 0 and site_family NONE.
  fam_counts[s][k] <= counts[s][k] and fam_sum[s] <= hit_sum[s]: both are integer sums over a subset with the same value
  function, so what lies OUTSIDE the family is the exact, never negative difference:
    outside_mm0 = counts[0] - fam_counts[0]      outside_hit_sum = hit_sum - fam_sum
    members_hit = popcount(fam_cover)            outside_specificity = search.specificity(outside_hit_sum)

This module holds the parser, the family table against an annotation's gene list and the per-arena rows the device takes.
"""
import numpy as np

NONE = 0xFFFFFFFF
MAX_MEMBERS = 64
LABEL_PREFIX = "gene:"


class FamilyInputError(ValueError):
    """A family file or table outside the definition."""


def parse_families(text):
    """[(gene, family)] of a family file's text (str or bytes), in file order, each gene once.  Refuses a line without
    exactly two tab-separated fields and a gene named twice with different families."""
    if isinstance(text, bytes):
        text = text.decode("utf-8", "replace")
    pairs, seen = [], {}
    for no, line in enumerate(text.splitlines(), 1):
        line = line.rstrip("\r")
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        fields = [f.strip() for f in line.split("\t")]
        if len(fields) != 2 or not fields[0] or not fields[1]:
            raise FamilyInputError("family file line %d: expected gene<TAB>family, got %r" % (no, line))
        gene, fam = fields
        if gene in seen:
            if seen[gene] != fam:
                raise FamilyInputError("family file line %d: gene %s is in family %s and in family %s" % (no, gene, seen[gene], fam))
            continue
        seen[gene] = fam
        pairs.append((gene, fam))
    return pairs


def read_families(path):
    try:
        with open(path, "rb") as f:
            return parse_families(f.read())
    except OSError as e:
        raise FamilyInputError("cannot read the family file %s: %s" % (path, e.strerror or e))


class FamilyTable:
    """The families of a gene list.  labels: the genes' labels in GFF order ("gene:<ident>", Annotation.genes()[0]).

    names        family tokens, in order of their first member in the GFF; a family's id is its index here
    gene_family  (genes,) uint32: the gene's family id, NONE for a gene in no family
    gene_member  (genes,) uint32: the gene's bit in its family's cover word (0 for a gene in no family)
    size         (families,) uint32: known members
    n_unknown    names of the file that the gene list does not hold
    A label that several GFF rows share names all of them."""

    def __init__(self, pairs, labels):
        want = dict(pairs)
        idents = [l[len(LABEL_PREFIX):] if l.startswith(LABEL_PREFIX) else l for l in labels]
        known = set(idents)
        self.n_unknown = sum(1 for g in want if g not in known)
        self.names, ids = [], {}
        n = len(idents)
        self.gene_family = np.full(n, NONE, dtype=np.uint32)
        self.gene_member = np.zeros(n, dtype=np.uint32)
        size = []
        for g, ident in enumerate(idents):
            fam = want.get(ident)
            if fam is None:
                continue
            f = ids.get(fam)
            if f is None:
                f = ids[fam] = len(self.names)
                self.names.append(fam)
                size.append(0)
            if size[f] >= MAX_MEMBERS:
                raise FamilyInputError("family %s has more than %d members in the annotation: the cover set is one 64-bit word "
                                       "per site" % (fam, MAX_MEMBERS))
            self.gene_family[g] = f
            self.gene_member[g] = size[f]
            size[f] += 1
        self.size = np.asarray(size, dtype=np.uint32)
        self.labels = list(labels)

    def family_size(self, g):
        """|f(g)|, 1 for a gene in no family."""
        f = int(self.gene_family[g])
        return 1 if f == NONE else int(self.size[f])

    def family_name(self, g):
        f = int(self.gene_family[g])
        return "" if f == NONE else self.names[f]

    def members(self, f):
        """Gene indices of family f, in member order."""
        return np.nonzero(self.gene_family == np.uint32(f))[0]

    def member_labels(self, g, cover):
        """Labels of the members of g's family whose bits are set in `cover`, GFF order."""
        f = int(self.gene_family[g])
        if f == NONE:
            return []
        return [self.labels[m] for j, m in enumerate(self.members(f).tolist()) if (int(cover) >> j) & 1]


class ArenaRows:
    """The family genes of one arena as crp_search_self_set_families takes them, in GFF order: lo, hi (closed ranges of
    arena positions), family, member (uint32) and gene (index into the gene list)."""

    def __init__(self, lo, hi, family, member, gene):
        self.lo, self.hi, self.family, self.member, self.gene = lo, hi, family, member, gene

    def __len__(self):
        return int(self.lo.size)


def arena_rows(table, lo, hi, gene):
    """ArenaRows from Annotation.gene_layout's (lo, hi, gene) of one arena: the rows of genes that have a family, ordered by
    gene index (stable: a gene that two texts of the arena hold keeps both rows)."""
    gene = np.asarray(gene, dtype=np.int64)
    fam = table.gene_family[gene] if gene.size else np.zeros(0, np.uint32)
    keep = np.nonzero(fam != np.uint32(NONE))[0]
    keep = keep[np.argsort(gene[keep], kind="stable")]
    g = gene[keep]
    return ArenaRows(np.ascontiguousarray(np.asarray(lo, np.uint32)[keep]), np.ascontiguousarray(np.asarray(hi, np.uint32)[keep]),
                     np.ascontiguousarray(table.gene_family[g]), np.ascontiguousarray(table.gene_member[g]), g.astype(np.uint32))


def genome_rows(table, genome, request):
    """One ArenaRows per arena of an engine.Genome (annotate.Request for its contigs)."""
    from .select import arena_layout
    return [arena_rows(table, *request.gene_layout(arena_layout(genome, a))) for a in range(len(genome.arenas))]


def popcount64(x):
    x = np.asarray(x, dtype=np.uint64)
    n = np.zeros(x.shape, dtype=np.uint32)
    for k in range(64):
        n += ((x >> np.uint64(k)) & np.uint64(1)).astype(np.uint32)
    return n


def outside(counts, hit_sum, fam_counts, fam_sum, fam_cover):
    """(outside_mm0 uint32, outside_hit_sum uint64 or None, members_hit uint32) of rows whose family columns apply."""
    mm0 = counts[:, 0] - fam_counts[:, 0]
    hs = None if hit_sum is None else hit_sum - fam_sum
    return mm0, hs, popcount64(fam_cover)
