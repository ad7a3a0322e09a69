"""Self selection: the K most specific guide sites of every gene, for any nuclease, chosen on the GPU.

Not in the reference, opt-in.  --select (select.py) ranks the rows of the NGG scan by their on-target
score, so it serves SpCas9 only.  The self search (search.py: search_self) is general -- any pattern of up to 32 letters, the
PAM on either side -- and leaves, per guide site of the genome, the exact mismatch counts and the specificity sum in HBM.
This module reduces those rows to "which guides do I order for this gene?", ranked by specificity, where they lie
(csrc/crp_select_self.hip).  It reads no scan tables.

Definition, per arena, on a self-search handle after all of its orders and compares -- a pattern of T letters, a PAM of P,
a guide region of G = T - P, M mismatches -- (tests/select_self_reference.py restates it twice):

  genes       select.py's: the layout rows lo[] / hi[] of crp_annotation_gene_layout, with the same genes, clipping and
              zero-row rules.
  cut offset  c, 1 <= c <= T - 1, in pattern coordinates: the cut lies before pattern position c of the oriented window.
              Default: G - 3 with the PAM on the 3' side; P + min(18, G - 1) with the PAM on the 5' side (the Cas12a cut of
              the non-target strand).  A staggered cutter is represented by this one offset.
  cut letter  of a guide site with forward start s: s + c on '+', s + T - c on '-'.  With ...NGG (T = 23) and c = 17 a '+'
              site's cut letter is section 16's i - 3.  The '-' rule is the true mirror, j + 6; section 16 keeps the
              reference's j there.
  in          only guide sites count; a candidate that is no guide site is ignored.  A site is IN a gene when lo <= cut <= hi.
  passes      a site PASSES when it is in the gene; counts[0] <= max_mm0; on a scored handle hit_sum <= max_hit_sum (the
              bound of select.max_hit_sum_for); with require_cds the CDS flag of the track interval under the cut letter is
              set (positional, as section 16's); gc_min <= GC <= gc_max, GC the popcount of the guide region's high code
              bits (A=00 T=01 C=10 G=11); and the longest run of T over the guide region is at most max_t_run.
  order       smaller e first, then the smaller cut letter, then '+' before '-': total, and independent of how the work is
              cut.  Scored handle: e = hit_sum + (counts[0] << 30) in 64 bits -- a perfect copy elsewhere weighs like a
              hit of full value 2^30.  Unscored handle: e packs saturated counts, the most significant first: counts[0]
              saturated at 65 535 in 16 bits, counts[1 .. M] saturated at 4 095 in 12 bits each, left-aligned in the 48
              bits below.
  result      per gene g: n_in[g], n_pass[g] and sel[g][0..K): the first min(K, n_pass) passing sites in that order, each
              as its candidate index in extraction order, 0xFFFFFFFF beyond.  K = 1..64.  A gene met in several texts gets
              the sums of its counts and the first K of its rows.

On-target models (ontarget.py): with a model on the search, Params(rank="on-target") orders by the model's
sum, larger first, in place of e, and Params(min_on_target=) bounds its value; every test above stays a filter, and a site
without a sum does not pass either of the two.  rank="specificity" without a bound is the selection above, bit for bit.

Limits: one device; on-target models are linear ones with adjacent pairs over one window of at most 64 letters, one
cut-independent model per run; no pairs, spacing, coding, edit, family or variant filters on this path; one representative
cut offset for staggered cutters.
"""
import numpy as np

from . import _native as nat
from . import select as sel_mod
from .properties import gc_count_bounds

MAX_K = nat.SELECT_MAX_K
NONE = nat.SELECT_NONE
NO_LIMIT = 0xFFFFFFFF  # crp_select_self_params: no bound on a count
SCORE_SHIFT = 30  # a hit's value is rint(h * 2^30) (search.py)
ROW_DTYPE = np.dtype([("gene", "<u4"), ("rank", "<u4"), ("contig", "<u4"), ("position", "<i8"), ("strand", "S1"), ("cut", "<i8")])


def default_cut(pattern_len, pam_len, pam3):
    """The default cut offset c of a pattern of T letters with a PAM of P on the 3' side (pam3) or the 5' side."""
    T, P = int(pattern_len), int(pam_len)
    G = T - P
    return G - 3 if pam3 else P + min(18, G - 1)


def check_cut(cut_offset, pattern_len, pam_len, pam3):
    """The checked cut offset (None: the default); ValueError outside 1 .. T - 1."""
    T = int(pattern_len)
    c = default_cut(T, pam_len, pam3) if cut_offset is None else cut_offset
    if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= int(c) <= T - 1:
        raise ValueError("the cut offset must be 1..%d (pattern positions of a pattern of %d letters), not %r" % (T - 1, T, c))
    return int(c)


def cut_letter(start, strand, pattern_len, cut_offset):
    """The cut letter of sites with forward starts `start` and strands `strand` (0 '+', 1 '-'): numbers or arrays."""
    start = np.asarray(start, dtype=np.int64)
    minus = np.asarray(strand).astype(bool)
    return np.where(minus, start + int(pattern_len) - int(cut_offset), start + int(cut_offset))


def scored_e(counts0, hit_sum):
    """e of a scored handle: hit_sum + (counts[0] << 30), uint64."""
    return np.asarray(hit_sum, dtype=np.uint64) + (np.asarray(counts0).astype(np.uint64) << np.uint64(SCORE_SHIFT))


def packed_e(counts):
    """e of an unscored handle from counts (n, M + 1): counts[0] saturated at 65 535 above counts[1 .. M] saturated at 4 095."""
    c = np.asarray(counts, dtype=np.uint64).reshape(-1, np.shape(counts)[-1])
    e = np.minimum(c[:, 0], np.uint64(65535)) << np.uint64(48)
    for j in range(1, c.shape[1]):
        e |= np.minimum(c[:, j], np.uint64(4095)) << np.uint64(48 - 12 * j)
    return e


def gc_bounds(pct_min, pct_max, guide_letters):
    """--select-gc-min / --select-gc-max as counts over the G guide letters: properties.gc_count_bounds' ceil / floor rule."""
    lo, hi = gc_count_bounds(pct_min, pct_max, guide_letters)
    return lo, (NO_LIMIT if pct_max is None else hi)


class Params:
    """What a self selection asks for: K, the cut offset c (None: the default of the handle's geometry, filled in by
    resolve()), max_perfect (most other perfect copies, counts[0]; None: no bound), min_specificity (None or <= 0: no bound;
    needs a scored search), require_cds, gc_min / gc_max (counts of guide letters) and max_t_run.  With an on-target model on
    the search (search_self(on_target=), ontarget.py): rank, "specificity" (the order above) or "on-target" (larger sum first,
    then the smaller cut letter, then '+' before '-'; a site without a sum does not pass), and min_on_target, a bound on the
    model's VALUE (a site passes only with a sum, and a value at least this), converted once to a bound on the sum --
    min_sum -- by bind_model()."""

    RANKS = ("specificity", "on-target")

    def __init__(self, k, cut_offset=None, max_perfect=None, min_specificity=None, require_cds=False, gc_min=None, gc_max=None,
                 max_t_run=None, rank="specificity", min_on_target=None):
        if rank not in self.RANKS:
            raise ValueError("rank is specificity or on-target, not %r" % (rank,))
        self.rank, self.min_on_target, self.min_sum = rank, min_on_target, None
        if min_on_target is not None and (isinstance(min_on_target, bool) or not isinstance(min_on_target, (int, float, np.integer, np.floating))
                                          or float(min_on_target) != float(min_on_target)):
            raise ValueError("min_on_target is a number, not %r" % (min_on_target,))
        self.k = int(k)
        if not 1 <= self.k <= MAX_K:
            raise ValueError("K must be 1..%d, not %d" % (MAX_K, self.k))
        self.cut_offset = cut_offset
        self.max_mm0 = sel_mod.NO_BOUND_MM0 if max_perfect is None else int(max_perfect)
        if not 0 <= self.max_mm0 <= sel_mod.NO_BOUND_MM0:
            raise ValueError("max_perfect must be a count, not %r" % (max_perfect,))
        self.max_hit_sum = sel_mod.NO_BOUND_SUM if min_specificity is None else sel_mod.max_hit_sum_for(min_specificity)
        self.needs_score = min_specificity is not None and float(min_specificity) > 0.0
        self.require_cds = bool(require_cds)
        vals = []
        for name, v, default in (("gc_min", gc_min, 0), ("gc_max", gc_max, NO_LIMIT), ("max_t_run", max_t_run, NO_LIMIT)):
            v = default if v is None else int(v)
            if not 0 <= v <= 0xFFFFFFFF:
                raise ValueError("%s must be a count, not %r" % (name, v))
            vals.append(v)
        self.gc_min, self.gc_max, self.max_t_run = vals
        if self.gc_min > self.gc_max:
            raise ValueError("gc_min %d is above gc_max %d" % (self.gc_min, self.gc_max))

    def resolve(self, pattern_len, pam_len, pam3):
        """The same Params with the cut offset checked against the pattern (None: its default)."""
        self.cut_offset = check_cut(self.cut_offset, pattern_len, pam_len, pam3)
        return self

    @property
    def uses_model(self):
        return self.rank == "on-target" or self.min_on_target is not None

    def bind_model(self, model):
        """Checks rank and min_on_target against the search's ontarget.Model (None: no model) and converts the bound on the
        value to min_sum, the bound on the sum: itself under identity, log(x / (1 - x)) under logistic, where it must lie in
        (0, 1).  ValueError otherwise."""
        from . import ontarget
        if model is None:
            if self.uses_model:
                raise ValueError("%s needs an on-target model (on_target=)" % ("rank on-target" if self.rank == "on-target" else "min_on_target"))
            return self
        self.min_sum = None if self.min_on_target is None else ontarget.min_sum(self.min_on_target, model.link)
        return self

    def native(self):
        return nat.SelectSelfParams(self.max_hit_sum, self.max_mm0, self.k, int(self.cut_offset), int(self.require_cds), self.gc_min,
                                    self.gc_max, self.max_t_run, 0)


class Request:
    """A self selection for search.search_self(select=): Params, the annotate.Request that names the genes (its names are
    the contigs' FASTA names, in the genome's order), and the work limits -- slice_rows (None: the library's default) and
    items_per_launch (None: 2^20); results depend on neither."""

    def __init__(self, params, annotation, slice_rows=None, items_per_launch=None):
        self.params, self.annotation, self.slice_rows, self.items_per_launch = params, annotation, slice_rows, items_per_launch


class Selection:
    """The self selection over all genes of the GFF, in file order: labels, n_in, n_pass (per gene) and, of the selected
    sites, gene after gene, rank 1 first: rows (ROW_DTYPE: position and cut are local to the contig string, 0-based), guides
    (S<G>), counts (n, M + 1) uint32, hit_sum (n,) uint64 and specificity (n,) float64 (both None when unscored), e (n,) uint64
    (the specificity ranking's key), and stats (the handles' kernel times and launch counts, summed over the arenas).  With an
    on-target model on the search: on_target_sum (n,) float64 (NaN: the site has none) and on_target (n,), its value under the
    model's link; both None without a model."""

    def __init__(self, labels, n_in, n_pass, rows, guides, counts, hit_sum, e, stats=None, on_target_sum=None, link=None):
        from .search import specificity
        self.labels, self.n_in, self.n_pass, self.rows, self.guides, self.counts = labels, n_in, n_pass, rows, guides, counts
        self.hit_sum, self.e, self.stats = hit_sum, e, stats or {}
        self.specificity = None if hit_sum is None else specificity(hit_sum)
        self.on_target_sum = self.on_target = None
        if on_target_sum is not None and link is not None:
            from . import ontarget
            self.on_target_sum, self.on_target = on_target_sum, ontarget.value(on_target_sum, link)

    def of_gene(self, g):
        return self.rows[self.rows["gene"] == g]


def select_arena(genome, a, request, handle, flags=None):
    """The self selection of one arena of an engine.Genome: (gene -- layout row -> gene index --, fetch_self()'s dict,
    self_stats()).  handle: the arena's search.ArenaSelfSearch after all of its orders and compares."""
    layout = sel_mod.arena_layout(genome, a)
    lo, hi, gene = request.annotation.gene_layout(layout)
    sel = sel_mod.ArenaSelect(genome.arenas[a], lo, hi)
    try:
        if request.params.require_cds:
            genome.arenas[a].annotate_set_track(*request.annotation.track(layout))
            sel.set_flags(flags if flags is not None else request.annotation.annotation.cds_flags())
        if request.slice_rows:
            sel.set_limits(request.slice_rows)
        if request.items_per_launch:
            sel.set_self_limits(request.items_per_launch)
        p = request.params
        if p.uses_model:
            if p.min_on_target is not None and p.min_sum is None:
                raise ValueError("min_on_target has not been converted to a bound on the sum (Params.bind_model)")
            sel.set_self_model(p.rank == "on-target", p.min_sum)
        sel.run_self(p, handle)
        got = sel.fetch_self()
        got["on_target_sum"] = sel.fetch_self_model()
        return gene, got, sel.self_stats()
    finally:
        sel.close()


def assemble(labels, k, pattern_len, cut_offset, region_lo, guide_letters, scored, arenas, rank="specificity", link=None):
    """One Selection from per-arena results.  arenas: dicts with offsets / lengths (of the arena's texts), group (their contig
    indices), gene (layout row -> gene index) and fetch_self()'s arrays.  A gene that has rows in several texts gets the sums of
    its counts and the first K of its rows in the definition's order, texts in arena order.  rank "on-target": the order is by
    the on-target sum, larger first, in place of e.  link: the search's model's (None: no model; the arenas' on_target_sum is
    then not read)."""
    from . import ontarget
    from .search import _guide_letters
    G = len(labels)
    n_in, n_pass = np.zeros(G, np.int64), np.zeros(G, np.int64)
    parts, gparts, cparts, sparts, eparts, tparts, aparts, mparts = [], [], [], [], [], [], [], []
    stride = 1
    for a_index, a in enumerate(arenas):
        gene = np.asarray(a["gene"], dtype=np.int64)
        np.add.at(n_in, gene, np.asarray(a["n_in"], dtype=np.int64))
        np.add.at(n_pass, gene, np.asarray(a["n_pass"], dtype=np.int64))
        sel = np.asarray(a["sel"], dtype=np.uint32).reshape(gene.size, -1)[:, :k]
        r, c = np.nonzero(sel != NONE)
        pos = np.asarray(a["arena_pos"]).reshape(gene.size, -1)[r, c].astype(np.int64)
        strand = np.asarray(a["strand"]).reshape(gene.size, -1)[r, c]
        counts = np.asarray(a["counts"], dtype=np.uint32)
        stride = counts.shape[-1]
        counts = counts.reshape(gene.size, -1, stride)[r, c]
        sums = np.asarray(a["hit_sum"], dtype=np.uint64).reshape(gene.size, -1)[r, c]
        offs = np.asarray(a["offsets"], dtype=np.int64)
        t = np.searchsorted(offs, pos, "right") - 1
        part = np.empty(r.size, ROW_DTYPE)
        part["gene"], part["rank"] = gene[r], c + 1
        part["contig"] = np.asarray(a["group"], dtype=np.uint32)[t] if r.size else 0
        part["position"] = pos - offs[t]
        part["strand"] = np.where(strand != 0, b"-", b"+")
        cut = cut_letter(pos, strand, pattern_len, cut_offset)
        part["cut"] = cut - offs[t]
        parts.append(part)
        gparts.append(_guide_letters(np.asarray(a["hi"]).reshape(gene.size, -1)[r, c], np.asarray(a["lo"]).reshape(gene.size, -1)[r, c],
                                     region_lo, guide_letters))
        cparts.append(counts)
        sparts.append(sums)
        eparts.append(scored_e(counts[:, 0], sums) if scored else packed_e(counts))
        tparts.append((cut.astype(np.uint64) << np.uint64(1)) | (strand != 0).astype(np.uint64))
        aparts.append(np.full(r.size, a_index, np.int64))
        if link is not None:
            mparts.append(np.asarray(a["on_target_sum"], dtype=np.float64).reshape(gene.size, -1)[r, c])
    msum = (np.concatenate(mparts) if mparts else np.empty(0, np.float64)) if link is not None else None
    rows = np.concatenate(parts) if parts else np.empty(0, ROW_DTYPE)
    guides = np.concatenate(gparts) if gparts else np.empty(0, "S%d" % guide_letters)
    counts = np.concatenate(cparts) if cparts else np.empty((0, stride), np.uint32)
    sums = np.concatenate(sparts) if sparts else np.empty(0, np.uint64)
    e = np.concatenate(eparts) if eparts else np.empty(0, np.uint64)
    tie = np.concatenate(tparts) if tparts else np.empty(0, np.uint64)
    arena_of = np.concatenate(aparts) if aparts else np.empty(0, np.int64)
    # genes in file order; a gene met in several texts: its rows by e; on equal e the texts in genome order -- the arenas in
    # order, and inside an arena the cut letter, which ascends with the texts -- then '+' before '-'.  (A cut letter is an
    # arena position: it is only compared inside one arena, so the order does not depend on how the genome was cut into arenas.)
    # Ranked by the model, the on-target sum takes e's place: larger first (~key ascends as the sum descends).
    if rank == "on-target":
        if msum is None:
            raise ValueError("rank on-target needs the model's link and the arenas' on_target_sum")
        first = ~ontarget.sort_key(msum)
    else:
        first = e
    order = np.lexsort((tie, arena_of, first, rows["gene"]))
    rows, guides, counts, sums, e = rows[order], guides[order], counts[order], sums[order], e[order]
    start = np.searchsorted(rows["gene"], rows["gene"], "left")
    at = np.arange(rows.size) - start
    keep = at < k
    rows = rows[keep]
    rows["rank"] = at[keep] + 1
    return Selection(list(labels), n_in, n_pass, rows, guides[keep], counts[keep], sums[keep] if scored else None, e[keep],
                     on_target_sum=None if msum is None else msum[order][keep], link=link)


def format_selection(contig_names, selection):
    """The selection file, as text: tab-separated gene, rank, passing, contig, position, strand, guide, cut, n0 .. nM and, when
    scored, hit_sum (as a sum of hit scores, hit_sum / 2^30) and specificity.  Genes in GFF order; a gene with nothing selected
    has no line.  With an on-target model every row ends with on_target: repr of the value, empty for a site without a sum."""
    M1 = selection.counts.shape[1]
    head = ["gene", "rank", "passing", "contig", "position", "strand", "guide", "cut"] + ["n%d" % j for j in range(M1)]
    scored = selection.hit_sum is not None
    model = selection.on_target is not None
    lines = ["\t".join(head + (["hit_sum", "specificity"] if scored else []) + (["on_target"] if model else []))]
    for i, row in enumerate(selection.rows):
        g = int(row["gene"])
        f = [selection.labels[g], str(int(row["rank"])), str(int(selection.n_pass[g])), contig_names[int(row["contig"])],
             str(int(row["position"])), row["strand"].decode(), selection.guides[i].decode(), str(int(row["cut"]))]
        f += [str(int(v)) for v in selection.counts[i]]
        if scored:
            f += ["%.6f" % (float(selection.hit_sum[i]) / float(1 << SCORE_SHIFT)), "%.6f" % float(selection.specificity[i])]
        if model:
            v = float(selection.on_target[i])
            f.append("" if v != v else repr(v))
        lines.append("\t".join(f))
    return "\n".join(lines) + "\n"
