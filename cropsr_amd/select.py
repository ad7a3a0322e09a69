"""--select K: the best K guides of every gene, chosen on the GPU.

Not in the reference, opt-in.  The guide table ends as one row per PAM hit; the question "which guides do I order for
this gene?" is a reduction of it, and it is computed where the columns already are: a segmented top-K over runs of the
resident hit tables (csrc/crp_select.hip).

Definition, per arena, after a crp_scan_score at guide length 20 (tests/select_reference.py restates it twice):

  genes     the GFF rows crp_annotation.cpp accepts with type `gene`, in file order.  A gene's label is the
            "gene:<ident>" text the annotation join prints, without the Phytozome suffix.  Its range [start, end]
            (1-based, closed) is mapped to arena positions by the rule of crp_annotation_track -- string index =
            coordinate + dec - 1, plus the text's arena offset -- and clipped to the text.  A gene has NO RANGE when
            start > end, when its seqid names no contig of the arena, or when clipping leaves nothing: it is still
            listed, with zero rows.  Genes may overlap, nest or repeat; each is selected for on its own, so a row may
            be chosen for several genes.
  cut site  of a row: i - 3 on the '+' table, j on the '-' table (as annot_lookup_kernel); only rows whose score is
            not -1 have one.
  in        a row is IN a gene when it has a cut site and lo <= cut site <= hi.  The tables ascend in position, so a
            gene's rows are one contiguous run per strand table.
  passes    a row PASSES when it is in the gene; its score >= min_score (float64); with joined specificity columns it
            is joined (counts[0] != 0xFFFFFFFF), counts[0] <= max_mm0 and hit_sum <= max_hit_sum (integer compares);
            with require_cds the flag byte of its label-set id is non-zero (NO_FEATURE fails; the flag is 1 for a
            label-set string that holds a `CDS:` label, computed on the host from the string table); and with property
            limits (properties.py) gc_min <= gc <= gc_max, run <= max_run, t_run <= max_t_run and stem <= max_stem; and
            with repair limits (repair.py) mh >= min_mh and 100 oof >= min_oof mh, and mh > 0 where min_oof > 0.
  order     among passing rows: higher score first -- scores are positive finite doubles, so their bit patterns order
            as unsigned 64-bit integers --, ties (repeats give identical 30-mers) by smaller cut site, then '+' before
            '-'.  The order is total: the result does not depend on how the work was cut.
  result    per gene g, all exact: n_in[g] (rows in the gene), n_pass[g] (passing rows) and sel[g][0..K): the first
            min(K, n_pass) passing rows in that order, each as row index | strand << 31, 0xFFFFFFFF beyond.  K = 1..64.

Guide pairs (csrc/crp_select_pairs.hip; tests/select_pairs_reference.py restates it twice): two
guides in one array that cut out the piece between them.  Per arena, after a scan at guide length 20, for the genes of
the same handle:

  eligible  the rows that PASS for gene g, as above: membership by the cut site, i - 3 or j, in [lo, hi]; the predicate is
            the full current one (min_score, joined columns, require_cds, property limits, repair limits).
  boundary  c of a row, as repair.py defines it and NOT the CSV's `cutsite`: c = i - 3 for a '+' row, c = j + 6 for a '-' row.
  pair      (a, b): two eligible rows of the same gene in the same arena text with c_a < c_b.  D = c_b - c_a is the
            deletion's length: the letters s[c_a : c_b) go.
  qualifies when dmin <= D <= dmax (1 <= dmin <= dmax <= 65 535); with frameshift, D mod 3 != 0; and the bit sa * 2 + sb
            (0 for '+', 1 for '-') of a 4-bit orientation mask is set: "any" = 0xF, "pam-out" = '-' left and '+' right =
            bit 2 only, "pam-in" = bit 1 only.  For a PAM-out pair at guide length 20 the published nickase offset -- the
            distance between the two protospacers' PAM-distal ends -- is D - 34; the conversion is the user's, nothing
            here applies it.
  order     among qualifying pairs: higher min(score_a, score_b), compared as the doubles' bit patterns (unsigned 64-bit);
            then higher max(score_a, score_b); then smaller c_a; then smaller c_b; then smaller strand bits sa * 2 + sb.
            The order is total: the result does not depend on how the work was cut.
  result    per gene g: n_pass[g] (uint32, as above), n_pairs[g] (uint64, all qualifying pairs) and pairs[g][0..KP): each
            pair two uint32 in the packing of sel (row | strand << 31), a then b, 0xFFFFFFFF beyond.  KP = 1..64,
            independent of K.  The top pairs may share one very good guide.

Distinct pairs (csrc/crp_select_pairs_distinct.hip; tests/select_pairs_distinct_reference.py restates
it twice): everything of the guide pairs stands -- eligible rows, the boundary c, qualifying pairs, the total order, n_pass
and n_pairs.  New, per arena text and per layout row g:

  distinct  walk the qualifying pairs of g in the pairs' order; take a pair iff NEITHER of its two rows is a row of a pair
            already taken; stop at KP taken.  By rounds: round t takes the first qualifying pair in the order that has no
            row among the picks of rounds < t.
  row       a table row of one strand, in sel's packing row | strand << 31.  Two rows with equal boundaries (a '+' row at
            i and the '-' row at i - 9) are different guides.  A row taken as the left guide a of one pair shuts out the
            pairs that offer it as b, and the other way round.
  result    per gene g: n_pass[g] and n_pairs[g] exactly as the pair selection gives them, whatever the picks;
            n_distinct[g], the pairs taken, at most min(KP, n_pairs, n_pass // 2); and pairs[g][0..KP) in pick order,
            0xFFFFFFFF beyond n_distinct.  The walk never goes back, so the picks are in the pairs' order.  At KP = 1 the
            result is the pair selection's at KP = 1, bit for bit.
  greedy    the best pair is always taken, whatever it shuts out.  A maximum-weight matching is another problem.
  texts     a pair never spans texts, so pairs of different texts share no row: the greedy over a gene's union is the
            merge of the per-text greedy lists in the pairs' order, and assemble_pairs takes its first KP as it does for
            the plain pairs.  The summed n_distinct is capped at KP.

Coding position (coding.py has the definition; csrc/crp_coding.h, csrc/crp_select_coding.hip): with
coding limits a row passes for gene g only if, beyond the above, g has a coding model, the row's cut boundary (repair.py's c)
is inside the coding sequence of g's primary transcript, its coding offset lies within the given percentages of that
transcript's coding length, and the cut is inside enough of g's coding transcripts.  The pair selection is refused then.

Base editing (baseedit.py has the definition; csrc/crp_edit.h, csrc/crp_select_edit.hip): with edit
limits a row passes for gene g only if, beyond the above, a cytosine base editor turns a codon of g's primary transcript
under the row's window into a stop, the codon lies within the given percentages of that transcript's coding length and
the window holds no more than the given number of targets.  Not together with coding limits or the pair selection.

Splice-site editing (baseedit.py has the definition; csrc/crp_splice.h, csrc/crp_select_splice.hip):
with splice limits a row passes for gene g only if, beyond the above, a cytosine or an adenine base editor changes a letter
of a canonical donor or acceptor site of g's primary transcript under the row's window, the intron lies within the given
percentages of that transcript's coding length and the window holds no more than the given number of targets.  With edit
limits as well (cytosine editor only) the two tests are alternatives.  Not together with coding limits or the pair selection.

Gene families (families.py has the definition; csrc/crp_select_family.hip): with a family table every
(gene g, row) has outside_mm0, outside_hit_sum, members_hit and family_size -- where the row's joined site_family is g's
family, counts[0] - fam_counts[0], hit_sum - fam_sum, popcount(fam_cover) and |F|; else counts[0], hit_sum, 1 and the size
of g's family (1 for none).  Family limits are ANDed onto the predicate after the rest: outside_mm0 <= max_perfect_outside,
outside_hit_sum <= max_hit_sum_for(min_specificity_outside), members_hit >= min_members ("all": family_size).  max_perfect
and min_specificity keep their meaning on the full counts.  Not together with coding, edit or splice limits or pairs.

Family sets (family_sets.py has the definition; csrc/crp_select_family_set.hip): with family_sets = S
the scan also chooses, per family, at most S passing rows of its member genes that together cover as many members as
possible, greedily: each step takes the candidate with the largest gain over what is covered so far.

Spaced selection (csrc/crp_select_spaced.hip; tests/select_spacing_reference.py restates it twice): the
K best rows of a gene cluster -- a good 30-mer context lifts its neighbours, a reverse palindrome gives two rows with one cut
site -- and guides that cut within a few letters of each other fail together.  With min_spacing = D (0 <= D <= 2^31 - 1), per
arena and per layout row g, after a scan at guide length 20:

  passing   the rows that PASS for gene g, as above: exactly those n_pass[g] counts under the handle's current row limits
            (min_score, joined columns, require_cds, property, repair and variant limits).
  order     the selection's: higher score bits as unsigned 64-bit, then smaller cut site, then '+' before '-'.  The cut site is
            i - 3 for '+' and j for '-': NOT the pairs' cut boundary.
  spaced    walk the passing rows of g in that order; take a row iff |cut - cut(p)| >= D for EVERY row p already taken; stop at
            K taken.  Equivalently: round t takes the best passing row that is not within D - 1 of any earlier pick.
  result    per gene g: n_pass[g], unchanged by D; n_spaced[g], the rows taken, at most min(K, n_pass); sel[g][0..K) in the
            packing above, in pick order, 0xFFFFFFFF beyond n_spaced.  Exact and integer-only: it does not depend on how the
            work was cut.  D = 0 is the plain selection bit for bit; D = 1 forbids only equal cut sites.

Spacing holds inside one arena text; a gene met in several texts keeps the rule above (the first K of the concatenation).  It
is greedy by score, not a maximum-weight spread, and D counts letters of the assembly.  Not together with coding, edit, splice
or family limits: their kernels own a predicate per gene and row, and the spaced rounds read one pass key per table row.

This module lays the genes out per arena, converts a wanted specificity into the integer bound the kernel compares,
drives crp_select_* and turns the per-arena results into one table over the genes of the GFF.
"""
import ctypes

import numpy as np

from . import _native as nat

MAX_K = nat.SELECT_MAX_K
NONE = nat.SELECT_NONE
NO_BOUND_MM0, NO_BOUND_SUM = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
GUIDE_LEN = 20  # the ranking key, the on-target score, exists only there
MAX_KP, MAX_DISTANCE = nat.SELECT_PAIRS_MAX_K, nat.SELECT_PAIRS_MAX_DISTANCE
MAX_SPACING = nat.SELECT_MAX_SPACING
ORIENTATIONS = {"any": 0xF, "pam-out": 0x4, "pam-in": 0x2}  # bit sa * 2 + sb, 0 for '+' and 1 for '-'
PAIR_DTYPE = np.dtype([("gene", "<u4"), ("rank", "<u4"), ("contig", "<u4"), ("position_a", "<i8"), ("strand_a", "S1"), ("score_a", "<f8"),
                       ("index_a", "<u4"), ("position_b", "<i8"), ("strand_b", "S1"), ("score_b", "<f8"), ("index_b", "<u4"),
                       ("deletion_length", "<u4")])
ROW_DTYPE = np.dtype([("gene", "<u4"), ("rank", "<u4"), ("contig", "<u4"), ("position", "<i8"), ("strand", "S1"), ("score", "<f8"),
                      ("index", "<u4")])
# a pick of a family set (family_sets): ROW_DTYPE's fields with family and step for gene's rank, then the pick's gain, its
# cover word c and the family's covered word after the step
FAMILY_SET_DTYPE = np.dtype([("family", "<u4"), ("step", "<u4"), ("gene", "<u4"), ("contig", "<u4"), ("position", "<i8"), ("strand", "S1"),
                             ("score", "<f8"), ("index", "<u4"), ("gain", "<u4"), ("cover", "<u8"), ("covered", "<u8")])
MAX_FAMILY_SET_STEPS = nat.FAMILY_SET_MAX_STEPS


def max_hit_sum_for(S):
    """The largest integer h with search.specificity(h) >= S, found by bisection on that very function (so that the
    threshold agrees with the printed `specificity` column); S <= 0: no bound (2^64 - 1).  S > 1 has no such h."""
    from .search import specificity
    S = float(S)
    if not S <= 1.0:
        raise ValueError("a specificity threshold above 1 (or not a number) keeps no guide: %r" % (S,))
    if S <= 0.0:
        return NO_BOUND_SUM
    ok = lambda h: bool(specificity(np.uint64(h)) >= S)
    lo, hi = 0, NO_BOUND_SUM  # ok(lo) holds: specificity(0) = 1
    if ok(hi):
        return hi
    while hi - lo > 1:  # ok(lo) and not ok(hi); specificity never rises with h
        mid = (lo + hi) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid
    return lo


class Params:
    """What a selection asks for: K, min_score, max_perfect (most other perfect copies, counts[0]; None: no bound),
    min_specificity (None or <= 0: no bound) and require_cds.  The two specificity thresholds need joined columns."""

    def __init__(self, k, min_score=0.0, max_perfect=None, min_specificity=None, require_cds=False):
        self.k = int(k)
        if not 1 <= self.k <= MAX_K:
            raise ValueError("K must be 1..%d, not %d" % (MAX_K, self.k))
        self.min_score = float(min_score)
        if self.min_score != self.min_score:
            raise ValueError("min_score is not a number")
        self.max_mm0 = NO_BOUND_MM0 if max_perfect is None else int(max_perfect)
        if not 0 <= self.max_mm0 <= NO_BOUND_MM0:
            raise ValueError("max_perfect must be a count, not %r" % (max_perfect,))
        self.max_hit_sum = NO_BOUND_SUM if min_specificity is None else max_hit_sum_for(min_specificity)
        self.needs_specificity = max_perfect is not None or (min_specificity is not None and float(min_specificity) > 0.0)
        self.require_cds = bool(require_cds)

    def native(self):
        return nat.SelectParams(self.min_score, self.max_hit_sum, self.max_mm0, self.k, int(self.require_cds), 0)


class PairParams:
    """What a pair selection asks for: KP, the window dmin <= D <= dmax on the deletion length, frameshift (D mod 3 != 0)
    and the orientation: "any", "pam-out", "pam-in", or a 4-bit mask over (strand of a, strand of b), bit sa * 2 + sb.
    distinct: the KP pairs of a gene share no guide (the module's "Distinct pairs"); a scan then runs the distinct pair
    selection instead of the plain one."""

    def __init__(self, k, dmin=50, dmax=500, frameshift=False, orientation="any", distinct=False):
        if not isinstance(distinct, (bool, np.bool_)):
            raise ValueError("distinct is True or False, not %r" % (distinct,))
        self.distinct = bool(distinct)
        self.k = int(k)
        if not 1 <= self.k <= MAX_KP:
            raise ValueError("KP must be 1..%d, not %d" % (MAX_KP, self.k))
        self.dmin, self.dmax = int(dmin), int(dmax)
        if not 1 <= self.dmin <= self.dmax <= MAX_DISTANCE:
            raise ValueError("the pair distances must be 1 <= dmin <= dmax <= %d, not %d and %d" % (MAX_DISTANCE, self.dmin, self.dmax))
        self.frameshift = bool(frameshift)
        if isinstance(orientation, str):
            if orientation not in ORIENTATIONS:
                raise ValueError("the pair orientation is one of %s, not %r" % (", ".join(sorted(ORIENTATIONS)), orientation))
            self.mask = ORIENTATIONS[orientation]
        else:
            self.mask = int(orientation)
        if not 1 <= self.mask <= 0xF:
            raise ValueError("the orientation mask must be 1..15, not %r" % (orientation,))

    def native(self):
        return nat.SelectPairParams(self.k, self.dmin, self.dmax, self.mask, int(self.frameshift))


class FamilyLimits:
    """The family limits of a selection: min_members (an int 1..64 or "all": every member of the gene's family),
    max_perfect_outside (perfect copies outside the family, at most) and min_specificity_outside (of what lies outside the
    family, at least; the bound on outside_hit_sum comes from max_hit_sum_for, like min_specificity's).  None: no bound."""

    def __init__(self, min_members=None, max_perfect_outside=None, min_specificity_outside=None):
        if min_members is None:
            self.min_members = 0
        elif isinstance(min_members, str):
            if min_members.strip().lower() != "all":
                raise ValueError("min_members is a number of members or 'all', not %r" % (min_members,))
            self.min_members = nat.SELECT_ALL_MEMBERS
        elif isinstance(min_members, (int, np.integer)) and 1 <= int(min_members) <= 64:
            self.min_members = int(min_members)
        else:
            raise ValueError("min_members is 1..64 (a family has at most 64 members) or 'all', not %r" % (min_members,))
        if max_perfect_outside is not None and (not isinstance(max_perfect_outside, (int, np.integer)) or not 0 <= int(max_perfect_outside) < NO_BOUND_MM0):
            raise ValueError("max_perfect_outside is a count, not %r" % (max_perfect_outside,))
        self.max_mm0_outside = NO_BOUND_MM0 if max_perfect_outside is None else int(max_perfect_outside)
        self.max_hit_sum_outside = NO_BOUND_SUM if min_specificity_outside is None else max_hit_sum_for(min_specificity_outside)

    def astuple(self):
        return self.max_hit_sum_outside, self.max_mm0_outside, self.min_members

    def passes(self, outside_mm0, outside_hit_sum, members_hit, family_size):
        """The host's statement of the device's test, on arrays or numbers."""
        need = family_size if self.min_members == nat.SELECT_ALL_MEMBERS else self.min_members
        return (outside_mm0 <= self.max_mm0_outside) & (outside_hit_sum <= self.max_hit_sum_outside) & (members_hit >= need)


class Request:
    """A selection for a backend's scan: Params, the annotate.Request that names the genes, slice_rows (None: the
    library's default; results do not depend on it) and the limits on the guide properties (properties.py), as counts:
    gc_min <= gc <= gc_max, run <= max_run, t_run <= max_t_run, stem <= max_stem.  With any of them given a row passes
    only if all hold, and the scan runs the property kernel before the selection.  Likewise the repair scores
    (repair.py): min_mh (tenths of the microhomology score) and min_oof (an integer percentage) are limits, repair_flank
    is the kernel's flank (None: 30).  With a limit or a flank the scan runs the repair kernel before the selection; with a
    flank the column is also fetched and the Selection carries mh and oof of its rows.  pairs (PairParams): the scan also
    selects the best pairs of every gene, right after the single guides (Selection.pairs, Selection.n_pairs);
    pair_slice_rows: the a-rows of one work item (None: the library's default; results do not depend on it).
    coding / coding_limits (coding.Limits): the coding position of the cut (coding.py).  With either the selection sets
    the genes' coding model and the Selection carries cds_offset, cds_length, transcripts_cut and transcripts of its rows;
    with limits a row passes only if they hold for the gene it is selected for.  Pairs are refused with coding limits.
    edit_window / edit_limits (baseedit.Window, baseedit.Limits): base editing (baseedit.py).  With either the selection
    sets the genes' coding model and the Selection carries edit_targets, stop_codons, stop_offset and cds_length of its
    rows (the window defaults to 4..8); with limits a row passes only if the edit writes a stop codon inside them for the
    gene it is selected for.  Edit limits are refused with coding limits and with pairs.
    editor / splice_limits (baseedit.Editor or its name, baseedit.SpliceLimits): splice-site editing (baseedit.py).  With
    either the selection sets the genes' coding model and the Selection carries splice_targets, donors, acceptors,
    donor_offset, acceptor_offset and cds_length of its rows under edit_window (default 4..8) for that editor (default
    cbe); with limits a row passes only if the edit destroys a splice site inside them for the gene it is selected for --
    or, with edit_limits given as well, writes a stop codon inside those.  Splice limits are refused with coding limits and
    with pairs, and the editor abe with edit limits.  edit: with the splice test, whether the stop-codon fields are wanted
    too (they always come with edit limits).
    families (families.FamilyTable of the annotation's genes): gene families (families.py).  The scan's specificity join then
    also computes and joins the family rows (family_cover_mm: the cover limit C), and the Selection carries family,
    family_size, members_hit, members, outside_mm0, outside_hit_sum and fam_cover of its rows, for the gene each was selected
    for.  min_members / max_perfect_outside / min_specificity_outside (FamilyLimits) are limits: a row passes only if they
    hold for the gene it is selected for.  They need families, and are refused with coding, edit or splice limits and with
    pairs: one kernel per predicate.
    family_sets (S, 1..64): after the per-gene selection the scan also chooses, per family, at most S guides that together
    cut as many members as possible (family_sets(); Selection.family_sets, Selection.family_complete).  Needs families, and
    is refused with coding, edit or splice limits and with pairs.
    variants (variants.Request): the scan counts the cultivar's variants under every hit (variants.py) before the selection --
    variant_seed is the seed length (None: min(12, guide length)) -- and the Selection carries the packed counts of its rows
    (Selection.variants).  max_variants / max_guide_variants / max_seed_variants / max_pam_variants (variants.Limits) are
    limits on the site, guide, seed and PAM counts: a row passes only if all hold, in every selection the request runs --
    single guides, pairs, coding, edit, splice, family limits and family sets.  They need variants.
    enzymes (sites.EnzymeSet): the scan runs the restriction-site kernel (sites.py) right before the selection, with amplicon
    half-width assay_flank (None: 300), and the Selection carries the two masks of its rows (Selection.guide_sites,
    Selection.assay_enzymes).  forbid_sites / need_assay (masks over the set, or lists of names for EnzymeSet.mask) are limits: a
    row passes only if no enzyme of forbid_sites lies inside its guide and -- need_assay given -- it has an assay with one of
    need_assay's, in every selection the request runs.  They need enzymes.  site_fields: whether the Selection carries the masks
    (None: only a request without limits; with limits alone the column stays on the device, like the repair column).
    min_spacing (D, 0..2^31 - 1): the guides of a gene cut at least D letters apart (the module's text has the definition): the
    scan runs the plain selection, which supplies n_in and n_pass, and then the spaced selection, whose rows the Selection
    carries in pick order.  The per-pick fields (coding, edit, splice, families) are those of the spaced picks; pairs and
    family sets are not affected.  Refused with coding, edit, splice or family limits."""

    def __init__(self, params, annotation, slice_rows=None, gc_min=None, gc_max=None, max_run=None, max_t_run=None, max_stem=None,
                 repair_flank=None, min_mh=None, min_oof=None, pairs=None, pair_slice_rows=None, coding=False, coding_limits=None,
                 edit_window=None, edit_limits=None, editor=None, splice_limits=None, edit=None, families=None, family_cover_mm=0,
                 min_members=None, max_perfect_outside=None, min_specificity_outside=None, family_sets=None, variants=None,
                 variant_seed=None, max_variants=None, max_guide_variants=None, max_seed_variants=None, max_pam_variants=None,
                 enzymes=None, assay_flank=None, forbid_sites=None, need_assay=None, site_fields=None,
                 min_spacing=None):
        self.min_spacing = None
        if min_spacing is not None:
            if isinstance(min_spacing, bool) or not isinstance(min_spacing, (int, np.integer)) or not 0 <= int(min_spacing) <= MAX_SPACING:
                raise ValueError("min_spacing is a number of letters 0..%d, not %r" % (MAX_SPACING, min_spacing))
            for given, name in ((coding_limits, "coding"), (edit_limits, "edit"), (splice_limits, "splice"),
                                (next((v for v in (min_members, max_perfect_outside, min_specificity_outside) if v is not None), None), "family")):
                if given is not None:
                    raise ValueError("%s limits are relative to the gene; the spaced selection's eligibility is per table row: one or the other" % name)
            self.min_spacing = int(min_spacing)
        self.enzymes, self.assay_flank, self.site_limits = enzymes, None, None
        if enzymes is None:
            if any(v is not None for v in (assay_flank, forbid_sites, need_assay)):
                raise ValueError("assay_flank, forbid_sites and need_assay need an enzyme set (enzymes=)")
        else:
            self.assay_flank = enzymes.check_flank(assay_flank)
            masks = []
            for name, v in (("forbid_sites", forbid_sites), ("need_assay", need_assay)):
                m = 0 if v is None else (int(v) if isinstance(v, (int, np.integer)) else enzymes.mask(v))
                if not 0 <= m < 1 << len(enzymes):
                    raise ValueError("%s is a mask over the set's %d enzymes, not %r" % (name, len(enzymes), v))
                masks.append(m)
            if any(masks):
                self.site_limits = tuple(masks)
        # the column comes to the host (Selection.guide_sites / assay_enzymes) unless it only bounds the selection
        self.site_fields = enzymes is not None and (self.site_limits is None if site_fields is None else bool(site_fields))
        self.variants, self.variant_seed, self.variant_limits = variants, variant_seed, None
        if any(v is not None for v in (max_variants, max_guide_variants, max_seed_variants, max_pam_variants)):
            if variants is None:
                raise ValueError("max_variants, max_guide_variants, max_seed_variants and max_pam_variants need a variant set (variants=)")
            from .variants import Limits as VariantLimits
            self.variant_limits = VariantLimits(max_variants, max_guide_variants, max_seed_variants, max_pam_variants)
        if variant_seed is not None and variants is None:
            raise ValueError("variant_seed needs a variant set (variants=)")
        self.families, self.family_cover_mm = families, int(family_cover_mm)
        self.family_sets = None
        if family_sets is not None:
            if families is None:
                raise ValueError("family_sets needs a family table (families=)")
            if coding_limits is not None or edit_limits is not None or splice_limits is not None:
                raise ValueError("family sets and coding, edit or splice limits are different kernels' predicates: one or the other")
            if pairs is not None:
                raise ValueError("family sets do not combine with the pair selection: one or the other")
            if not isinstance(family_sets, (int, np.integer)) or not 1 <= int(family_sets) <= MAX_FAMILY_SET_STEPS:
                raise ValueError("family_sets is a number of guides 1..%d, not %r" % (MAX_FAMILY_SET_STEPS, family_sets))
            self.family_sets = int(family_sets)
        self.family_limits = None
        if any(v is not None for v in (min_members, max_perfect_outside, min_specificity_outside)):
            if families is None:
                raise ValueError("min_members, max_perfect_outside and min_specificity_outside need a family table (families=)")
            if coding_limits is not None or edit_limits is not None or splice_limits is not None:
                raise ValueError("family limits and coding, edit or splice limits are different kernels' predicates: one or the other")
            if pairs is not None:
                raise ValueError("family limits are relative to the gene; the pair selection's eligibility is per table row: one or the other")
            self.family_limits = FamilyLimits(min_members, max_perfect_outside, min_specificity_outside)
        self.pairs, self.pair_slice_rows = pairs, pair_slice_rows
        self.splice = editor is not None or splice_limits is not None
        self.splice_limits = splice_limits
        self.editor = None
        if self.splice:
            from .baseedit import Editor, Window
            self.editor = Editor("cbe" if editor is None else editor)
            self.splice_window = Window() if edit_window is None else edit_window
            if self.editor.name == "abe" and edit_limits is not None:
                raise ValueError("an adenine editor writes no stop codon: edit limits belong to the editor cbe")
        if splice_limits is not None and coding_limits is not None:
            raise ValueError("splice limits and coding limits are two kernels' predicates: one or the other")
        if splice_limits is not None and pairs is not None:
            raise ValueError("splice limits are relative to the gene; the pair selection's eligibility is per table row: one or the other")
        # (the window is shared by both tests: without the splice test it asks for the stop-codon fields by itself, with it `edit` says)
        self.edit = edit_limits is not None or (bool(edit) if self.splice else edit_window is not None)
        self.edit_window, self.edit_limits = edit_window, edit_limits
        if self.edit and edit_window is None:
            from .baseedit import Window
            self.edit_window = Window()
        if edit_limits is not None and coding_limits is not None:
            raise ValueError("edit limits and coding limits are two kernels' predicates: one or the other")
        if edit_limits is not None and pairs is not None:
            raise ValueError("edit limits are relative to the gene; the pair selection's eligibility is per table row: one or the other")
        self.coding_limits = coding_limits
        self.coding = bool(coding) or coding_limits is not None
        if coding_limits is not None and pairs is not None:
            raise ValueError("coding limits are relative to the gene; the pair selection's eligibility is per table row: one or the other")
        from . import repair
        from .properties import Limits
        self.repair_flank = None if repair_flank is None else repair.check_flank(repair_flank)
        self.repair_limits = repair.Limits(min_mh, min_oof) if (min_mh is not None or min_oof is not None) else None
        self.flank = repair.DEFAULT_FLANK if self.repair_flank is None else self.repair_flank
        self.runs_repair = self.repair_flank is not None or self.repair_limits is not None
        self.params, self.annotation, self.slice_rows = params, annotation, slice_rows
        given = [v is not None for v in (gc_min, gc_max, max_run, max_t_run, max_stem)]
        self.property_limits = Limits(gc_min, gc_max, max_run, max_t_run, max_stem) if any(given) else None


class ArenaSelect:
    """One crp_select handle: the genes of one arena as closed ranges of arena positions."""

    def __init__(self, arena, lo, hi):
        self._arena = arena
        self._ctx = arena._engine._ctx
        self._h = None
        lo, hi = np.ascontiguousarray(lo, dtype=np.uint32), np.ascontiguousarray(hi, dtype=np.uint32)
        if lo.shape != hi.shape or lo.ndim != 1:
            raise ValueError("lo and hi must be 1-d arrays of one length")
        self.n_genes, self.k, self.kp, self.ks = int(lo.size), 0, 0, 0
        self.kpd = 0  # KP of the last run_pairs_distinct
        self.kself, self._self_stride = 0, 1  # of the last run_self
        h = ctypes.c_void_p()
        nat.check(nat.lib().crp_select_create(arena._h, lo.ctypes.data_as(nat.u32p), hi.ctypes.data_as(nat.u32p), lo.size, ctypes.byref(h)),
                  "crp_select_create", self._ctx)
        self._h = h

    def close(self):
        if self._h:
            nat.lib().crp_select_destroy(self._h)
            self._h = None

    __del__ = close

    def set_flags(self, flags):
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        nat.check(nat.lib().crp_select_set_flags(self._h, flags.ctypes.data_as(nat.u8p), flags.size), "crp_select_set_flags", self._ctx)

    def set_limits(self, slice_rows=0):
        nat.check(nat.lib().crp_select_set_limits(self._h, int(slice_rows)), "crp_select_set_limits", self._ctx)

    def set_property_limits(self, limits):
        """limits: properties.Limits, or None to clear them."""
        lim = None if limits is None else ctypes.byref(nat.SelectPropertyLimits(*limits.astuple()))
        nat.check(nat.lib().crp_select_set_property_limits(self._h, lim), "crp_select_set_property_limits", self._ctx)

    def set_repair_limits(self, limits):
        """limits: repair.Limits, or None to clear them."""
        lim = None if limits is None else ctypes.byref(nat.SelectRepairLimits(*limits.astuple()))
        nat.check(nat.lib().crp_select_set_repair_limits(self._h, lim), "crp_select_set_repair_limits", self._ctx)

    def set_site_limits(self, limits):
        """limits: (forbid_sites, need_assay) masks over the arena's enzyme set, or None to clear them."""
        forbid, need = (0, 0) if limits is None else limits
        nat.check(nat.lib().crp_select_set_site_limits(self._h, int(forbid), int(need)), "crp_select_set_site_limits", self._ctx)

    def set_variant_limits(self, limits):
        """limits: variants.Limits, or None to clear them."""
        lim = None if limits is None else ctypes.byref(nat.SelectVariantLimits(*limits.astuple()))
        nat.check(nat.lib().crp_select_set_variant_limits(self._h, lim), "crp_select_set_variant_limits", self._ctx)

    def run(self, params, self_search=None):
        """params: Params; self_search: the search.ArenaSelfSearch of this arena after its join_hits, or None."""
        p = params.native()
        nat.check(nat.lib().crp_select_run(self._h, ctypes.byref(p), self_search._h if self_search is not None else None),
                  "crp_select_run", self._ctx)
        self.k = params.k

    def fetch(self):
        """(n_in uint32 (G,), n_pass uint32 (G,), sel uint32 (G, K)) of the last run."""
        n_in, n_pass = np.empty(self.n_genes, np.uint32), np.empty(self.n_genes, np.uint32)
        sel = np.empty((self.n_genes, max(1, self.k)), np.uint32)
        nat.check(nat.lib().crp_select_fetch(self._h, n_in.ctypes.data_as(nat.u32p), n_pass.ctypes.data_as(nat.u32p),
                                             sel.ctypes.data_as(nat.u32p)), "crp_select_fetch", self._ctx)
        return n_in, n_pass, sel

    def stats(self):
        out = np.zeros(9, dtype=np.float64)
        nat.check(nat.lib().crp_select_stats(self._h, out.ctypes.data_as(nat.f64p), 9), "crp_select_stats", self._ctx)
        keys = ("bounds_ms", "select_ms", "merge_ms", "items", "launches", "longest_launch_ms", "rows_in_runs", "bytes_per_row",
                "merged_genes")
        return dict(zip(keys, (float(v) for v in out)))

    def run_spaced(self, params, min_spacing, self_search=None):
        """params: Params (its thresholds and K); min_spacing: D, 0..MAX_SPACING; self_search as run()."""
        if isinstance(min_spacing, bool) or not isinstance(min_spacing, (int, np.integer)) or not 0 <= int(min_spacing) <= 0xFFFFFFFF:
            raise ValueError("min_spacing is a number of letters 0..%d, not %r" % (MAX_SPACING, min_spacing))
        p = params.native()
        nat.check(nat.lib().crp_select_run_spaced(self._h, ctypes.byref(p), int(min_spacing), self_search._h if self_search is not None else None),
                  "crp_select_run_spaced", self._ctx)
        self.ks = params.k

    def fetch_spaced(self):
        """(n_pass uint32 (G,), n_spaced uint32 (G,), sel uint32 (G, K)) of the last run_spaced."""
        n_pass, n_spaced = np.empty(self.n_genes, np.uint32), np.empty(self.n_genes, np.uint32)
        sel = np.empty((self.n_genes, max(1, self.ks)), np.uint32)
        nat.check(nat.lib().crp_select_fetch_spaced(self._h, n_pass.ctypes.data_as(nat.u32p), n_spaced.ctypes.data_as(nat.u32p),
                                                    sel.ctypes.data_as(nat.u32p)), "crp_select_fetch_spaced", self._ctx)
        return n_pass, n_spaced, sel

    def spaced_stats(self):
        out = np.zeros(9, dtype=np.float64)
        nat.check(nat.lib().crp_select_spaced_stats(self._h, out.ctypes.data_as(nat.f64p), 9), "crp_select_spaced_stats", self._ctx)
        keys = ("spaced_key_ms", "spaced_items_ms", "spaced_step_ms", "spaced_pick_ms", "spaced_rounds", "spaced_launches",
                "spaced_longest_launch_ms", "spaced_items", "spaced_cut_genes")
        return dict(zip(keys, (float(v) for v in out)))

    # ---- self selection (select_self.py has the definition)
    def set_self_limits(self, items_per_launch=0):
        nat.check(nat.lib().crp_select_set_self_limits(self._h, int(items_per_launch)), "crp_select_set_self_limits", self._ctx)

    def run_self(self, params, self_search):
        """params: select_self.Params (or a nat.SelectSelfParams); self_search: the search.ArenaSelfSearch of this arena after
        all of its orders and compares."""
        p = params.native() if hasattr(params, "native") else params
        nat.check(nat.lib().crp_select_run_self(self._h, ctypes.byref(p), self_search._h), "crp_select_run_self", self._ctx)
        self.kself, self._self_stride = int(p.k), self_search.max_mm + 1

    def fetch_self(self):
        """dict of the last run_self: n_in, n_pass uint32 (G,), sel uint32 (G, K) -- candidate indices in extraction order --
        and of the selected candidates, beside sel: arena_pos, hi, lo uint32 (G, K), strand uint8 (G, K), counts uint32
        (G, K, M + 1), hit_sum uint64 (G, K); all-ones where sel has no candidate."""
        G, K = self.n_genes, max(1, self.kself)
        out = dict(n_in=np.empty(G, np.uint32), n_pass=np.empty(G, np.uint32), sel=np.empty((G, K), np.uint32),
                   arena_pos=np.empty((G, K), np.uint32), strand=np.empty((G, K), np.uint8), hi=np.empty((G, K), np.uint32),
                   lo=np.empty((G, K), np.uint32), counts=np.empty((G, K, self._self_stride), np.uint32),
                   hit_sum=np.empty((G, K), np.uint64))
        types = dict(strand=nat.u8p, hit_sum=nat.u64p)
        order = ("n_in", "n_pass", "sel", "arena_pos", "strand", "hi", "lo", "counts", "hit_sum")
        nat.check(nat.lib().crp_select_fetch_self(self._h, *[out[key].ctypes.data_as(types.get(key, nat.u32p)) for key in order]),
                  "crp_select_fetch_self", self._ctx)
        return out

    def set_self_model(self, rank_by_model=False, min_sum=None):
        """crp_select_set_self_model, for the later run_self calls: rank by the on-target sum of the handle's model, and / or
        pass only sites whose sum is at least min_sum (None: no bound)."""
        nat.check(nat.lib().crp_select_set_self_model(self._h, int(bool(rank_by_model)), int(min_sum is not None),
                                                      0.0 if min_sum is None else float(min_sum)), "crp_select_set_self_model", self._ctx)

    def fetch_self_model(self):
        """float64 (G, K) beside fetch_self(): the on-target sums of the selected candidates, NaN where there is none."""
        out = np.empty((self.n_genes, max(1, self.kself)), np.float64)
        nat.check(nat.lib().crp_select_fetch_self_model(self._h, out.ctypes.data_as(nat.f64p)), "crp_select_fetch_self_model", self._ctx)
        return out

    def self_stats(self):
        out = np.zeros(7, dtype=np.float64)
        nat.check(nat.lib().crp_select_self_stats(self._h, out.ctypes.data_as(nat.f64p), 7), "crp_select_self_stats", self._ctx)
        keys = ("self_bounds_ms", "self_items_ms", "self_merge_ms", "self_gather_ms", "self_launches", "self_items", "self_rows_in_runs")
        return dict(zip(keys, (float(v) for v in out)))

    def set_coding(self, model):
        """model: the dict of annotate.Request.coding_layout for this handle's genes, or None to clear it."""
        if model is None:
            nat.check(nat.lib().crp_select_set_coding(self._h, None, None, None, 0, None, None, None, 0), "crp_select_set_coding", self._ctx)
            return
        info, length, at, word, cum = (np.ascontiguousarray(model[key], dtype=np.uint32) for key in ("info", "length", "at", "word", "cum"))
        first = np.ascontiguousarray(model["first"], dtype=np.uint64)
        if first.size != info.size + 1 or length.size != info.size or not at.size == word.size == cum.size:
            raise ValueError("a coding model has info and length per row, first with one more element, and at / word / cum per step")
        nat.check(nat.lib().crp_select_set_coding(self._h, info.ctypes.data_as(nat.u32p), length.ctypes.data_as(nat.u32p),
                                                  first.ctypes.data_as(nat.u64p), info.size, at.ctypes.data_as(nat.u32p),
                                                  word.ctypes.data_as(nat.u32p), cum.ctypes.data_as(nat.u32p), at.size),
                  "crp_select_set_coding", self._ctx)

    def set_coding_limits(self, limits):
        """limits: coding.Limits, or None to clear them."""
        lim = None if limits is None else ctypes.byref(nat.SelectCodingLimits(*limits.astuple()))
        nat.check(nat.lib().crp_select_set_coding_limits(self._h, lim), "crp_select_set_coding_limits", self._ctx)

    def coding_eval(self, gene_row, packed_row):
        """(off uint32, cover uint32) of the cuts of packed_row (sel's packing) for the genes gene_row of this handle;
        off = coding.NOT_INSIDE where the cut is not inside the primary transcript's coding sequence."""
        gene_row, packed_row = np.ascontiguousarray(gene_row, dtype=np.uint32), np.ascontiguousarray(packed_row, dtype=np.uint32)
        if gene_row.shape != packed_row.shape or gene_row.ndim != 1:
            raise ValueError("gene_row and packed_row must be 1-d arrays of one length")
        off, cover = np.zeros(max(1, gene_row.size), np.uint32), np.zeros(max(1, gene_row.size), np.uint32)
        nat.check(nat.lib().crp_select_coding_eval(self._h, gene_row.ctypes.data_as(nat.u32p), packed_row.ctypes.data_as(nat.u32p), gene_row.size,
                                                   off.ctypes.data_as(nat.u32p), cover.ctypes.data_as(nat.u32p)), "crp_select_coding_eval", self._ctx)
        return off[:gene_row.size], cover[:gene_row.size]

    def set_family(self, gene_family, family_size):
        """Per gene of this handle its family id (families.NONE: none) and that family's size (1 for none); None, None clears."""
        if gene_family is None:
            nat.check(nat.lib().crp_select_set_family(self._h, None, None, 0), "crp_select_set_family", self._ctx)
            return
        f, n = np.ascontiguousarray(gene_family, dtype=np.uint32), np.ascontiguousarray(family_size, dtype=np.uint32)
        if f.shape != n.shape or f.ndim != 1:
            raise ValueError("gene_family and family_size must be 1-d arrays of one length")
        pad = lambda a: a if a.size else np.zeros(1, np.uint32)  # (a handle without genes still gets pointers)
        nat.check(nat.lib().crp_select_set_family(self._h, pad(f).ctypes.data_as(nat.u32p), pad(n).ctypes.data_as(nat.u32p), f.size),
                  "crp_select_set_family", self._ctx)

    def set_family_limits(self, limits):
        """limits: FamilyLimits, or None to clear them."""
        lim = None if limits is None else ctypes.byref(nat.SelectFamilyLimits(*limits.astuple()))
        nat.check(nat.lib().crp_select_set_family_limits(self._h, lim), "crp_select_set_family_limits", self._ctx)

    def family_eval(self, self_search, gene_row, packed_row):
        """(outside_mm0 uint32, outside_hit_sum uint64, members_hit uint32, family_size uint32, fam_cover uint64) of the rows
        packed_row (sel's packing) for the genes gene_row of this handle, from the joined columns of self_search
        (search.ArenaSelfSearch); fam_cover is 0 where the row's family is not the gene's."""
        gene_row, packed_row = np.ascontiguousarray(gene_row, dtype=np.uint32), np.ascontiguousarray(packed_row, dtype=np.uint32)
        if gene_row.shape != packed_row.shape or gene_row.ndim != 1:
            raise ValueError("gene_row and packed_row must be 1-d arrays of one length")
        n = gene_row.size
        mm0, hit, size = (np.zeros(max(1, n), np.uint32) for _ in range(3))
        hs, cover = np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint64)
        nat.check(nat.lib().crp_select_family_eval(self._h, self_search._h if self_search is not None else None,
                                                   gene_row.ctypes.data_as(nat.u32p), packed_row.ctypes.data_as(nat.u32p), n,
                                                   mm0.ctypes.data_as(nat.u32p), hs.ctypes.data_as(nat.u64p), hit.ctypes.data_as(nat.u32p),
                                                   size.ctypes.data_as(nat.u32p), cover.ctypes.data_as(nat.u64p)), "crp_select_family_eval",
                  self._ctx)
        return mm0[:n], hs[:n], hit[:n], size[:n], cover[:n]

    def family_stats(self):
        out = np.zeros(2, dtype=np.float64)
        nat.check(nat.lib().crp_select_family_stats(self._h, out.ctypes.data_as(nat.f64p), 2), "crp_select_family_stats", self._ctx)
        return dict(zip(("family_select_ms", "family_eval_ms"), (float(v) for v in out)))

    def set_family_members(self, gene_member):
        """Per gene of this handle its bit in its family's cover word (FamilyTable.gene_member); None clears.  After set_family."""
        if gene_member is None:
            nat.check(nat.lib().crp_select_set_family_members(self._h, None, 0), "crp_select_set_family_members", self._ctx)
            return
        m = np.ascontiguousarray(gene_member, dtype=np.uint32)
        if m.ndim != 1:
            raise ValueError("gene_member must be a 1-d array")
        pad = m if m.size else np.zeros(1, np.uint32)  # (a handle without genes still gets a pointer)
        nat.check(nat.lib().crp_select_set_family_members(self._h, pad.ctypes.data_as(nat.u32p), m.size), "crp_select_set_family_members",
                  self._ctx)

    def family_step(self, params, self_search, covered):
        """One greedy step in this arena: per family id the best candidate against covered (uint64 per family), as records of
        nat.FAMILY_STEP_BEST_DTYPE; gain 0: none."""
        covered = np.ascontiguousarray(covered, dtype=np.uint64)
        if covered.ndim != 1:
            raise ValueError("covered must be a 1-d array, one word per family")
        best = np.zeros(max(1, covered.size), dtype=nat.FAMILY_STEP_BEST_DTYPE)
        pad = covered if covered.size else np.zeros(1, np.uint64)
        p = params.native()
        nat.check(nat.lib().crp_select_family_step(self._h, ctypes.byref(p), self_search._h if self_search is not None else None,
                                                   pad.ctypes.data_as(nat.u64p), covered.size, best.ctypes.data_as(ctypes.c_void_p)),
                  "crp_select_family_step", self._ctx)
        return best[:covered.size]

    def family_step_stats(self):
        out = np.zeros(6, dtype=np.float64)
        nat.check(nat.lib().crp_select_family_step_stats(self._h, out.ctypes.data_as(nat.f64p), 6), "crp_select_family_step_stats", self._ctx)
        return dict(zip(("step_ms", "pick_ms", "items", "rows_in_runs", "bytes_per_row", "plan_builds"), (float(v) for v in out)))

    def coding_stats(self):
        out = np.zeros(3, dtype=np.float64)
        nat.check(nat.lib().crp_select_coding_stats(self._h, out.ctypes.data_as(nat.f64p), 3), "crp_select_coding_stats", self._ctx)
        return dict(zip(("coding_select_ms", "coding_eval_ms", "coding_steps"), (float(v) for v in out)))

    def set_edit_limits(self, window=None, limits=None):
        """window: baseedit.Window (None: 4..8); limits: baseedit.Limits, or None to clear them."""
        win = None if window is None else ctypes.byref(nat.SelectEditWindow(*window.astuple()))
        lim = None if limits is None else ctypes.byref(nat.SelectEditLimits(*limits.astuple()))
        nat.check(nat.lib().crp_select_set_edit_limits(self._h, win, lim), "crp_select_set_edit_limits", self._ctx)

    def edit_eval(self, window, gene_row, packed_row):
        """(targets, stops, stop_off), uint32 each, of the rows packed_row (sel's packing) for the genes gene_row of this
        handle under window (baseedit.Window; None: 4..8); stop_off = baseedit.NO_STOP where the edit writes no stop."""
        gene_row, packed_row = np.ascontiguousarray(gene_row, dtype=np.uint32), np.ascontiguousarray(packed_row, dtype=np.uint32)
        if gene_row.shape != packed_row.shape or gene_row.ndim != 1:
            raise ValueError("gene_row and packed_row must be 1-d arrays of one length")
        win = None if window is None else ctypes.byref(nat.SelectEditWindow(*window.astuple()))
        counts, off = np.zeros(max(1, gene_row.size), np.uint32), np.zeros(max(1, gene_row.size), np.uint32)
        nat.check(nat.lib().crp_select_edit_eval(self._h, win, gene_row.ctypes.data_as(nat.u32p), packed_row.ctypes.data_as(nat.u32p), gene_row.size,
                                                 counts.ctypes.data_as(nat.u32p), off.ctypes.data_as(nat.u32p)), "crp_select_edit_eval", self._ctx)
        counts = counts[:gene_row.size]
        return counts & np.uint32(0xFF), counts >> np.uint32(8), off[:gene_row.size]

    def edit_stats(self):
        out = np.zeros(3, dtype=np.float64)
        nat.check(nat.lib().crp_select_edit_stats(self._h, out.ctypes.data_as(nat.f64p), 3), "crp_select_edit_stats", self._ctx)
        return dict(zip(("edit_select_ms", "edit_eval_ms", "edit_targets_window"), (float(v) for v in out)))

    def set_splice_limits(self, window=None, editor="cbe", limits=None):
        """window: baseedit.Window (None: 4..8); editor: baseedit.Editor or its name; limits: baseedit.SpliceLimits, or None
        to clear them."""
        from .baseedit import Editor
        win = None if window is None else ctypes.byref(nat.SelectEditWindow(*window.astuple()))
        lim = None if limits is None else ctypes.byref(nat.SelectSpliceLimits(*limits.astuple()))
        nat.check(nat.lib().crp_select_set_splice_limits(self._h, win, Editor(editor).code, lim), "crp_select_set_splice_limits", self._ctx)

    def splice_eval(self, window, editor, gene_row, packed_row):
        """(targets, donors, acceptors, donor_off, acceptor_off), uint32 each, of the rows packed_row (sel's packing) for the
        genes gene_row of this handle under window (baseedit.Window; None: 4..8) and editor (baseedit.Editor or its name);
        an off is baseedit.NO_SITE where the edit destroys no site of that kind."""
        from .baseedit import Editor
        gene_row, packed_row = np.ascontiguousarray(gene_row, dtype=np.uint32), np.ascontiguousarray(packed_row, dtype=np.uint32)
        if gene_row.shape != packed_row.shape or gene_row.ndim != 1:
            raise ValueError("gene_row and packed_row must be 1-d arrays of one length")
        win = None if window is None else ctypes.byref(nat.SelectEditWindow(*window.astuple()))
        counts, off = np.zeros(max(1, gene_row.size), np.uint32), np.zeros(2 * max(1, gene_row.size), np.uint32)
        nat.check(nat.lib().crp_select_splice_eval(self._h, win, Editor(editor).code, gene_row.ctypes.data_as(nat.u32p), packed_row.ctypes.data_as(nat.u32p),
                                                   gene_row.size, counts.ctypes.data_as(nat.u32p), off.ctypes.data_as(nat.u32p)),
                  "crp_select_splice_eval", self._ctx)
        counts, off = counts[:gene_row.size], off[:2 * gene_row.size].reshape(-1, 2)
        return counts & np.uint32(0xFF), counts >> np.uint32(8) & np.uint32(0xFF), counts >> np.uint32(16), off[:, 0].copy(), off[:, 1].copy()

    def splice_stats(self):
        out = np.zeros(3, dtype=np.float64)
        nat.check(nat.lib().crp_select_splice_stats(self._h, out.ctypes.data_as(nat.f64p), 3), "crp_select_splice_stats", self._ctx)
        return dict(zip(("splice_select_ms", "splice_eval_ms", "splice_window"), (float(v) for v in out)))

    def set_pair_limits(self, pair_slice_rows=0):
        nat.check(nat.lib().crp_select_set_pair_limits(self._h, int(pair_slice_rows)), "crp_select_set_pair_limits", self._ctx)

    def run_pairs(self, params, pair_params, self_search=None):
        """params: Params (its thresholds; K is not read); pair_params: PairParams; self_search as run()."""
        p, q = params.native(), pair_params.native()
        nat.check(nat.lib().crp_select_run_pairs(self._h, ctypes.byref(p), ctypes.byref(q), self_search._h if self_search is not None else None),
                  "crp_select_run_pairs", self._ctx)
        self.kp = pair_params.k

    def fetch_pairs(self):
        """(n_pass uint32 (G,), n_pairs uint64 (G,), pairs uint32 (G, KP, 2)) of the last run_pairs."""
        n_pass, n_pairs = np.empty(self.n_genes, np.uint32), np.empty(self.n_genes, np.uint64)
        pairs = np.empty((self.n_genes, max(1, self.kp), 2), np.uint32)
        nat.check(nat.lib().crp_select_fetch_pairs(self._h, n_pass.ctypes.data_as(nat.u32p), n_pairs.ctypes.data_as(nat.u64p),
                                                   pairs.ctypes.data_as(nat.u32p)), "crp_select_fetch_pairs", self._ctx)
        return n_pass, n_pairs, pairs

    def pairs_stats(self):
        out = np.zeros(8, dtype=np.float64)
        nat.check(nat.lib().crp_select_pairs_stats(self._h, out.ctypes.data_as(nat.f64p), 8), "crp_select_pairs_stats", self._ctx)
        keys = ("pass_key_ms", "pairs_ms", "merge_ms", "items", "launches", "longest_launch_ms", "pair_evaluations", "qualifying_pairs")
        return dict(zip(keys, (float(v) for v in out)))

    def set_pair_distinct_limits(self, items_per_launch=0):
        nat.check(nat.lib().crp_select_set_pair_distinct_limits(self._h, int(items_per_launch)), "crp_select_set_pair_distinct_limits", self._ctx)

    def run_pairs_distinct(self, params, pair_params, self_search=None):
        """As run_pairs(); the KP pairs of a gene share no guide (pair_params.distinct is not read)."""
        p, q = params.native(), pair_params.native()
        nat.check(nat.lib().crp_select_run_pairs_distinct(self._h, ctypes.byref(p), ctypes.byref(q),
                                                          self_search._h if self_search is not None else None),
                  "crp_select_run_pairs_distinct", self._ctx)
        self.kpd = pair_params.k

    def fetch_pairs_distinct(self):
        """(n_pass uint32 (G,), n_pairs uint64 (G,), n_distinct uint32 (G,), pairs uint32 (G, KP, 2)) of the last run_pairs_distinct."""
        n_pass, n_pairs, n_distinct = np.empty(self.n_genes, np.uint32), np.empty(self.n_genes, np.uint64), np.empty(self.n_genes, np.uint32)
        pairs = np.empty((self.n_genes, max(1, self.kpd), 2), np.uint32)
        nat.check(nat.lib().crp_select_fetch_pairs_distinct(self._h, n_pass.ctypes.data_as(nat.u32p), n_pairs.ctypes.data_as(nat.u64p),
                                                            n_distinct.ctypes.data_as(nat.u32p), pairs.ctypes.data_as(nat.u32p)),
                  "crp_select_fetch_pairs_distinct", self._ctx)
        return n_pass, n_pairs, n_distinct, pairs

    def pairs_distinct_stats(self):
        out = np.zeros(12, dtype=np.float64)
        nat.check(nat.lib().crp_select_pairs_distinct_stats(self._h, out.ctypes.data_as(nat.f64p), 12), "crp_select_pairs_distinct_stats", self._ctx)
        keys = ("pass_key_ms", "distinct_items_ms", "distinct_step_ms", "distinct_pick_ms", "distinct_rounds", "launches", "longest_launch_ms",
                "items", "cut_genes", "pair_evaluations", "pairs_taken", "qualifying_pairs")
        return dict(zip(keys, (float(v) for v in out)))


def arena_layout(genome, a):
    """[(contig index, arena offset, length)] of arena `a` of an engine.Genome, as annotate.Request.track takes it."""
    arena = genome.arenas[a]
    return [(k, int(arena.offsets[j]), int(arena.lengths[j])) for j, k in enumerate(genome.groups[a])]


class HitList(list):
    """A backend's per-contig hit dicts, with .selection (Selection) when the scan was asked to select."""
    selection = None


class Selection:
    """The selection over all genes of the GFF, in file order: labels, n_in, n_pass (per gene) and rows (ROW_DTYPE, gene
    after gene, rank 1 first; `index` is the row's place in its contig's strand table, `position` its match index local
    to the contig string), with counts (n, M + 1) uint32 and hit_sum (n,) uint64 of the rows when they were joined, and
    mh / oof (n,) uint32 of the rows when the repair scores were fetched (None otherwise).  With a pair selection: pairs
    (PAIR_DTYPE, gene after gene, rank 1 first; a is the left guide), n_pairs (per gene, all qualifying pairs), pairs_stats
    (with PairParams(distinct=True) the distinct run's, and n_pairs_distinct: per gene the pairs taken, at most KP)
    and, when the repair scores were fetched, pairs_repair (n, 2) uint64, packed, of a and b; None otherwise.  With the
    coding position (coding.py): cds_offset (coding.NOT_INSIDE where the cut is not inside the primary transcript),
    cds_length, transcripts_cut and transcripts (n,) uint32 of the rows, for the gene each was selected for; None otherwise.
    With base editing (baseedit.py): edit_targets, stop_codons and stop_offset (baseedit.NO_STOP where the edit writes no
    stop) (n,) uint32 of the rows, for the gene each was selected for, and cds_length; None otherwise.  With splice-site
    editing: splice_targets, donors, acceptors, donor_offset and acceptor_offset (baseedit.NO_SITE without a destroyed site of
    that kind) (n,) uint32 likewise, and cds_length; None otherwise."""

    def __init__(self, labels, n_in, n_pass, rows, counts=None, hit_sum=None, stats=None, mh=None, oof=None):
        self.labels, self.n_in, self.n_pass, self.rows = labels, n_in, n_pass, rows
        self.counts, self.hit_sum, self.stats = counts, hit_sum, stats or {}
        self.mh, self.oof = mh, oof
        self.variants = None  # (n,) uint32, packed (variants.unpack), of the rows when the variant counts were fetched
        self.guide_sites = self.assay_enzymes = None  # (n,) uint32 masks (sites.unpack) of the rows when the site column was fetched
        self.pairs = self.n_pairs = self.pairs_repair = self.n_pairs_distinct = None
        self.pairs_stats = {}
        self.cds_offset = self.cds_length = self.transcripts_cut = self.transcripts = None
        self.edit_targets = self.stop_codons = self.stop_offset = None
        self.splice_targets = self.donors = self.acceptors = self.donor_offset = self.acceptor_offset = None
        # with gene families (families.py), for the gene each row was selected for: (n,) arrays, and members: per row the
        # labels of the family members the guide covers (the gene itself where the row's family is not the gene's)
        self.outside_mm0 = self.outside_hit_sum = self.members_hit = self.family_size = self.fam_cover = self.members = None
        # with Request(family_sets=S): the picks (FAMILY_SET_DTYPE; families in table order, steps ascending), per family of the
        # table whether its set covers every member, and the driver's stats
        self.family_sets = self.family_complete = None
        self.family_sets_stats = {}

    def of_gene(self, g):
        return self.rows[self.rows["gene"] == g]


def _take(plus, minus, is_minus, row, dtype):
    """plus[row] where the row is a '+' row, minus[row] where it is a '-' row."""
    out = np.empty(row.size, dtype)
    out[~is_minus] = np.asarray(plus)[row[~is_minus]]
    out[is_minus] = np.asarray(minus)[row[is_minus]]
    return out


def assemble(labels, k, arenas, stats=None):
    """One Selection from per-arena results.  arenas: dicts with offsets / lengths (of the arena's texts), group (their
    contig indices), pos_plus / score_plus / pos_minus / score_minus (the tables, arena positions), gene (layout row ->
    gene index), n_in, n_pass, sel (layout rows x K), and optionally counts_plus / sum_plus / counts_minus / sum_minus
    and repair_plus / repair_minus (the packed repair scores of the tables' rows), and coding (dict: off and cover, layout
    rows x K beside sel, and length and n_tx per layout row) and edit (dict: targets, stops and stop_off, layout rows x K
    beside sel, and length per layout row) and splice (dict: targets, donors, acceptors, donor_off and acceptor_off, layout
    rows x K beside sel, and length per layout row).
    A gene that has rows in several texts (two contigs of one name) gets the sums of its counts and the first K of its
    rows in the definition's order, texts in arena order."""
    G = len(labels)
    n_in, n_pass = np.zeros(G, np.int64), np.zeros(G, np.int64)
    parts, cparts, sparts = [], [], []
    joined = any(a.get("counts_plus") is not None for a in arenas)
    repaired = any(a.get("repair_plus") is not None for a in arenas)
    varied = any(a.get("var_plus") is not None for a in arenas)
    vparts = []
    sited = any(a.get("sites_plus") is not None for a in arenas)
    stparts = []
    coded = any(a.get("coding") is not None for a in arenas)
    edited = any(a.get("edit") is not None for a in arenas)
    spliced = any(a.get("splice") is not None for a in arenas)
    familied = any(a.get("family") is not None for a in arenas)
    rparts, kparts, eparts, xparts, fparts = [], [], [], [], []
    for a in arenas:
        gene = np.asarray(a["gene"], dtype=np.int64)
        np.add.at(n_in, gene, np.asarray(a["n_in"], dtype=np.int64))
        np.add.at(n_pass, gene, np.asarray(a["n_pass"], dtype=np.int64))
        sel = np.asarray(a["sel"], dtype=np.uint32).reshape(gene.size, -1)[:, :k]
        r, c = np.nonzero(sel != NONE)
        packed = sel[r, c]
        minus = (packed >> np.uint32(31)).astype(bool)
        row = (packed & np.uint32(0x7FFFFFFF)).astype(np.int64)
        part = np.empty(row.size, ROW_DTYPE)
        offs = np.asarray(a["offsets"], dtype=np.int64)
        pos = _take(a["pos_plus"], a["pos_minus"], minus, row, np.int64)
        t = np.searchsorted(offs, pos, "right") - 1
        part["gene"], part["rank"] = gene[r], c + 1
        part["contig"] = np.asarray(a["group"], dtype=np.uint32)[t]
        part["position"] = pos - offs[t]
        part["strand"] = np.where(minus, b"-", b"+")
        part["score"] = _take(a["score_plus"], a["score_minus"], minus, row, np.float64)
        # the row's place in its contig's strand table: the rows of the texts before it, taken off
        first_plus = np.searchsorted(np.asarray(a["pos_plus"]), offs.astype(np.uint32), "left")
        first_minus = np.searchsorted(np.asarray(a["pos_minus"]), offs.astype(np.uint32), "left")
        part["index"] = row - np.where(minus, first_minus[t], first_plus[t])
        parts.append(part)
        if joined:
            cp, cm = np.asarray(a["counts_plus"], dtype=np.uint32), np.asarray(a["counts_minus"], dtype=np.uint32)
            width = cp.shape[1] if cp.ndim == 2 else cm.shape[1]
            cp, cm = cp.reshape(-1, width), cm.reshape(-1, width)
            c_rows = np.empty((row.size, width), np.uint32)
            c_rows[~minus], c_rows[minus] = cp[row[~minus]], cm[row[minus]]
            cparts.append(c_rows)
            sparts.append(_take(a["sum_plus"], a["sum_minus"], minus, row, np.uint64))
        if repaired:
            rparts.append(_take(a["repair_plus"], a["repair_minus"], minus, row, np.uint64))
        if varied:
            vparts.append(_take(a["var_plus"], a["var_minus"], minus, row, np.uint32))
        if sited:
            stparts.append(_take(a["sites_plus"], a["sites_minus"], minus, row, np.uint64))
        if coded:
            cod = a["coding"]
            kparts.append(np.stack([np.asarray(cod["off"], np.uint32).reshape(gene.size, -1)[r, c],
                                    np.asarray(cod["length"], np.uint32)[r],
                                    np.asarray(cod["cover"], np.uint32).reshape(gene.size, -1)[r, c],
                                    np.asarray(cod["n_tx"], np.uint32)[r]], axis=1) if r.size else np.empty((0, 4), np.uint32))
        if edited:
            ed = a["edit"]
            eparts.append(np.stack([np.asarray(ed[key], np.uint32).reshape(gene.size, -1)[r, c] for key in ("targets", "stops", "stop_off")]
                                   + [np.asarray(ed["length"], np.uint32)[r]], axis=1) if r.size else np.empty((0, 4), np.uint32))
        if spliced:
            sp = a["splice"]
            xparts.append(np.stack([np.asarray(sp[key], np.uint32).reshape(gene.size, -1)[r, c]
                                    for key in ("targets", "donors", "acceptors", "donor_off", "acceptor_off")]
                                   + [np.asarray(sp["length"], np.uint32)[r]], axis=1) if r.size else np.empty((0, 6), np.uint32))
        if familied:
            fm = a["family"]
            fparts.append(np.stack([np.asarray(fm[key]).reshape(gene.size, -1)[r, c].astype(np.uint64)
                                    for key in ("outside_mm0", "outside_hit_sum", "members_hit", "family_size", "fam_cover")], axis=1)
                          if r.size else np.empty((0, 5), np.uint64))
    rows = np.concatenate(parts) if parts else np.empty(0, ROW_DTYPE)
    counts = np.concatenate(cparts) if cparts else None
    sums = np.concatenate(sparts) if sparts else None
    packed_repair = np.concatenate(rparts) if rparts else None
    # genes in file order; a gene met in several texts: its rows in the definition's order, the first K of them
    key = rows["score"].view(np.uint64)
    order = np.lexsort((np.arange(rows.size), np.iinfo(np.uint64).max - key, rows["gene"]))
    rows = rows[order]
    start = np.searchsorted(rows["gene"], rows["gene"], "left")
    rank = np.arange(rows.size) - start
    keep = rank < k
    rows = rows[keep]
    rows["rank"] = rank[keep] + 1
    if counts is not None:
        counts, sums = counts[order][keep], sums[order][keep]
    mh = oof = None
    if packed_repair is not None:
        from .repair import unpack
        mh, oof = unpack(packed_repair[order][keep])
    out = Selection(list(labels), n_in, n_pass, rows, counts, sums, stats, mh, oof)
    if vparts:
        out.variants = np.concatenate(vparts)[order][keep]
    if stparts:
        from .sites import unpack as unpack_sites
        out.guide_sites, out.assay_enzymes = unpack_sites(np.concatenate(stparts)[order][keep])
    if kparts:
        cod = np.concatenate(kparts)[order][keep]
        out.cds_offset, out.cds_length, out.transcripts_cut, out.transcripts = (cod[:, j].copy() for j in range(4))
    if eparts:
        ed = np.concatenate(eparts)[order][keep]
        out.edit_targets, out.stop_codons, out.stop_offset, out.cds_length = (ed[:, j].copy() for j in range(4))
    if fparts:
        fm = np.concatenate(fparts)[order][keep]
        out.outside_mm0, out.members_hit, out.family_size = (fm[:, j].astype(np.uint32) for j in (0, 2, 3))
        out.outside_hit_sum, out.fam_cover = fm[:, 1].copy(), fm[:, 4].copy()
    if xparts:
        sp = np.concatenate(xparts)[order][keep]
        out.splice_targets, out.donors, out.acceptors, out.donor_offset, out.acceptor_offset, out.cds_length = (sp[:, j].copy() for j in range(6))
    return out


def assemble_pairs(n_genes, kp, arenas):
    """(pairs PAIR_DTYPE, n_pairs int64 (n_genes,), repair (n, 2) uint64 or None) from per-arena results.  arenas: the dicts
    assemble() takes, with pair_n_pairs and pair_list (layout rows x KP x 2) beside them.  A pair never spans texts; a gene
    met in several texts gets the sum of its n_pairs and the first KP of its pairs in the definition's order."""
    n_pairs = np.zeros(n_genes, np.int64)
    parts, keys, rparts = [], [], []
    repaired = any(a.get("repair_plus") is not None for a in arenas)
    for a in arenas:
        gene = np.asarray(a["gene"], dtype=np.int64)
        np.add.at(n_pairs, gene, np.asarray(a["pair_n_pairs"]).astype(np.int64))
        lst = np.asarray(a["pair_list"], dtype=np.uint32).reshape(gene.size, -1, 2)[:, :kp]
        r, c = np.nonzero(lst[:, :, 0] != NONE)
        part = np.empty(r.size, PAIR_DTYPE)
        part["gene"], part["rank"] = gene[r], c + 1
        offs = np.asarray(a["offsets"], dtype=np.int64)
        first = {False: np.searchsorted(np.asarray(a["pos_plus"]), offs.astype(np.uint32), "left"),
                 True: np.searchsorted(np.asarray(a["pos_minus"]), offs.astype(np.uint32), "left")}
        cut, sbits, rep = [], [], []
        for side, which in (("a", 0), ("b", 1)):
            packed = lst[r, c, which]
            minus = (packed >> np.uint32(31)).astype(bool)
            row = (packed & np.uint32(0x7FFFFFFF)).astype(np.int64)
            pos = _take(a["pos_plus"], a["pos_minus"], minus, row, np.int64)
            t = np.searchsorted(offs, pos, "right") - 1
            if which == 0:
                part["contig"] = np.asarray(a["group"], dtype=np.uint32)[t] if r.size else 0
            part["position_" + side] = pos - offs[t]
            part["strand_" + side] = np.where(minus, b"-", b"+")
            part["score_" + side] = _take(a["score_plus"], a["score_minus"], minus, row, np.float64)
            part["index_" + side] = row - np.where(minus, first[True][t], first[False][t])
            cut.append(part["position_" + side] + np.where(minus, 6, -3))
            sbits.append(minus.astype(np.int64))
            if repaired:
                rep.append(_take(a["repair_plus"], a["repair_minus"], minus, row, np.uint64))
        part["deletion_length"] = cut[1] - cut[0]
        parts.append(part)
        big = np.iinfo(np.uint64).max
        ka, kb = part["score_a"].view(np.uint64), part["score_b"].view(np.uint64)
        # (texts in arena order: a gene's pairs from different texts cannot tie on everything, and if two texts give equal
        # keys the earlier text goes first, as assemble() has it)
        keys.append(np.stack([big - np.minimum(ka, kb), big - np.maximum(ka, kb), cut[0].astype(np.uint64), cut[1].astype(np.uint64),
                              (sbits[0] * 2 + sbits[1]).astype(np.uint64)], axis=1) if r.size else np.empty((0, 5), np.uint64))
        if repaired:
            rparts.append(np.stack(rep, axis=1) if r.size else np.empty((0, 2), np.uint64))
    pairs = np.concatenate(parts) if parts else np.empty(0, PAIR_DTYPE)
    key = np.concatenate(keys) if keys else np.empty((0, 5), np.uint64)
    order = np.lexsort((np.arange(pairs.size), key[:, 4], key[:, 3], key[:, 2], key[:, 1], key[:, 0], pairs["gene"]))
    pairs = pairs[order]
    start = np.searchsorted(pairs["gene"], pairs["gene"], "left")
    rank = np.arange(pairs.size) - start
    keep = rank < kp
    pairs = pairs[keep]
    pairs["rank"] = rank[keep] + 1
    repair = np.concatenate(rparts)[order][keep] if rparts else None
    return pairs, n_pairs, repair


def assemble_n_distinct(n_genes, kp, arenas):
    """Per gene the distinct pairs taken (int64): the sum of pair_n_distinct over the gene's texts, capped at KP -- pairs of
    different texts share no row, so the merged list holds that many."""
    total = np.zeros(n_genes, np.int64)
    for a in arenas:
        np.add.at(total, np.asarray(a["gene"], dtype=np.int64), np.asarray(a["pair_n_distinct"]).astype(np.int64))
    return np.minimum(total, kp)


def select_arena_pairs(sel, request, handle=None):
    """The pair selection of one arena on the ArenaSelect that has just run the single-guide selection (its flags and
    limits are set): (n_pass, n_pairs, pairs, stats).  With request.pairs.distinct the distinct run INSTEAD of the plain
    one -- it returns n_pass and n_pairs itself -- and a fifth element, n_distinct."""
    if request.pair_slice_rows:
        sel.set_pair_limits(request.pair_slice_rows)
    if getattr(request.pairs, "distinct", False):
        sel.run_pairs_distinct(request.params, request.pairs, handle)
        n_pass, n_pairs, n_distinct, pairs = sel.fetch_pairs_distinct()
        return n_pass, n_pairs, pairs, sel.pairs_distinct_stats(), n_distinct
    sel.run_pairs(request.params, request.pairs, handle)
    return sel.fetch_pairs() + (sel.pairs_stats(),)


def _set_row_limits(sel, request, flags=None):
    """The terms of the predicate that do not depend on the gene, on an ArenaSelect: the CDS flags, the slices, the property,
    the repair and the variant limits of a Request."""
    if request.params.require_cds:
        sel.set_flags(flags if flags is not None else request.annotation.annotation.cds_flags())
    if request.slice_rows:
        sel.set_limits(request.slice_rows)
    if getattr(request, "property_limits", None) is not None:
        sel.set_property_limits(request.property_limits)
    if getattr(request, "repair_limits", None) is not None:
        sel.set_repair_limits(request.repair_limits)
    if getattr(request, "variant_limits", None) is not None:
        sel.set_variant_limits(request.variant_limits)
    if getattr(request, "site_limits", None) is not None:
        sel.set_site_limits(request.site_limits)


def _set_families(sel, request, gene):
    """The families of an ArenaSelect's layout rows (gene: layout row -> gene index) and the request's family limits."""
    table = request.families
    g = np.asarray(gene, dtype=np.int64)
    gene_family = table.gene_family[g] if g.size else np.zeros(0, np.uint32)
    size = np.array([table.family_size(int(x)) for x in g.tolist()], dtype=np.uint32)
    sel.set_family(gene_family, size)
    sel.set_family_limits(request.family_limits)


def select_arena(genome, a, request, handle=None, flags=None, extras=None):
    """The selection of one arena of an engine.Genome whose tables are resident: (lo, hi, gene, n_in, n_pass, sel, stats),
    and with request.pairs one more element: (n_pass, n_pairs, pairs, pairs_stats) of the pair selection.  extras: a dict
    that receives the optional parts by name -- with request.coding, extras["coding"] = dict(off, cover: of the selected
    rows, beside sel; where sel has no row, coding.NOT_INSIDE and 0; length, n_tx: per layout row).  Without extras the model
    and the limits are still set, and the selected rows are not evaluated.  With request.edit likewise extras["edit"] =
    dict(targets, stops, stop_off: of the selected rows, beside sel; where sel has no row, 0, 0 and baseedit.NO_STOP; length:
    per layout row), and with request.splice extras["splice"] = dict(targets, donors, acceptors, donor_off, acceptor_off: of
    the selected rows; where sel has no row, 0, 0, 0 and baseedit.NO_SITE twice; length: per layout row).
    handle: the arena's search.ArenaSelfSearch after join_hits, or None."""
    lo, hi, gene = request.annotation.gene_layout(arena_layout(genome, a))
    sel = ArenaSelect(genome.arenas[a], lo, hi)
    try:
        _set_row_limits(sel, request, flags)
        model = None
        edit = getattr(request, "edit", False)
        splice = getattr(request, "splice", False)
        if getattr(request, "coding", False) or edit or splice:
            model = request.annotation.coding_layout(arena_layout(genome, a))
            sel.set_coding(model)
            if getattr(request, "coding_limits", None) is not None:
                sel.set_coding_limits(request.coding_limits)
            if edit and request.edit_limits is not None:
                sel.set_edit_limits(request.edit_window, request.edit_limits)
            if splice and request.splice_limits is not None:
                sel.set_splice_limits(request.splice_window, request.editor, request.splice_limits)
        table = getattr(request, "families", None)
        if table is not None:
            _set_families(sel, request, gene)
        sel.run(request.params, handle)
        n_in, n_pass, picked = sel.fetch()
        stats = sel.stats()
        if getattr(request, "min_spacing", None) is not None:  # the plain run gave n_in and n_pass; the picks are the spaced run's
            sel.run_spaced(request.params, request.min_spacing, handle)
            spaced_pass, _, picked = sel.fetch_spaced()
            assert np.array_equal(spaced_pass, n_pass), "the spaced selection and the plain selection count different passing rows"
            stats.update(sel.spaced_stats())
        if table is not None and extras is not None:
            r, c = np.nonzero(picked != NONE)
            fm = dict(outside_mm0=np.zeros(picked.shape, np.uint32), outside_hit_sum=np.zeros(picked.shape, np.uint64),
                      members_hit=np.zeros(picked.shape, np.uint32), family_size=np.zeros(picked.shape, np.uint32),
                      fam_cover=np.zeros(picked.shape, np.uint64))
            got = sel.family_eval(handle, r.astype(np.uint32), picked[r, c])
            for key, v in zip(("outside_mm0", "outside_hit_sum", "members_hit", "family_size", "fam_cover"), got):
                fm[key][r, c] = v
            extras["family"] = fm
        if table is not None:
            stats.update(sel.family_stats())
        if edit and extras is not None:
            from .baseedit import NO_STOP
            r, c = np.nonzero(picked != NONE)
            targets, stops, stop_off = np.zeros(picked.shape, np.uint32), np.zeros(picked.shape, np.uint32), np.full(picked.shape, NO_STOP, np.uint32)
            targets[r, c], stops[r, c], stop_off[r, c] = sel.edit_eval(request.edit_window, r.astype(np.uint32), picked[r, c])
            extras["edit"] = dict(targets=targets, stops=stops, stop_off=stop_off, length=model["length"])
        if edit:
            stats.update(sel.edit_stats())
        if splice and extras is not None:
            from .baseedit import NO_SITE
            r, c = np.nonzero(picked != NONE)
            zero, none = (lambda: np.zeros(picked.shape, np.uint32)), (lambda: np.full(picked.shape, NO_SITE, np.uint32))
            sp = dict(targets=zero(), donors=zero(), acceptors=zero(), donor_off=none(), acceptor_off=none(), length=model["length"])
            got = sel.splice_eval(request.splice_window, request.editor, r.astype(np.uint32), picked[r, c])
            for key, v in zip(("targets", "donors", "acceptors", "donor_off", "acceptor_off"), got):
                sp[key][r, c] = v
            extras["splice"] = sp
        if splice:
            stats.update(sel.splice_stats())
            stats["editor"] = request.editor.name
        if getattr(request, "coding", False) and extras is not None:
            from .coding import NOT_INSIDE
            r, c = np.nonzero(picked != NONE)
            off, cover = np.full(picked.shape, NOT_INSIDE, np.uint32), np.zeros(picked.shape, np.uint32)
            off[r, c], cover[r, c] = sel.coding_eval(r.astype(np.uint32), picked[r, c])
            extras["coding"] = dict(off=off, cover=cover, length=model["length"], n_tx=model["info"] & np.uint32(0xFFFF))
        if getattr(request, "coding", False):
            stats.update(sel.coding_stats())
        out = lo, hi, gene, n_in, n_pass, picked, stats
        if getattr(request, "pairs", None) is not None:  # right after the single guides, on the same handle
            out += (select_arena_pairs(sel, request, handle),)
        return out
    finally:
        sel.close()


def family_sets(genome, request, handle_of, hits, flags=None):
    """The greedy family sets of a Request(family_sets=S): family_sets.py has the definition and the driver."""
    from .family_sets import family_sets as run
    return run(genome, request, handle_of, hits, flags)


def sum_stats(total, one):
    for key, v in one.items():
        if key == "spaced_longest_launch_ms":
            total[key] = max(total.get(key, 0.0), v)
        elif key in ("bytes_per_row", "edit_targets_window", "splice_window", "editor"):
            total[key] = v
        else:
            total[key] = max(total.get(key, 0.0), v) if key == "longest_launch_ms" else total.get(key, 0.0) + v
    return total
