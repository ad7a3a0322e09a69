"""--coding: where in the coding sequence a guide cuts.

Not in the reference, opt-in.  The selection (select.py) knows a guide's score, its specificity, its sequence and the
repair outcome of its cut; this adds what the cut does to the PROTEIN: how far into the coding sequence of the gene it
lies, and in how many of the gene's transcripts.  The model of every gene is built on the host from the GFF
(csrc/crp_annotation.cpp); the test of every row against the model of the gene it is being selected for runs on the device
inside the selection (csrc/crp_coding.h, csrc/crp_select_coding.hip).  tests/select_coding_reference.py restates the
definition twice.

Definition.

  rows read    as the annotation join reads them: lines not starting with '#', with at least 9 tab-separated fields and
               all-digit start / end; attributes split as there (at ';', parts stripped, key before the first '=', the
               first occurrence of a key wins).  The types are `gene`, `CDS`, `mRNA` and `transcript`.
  transcripts  A transcript of gene G (G has a non-empty ID) is an mRNA or transcript row on G's seqid of whose Parent
               values (a comma-separated list; empty values name nothing) one equals G's ID.  Its CDS rows are the CDS rows
               on that seqid with a Parent value equal to the transcript's ID.  CDS rows whose Parent equals G's ID directly
               form one more, implicit, transcript of G.  Children may come before parents: links are resolved after the
               whole file is read.  Of several gene rows, or several transcript rows, with one ID (on one seqid) the first
               in file order owns the children; the later ones get none.  A transcript without usable CDS rows is not a
               coding transcript and is not counted.  CDS rows with start > end are dropped.
  coding       The coding letters of transcript T are the union of its CDS rows' closed ranges; overlaps and duplicates
  letters      merge; they are not clipped to the gene's range.  L_T is their number.
  strand       the gene row's column 7; anything but + or - means the gene has no model.  The CDS rows' own strand and phase
               columns are not read.
  primary P    the coding transcript with the largest L_T; on a tie the earlier transcript row, the implicit transcript
               counting as placed at the gene row.  (Phytozome's longest=1 attribute is not read.)
  n_tx         the number of coding transcripts.  A gene with n_tx = 0 has no model; nor has one whose L_P exceeds
               2^32 - 1, more than a contig holds.
  cut          of a row: the boundary c of repair.py, between s[c - 1] and s[c], c = i - 3 on the '+' table and c = j + 6
               on the '-' table.  NOT the cut site that decides membership in the gene, which stays as it is.  Coordinates
               map to string indices by the rule of crp_annotation_track: index = coordinate + dec - 1.
  inside       the cut is inside T's coding sequence when s[c - 1] and s[c] are both coding letters of T (a cut exactly on
               an exon edge is not inside, and a one-letter CDS holds no cut).
  cover        the number of coding transcripts of G the cut is inside.
  off          defined when the cut is inside P: P's coding letters 5' of the cut in the gene's orientation, counted on the
               whole contig.  With cum_P(c) = P's coding letters with index < c: off = cum_P(c) for a '+' gene and
               L_P - cum_P(c) for a '-' gene, so 1 <= off <= L_P - 1.
  limits       min_pct <= max_pct and min_transcripts_pct, integers 0..100.  With coding limits a row passes for gene g
               only if, beyond select.py's predicate, g has a model, the cut is inside P,
               min_pct L_P <= 100 off <= max_pct L_P and 100 cover >= min_transcripts_pct n_tx (integers, 64-bit products).
               n_in is unchanged; n_pass counts the rows that pass this too.  The test is relative to g: a row shared by
               two overlapping genes may pass for one and fail for the other.  Pairs are refused with coding limits.
"""
import numpy as np

NOT_INSIDE = 0xFFFFFFFF  # `off` of a cut that is not inside P
MODEL_BIT, MINUS_BIT = 1 << 17, 1 << 16  # of a layout row's info word (n_tx in its low 16 bits)
HEADER = ["cds_offset", "cds_length", "cds_percent", "transcripts_cut", "transcripts"]


class Limits:
    """The bounds a selection puts on the coding position: min_pct L_P <= 100 off <= max_pct L_P and
    100 cover >= min_transcripts_pct n_tx, all integer percentages 0..100."""

    def __init__(self, min_pct=0, max_pct=100, min_transcripts_pct=0):
        vals = []
        for name, v in (("min_pct", min_pct), ("max_pct", max_pct), ("min_transcripts_pct", min_transcripts_pct)):
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 100:
                raise ValueError("%s is a percentage, an integer 0..100, not %r" % (name, v))
            vals.append(int(v))
        self.min_pct, self.max_pct, self.min_transcripts_pct = vals
        if self.min_pct > self.max_pct:
            raise ValueError("min_pct %d lies above max_pct %d" % (self.min_pct, self.max_pct))

    def astuple(self):
        return (self.min_pct, self.max_pct, self.min_transcripts_pct)

    def passes(self, model, off, cover, length, n_tx):
        """Boolean array from arrays: model (the gene has one), off (NOT_INSIDE outside P), cover, L_P and n_tx."""
        off, cover, length, n_tx = (np.asarray(v).astype(object) for v in (off, cover, length, n_tx))  # (exact integers)
        inside = np.asarray(model, dtype=bool) & (off != NOT_INSIDE)
        ok = (self.min_pct * length <= 100 * off) & (100 * off <= self.max_pct * length) & (100 * cover >= self.min_transcripts_pct * n_tx)
        return inside & ok.astype(bool)


def percent(off, length):
    """cds_percent of the selection file: 100 off / L_P with one decimal, rounded half up in integers."""
    tenths = (2000 * int(off) + int(length)) // (2 * int(length))
    return "%d.%d" % divmod(tenths, 10)


def fields(off, length, cover, n_tx):
    """The five fields of a selection row: cds_offset, cds_length, cds_percent (empty when the cut is not inside P),
    transcripts_cut, transcripts."""
    if int(off) == NOT_INSIDE:
        return ("", "", "", int(cover), int(n_tx))
    return (int(off), int(length), percent(off, length), int(cover), int(n_tx))
