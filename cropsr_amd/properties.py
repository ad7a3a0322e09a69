"""--properties: GC content, homopolymer runs, poly-T and hairpin stem of every guide.

Not in the reference, opt-in.  Design tools report and filter on the guide's own sequence quality; Rule Set 1's GC term
was dropped by the reference, so it cannot be recovered from on_site_score.  Every one of
these quantities is a pure function of the l letters of the guide, which already sit in the arena's bit-planes next to
the hit tables: one more per-hit kernel (csrc/crp_properties.hip) and one more column.

Definition, per row of an arena's hit tables after a scan at guide length l, 1 <= l <= 50
(tests/guide_properties_reference.py restates it twice):

  window   l characters of the forward text: s[i - l : i] for a '+' row with match index i, s[j + 3 : j + 3 + l] for a
           '-' row with match index j (the i and j of the CSV join and of crp_annotate_lookup).
  bases    a window letter is a BASE when its `ac` bit is set; its code comes from the `hi` / `lo` planes.  Case is
           ignored (the `up` plane is not read) and U is A, as the arena packs it.  Everything else is a non-base: N,
           IUPAC letters, Z, decoration, and void positions -- a '-' row may have up to 10 of those, because the
           reference keeps '-' rows up to len + 10.  A plane word beyond the arena's last word is never read; the
           positions there are non-bases.
  gc       the number of window letters that are C or G.
  run      the length of the longest run of equal bases.  A non-base ends a run; 0 if the window holds no base.
  t_run    the longest run of T in the spacer's own orientation (four of them end Pol III transcription): a run of T in
           the window of a '+' row, a run of A in the window of a '-' row, whose spacer is the window's reverse
           complement.
  stem     the largest s >= 0 such that indices a, b exist in the window with w[a + t] complementary to w[b - t] for
           t = 0 .. s - 1 and (b - s + 1) - (a + s) >= 3.  Complementary means A-T or C-G with both letters bases; no
           wobble pair.  The second condition leaves at least 3 unpaired letters in the loop.  The value does not
           change under reverse complement, so it needs no strand rule; it is at most (l - 3) // 2.
           Equivalently: over every anti-diagonal c = p + q, the longest run in p of pairs (p, q) that are
           complementary and have q - p >= 4 -- the form the kernel computes.
  packing  one uint32 per row: gc | run << 8 | t_run << 16 | stem << 24.

This module names the columns, unpacks the word and turns the command line's GC percentages into counts.
"""
import numpy as np

HEADER = ["guide_gc", "guide_run", "guide_t_run", "guide_stem"]  # the four opt-in CSV columns, after the specificity columns
GUIDE_LENGTHS = (1, 50)
NO_LIMIT = 0xFF  # every value is one byte


def pack(gc, run, t_run, stem):
    g, r, t, s = (np.asarray(v).astype(np.uint32) for v in (gc, run, t_run, stem))
    return g | r << np.uint32(8) | t << np.uint32(16) | s << np.uint32(24)


def unpack(packed):
    """(gc, run, t_run, stem) uint8 arrays of a packed column."""
    p = np.asarray(packed, dtype=np.uint32)
    return tuple(((p >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.uint8) for k in range(4))


def gc_count_bounds(pct_min, pct_max, guide_len):
    """GC percentages (integers 0..100, None: no bound) as counts of a guide of guide_len letters, exactly:
    ceil(pct_min * l / 100) and floor(pct_max * l / 100), in integer arithmetic."""
    l = int(guide_len)
    lo = 0 if pct_min is None else -((-int(pct_min) * l) // 100)
    hi = NO_LIMIT if pct_max is None else (int(pct_max) * l) // 100
    return lo, hi


class Limits:
    """The bounds a selection puts on the properties, as counts: gc_min <= gc <= gc_max, run <= max_run, t_run <=
    max_t_run, stem <= max_stem (None: no bound)."""

    def __init__(self, gc_min=None, gc_max=None, max_run=None, max_t_run=None, max_stem=None):
        vals = []
        for name, v, default in (("gc_min", gc_min, 0), ("gc_max", gc_max, NO_LIMIT), ("max_run", max_run, NO_LIMIT),
                                 ("max_t_run", max_t_run, NO_LIMIT), ("max_stem", max_stem, NO_LIMIT)):
            v = default if v is None else int(v)
            if not 0 <= v <= 0xFFFFFFFF:
                raise ValueError("%s must be a count, not %r" % (name, v))
            vals.append(v)
        self.gc_min, self.gc_max, self.max_run, self.max_t_run, self.max_stem = vals

    def astuple(self):
        return (self.gc_min, self.gc_max, self.max_run, self.max_t_run, self.max_stem)

    def passes(self, packed):
        """Boolean array: which rows of a packed column pass."""
        gc, run, t_run, stem = (v.astype(np.int64) for v in unpack(packed))
        return (gc >= self.gc_min) & (gc <= self.gc_max) & (run <= self.max_run) & (t_run <= self.max_t_run) & (stem <= self.max_stem)
