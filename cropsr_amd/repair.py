"""--repair-scores: the microhomology score and the out-of-frame score of every guide's cut.

Not in the reference, opt-in.  A double-strand break next to microhomologies is mostly repaired by microhomology-mediated
end joining, and the deletions it leaves are predictable from the letters around the cut (Bae, Kweon, Kim and Kim 2014).
If most of the predicted deletions have a length that is a multiple of 3 the gene stays in frame, and the guide is a poor
choice for a knock-out however well it cuts.  Both numbers are pure functions of letters that already sit in the arena's
bit-planes next to the hit tables: one more per-hit kernel (csrc/crp_repair.hip) and one 8-byte column that stays on the
device for the selection (select.py).  The column is not part of the main guide table.

Definition, per row of an arena's hit tables after any scan (tests/repair_reference.py restates it twice).  The guide
length is not used; the one parameter is the flank F, 2 <= F <= 32, default 30.

  cut       the boundary c between s[c - 1] and s[c]: c = i - 3 for a '+' row with match index i, c = j + 6 for a '-' row
            with match index j (`CC.` at j).  That is three letters into the protospacer from the PAM on either strand.
            It is NOT the CSV's `cutsite` column, which for '-' rows is the reference's end_pos - 3 = j.
  window    w[p] = s[c - F + p] for p = 0 .. 2 F - 1; the left flank is p < F, the right flank p >= F.
  bases     a window letter is a BASE when its `ac` bit is set; its code comes from the `hi` / `lo` planes.  Case is
            ignored (the `up` plane is not read) and U is A, as the arena packs it.  Everything else is a non-base: N,
            IUPAC letters, Z, decoration, void positions, positions below 0 and positions in a plane word at or beyond
            the arena's word count (never read).  Contigs lie at least 64 void positions apart, so a flank of at most
            32 never reaches a neighbour.
  diagonal  for a deletion length d = 1 .. 2 F - 1 the left copy's letters are p in [max(0, F - d), min(F, 2 F - d)) and
            the right copy's are p + d, which lie in [F, 2 F).  m_d(p) holds when w[p] and w[p + d] are bases and equal.
            A MICROHOMOLOGY is a maximal run of m_d inside that range of length k >= 2; it adds k + (its letters that
            are C or G) to n_d.  Equivalently: every (k >= 2, i, j) with w[i : i + k] == w[j : j + k], all bases,
            i + k <= F, j >= F, j + k <= 2 F, longest first, dropping a pattern nested in a kept one on the same
            diagonal; each kept pattern adds k + gc.  No cap on k.
  weights   W[d] = floor(1000 exp(-d / 20) + 1/2) for d = 1 .. 63, a committed table of 63 integers
            (csrc/microhomology_weights.def).  The table is the definition.
  result    mh = sum over d of W[d] n_d; oof = the same over the d with d mod 3 != 0.  Integers: exact, in any order.
            One uint64 per row, mh | oof << 32; both stay below 2^20.  Every row gets a value, the unscored ones too; a
            window without a microhomology gives 0.  The pair does not change under reverse complement of the window,
            so the strand enters through c alone.
  published microhomology score = mh / 10, out-of-frame score = 100 oof / mh.

This module reads the weight table, unpacks the column, formats the two CSV fields and turns the command line's
thresholds into the integers the selection kernel compares.
"""
import os

import numpy as np

HEADER = ["mh_score", "oof_score"]  # the two opt-in fields at the end of a selection-file row
FLANKS = (2, 32)
DEFAULT_FLANK = 30


def _read_weights():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "microhomology_weights.def")
    with open(path) as f:
        body = "".join(line for line in f if not line.lstrip().startswith("//"))
    w = [int(v) for v in body.replace(",", " ").split()]
    if len(w) != 63:
        raise RuntimeError("microhomology_weights.def holds %d weights, not 63" % len(w))
    return tuple(w)


WEIGHTS = _read_weights()  # WEIGHTS[d - 1] = W[d]


def check_flank(flank):
    f = int(flank)
    if not FLANKS[0] <= f <= FLANKS[1]:
        raise ValueError("a flank of %d..%d letters on either side of the cut is scored, not %r" % (FLANKS + (flank,)))
    return f


def pack(mh, oof):
    return np.asarray(mh).astype(np.uint64) | np.asarray(oof).astype(np.uint64) << np.uint64(32)


def unpack(col):
    """(mh, oof) uint32 arrays of a packed column."""
    c = np.asarray(col, dtype=np.uint64)
    return (c & np.uint64(0xFFFFFFFF)).astype(np.uint32), (c >> np.uint64(32)).astype(np.uint32)


def scores(col):
    """(microhomology score mh / 10, out-of-frame score 100 oof / mh with -1 where mh = 0) as float64 arrays."""
    mh, oof = (v.astype(np.float64) for v in unpack(col))
    with np.errstate(divide="ignore", invalid="ignore"):
        pct = np.where(mh > 0, (100.0 * oof) / mh, -1.0)
    return mh / 10.0, pct


def fields(value):
    """The two CSV fields of one packed value: mh_score printed exactly, oof_score as Python divides (-1 at mh = 0)."""
    mh, oof = int(value) & 0xFFFFFFFF, int(value) >> 32
    return "%d.%d" % divmod(mh, 10), (100 * oof) / mh if mh else -1


def parse_min_mh(text):
    """A microhomology score threshold -- a decimal with at most one fractional digit, e.g. 12 or 12.5 -- as tenths, in
    integer arithmetic."""
    t = str(text).strip()
    whole, dot, frac = t.partition(".")
    if not whole or not whole.isdigit() or not whole.isascii() or (dot and not (len(frac) == 1 and frac.isdigit() and frac.isascii())):
        raise ValueError("a microhomology score is a decimal with at most one fractional digit, not %r" % (text,))
    tenths = int(whole) * 10 + (int(frac) if frac else 0)
    if tenths > 0xFFFFFFFF:
        raise ValueError("a microhomology score of %s keeps no guide" % t)
    return tenths


class Limits:
    """The bounds a selection puts on the repair scores: mh >= min_mh (tenths) and 100 oof >= min_oof mh (min_oof an
    integer percentage 0..100; None: no bound).  With min_oof > 0 a row with mh = 0 fails."""

    def __init__(self, min_mh=None, min_oof=None):
        self.min_mh = 0 if min_mh is None else int(min_mh)
        self.min_oof = 0 if min_oof is None else int(min_oof)
        if not 0 <= self.min_mh <= 0xFFFFFFFF:
            raise ValueError("min_mh is a score in tenths, not %r" % (min_mh,))
        if not 0 <= self.min_oof <= 100:
            raise ValueError("min_oof is a percentage, an integer 0..100, not %r" % (min_oof,))

    def astuple(self):
        return (self.min_mh, self.min_oof)

    def passes(self, col):
        """Boolean array: which rows of a packed column pass."""
        mh, oof = (v.astype(np.int64) for v in unpack(col))
        return (mh >= self.min_mh) & (100 * oof >= self.min_oof * mh) & ((mh > 0) | (self.min_oof == 0))
