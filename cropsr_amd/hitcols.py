"""The per-hit columns of the host's hit tables, declared once (their device side: csrc/crp_gather_cols.h).

A hit table is a plain dict keyed <stem>_plus / <stem>_minus (one array per strand, rows ascending by position); engine.Hits
and node.NodeHits hold the same columns as attributes of those names.  COLUMNS is the one list of stems, and everything that
slices, filters, joins or prints hit tables walks it through the helpers below: a new column is declared here and filled by
its producer, nowhere else.  numpy only: no library, no GPU.
"""
import collections

import numpy as np

STRANDS = ("plus", "minus")
UNJOINED_COUNT, UNJOINED_SUM = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF  # --specificity: a hit without a guide site's row (search.py, CSV join)
OFFTARGET_HEADER = ["offtarget_seed_mm0", "offtarget_seed_mm1", "offtarget_seed_mm2", "offtarget_seed_mm3"]  # --offtarget
PROPERTIES_HEADER = ["guide_gc", "guide_run", "guide_t_run", "guide_stem"]  # --properties (properties.py)
ANY_WIDTH = -1  # trailing shape (n, whatever the arrays have): self_counts is (n, M + 1)


def SPECIFICITY_HEADER(M):
    """The M + 3 opt-in column names of --specificity at M mismatches: self_mm0 .. self_mmM, self_hit_sum, specificity."""
    return ["self_mm%d" % k for k in range(int(M) + 1)] + ["self_hit_sum", "specificity"]


def _count_fields(v):  # one row's counts; 0xFFFFFFFF (not a site / UNJOINED_COUNT) prints as -1
    return tuple(-1 if int(x) == UNJOINED_COUNT else int(x) for x in v)


def _sum_fields(v):  # hit_sum and the specificity (search.specificity's expression; csv writes repr(float)); unjoined: -1, -1
    hs = int(v)
    return (-1, -1) if hs == UNJOINED_SUM else (hs, float(1.0 / (1.0 + np.float64(np.uint64(hs)) / float(1 << 30))))


def _property_fields(v):  # guide_gc, guide_run, guide_t_run, guide_stem: the four bytes of the packed word
    return tuple(int(v) >> (8 * b) & 255 for b in range(4))


# stem; dtype; width: None for (n,), else the trailing shape (n, width); always: every table has it; and for the opt-in CSV
# columns, in CSV order: option, the keyword of rows.extra_header that switches it on; header(option's value) -> names;
# fields(one row's value) -> the fields of the tuple path (rows.ContigRows, the specification of crp_format.cpp's bytes).
Column = collections.namedtuple("Column", "stem dtype width always option header fields", defaults=(None, False, None, None, None))
COLUMNS = [
    Column("pos", np.uint32, always=True),
    Column("score", np.float64, always=True),
    Column("pre", np.float64),  # the pre-sigmoid sum (want_pre)
    Column("ot", np.uint32, 4, option="offtarget", header=lambda on: OFFTARGET_HEADER, fields=_count_fields),
    Column("feat", np.uint32),  # label-set ids (--annotate); printed through the string table, not as fields of its own
    Column("self_counts", np.uint32, ANY_WIDTH, option="specificity", header=lambda M: SPECIFICITY_HEADER(M)[:-2], fields=_count_fields),
    Column("self_sum", np.uint64, option="specificity", header=lambda M: SPECIFICITY_HEADER(M)[-2:], fields=_sum_fields),
    Column("props", np.uint32, option="properties", header=lambda on: PROPERTIES_HEADER, fields=_property_fields),
]


def keys(stems=None):
    """(<stem>_plus, <stem>_minus) of every stem of the list `stems`, in its order; by default of every column of COLUMNS."""
    return tuple("%s_%s" % (stem, strand) for stem in ([c.stem for c in COLUMNS] if stems is None else stems) for strand in STRANDS)


def csv_columns():
    """The columns that print as opt-in CSV fields, in CSV order."""
    return [c for c in COLUMNS if c.fields is not None]


def csv_header(**options):
    """The opt-in column names in the order the rows carry them; options: offtarget=True, specificity=M, properties=True."""
    out = []
    for c in csv_columns():
        value = options.get(c.option)
        if value is not None and value is not False:
            out += c.header(value)
    return out


def take(hits, plus, minus, origin=None):
    """The rows plus / minus (a slice -- the result is then a view --, a mask or an index array) of every column `hits`
    (a mapping by key; an object's vars() will do) holds, as a new hit dict.  A key that is absent stays absent, one that
    holds None stays None.  origin: positions are counted from there (pos - origin, a copy, origin == 0 too)."""
    out = {}
    for c in COLUMNS:
        for strand, rows in zip(STRANDS, (plus, minus)):
            key = c.stem + "_" + strand
            if key in hits:
                col = hits[key]
                if col is not None:
                    col = np.asarray(col)[rows]
                    if c.stem == "pos" and origin is not None:
                        col = col - np.uint32(origin) if origin >= 0 else col + np.uint32(-origin)
                out[key] = col
    return out


def concat(parts):
    """One hit dict from a list of them, rows part after part; a column the first part lacks (absent or None) is left out,
    the always-present ones exist (empty) even without parts."""
    out = {}
    for c in COLUMNS:
        for key in keys([c.stem]):
            if parts and parts[0].get(key) is not None:
                out[key] = np.concatenate([p[key] for p in parts])
            elif c.always:
                out[key] = np.empty(0, c.dtype)
    return out


def both(hits, stem):
    """One column's '+' rows, then its '-' rows, as one contiguous array of the column's dtype and trailing shape -- the order
    rows.ContigRows / ContigTable hold a contig's rows in -- or None when the dict lacks the column."""
    p, m = (hits.get(key) for key in keys([stem]))
    if p is None:
        return None
    c = next(c for c in COLUMNS if c.stem == stem)
    p, m = np.asarray(p, dtype=c.dtype), np.asarray(m, dtype=c.dtype)
    if c.width is not None:  # (an empty strand may have lost its trailing shape on the way)
        width = c.width if c.width != ANY_WIDTH else (p.shape[1] if p.ndim == 2 else m.shape[1])
        p, m = p.reshape(-1, width), m.reshape(-1, width)
    return np.ascontiguousarray(np.concatenate([p, m]), dtype=c.dtype)


class Table:
    """Base of engine.Hits and node.NodeHits: the columns of a whole table as attributes <stem>_plus / <stem>_minus (one that
    nobody has set reads as None), cut into contigs.  A subclass sets _cuts, per strand the (first row, end row) of every
    contig, and _origins, per contig the position its own count from, where the table's positions are not local already."""
    _origins = None
    n_plus = property(lambda self: int(self.pos_plus.size))
    n_minus = property(lambda self: int(self.pos_minus.size))

    def __getattr__(self, name):  # (only reached for names the instance does not hold)
        if name in keys():
            return None
        raise AttributeError(name)

    def contig(self, k):
        """Contig k's rows of every column that is set, as a hit dict: views of the table, but for shifted positions."""
        plus, minus = [slice(int(first[k]), int(end[k])) for first, end in self._cuts]
        return take(vars(self), plus, minus, None if self._origins is None else int(self._origins[k]))
