"""--base-edit / --select-stop: guides with which a cytosine base editor writes a stop codon.

Not in the reference, opt-in.  The selection (select.py) designs knock-outs for a cutting Cas9: score, specificity,
repair outcome, deletion pairs, the coding position of the cut.  A cytosine base editor (CBE) makes no cut: it deaminates
the C's in a small window of the protospacer, which turns CAA, CAG, CGA into TAA, TAG, TGA -- or TGG into a stop from the
other strand -- and leaves no indels (CRISPR-STOP, iSTOP).  Whether a guide does that needs the letters under its window
(the arena's bit-planes) and their reading frame in the gene's primary transcript (coding.py's step function); the test
of every row against the model of the gene it is being selected for runs on the device inside the selection
(csrc/crp_edit.h, csrc/crp_select_edit.hip).  tests/base_edit_reference.py restates the definition.

Definition.  The row is a row of an arena's hit tables after a scan at guide length 20.

  window     Window(lo, hi), 1 <= lo <= hi <= 20, default 4..8: protospacer positions counted from the PAM-distal end.
             Window letter p of a '+' row with match index i is the arena position x = i - 21 + p; of a '-' row (CC. at j)
             it is x = j + 23 - p.
  letters    a letter is a base when its `ac` bit is set; its code is (hi, lo); case is not read and U is A, as in
             repair.py.  A position below 0, or in a plane word at or beyond the arena's word count, is a non-base and
             is never read.
  targets    on a '+' row the window letters that are base C: they become T.  On a '-' row the window letters that are
             base G: they become A (the protospacer's C, read on the forward strand).  `targets` is their number, 0..20;
             it depends on no gene.
  codons     relative to a gene g with a coding model (coding.py: the primary transcript P, its length L_P, the gene row's
             strand): letter x is a coding letter of P when the step function's grow bit holds at boundary x; its coding
             index is cum_P(x) for a '+' gene and L_P - 1 - cum_P(x) for a '-' gene.  Codon q has the letters with
             indices 3 q, 3 q + 1, 3 q + 2.  It is EVALUATED when all three indices are below L_P, its letters are three
             adjacent arena positions and all three are bases: a codon split by an intron, clipped by the text, or a
             trailing partial codon is not.  It is read in the gene's orientation, complemented for a '-' gene.
  stops      the evaluated codons that are no stop (TAA, TAG, TGA) and whose edited form -- every target among their
             letters converted -- is one.  `stop_off` is 3 q of the one with the smallest q, NO_STOP if there is none.  A gene
             without a model has stops = 0.
  closed     equivalently: where the edit reads C -> T in the gene's orientation, a codon CAA, CAG or CGA whose first
  form       letter is a window letter; where it reads G -> A, TGG with its second or third letter in the window.
  limits     Limits(min_pct=0, max_pct=100, max_targets=20): beyond select.py's predicate a row passes when stop_off is not
             NO_STOP, min_pct L_P <= 100 stop_off <= max_pct L_P (64-bit products) and targets <= max_targets.  n_in is
             unchanged, n_pass counts the rows that pass this too; order, ties and K are select.py's.

Limits of the model: the CDS phase column is not read, split codons are skipped, stop codons from a
cytosine editor only (an adenine editor writes none), NGG rows only, all targets of the window convert together, one device.

--splice-edit / --select-splice: guides with which a base editor destroys a splice site.  The other
standard knock-out route of a base editor, and the only one of an adenine editor: change a letter of the canonical GT that
opens an intron of the coding transcript or of the AG that closes it (csrc/crp_splice.h, csrc/crp_select_splice.hip;
tests/splice_edit_reference.py restates the definition).  Rows, window, letters and the step function are those above.

  editor     Editor("cbe") or Editor("abe").  CBE targets are the window's base C on a '+' row (-> T) and base G on a '-'
             row (-> A), as above; ABE targets are base A on a '+' row (-> G) and base T on a '-' row (-> C).  `targets` is
             their number, 0..20; it depends on no gene.
  introns    relative to a gene g with a model (P, L_P, the gene row's strand): in ascending arena positions an intron START
             is a boundary x where x - 1 is a coding letter of P, x is not and cum_P(x) < L_P; an intron END is a boundary x'
             where x' - 1 is no coding letter of P, x' is and cum_P(x') > 0.  Only the gaps between P's own merged CDS
             segments count: not other transcripts' change points, nothing outside P's first and last coding letter (no
             UTR introns).  Evidence comes only from steps inside the row's text: before at[0] nothing holds.
  sites      the start site is the letters x, x + 1, the end site x' - 2, x' - 1.  A site is EVALUATED when both letters are
             bases, both are no coding letters of P and it is canonical in the gene's orientation: on a '+' gene the start
             site is the donor, forward GT, and the end site the acceptor, forward AG; on a '-' gene the start site is the
             acceptor, forward CT, and the end site the donor, forward AC.  GC-AG and AT-AC introns are not evaluated.
  destroyed  an evaluated site with at least one of its two letters a target inside the window: any change breaks the
             dinucleotide.  `donors` and `acceptors` are the numbers of destroyed sites of each kind.
  off        donor_off and acceptor_off: for the destroyed site of that kind nearest the gene's 5' end, the number of P's
             coding letters 5' of its intron -- cum_P(x) at the intron's boundary for a '+' gene, L_P - cum_P(x) for a '-'
             gene: 1 .. L_P - 1, NO_SITE without such a site.  A gene without a model has no sites.
  limits     SpliceLimits(min_pct=0, max_pct=100, max_targets=20, kinds="any"), kinds one of donor, acceptor, any: beyond
             select.py's predicate a row passes when for some allowed kind its off is not NO_SITE and min_pct L_P <= 100 off
             <= max_pct L_P (64-bit products), and targets <= max_targets.  n_in is unchanged, n_pass counts the rows that
             pass this too; order, ties and K are select.py's.
  together   with the stop limits above (CBE only) the two are alternatives: a row passes when the stop test or the splice
             test holds, each under its own limits.  ABE with stop limits is refused.

Limits of this model: only P's CDS-CDS introns, canonical GT / AG only, ABE's donor edit gives GC (which
a minority of natural introns use: `acceptor` is the strict choice), a destroyed site is reported and not what the
spliceosome does next, one device.
"""
import numpy as np

NO_STOP = 0xFFFFFFFF  # `stop_off` of a row whose edit writes no stop codon
GUIDE_LEN = 20
HEADER = ["edit_targets", "stop_codons", "stop_codon", "stop_percent"]
STOPS = ("TAA", "TAG", "TGA")
NO_SITE = 0xFFFFFFFF  # `donor_off` / `acceptor_off` of a row whose edit destroys no such site
SPLICE_HEADER = ["splice_targets", "splice_sites", "donor_percent", "acceptor_percent"]
KINDS = {"donor": 1, "acceptor": 2, "any": 3}  # SpliceLimits.kinds -> the bits of crp_select_splice_limits.kinds
_BASE = {ord(c): b for c, b in zip("ACGTUacgtu", "ACGTAACGTA")}
_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


class Window:
    """The editing window: protospacer positions lo..hi counted from the PAM-distal end, 1 <= lo <= hi <= 20."""

    def __init__(self, lo=4, hi=8):
        for name, v in (("lo", lo), ("hi", hi)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError("the window's %s is a protospacer position, an integer 1..%d, not %r" % (name, GUIDE_LEN, v))
        self.lo, self.hi = int(lo), int(hi)
        if not 1 <= self.lo <= self.hi <= GUIDE_LEN:
            raise ValueError("the window is 1 <= lo <= hi <= %d, not %d-%d" % (GUIDE_LEN, self.lo, self.hi))

    @classmethod
    def parse(cls, text):
        """Window from the command line's LO-HI."""
        parts = str(text).split("-")
        if len(parts) != 2 or not all(p.isdigit() and len(p) <= 3 for p in parts):
            raise ValueError("a window is LO-HI, two protospacer positions 1..%d, not %r" % (GUIDE_LEN, text))
        return cls(int(parts[0]), int(parts[1]))

    def astuple(self):
        return (self.lo, self.hi)

    def __len__(self):
        return self.hi - self.lo + 1

    def positions(self, pos, minus):
        """The arena positions of the window's letters of a row with match index pos, ascending."""
        pos = int(pos)
        return list(range(pos + 23 - self.hi, pos + 24 - self.lo)) if minus else list(range(pos - 21 + self.lo, pos - 20 + self.hi))


class Limits:
    """The bounds a selection puts on the stop codon: min_pct L_P <= 100 stop_off <= max_pct L_P (integer percentages
    0..100) and targets <= max_targets (0..20)."""

    def __init__(self, min_pct=0, max_pct=100, max_targets=GUIDE_LEN):
        vals = []
        for name, v, top in (("min_pct", min_pct, 100), ("max_pct", max_pct, 100), ("max_targets", max_targets, GUIDE_LEN)):
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= top:
                raise ValueError("%s is an integer 0..%d, not %r" % (name, top, v))
            vals.append(int(v))
        self.min_pct, self.max_pct, self.max_targets = vals
        if self.min_pct > self.max_pct:
            raise ValueError("min_pct %d lies above max_pct %d" % (self.min_pct, self.max_pct))

    def astuple(self):
        return (self.min_pct, self.max_pct, self.max_targets)

    def passes(self, targets, stop_off, length):
        """Boolean array from arrays: targets, stop_off (NO_STOP without a stop) and L_P."""
        targets, stop_off, length = (np.asarray(v).astype(object) for v in (targets, stop_off, length))  # (exact integers)
        ok = (self.min_pct * length <= 100 * stop_off) & (100 * stop_off <= self.max_pct * length) & (targets <= self.max_targets)
        return (stop_off != NO_STOP) & ok.astype(bool)


def outcome(text, pos, minus, window, index_of=None, length=0, gene_minus=False):
    """(targets, stops, stop_off) of one row, by the definition's general statement.  text: the letters by arena position
    (bytes; positions outside it are non-bases); pos, minus: the row's match index and strand; index_of: None for a gene
    without a model, else a function from an arena position to the coding index of that letter in P, in the gene's
    orientation, or None where the letter is no coding letter of P inside the text; length: L_P; gene_minus: the gene's
    strand."""
    text = bytes(text)
    base = lambda x: _BASE.get(text[x]) if 0 <= x < len(text) else None
    src, dst = ("G", "A") if minus else ("C", "T")
    targets = [x for x in window.positions(pos, minus) if base(x) == src]
    if index_of is None or not targets:
        return len(targets), 0, NO_STOP
    read = (lambda b: _COMPLEMENT[b]) if gene_minus else (lambda b: b)
    found = []
    step = -1 if gene_minus else 1
    for x in range(min(targets, default=0) - 2, max(targets, default=-3) + 3):  # the first letter of a codon that holds a target
        i = index_of(x)
        if i is None or i % 3 or i + 2 >= length:
            continue
        xs = [x, x + step, x + 2 * step]
        if [index_of(y) for y in xs] != [i, i + 1, i + 2] or any(base(y) is None for y in xs):
            continue
        before = "".join(read(base(y)) for y in xs)
        after = "".join(read(dst if y in targets else base(y)) for y in xs)
        if before not in STOPS and after in STOPS:
            found.append(i)
    return len(targets), len(found), min(found, default=NO_STOP)


def percent(stop_off, length):
    """stop_percent of the selection file: 100 stop_off / L_P with one decimal, as coding.percent rounds."""
    from .coding import percent as pct
    return pct(stop_off, length)


def fields(targets, stops, stop_off, length):
    """The four fields of a selection row: edit_targets, stop_codons, stop_codon (stop_off / 3 + 1) and stop_percent; the
    last two are empty when the edit writes no stop."""
    if int(stop_off) == NO_STOP:
        return (int(targets), int(stops), "", "")
    return (int(targets), int(stops), int(stop_off) // 3 + 1, percent(stop_off, length))


class Editor:
    """The base editor: "cbe" (cytosine: C -> T, read G -> A on a '-' row) or "abe" (adenine: A -> G, read T -> C)."""
    NAMES = ("cbe", "abe")

    def __init__(self, name="cbe"):
        if isinstance(name, Editor):
            name = name.name
        if not isinstance(name, str) or name.lower() not in self.NAMES:
            raise ValueError("the editor is one of %s, not %r" % (", ".join(self.NAMES), name))
        self.name = name.lower()
        self.code = self.NAMES.index(self.name)  # CRP_EDITOR_CBE, CRP_EDITOR_ABE

    def edit(self, minus):
        """(the forward letter converted on a row of that strand, what it becomes)."""
        return ((("C", "T"), ("G", "A")), (("A", "G"), ("T", "C")))[self.code][bool(minus)]

    def __eq__(self, other):
        return isinstance(other, Editor) and other.name == self.name

    def __hash__(self):
        return hash(self.name)

    def __repr__(self):
        return "Editor(%r)" % self.name


class SpliceLimits:
    """The bounds a selection puts on the destroyed splice site: for a kind in `kinds` (donor, acceptor, any)
    min_pct L_P <= 100 off <= max_pct L_P (integer percentages 0..100), and targets <= max_targets (0..20)."""

    def __init__(self, min_pct=0, max_pct=100, max_targets=GUIDE_LEN, kinds="any"):
        vals = []
        for name, v, top in (("min_pct", min_pct, 100), ("max_pct", max_pct, 100), ("max_targets", max_targets, GUIDE_LEN)):
            if isinstance(v, bool) or isinstance(v, str) or int(v) != v or not 0 <= int(v) <= top:
                raise ValueError("%s is an integer 0..%d, not %r" % (name, top, v))
            vals.append(int(v))
        self.min_pct, self.max_pct, self.max_targets = vals
        if self.min_pct > self.max_pct:
            raise ValueError("min_pct %d lies above max_pct %d" % (self.min_pct, self.max_pct))
        if not isinstance(kinds, str) or kinds not in KINDS:
            raise ValueError("kinds is one of donor, acceptor, any, not %r" % (kinds,))
        self.kinds = kinds

    def astuple(self):
        """(min_pct, max_pct, max_targets, the kinds' bits), as crp_select_splice_limits has them."""
        return (self.min_pct, self.max_pct, self.max_targets, KINDS[self.kinds])

    def passes(self, targets, donor_off, acceptor_off, length):
        """Boolean array from arrays: targets, the two offs (NO_SITE without a site) and L_P."""
        targets, donor_off, acceptor_off, length = (np.asarray(v).astype(object) for v in (targets, donor_off, acceptor_off, length))  # (exact integers)
        ok = np.zeros(targets.shape, bool)
        for bit, off in ((1, donor_off), (2, acceptor_off)):
            if KINDS[self.kinds] & bit:
                ok |= (off != NO_SITE) & ((self.min_pct * length <= 100 * off) & (100 * off <= self.max_pct * length)).astype(bool)
        return ok & (targets <= self.max_targets).astype(bool)


def splice_outcome(text, pos, minus, window, editor, index_of=None, length=0, gene_minus=False):
    """(targets, donors, acceptors, donor_off, acceptor_off) of one row, by the definition's general statement.  text, pos,
    minus, window, index_of, length and gene_minus are outcome()'s; editor: an Editor.  Read in the gene's orientation: a
    donor is the two letters 3' of a coding letter of P with index i < L_P - 1, GT, neither a coding letter of P; an
    acceptor the two letters 5' of a coding letter with index i > 0, AG, neither a coding letter of P; the coding letters
    5' of the intron number i + 1 resp. i."""
    text = bytes(text)
    base = lambda x: _BASE.get(text[x]) if 0 <= x < len(text) else None
    src, _ = Editor(editor).edit(minus)
    targets = [x for x in window.positions(pos, minus) if base(x) == src]
    if index_of is None or not targets:
        return len(targets), 0, 0, NO_SITE, NO_SITE
    read = (lambda b: _COMPLEMENT[b]) if gene_minus else (lambda b: b)
    step = -1 if gene_minus else 1
    found = ([], [])
    for x in range(min(targets) - 3, max(targets) + 4):  # the coding letter next to a site that holds a target
        i = index_of(x)
        if i is None:
            continue
        for kind, (first, second), before, canon in ((0, (x + step, x + 2 * step), i + 1, "GT"), (1, (x - 2 * step, x - step), i, "AG")):
            if not 0 < before < length or index_of(first) is not None or index_of(second) is not None:
                continue
            if base(first) is None or base(second) is None or read(base(first)) + read(base(second)) != canon:
                continue
            if first in targets or second in targets:
                found[kind].append(before)
    return len(targets), len(found[0]), len(found[1]), min(found[0], default=NO_SITE), min(found[1], default=NO_SITE)


def splice_fields(targets, donors, acceptors, donor_off, acceptor_off, length):
    """The four fields of a selection row: splice_targets, splice_sites (donors + acceptors), donor_percent and
    acceptor_percent (100 off / L_P, formatted as stop_percent; empty without a destroyed site of that kind)."""
    return (int(targets), int(donors) + int(acceptors), "" if int(donor_off) == NO_SITE else percent(donor_off, length),
            "" if int(acceptor_off) == NO_SITE else percent(acceptor_off, length))
