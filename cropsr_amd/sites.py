"""Restriction enzyme sites of every guide -- can it be cloned, can the edit be genotyped.

Plant CRISPR vectors are assembled by Golden Gate; a spacer that holds the recognition sequence of the assembly enzyme, on
either strand, is cut during the reaction.  The standard first screen of edited plants is a PCR / restriction-enzyme assay:
if a recognition site spans the Cas9 cut, an indel destroys it, and the assay is readable when that enzyme has no other
site in the amplicon.  Per kept hit the GPU gives two masks over an enzyme set that the selection can bound
(select.Request(forbid_sites=..., need_assay=...)).

Definition (include/cropsr_hip.h states the same; tests/site_reference.py restates it twice).

  enzyme set  E enzymes, 1 <= E <= 32; enzyme e is bit e of every mask.  An enzyme has a name and a recognition motif of m
              letters, 4 <= m <= 16, over the 15 IUPAC letters ACGTRYSWKMBDHVN; case is ignored and U is read as T.  A motif
              letter stands for a set of bases (SETS).  The reverse complement rc(M) reverses the motif and complements each
              set.
  occurrence  enzyme e occurs at arena position q when every letter of s[q : q + m] is a base and lies in the set of the
              motif letter at its place, for M or for rc(M).  A base is a letter whose `ac` bit is set (A, C, G, T in either
              case; a genome U is A as packed).  A non-base matches nothing, not even a motif N: N, IUPAC letters, Z,
              decoration, void, a position below 0 and a position in a plane word at or beyond the arena's word count.  A
              palindromic motif occurring at q is one occurrence.  Occurrences cannot contain void, so a footprint
              [q, q + m) always lies inside one text.
  per row     of an arena's hit tables after a scan at guide length l (1 <= l <= 50), with amplicon half-width A
              (m_max <= A <= 100 000, default 300); pos is the match index i ('+' row) or j ('-' row):
                cut boundary c   i - 3 ('+'), j + 6 ('-'): letters c - 1 and c lie around the cut
                guide window     [g0, g0 + l), g0 = i - l ('+'), j + 3 ('-'): the protospacer alone, without the PAM
                text [t0, t1)    the arena text that contains c; where none does the amplicon is empty
                in_guide bit e   an occurrence with g0 <= q and q + m <= g0 + l exists (never when m > l)
                span_e           occurrences with c - m + 1 <= q <= c - 1: both letters around the cut belong to the site
                amp_e            occurrences with max(c - A, t0) <= q and q + m <= min(c + A, t1)
                assay bit e      span_e >= 1 and amp_e == 1 (overlapping sites across the cut give amp_e = 2 and no bit)
              One uint64 per row: in_guide | assay << 32.  Every row has a value; nothing saturates.

Not modelled: Type IIS cut offsets, methylation sensitivity, sites created at the spacer-vector junction, primers (the
amplicon is +-A around the cut).
"""
import numpy as np

HEADER = ["guide_sites", "assay_enzymes"]
MAX_ENZYMES = 32
MIN_MOTIF, MAX_MOTIF = 4, 16
MAX_GUIDE = 50
DEFAULT_FLANK = 300
MAX_FLANK = 100000
N_CLONING = 5  # the built-in set's first enzymes: the Golden Gate assembly enzymes

# bit 0 A, bit 1 C, bit 2 G, bit 3 T
SETS = {"A": 1, "C": 2, "G": 4, "T": 8, "R": 1 | 4, "Y": 2 | 8, "S": 2 | 4, "W": 1 | 8, "K": 4 | 8, "M": 1 | 2, "B": 2 | 4 | 8,
        "D": 1 | 4 | 8, "H": 1 | 2 | 8, "V": 1 | 2 | 4, "N": 15}
_LETTER_OF_SET = {v: k for k, v in SETS.items()}

BUILTIN = (
    ("BsaI", "GGTCTC"), ("BbsI", "GAAGAC"), ("BsmBI", "CGTCTC"), ("SapI", "GCTCTTC"), ("AarI", "CACCTGC"),
    ("EcoRI", "GAATTC"), ("BamHI", "GGATCC"), ("HindIII", "AAGCTT"), ("XbaI", "TCTAGA"), ("PstI", "CTGCAG"), ("SacI", "GAGCTC"),
    ("KpnI", "GGTACC"), ("SalI", "GTCGAC"), ("XhoI", "CTCGAG"), ("NcoI", "CCATGG"), ("NdeI", "CATATG"), ("EcoRV", "GATATC"),
    ("SmaI", "CCCGGG"), ("SpeI", "ACTAGT"), ("NheI", "GCTAGC"), ("BglII", "AGATCT"), ("ClaI", "ATCGAT"), ("SphI", "GCATGC"),
    ("ApaI", "GGGCCC"),
    ("NotI", "GCGGCCGC"),
    ("MspI", "CCGG"), ("HaeIII", "GGCC"), ("AluI", "AGCT"), ("TaqI", "TCGA"), ("RsaI", "GTAC"), ("HinfI", "GANTC"), ("BstNI", "CCWGG"),
)


def normalize(motif):
    """The motif in upper case with U read as T, or ValueError: 4..16 IUPAC letters."""
    m = str(motif).upper().replace("U", "T")
    if not MIN_MOTIF <= len(m) <= MAX_MOTIF:
        raise ValueError("a recognition motif has %d..%d letters, %r has %d" % (MIN_MOTIF, MAX_MOTIF, motif, len(m)))
    for ch in m:
        if ch not in SETS:
            raise ValueError("%r in motif %r is not one of the IUPAC letters ACGTRYSWKMBDHVN" % (ch, motif))
    return m


def motif_sets(motif):
    """The sets of bases of a motif's letters (bit 0 A, 1 C, 2 G, 3 T), first letter first."""
    return [SETS[ch] for ch in normalize(motif)]


def complement_set(s):
    """The complement of a set of bases: A <-> T, C <-> G."""
    return (s & 1) << 3 | (s & 2) << 1 | (s & 4) >> 1 | (s & 8) >> 3


def reverse_complement(motif):
    """rc(M): the motif reversed, each letter's set complemented."""
    return "".join(_LETTER_OF_SET[complement_set(s)] for s in reversed(motif_sets(motif)))


def is_palindrome(motif):
    return reverse_complement(motif) == normalize(motif)


class EnzymeSet:
    """An ordered set of (name, motif): enzyme e is bit e of the masks.  ValueError for an empty set, more than 32, a bad
    motif, an empty or repeated name."""

    def __init__(self, enzymes=BUILTIN, builtin=None):
        enzymes = [(str(n), normalize(m)) for n, m in enzymes]
        if not 1 <= len(enzymes) <= MAX_ENZYMES:
            raise ValueError("an enzyme set has 1..%d enzymes, not %d" % (MAX_ENZYMES, len(enzymes)))
        self.names = [n for n, _ in enzymes]
        self.motifs = [m for _, m in enzymes]
        for n in self.names:
            if not n or any(c in n for c in ",;\t ") or n.lower() in ("any", "cloning"):
                raise ValueError("%r is not an enzyme name" % n)
        if len({n.lower() for n in self.names}) != len(self.names):
            raise ValueError("an enzyme name is given twice")
        self.builtin = (tuple(enzymes) == tuple(BUILTIN)) if builtin is None else bool(builtin)
        self.m_max = max(len(m) for m in self.motifs)

    def __len__(self):
        return len(self.names)

    def mask(self, names):
        """The mask of a list of enzyme names (case ignored); `cloning`: the built-in set's first five (refused for another
        set), `any`: every enzyme.  ValueError for an unknown name."""
        index = {n.lower(): e for e, n in enumerate(self.names)}
        out = 0
        for n in names:
            key = str(n).strip().lower()
            if key == "cloning":
                if not self.builtin:
                    raise ValueError("`cloning` names the first five enzymes of the built-in set; name the enzymes of your own set")
                out |= (1 << N_CLONING) - 1
            elif key == "any":
                out |= (1 << len(self.names)) - 1
            elif key in index:
                out |= 1 << index[key]
            else:
                raise ValueError("no enzyme %r in the set (%s)" % (n, ", ".join(self.names)))
        return out

    def names_of(self, mask):
        return names(mask, self.names)

    def check_flank(self, flank):
        """The amplicon half-width A (None: the default), or ValueError."""
        a = DEFAULT_FLANK if flank is None else int(flank)
        if not self.m_max <= a <= MAX_FLANK:
            raise ValueError("the amplicon half-width is %d (the longest motif) .. %d, not %r" % (self.m_max, MAX_FLANK, flank))
        return a


def parse(text):
    """The EnzymeSet of a user file's text: `name<TAB>motif` lines, `#` comments and empty lines skipped.  ValueError names
    the line."""
    out = []
    for n, line in enumerate(str(text).splitlines(), 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        cols = line.split("\t")
        if len(cols) != 2 or not cols[0].strip() or not cols[1].strip():
            raise ValueError("line %d: expected name<TAB>motif" % n)
        try:
            out.append((cols[0].strip(), normalize(cols[1].strip())))
        except ValueError as e:
            raise ValueError("line %d: %s" % (n, e))
    try:
        return EnzymeSet(out, builtin=False)
    except ValueError as e:
        raise ValueError("enzyme file: %s" % e)


def load(path):
    with open(path) as f:
        return parse(f.read())


def pack(in_guide, assay):
    return np.asarray(in_guide, dtype=np.uint64) | np.asarray(assay, dtype=np.uint64) << np.uint64(32)


def unpack(col):
    """(in_guide, assay) uint32 arrays of a packed column."""
    c = np.asarray(col, dtype=np.uint64)
    return (c & np.uint64(0xFFFFFFFF)).astype(np.uint32), (c >> np.uint64(32)).astype(np.uint32)


def names(mask, enzyme_names=None):
    """The names of a mask's enzymes, in the set's order (default: the built-in set's)."""
    enzyme_names = [n for n, _ in BUILTIN] if enzyme_names is None else list(enzyme_names)
    return [n for e, n in enumerate(enzyme_names) if int(mask) >> e & 1]


def fields(value, enzyme_names=None):
    """The two CSV fields of one packed value: the enzymes inside the guide and the assay enzymes, each joined by `;`."""
    v = int(value)
    return ";".join(names(v & 0xFFFFFFFF, enzyme_names)), ";".join(names(v >> 32, enzyme_names))


def passes(col, forbid_sites=0, need_assay=0):
    """Boolean array: which rows of a packed column pass the two limits (the selection's predicate term)."""
    in_guide, assay = unpack(col)
    ok = (in_guide & np.uint32(forbid_sites)) == 0
    if need_assay:
        ok &= (assay & np.uint32(need_assay)) != 0
    return ok
