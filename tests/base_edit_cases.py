"""The inputs of tests/test_base_edit.py.

random_case(seed): a small contig of random letters (ACGTN and lower case) with random exon structures on both strands, for
the comparison of the three restatements at every row.

build(orc): an ~80 kb genome of four contigs (30 000, 6 000, 22 000 and 22 000 letters: one arena, or three of at most 600
words) with a GFF of its own.  Most of it is random background, whose genes hold natural cases by the hundred; into it are
PLANTED 30-letter constructs -- a guide whose window holds a chosen codon at a chosen place, in a stretch of A / T that the
editor does not touch -- each with a gene around it whose frame puts the codon at coding index 30.  `planted` lists, per
construct, what the definition must give there; the tests assert that on the reference's rows before they look at the device.
"""
import numpy as np

from select_coding_cases import _Gff

NAMES = ["e0", "e1", "e2", "e3"]
LENGTHS = (30000, 6000, 22000, 22000)
WINDOW = (4, 8)
NO_STOP = 0xFFFFFFFF
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(b):
    return bytes(b).translate(_COMP)[::-1]


def random_case(seed, n=700):
    """(text, GFF text) of one contig `s`: letters ACGT with N and lower case mixed in, six genes of random exons."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTacgtNn", dtype=np.uint8) if seed % 2 else np.frombuffer(b"ACGT", dtype=np.uint8)
    text = bytearray(rng.choice(alpha, n).tobytes())
    for at in rng.integers(30, n - 30, 12).tolist():  # what the editor turns into stops, so that short texts hold enough of it
        text[at:at + 3] = [b"CAA", b"CAG", b"CGA", b"TGG", b"TTG", b"CTG", b"TCG", b"CCA"][int(rng.integers(8))]
    gff = _Gff()
    for g in range(6):
        lo = int(rng.integers(15, n - 300))
        strand = "+-"[g % 2]
        ident = "r%d" % g
        gff.gene("s", lo, lo + 290, ident, strand)
        x, exons = lo - int(rng.integers(0, 3)) * 5, []  # (some coding sequences begin before the gene row)
        for _ in range(int(rng.integers(1, 6))):
            length = int(rng.integers(1, 70))
            exons.append((x, x + length - 1))
            x += length + int(rng.integers(1, 40))
        gff.cds("s", exons, ident, strand)
    return bytes(text), "\n".join(gff.lines) + "\n"


class _Builder:
    def __init__(self):
        rng = np.random.default_rng(2021)
        self.rng = rng
        self.texts = [bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()) for n in LENGTHS]
        self.gff = _Gff()
        self.planted = []
        self.next = [200, 200, 200, 200]  # where the next construct goes, per contig

    def quiet(self, k, lo, hi):
        """A / T over [lo, hi): nothing the editor converts, no PAM."""
        self.texts[k][lo:hi] = self.rng.choice(np.frombuffer(b"AT", dtype=np.uint8), hi - lo).tobytes()

    def guide(self, k, minus_row, at=None):
        """A guide in a quiet stretch: returns (match index, the arena-free positions of its window's letters, ascending).  The
        quiet stretch covers the 30 letters the score reads and 10 more on either side."""
        if at is None:
            at = self.next[k]
            self.next[k] += 160
        t = self.texts[k]
        if not minus_row:  # 30-mer s[i - 25 : i + 5], NGG at i
            i = at + 35
            self.quiet(k, i - 35, i + 15)
            t[i:i + 3] = b"AGG"
            return i, list(range(i - 21 + WINDOW[0], i - 20 + WINDOW[1]))
        j = at + 12             # 30-mer s[j - 2 : j + 28], CCN at j
        self.quiet(k, j - 12, j + 38)
        t[j:j + 3] = b"CCT"
        return j, list(range(j + 23 - WINDOW[1], j + 24 - WINDOW[0]))

    def put(self, k, x, letters):
        self.texts[k][x:x + len(letters)] = letters

    def expect(self, ident, k, pos, minus_row, targets, stops, stop_off, what):
        self.planted.append(dict(gene=ident, contig=k, pos=pos, minus=minus_row, targets=targets, stops=stops,
                                 stop_off=stop_off if stops else NO_STOP, what=what))


def _closed(codon, inside, reads_ct):
    """Whether the closed form gives a stop: inside = which of the codon's letters (gene orientation) lie in the window."""
    return (codon in ("CAA", "CAG", "CGA") and inside[0]) if reads_ct else (codon == "TGG" and (inside[1] or inside[2]))


def build(orc):
    """dict(contigs, names, gff, hits, ids, planted)."""
    b = _Builder()
    gff = b.gff
    n_gene = [0]

    def name(stem):
        n_gene[0] += 1
        return "%s_%d" % (stem, n_gene[0])

    # ---- every stop-making codon with 1, 2 and 3 letters inside the window at either edge, genes x rows on both strands
    for codon in ("CAA", "CAG", "CGA", "TGG"):
        for minus_gene in (False, True):
            for minus_row in (False, True):
                for edge, n_in in (("low", 1), ("low", 2), ("low", 3), ("high", 3), ("high", 2), ("high", 1)):
                    k = 0 if not minus_gene else 2
                    pos, win = b.guide(k, minus_row)
                    x = win[0] - (3 - n_in) if edge == "low" else win[-1] - (n_in - 1)  # the triple's lowest position
                    forward = codon.encode() if not minus_gene else revcomp(codon.encode())
                    b.put(k, x, forward)
                    ident = name("%s_%s%d" % (codon, edge, n_in))
                    strand = "-" if minus_gene else "+"
                    gff.gene(NAMES[k], x - 40, x + 42, ident, strand)
                    gff.cds(NAMES[k], [(x - 30, x + 32)], ident, strand)  # 63 letters; the codon's first letter has index 30 on either strand
                    in_window = [x + j in win for j in range(3)]
                    inside = in_window[::-1] if minus_gene else in_window
                    targets = sum(1 for j in range(3) if in_window[j] and forward[j:j + 1] == (b"G" if minus_row else b"C"))
                    stop = _closed(codon, inside, minus_gene == minus_row)
                    b.expect(ident, k, pos, minus_row, targets, int(stop), 30, "%s %s gene %s row %s edge %d inside" % (
                        codon, strand, "-" if minus_row else "+", edge, n_in))

    def simple(k, stem, forward, offset, minus_row, exons_of, strand, targets, stops, stop_off, what, at_window=0):
        """One construct: `forward` written with its first letter at the window's letter `at_window` plus offset; exons_of(x)
        gives the gene's exons from that position."""
        pos, win = b.guide(k, minus_row)
        x = win[at_window] + offset
        b.put(k, x, forward)
        ident = name(stem)
        exons = exons_of(x)
        if strand is not None:
            gff.gene(NAMES[k], min(x - 30, min(e[0] for e in exons)) - 10, max(x + 32, max(e[1] for e in exons)) + 10, ident, strand)  # (the guide's cut site inside)
            gff.cds(NAMES[k], exons, ident, strand)
        b.expect(ident, k, pos, minus_row, targets, stops, stop_off, what)
        return ident, pos, x

    whole = lambda x: [(x - 30, x + 32)]
    # a target codon split by an intron: C | AA
    simple(0, "split", b"C", 1, False, lambda x: [(x - 30, x), (x + 60, x + 91)], "+", 1, 0, 0, "a target codon split by an intron")
    # L_P = 1 and 2 mod 3 with the would-be stop in the partial codon
    simple(0, "partial1", b"CAA", 1, False, lambda x: [(x - 30, x)], "+", 1, 0, 0, "L_P = 1 mod 3: the partial codon")
    simple(0, "partial2", b"CAA", 1, False, lambda x: [(x - 30, x + 1)], "+", 1, 0, 0, "L_P = 2 mod 3: the partial codon")
    simple(2, "partial1_minus", b"TTG", 1, True, lambda x: [(x + 2, x + 32)], "-", 1, 0, 0, "L_P = 1 mod 3 on a '-' gene")
    # an original stop in the window; a window without targets; N and lower case inside a target codon
    simple(0, "was_stop", b"TAG", 1, True, whole, "+", 1, 0, 0, "an original TAG with its G in the window")
    simple(0, "no_targets", b"ATA", 1, False, whole, "+", 0, 0, 0, "a window without targets")
    simple(0, "with_n", b"CAN", 1, False, whole, "+", 1, 0, 0, "an N inside a target codon")
    simple(0, "lower_case", b"cAa", 1, False, whole, "+", 1, 1, 30, "lower-case letters inside a target codon")
    # two stops from one guide (three with the window 1-20)
    simple(0, "two_stops", b"CAACAGCGA", 0, False, whole, "+", 2, 2, 30, "two stops from one guide")
    simple(2, "two_stops_ga", b"TGGTGG", -1, True, whole, "+", 4, 2, 30, "two TGG from one guide")
    # genes without a model over a construct: no CDS, and a strand that is none
    pos, win = b.guide(0, False)
    b.put(0, win[1], b"CAA")
    gff.gene(NAMES[0], win[1] - 40, win[1] + 42, "no_cds", "+")
    b.expect("no_cds", 0, pos, False, 1, 0, 0, "a gene without CDS rows")
    simple(0, "no_strand", b"CAA", 1, False, whole, ".", 1, 0, 0, "a gene whose strand is none")
    # the first three and the last three letters of an exon, P's first and last codon
    a = b.next[0]
    b.next[0] += 420
    for off, codon in ((0, b"CAA"), (60, b"CAG"), (150, b"CGA"), (210, b"CAA")):
        pos, win = b.guide(0, False, at=a + off + 11)  # the window's second letter lands on a + 30 + off
        x = win[1]
        assert x == a + 30 + off, (x, a + 30 + off)
        b.put(0, x, codon)
        b.expect("exon_ends", 0, pos, False, 1, 1, {0: 0, 60: 60, 150: 63, 210: 123}[off],
                 {0: "P's first codon, the first three letters of an exon", 60: "the last three letters of an exon",
                  150: "the first three letters of an exon", 210: "P's last codon"}[off])
    gff.gene(NAMES[0], a + 20, a + 260, "exon_ends", "+")
    gff.cds(NAMES[0], [(a + 30, a + 92), (a + 180, a + 242)], "exon_ends", "+")
    # limits hit with equality: L_P = 300, stops at the offsets 15 (5 %) and 195 (65 %)
    a = b.next[0]
    b.next[0] += 500
    b.quiet(0, a, a + 420)
    for off in (15, 195):
        pos, win = b.guide(0, False, at=a + off + 21)
        assert win[1] == a + 40 + off, (win[1], a + 40 + off)
        b.put(0, win[1], b"CAA")
        b.expect("exact300", 0, pos, False, 1, 1, off, "a stop at %d of 300" % off)
    gff.gene(NAMES[0], a + 30, a + 350, "exact300", "+")
    gff.cds(NAMES[0], [(a + 40, a + 339)], "exact300", "+")
    # a gene nested in an intron and an antisense gene sharing rows, with different answers
    a = b.next[0]
    b.next[0] += 700
    pos, win = b.guide(0, False, at=a + 30)
    x = win[1]
    b.put(0, x, b"CAA")
    gff.gene(NAMES[0], x - 40, x + 560, "outer", "+")
    gff.cds(NAMES[0], [(x - 30, x + 32), (x + 470, x + 532)], "outer", "+")
    gff.gene(NAMES[0], x - 35, x + 40, "antisense", "-")
    gff.cds(NAMES[0], [(x - 30, x + 32)], "antisense", "-")
    b.expect("outer", 0, pos, False, 1, 1, 30, "the outer gene: its own exon")
    b.expect("antisense", 0, pos, False, 1, 0, 0, "the antisense gene over the same row")
    pos, win = b.guide(0, False, at=a + 250)
    y = win[1]
    b.put(0, y, b"CAG")
    gff.gene(NAMES[0], y - 40, y + 42, "nested", "+")
    gff.cds(NAMES[0], [(y - 30, y + 32)], "nested", "+")
    b.expect("nested", 0, pos, False, 1, 1, 30, "the gene nested in the intron")
    b.expect("outer", 0, pos, False, 1, 0, 0, "the outer gene: a row in its intron")
    # '-' rows at every contig end whose window reaches past the end, over a gene that runs past it: TGG ends the contig
    for k, n in enumerate(LENGTHS):
        j = n - 16
        b.quiet(k, n - 60, n)
        b.put(k, j, b"CCT")
        b.put(k, n - 3, b"TGG")
        ident = "end_%d" % k
        gff.gene(NAMES[k], n - 50, n + 60, ident, "+")
        gff.cds(NAMES[k], [(n - 33, n + 50)], ident, "+")
        b.expect(ident, k, j, True, 1, 1, 30, "a '-' row whose window reaches past the end of contig %d" % k)
    # a gene with a model and no step in the text; step counts 2, 64 and 65 in random background (select_coding_cases' recipe)
    gff.gene(NAMES[1], 100, 900, "steps0", "+")
    gff.cds(NAMES[1], [(LENGTHS[1] + 100, LENGTHS[1] + 400)], "steps0", "+")
    at = 1000
    for steps, full, single in ((2, 0, 1), (64, 20, 2), (65, 21, 1)):
        exons, x = [], at + 10
        for j in range(full + single):
            n = 12 if j < full else 1
            exons.append((x, x + n - 1))
            x += n + 8
        ident = "steps%d" % steps
        strand = "+" if steps % 2 else "-"
        gff.gene(NAMES[3], at, x + 10, ident, strand)
        gff.mrna(NAMES[3], at, x + 10, ident + ".1", ident, strand)
        gff.cds(NAMES[3], exons, ident + ".1", strand)
        at = x + 100
    # random background genes of a few exons each, both strands: natural cases by the hundred
    rng = np.random.default_rng(8)
    for k, first in ((0, 13000), (1, 1200), (2, 9000), (3, 4000)):
        x = first
        for g in range(16):
            if x + 900 > LENGTHS[k] - 200:
                break
            ident = name("bg%d" % k)
            strand = "+-"[g % 2]
            exons, y = [], x + 20
            for _ in range(int(rng.integers(1, 5))):
                n = int(rng.integers(30, 200))
                exons.append((y, y + n - 1))
                y += n + int(rng.integers(20, 90))
            gff.gene(NAMES[k], x, y, ident, strand)
            gff.mrna(NAMES[k], x, y, ident + ".1", ident, strand)
            gff.cds(NAMES[k], exons, ident + ".1", strand)
            x = y + 40
    assert b.next[0] < LENGTHS[0] - 200 and b.next[2] < LENGTHS[2] - 200, b.next
    texts = [bytes(t) for t in b.texts]
    hits = [orc.scan_score(t, 20) for t in texts]
    return dict(contigs=texts, names=list(NAMES), gff="\n".join(gff.lines) + "\n", hits=hits, ids=gff.ids, planted=b.planted)
