"""The inputs of tests/test_splice_edit.py.

random_case(seed): a small contig of random letters (ACGTN and lower case) with random exon structures on both strands --
short introns among them, and site letters written at many exon edges -- for the comparison of the restatements at every row.

build(orc): an ~80 kb genome of four contigs (30 000, 6 000, 22 000 and 22 000 letters: one arena, or three of at most 600
words) with a GFF of its own.  Most of it is random background, whose genes hold natural cases by the hundred; into it are
PLANTED constructs: a guide in a stretch of letters its editor does not touch (A / T for a cytosine editor, T alone for an
adenine editor's '+' row, A alone for its '-' row), a splice site written at a chosen letter of its window, and a gene
around it whose primary transcript has that site at an intron with 31 coding letters 5' of it.  `planted` lists, per
construct, what the definition must give there; the tests assert that on the reference's rows before they look at the device.
"""
import numpy as np

from select_coding_cases import _Gff

NAMES = ["p0", "p1", "p2", "p3"]
LENGTHS = (30000, 6000, 22000, 22000)
WINDOW = (4, 8)
NO_SITE = 0xFFFFFFFF
EDITS = {"C": ("cbe", False), "G": ("cbe", True), "A": ("abe", False), "T": ("abe", True)}  # the letter -> (editor, '-' row) that converts it
SITES = {("+", "start"): (b"GT", "donor"), ("+", "end"): (b"AG", "acceptor"), ("-", "start"): (b"CT", "acceptor"), ("-", "end"): (b"AC", "donor")}


def random_case(seed, n=700):
    """(text, GFF text) of one contig `s`: letters ACGT with N and lower case mixed in, six genes of random exons with introns
    from one letter on, and GT / CT / AG / AC (or near misses) at most exon edges."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTacgtNn", dtype=np.uint8) if seed % 2 else np.frombuffer(b"ACGT", dtype=np.uint8)
    text = bytearray(rng.choice(alpha, n).tobytes())
    gff = _Gff()
    sites = {"+": ([b"GT", b"GT", b"GT", b"gt", b"GC", b"NT"], [b"AG", b"AG", b"AG", b"ag", b"AT", b"AN"]),
             "-": ([b"CT", b"CT", b"CT", b"cT", b"CC", b"Ct"], [b"AC", b"AC", b"AC", b"aC", b"GC", b"NC"])}
    for g in range(6):
        lo = int(rng.integers(15, n - 300))
        strand = "+-"[g % 2]
        ident = "r%d" % g
        gff.gene("s", lo, lo + 290, ident, strand)
        x, exons = lo - int(rng.integers(0, 3)) * 5, []  # (some coding sequences begin before the gene row)
        for _ in range(int(rng.integers(2, 7))):
            length = int(rng.integers(1, 60))
            exons.append((x, x + length - 1))
            x += length + (int(rng.integers(1, 6)) if rng.integers(3) == 0 else int(rng.integers(6, 40)))
        gff.cds("s", exons, ident, strand)
        opens, closes = sites[strand]
        for a, b in exons:
            if rng.integers(6) and 2 <= a:
                text[a - 2:a] = closes[int(rng.integers(len(closes)))]
            if rng.integers(6) and b + 3 <= n:
                text[b + 1:b + 3] = opens[int(rng.integers(len(opens)))]
    return bytes(text), "\n".join(gff.lines) + "\n"


class _Builder:
    def __init__(self):
        rng = np.random.default_rng(2022)
        self.rng = rng
        self.texts = [bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()) for n in LENGTHS]
        self.gff = _Gff()
        self.planted = []
        self.next = [200, 200, 200, 200]  # where the next construct goes, per contig
        self.n_gene = 0

    def name(self, stem):
        self.n_gene += 1
        return "%s_%d" % (stem, self.n_gene)

    def room(self, k, n=260):
        a = self.next[k]
        self.next[k] += n
        return a

    def quiet(self, k, lo, hi, editor, minus_row):
        """Over [lo, hi): nothing the editor converts on that row, no PAM."""
        lo, hi = max(lo, 0), min(hi, LENGTHS[k])
        letters = b"AT" if editor == "cbe" else (b"A" if minus_row else b"T")
        self.texts[k][lo:hi] = self.rng.choice(np.frombuffer(letters, dtype=np.uint8), hi - lo).tobytes()

    def guide(self, k, editor, minus_row, x, w):
        """A guide whose default window's letter w (ascending, 0 .. 4; -1: the letter just below it, 5: just above) is the
        position x, in a quiet stretch over the 30 letters the score reads and 10 more on either side.  Returns the match index."""
        t = self.texts[k]
        if not minus_row:  # 30-mer s[i - 25 : i + 5], NGG at i; window letter p at i - 21 + p
            i = x - w + 17
            self.quiet(k, i - 35, i + 15, editor, minus_row)
            t[i + 1:i + 3] = b"GG"
            return i
        j = x - w - 15          # 30-mer s[j - 2 : j + 28], CCN at j; window letter p at j + 23 - p
        self.quiet(k, j - 12, j + 38, editor, minus_row)
        t[j:j + 2] = b"CC"
        return j

    def put(self, k, x, letters):
        self.texts[k][x:x + len(letters)] = letters

    def expect(self, ident, k, pos, minus_row, editor, donors, acceptors, donor_off, acceptor_off, what):
        self.planted.append(dict(gene=ident, contig=k, pos=pos, minus=minus_row, editor=editor, donors=donors, acceptors=acceptors,
                                 donor_off=donor_off if donors else NO_SITE, acceptor_off=acceptor_off if acceptors else NO_SITE, what=what))


def _exons(side, X):
    """Two exons of 31 letters with a 60-letter intron whose start site (side 'start') or end site ('end') has its lower
    letter at X: 31 coding letters lie 5' of the intron on either gene strand (L_P = 62)."""
    return [(X - 31, X - 1), (X + 60, X + 90)] if side == "start" else [(X - 89, X - 59), (X + 2, X + 32)]


def build(orc):
    """dict(contigs, names, gff, hits, ids, planted)."""
    b = _Builder()
    gff = b.gff

    def one(k, stem, strand, side, letters, editor, minus_row, x_of, w, counts, what, exons_of=None, gene=True):
        """A site `letters` with its lower letter at X and a guide whose window letter w is X + x_of; counts: whether the site
        is destroyed."""
        a = b.room(k)
        X = a + 120
        pos = b.guide(k, editor, minus_row, X + x_of, w)
        b.put(k, X, letters)
        ident = b.name(stem)
        exons = (exons_of or (lambda X: _exons(side, X)))(X)
        gff.gene(NAMES[k], a + 10, a + 250, ident, strand)
        if gene:
            gff.cds(NAMES[k], exons, ident, strand)
        kind = SITES[strand if strand in "+-" else "+", side][1]
        b.expect(ident, k, pos, minus_row, editor, int(counts and kind == "donor"), int(counts and kind == "acceptor"), 31, 31, what)
        return ident, pos, X

    # ---- every destroying case of the definition's table: the edited letter at either edge of the window (with its partner just
    # outside where it is the outer one) and just outside either edge; then the same sites under the editors and rows that do not
    # touch them
    for strand in "+-":
        k = 0 if strand == "+" else 2
        for side in ("start", "end"):
            letters, kind = SITES[strand, side]
            for e in (0, 1):
                editor, minus_row = EDITS[chr(letters[e])]
                for w, place, counts in ((0, "the window's first letter", True), (4, "the window's last letter", True),
                                         (-1, "just below the window", False), (5, "just above the window", False)):
                    partner = " (its partner outside)" if (w, e) in ((0, 1), (4, 0)) else ""
                    one(k, "%s_%s%d" % (kind, strand == "+" and "p" or "m", e), strand, side, letters, editor, minus_row, e, w, counts,
                        "%s gene %s %s: %s of a %s row at %s%s" % (strand, kind, letters.decode(), chr(letters[e]), "-" if minus_row else "+", place, partner))
            for editor in ("cbe", "abe"):
                for minus_row in (False, True):
                    if (editor, minus_row) not in (EDITS[chr(letters[0])], EDITS[chr(letters[1])]):
                        one(k, "untouched", strand, side, letters, editor, minus_row, 0, 2, False,
                            "%s gene %s %s under %s on a %s row: no letter of it converts" % (strand, kind, letters.decode(), editor, "-" if minus_row else "+"))
    # ---- sites that are not evaluated, all with a converted letter in the window
    one(0, "gc_donor", "+", "start", b"GC", "cbe", True, 0, 2, False, "a GC donor")
    one(0, "at_ac_start", "+", "start", b"AT", "abe", False, 0, 2, False, "the AT of an AT-AC intron")
    one(0, "at_ac_end", "+", "end", b"AC", "abe", False, 0, 2, False, "the AC of an AT-AC intron")
    one(0, "with_n", "+", "start", b"GN", "cbe", True, 0, 2, False, "an N in a site")
    one(0, "lower_case", "+", "start", b"gt", "cbe", True, 0, 2, True, "lower-case letters in a site")
    one(2, "lower_case_m", "-", "end", b"aC", "abe", False, 0, 2, True, "lower-case letters in a site of a '-' gene")
    # ---- the boundary before P's first exon and behind its last: an AG before, a GT behind, one exon
    one(0, "before_first", "+", "end", b"AG", "cbe", True, 1, 2, False, "the boundary before P's first exon", exons_of=lambda X: [(X + 2, X + 62)])
    one(0, "behind_last", "+", "start", b"GT", "cbe", True, 0, 2, False, "the boundary behind P's last exon", exons_of=lambda X: [(X - 61, X - 1)])
    one(2, "before_first_m", "-", "end", b"AC", "abe", False, 0, 2, False, "the boundary behind P's last exon of a '-' gene", exons_of=lambda X: [(X + 2, X + 62)])
    # ---- genes without a model over a construct: no CDS, and a strand that is none
    one(0, "no_cds", "+", "start", b"GT", "cbe", True, 0, 2, False, "a gene without CDS rows", gene=False)
    one(0, "no_strand", ".", "start", b"GT", "cbe", True, 0, 2, False, "a gene whose strand is none")
    # ---- introns of 3, 2 and 1 letters: GTA and GT are donors whose letters are no coding letters; a lone G is no site
    one(0, "intron3", "+", "start", b"GTA", "cbe", True, 0, 2, True, "a 3-letter intron", exons_of=lambda X: [(X - 31, X - 1), (X + 3, X + 33)])
    one(0, "intron2", "+", "start", b"GT", "cbe", True, 0, 2, True, "a 2-letter intron", exons_of=lambda X: [(X - 31, X - 1), (X + 2, X + 32)])
    one(0, "intron1", "+", "start", b"G", "cbe", True, 0, 2, False, "a 1-letter intron", exons_of=lambda X: [(X - 31, X - 1), (X + 1, X + 31)])
    # ---- P's first and last intron of three; the acceptor of the last has 31 + 40 letters 5' of it
    a = b.room(0, 520)
    X1, X2 = a + 120, a + 120 + 60 + 40 + 58  # the first intron's start site; the last intron's end site (its lower letter)
    exons = [(X1 - 31, X1 - 1), (X1 + 60, X1 + 99), (X2 + 2, X2 + 32)]
    pos = b.guide(0, "cbe", True, X1, 0)
    b.put(0, X1, b"GT")
    b.expect("three_exons", 0, pos, True, "cbe", 1, 0, 31, 0, "P's first intron: its donor")
    pos = b.guide(0, "abe", False, X2, 4)
    b.put(0, X2, b"AG")
    b.expect("three_exons", 0, pos, False, "abe", 0, 1, 0, 71, "P's last intron: its acceptor")
    gff.gene(NAMES[0], a + 10, a + 500, "three_exons", "+")
    gff.cds(NAMES[0], exons, "three_exons", "+")
    # ---- an intron of another transcript only: P is one exon, a shorter transcript has an intron behind it
    a = b.room(0, 520)
    X = a + 300
    pos = b.guide(0, "cbe", True, X, 2)
    b.put(0, X, b"GT")
    gff.gene(NAMES[0], a + 10, a + 500, "other_tx", "+")
    gff.mrna(NAMES[0], a + 10, a + 500, "other_tx.1", "other_tx", "+")
    gff.cds(NAMES[0], [(a + 100, a + 199)], "other_tx.1", "+")
    gff.mrna(NAMES[0], a + 10, a + 500, "other_tx.2", "other_tx", "+")
    gff.cds(NAMES[0], [(X - 21, X - 1), (X + 60, X + 80)], "other_tx.2", "+")
    b.expect("other_tx", 0, pos, True, "cbe", 0, 0, 0, 0, "an intron of another transcript only")
    # ---- two introns around a 3-letter exon: under the window 1-20 one '-' row destroys two donors and two acceptors
    a = b.room(0)
    X = a + 120
    j = X - 5  # the window 1-20 is j + 3 .. j + 22, the default window j + 15 .. j + 19 = X + 10 .. X + 14
    b.quiet(0, j - 12, j + 38, "cbe", True)
    b.put(0, j, b"CC")
    for at, letters in ((X, b"GT"), (X + 4, b"AG"), (X + 9, b"GT"), (X + 13, b"AG")):
        b.put(0, at, letters)
    gff.gene(NAMES[0], a + 10, a + 250, "two_introns", "+")
    gff.cds(NAMES[0], [(X - 31, X - 1), (X + 6, X + 8), (X + 15, X + 45)], "two_introns", "+")
    b.expect("two_introns", 0, j, True, "cbe", 0, 1, 0, 34, "two introns under one guide")
    # ---- a gene nested in an intron: the row destroys the inner gene's donor and nothing of the outer gene
    a = b.room(0, 900)
    X = a + 400
    pos = b.guide(0, "cbe", True, X, 2)
    b.put(0, X, b"GT")
    gff.gene(NAMES[0], a + 10, a + 880, "outer", "+")
    gff.cds(NAMES[0], [(a + 50, a + 110), (a + 800, a + 860)], "outer", "+")
    gff.gene(NAMES[0], X - 60, X + 120, "nested", "+")
    gff.cds(NAMES[0], _exons("start", X), "nested", "+")
    b.expect("nested", 0, pos, True, "cbe", 1, 0, 31, 0, "the gene nested in the intron")
    b.expect("outer", 0, pos, True, "cbe", 0, 0, 0, 0, "the outer gene: a row inside its intron")
    # ---- limits hit with equality: L_P = 300, introns behind the coding letters 15 and 195
    a = b.room(0, 700)
    exons = [(a + 100, a + 114), (a + 175, a + 354), (a + 415, a + 519)]
    for X, off in ((a + 115, 15), (a + 355, 195)):
        pos = b.guide(0, "cbe", True, X, 0)
        b.put(0, X, b"GT")
        b.expect("exact300", 0, pos, True, "cbe", 1, 0, off, 0, "a donor behind %d of 300" % off)
    gff.gene(NAMES[0], a + 10, a + 650, "exact300", "+")
    gff.cds(NAMES[0], exons, "exact300", "+")
    # ---- '-' rows at every contig end whose window reaches past the end: the T of a donor is the contig's last letter
    for k, n in enumerate(LENGTHS):
        j = n - 16  # the default window is j + 15 .. j + 19 = n - 1 .. n + 3
        b.quiet(k, n - 60, n, "abe", True)
        b.put(k, j, b"CC")
        b.put(k, n - 2, b"GT")
        ident = "end_%d" % k
        gff.gene(NAMES[k], n - 50, n + 120, ident, "+")
        gff.cds(NAMES[k], [(n - 33, n - 3), (n + 60, n + 90)], ident, "+")
        b.expect(ident, k, j, True, "abe", 1, 0, 31, 0, "a '-' row whose window reaches past the end of contig %d" % k)
    # ---- a gene with a model and no step in the text; step counts 2, 64 and 65 in random background (select_coding_cases' recipe)
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
        for (ea, eb), nxt in zip(exons[:-1], exons[1:]):  # canonical sites at its many introns: natural cases under every window
            b.put(3, eb + 1, b"GT" if strand == "+" else b"CT")
            b.put(3, nxt[0] - 2, b"AG" if strand == "+" else b"AC")
        at = x + 100
    # ---- random background genes of a few exons each, both strands, canonical sites at most introns: natural cases by the hundred
    rng = np.random.default_rng(9)
    for k, first in ((0, 19000), (1, 1200), (2, 9000), (3, 4000)):
        x = first
        for g in range(16):
            if x + 900 > LENGTHS[k] - 200:
                break
            ident = b.name("bg%d" % k)
            strand = "+-"[g % 2]
            exons, y = [], x + 20
            for _ in range(int(rng.integers(2, 6))):
                n = int(rng.integers(30, 200))
                exons.append((y, y + n - 1))
                y += n + int(rng.integers(20, 90))
            gff.gene(NAMES[k], x, y, ident, strand)
            gff.mrna(NAMES[k], x, y, ident + ".1", ident, strand)
            gff.cds(NAMES[k], exons, ident + ".1", strand)
            for (ea, eb), nxt in zip(exons[:-1], exons[1:]):
                if rng.integers(5):
                    b.put(k, eb + 1, b"GT" if strand == "+" else b"CT")
                if rng.integers(5):
                    b.put(k, nxt[0] - 2, b"AG" if strand == "+" else b"AC")
            x = y + 40
    assert b.next[0] < 19000 and b.next[2] < 9000, b.next
    texts = [bytes(t) for t in b.texts]
    for p in b.planted:  # the window's converted letters, counted on the finished text
        src = {v: c for c, v in EDITS.items()}[p["editor"], p["minus"]]
        xs = range(p["pos"] + 15, p["pos"] + 20) if p["minus"] else range(p["pos"] - 17, p["pos"] - 12)
        p["targets"] = sum(1 for x in xs if 0 <= x < len(texts[p["contig"]]) and chr(texts[p["contig"]][x]).upper() == src)
    hits = [orc.scan_score(t, 20) for t in texts]
    return dict(contigs=texts, names=list(NAMES), gff="\n".join(gff.lines) + "\n", hits=hits, ids=gff.ids, planted=b.planted)
