"""The arenas of tests/test_high_positions.py: small case contigs behind one long filler contig, so that every arena position
the post-scan kernels see has bit 30 set, or lies on either side of 2^30, or within 2^20 of the arena's top at 2^31.

FILLER    contig 0, upper-case A only: no GG, CC, AG or CT, so it yields no hit row, no NGG / NRG candidate on either strand
          and no seed.  Every search pattern the module uses has a G in its PAM.
CASES     five contigs behind it, in this order:
            sj_c0, sj_c1, sj_c2   the genome of specificity_join_cases (6 kb, planted guide copies on both strands)
            hp_tie                BLOCK twice (see tie_contig), second in the list: the straddle placement puts 2^30 between
                                  the two copies, sj_c0 wholly below and sj_c1, sj_c2, hp_tail wholly above
            hp_tail               two words of text that end with TGG: rows whose repair and property windows reach past the
                                  last word that holds text
LAYOUT    restated here as the device lays an arena out: word 0 is a separator, a contig of n letters takes
          (n + 63) // 64 + 1 words (its text and one separator), offset[k] = 64 * (1 + the words before it).
PLACEMENT straddle: the filler's length puts hp_tie at 2^30 - TIE_AT;  top: it makes the arena exactly max_words words long,
          so hp_tail's text ends in the last word that holds text.
Results are contig-relative, so the references of the suite run on the case contigs alone; contig k of the cases is contig
k + 1 of the device's genome.  The references that take arena positions -- the spaced selection, the distinct pairs, the self
selection -- run on the case contigs' tables at their placed positions (arena_tables), and the restriction-site reference on the
same letters moved down by a multiple of 64 (tests/high_position_site_cases.py has its enzymes and flanks)."""
import numpy as np

import specificity_join_cases as join_cases

TWO30, TWO31 = 1 << 30, 1 << 31
FILLER_NAME = "filler"
NAMES = ["sj_c0", "hp_tie", "sj_c1", "sj_c2", "hp_tail"]
TIE = 1                       # index of hp_tie among the cases
BLOCK, LEAD, GAP = 420, 64, 1002
TIE_AT = 1024                 # straddle: arena position 2^30 is letter TIE_AT of hp_tie, inside the gap
COPY = (LEAD, LEAD + BLOCK + GAP)    # first letters of the two copies
INTRON = (151, 258)           # block-local first and last letter of tie_introns' intron, in either copy
STOP_AT = 300                 # block-local first letter of a planted CAA, in frame in both genes and both copies
TAIL_LEN = 128
PLACEMENTS = ("straddle", "top")
assert (BLOCK + GAP) % 3 == 0 and STOP_AT % 3 == 0             # the copies lie in one reading frame of the one-exon CDS
assert (INTRON[1] - INTRON[0] + 1) % 3 == 0 and INTRON[1] < STOP_AT  # ... and of the three exons
assert COPY[0] + BLOCK <= TIE_AT - 64 and TIE_AT + 64 <= COPY[1]  # 2^30 lies between them, a word away from either


def words_for(n):
    return (n + 63) // 64 + 1


def offsets_of(lengths):
    """(offset of every contig, words the arena uses) for contigs of these lengths in this order."""
    out, w = [], 1
    for n in lengths:
        out.append(64 * w)
        w += words_for(n)
    return out, w


def filler_length(placement, case_lengths, max_words):
    """The filler's length, a multiple of 64."""
    if placement == "straddle":
        before = sum(words_for(n) for n in case_lengths[:TIE])
        return 64 * ((TWO30 - TIE_AT) // 64 - 2 - before)
    assert placement == "top"
    return 64 * (max_words - 2 - sum(words_for(n) for n in case_lengths))


def filler(n):
    return np.full(n, ord("A"), np.uint8)


def block():
    """BLOCK random letters with some 50 NGG / CCN sites, and planted: GT .. AG at the ends of INTRON, and a CC 17 letters
    before the G of either, so that a '-' row's editing window 4..8 holds that G; CAA at STOP_AT with a GG 16 letters behind
    its C, so that a '+' row's window holds that C and the edit writes TAA."""
    rng = np.random.default_rng(30)
    b = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), BLOCK).tobytes())
    a, z = INTRON
    b[a:a + 2], b[z - 1:z + 1] = b"GT", b"AG"
    b[a - 17:a - 15], b[z - 17:z - 15] = b"CC", b"CC"
    b[STOP_AT:STOP_AT + 3], b[STOP_AT + 16:STOP_AT + 18] = b"CAA", b"GG"
    return bytes(b)


def tie_contig():
    """A * LEAD, BLOCK, A * GAP, BLOCK, A * LEAD: every row of one copy has a partner in the other with the same letters
    around it (30 and more), so their scores are bit-equal and only the cut site orders them."""
    b = block()
    return b"A" * LEAD + b + b"A" * GAP + b + b"A" * LEAD


def tail_contig():
    rng = np.random.default_rng(31)
    t = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), TAIL_LEN).tobytes())
    t[100:103], t[TAIL_LEN - 3:] = b"CCA", b"TGG"
    return bytes(t)


def contigs():
    (c0, c1, c2), guides = join_cases.genome()
    return [c0, tie_contig(), c1, c2, tail_contig()], guides


def _row(seq, typ, lo, hi, strand, attrs):
    """string indices lo..hi (dec = 0) -> 1-based coordinates"""
    return "%s\ttest\t%s\t%d\t%d\t.\t%s\t.\t%s" % (seq, typ, lo + 1, hi + 1, strand, attrs)


def build(orc):
    """dict(contigs, names, guides, hits (the oracle's per contig), gff (text), genes [(ident, contig, lo, hi)] in GFF order
    and clipped to their contig, families (text of a family file))."""
    texts, guides = contigs()
    n = [len(t) for t in texts]
    lo, hi = COPY[0], COPY[1] + BLOCK - 1
    a, z = INTRON
    genes = [("tie", 1, lo, hi, "+"), ("tie_introns", 1, lo, hi, "+"), ("sj_g0", 0, 0, n[0] - 1, "-"), ("sj_g1", 2, 80, 1100, "+"),
             ("sj_g2", 3, 0, n[3] - 1, "+"), ("tail_gene", 4, 0, n[4] + 499, "+")]
    lines = ["##gff-version 3"] + [_row(NAMES[k], "gene", g_lo, g_hi, s, "ID=" + i) for i, k, g_lo, g_hi, s in genes]
    lines += [_row("hp_tie", "CDS", lo, hi, "+", "Parent=tie")]                                   # one exon over the gene
    lines += [_row("hp_tie", "CDS", e_lo, e_hi, "+", "Parent=tie_introns")                        # an intron in either copy
              for e_lo, e_hi in ((lo, COPY[0] + a - 1), (COPY[0] + z + 1, COPY[1] + a - 1), (COPY[1] + z + 1, hi))]
    lines += [_row("sj_c0", "CDS", 100, 2000, "-", "ID=sj_g0.cds;Parent=sj_g0"),
              _row("sj_c2", "CDS", 30, 400, "+", "Parent=sj_g2"), _row("sj_c2", "CDS", 500, 900, "+", "Parent=sj_g2")]
    families = "# gene\tfamily\nsj_g0\thomeo\nsj_g1\thomeo\nsj_g2\thomeo\ntie\ttwins\n"
    return dict(contigs=texts, names=list(NAMES), guides=guides, hits=[orc.scan_score(t, 20) for t in texts],
                gff="\n".join(lines) + "\n", families=families,
                genes=[(i, k, g_lo, min(g_hi, n[k] - 1)) for i, k, g_lo, g_hi, _ in genes])


def arena_tables(hits, offsets):
    """The tables of one arena from per-contig hits and the texts' arena offsets (uint32 positions, as the device has them)."""
    cat = lambda key, dt, add: np.concatenate([h[key].astype(dt) + (dt(o) if add else dt(0)) for h, o in zip(hits, offsets)])
    return dict(pos_plus=cat("pos_plus", np.uint32, True), score_plus=cat("score_plus", np.float64, False),
                pos_minus=cat("pos_minus", np.uint32, True), score_minus=cat("score_minus", np.float64, False))


def tie_pairs(hits, strand):
    """[(row in copy 1, row in copy 2)] of hp_tie's table of one strand, by position: rows COPY[1] - COPY[0] apart."""
    pos = hits[TIE]["pos_" + strand].astype(np.int64)
    at = {int(p): r for r, p in enumerate(pos)}
    shift = COPY[1] - COPY[0]
    return [(r, at[int(p) + shift]) for r, p in enumerate(pos) if int(p) + shift in at]
