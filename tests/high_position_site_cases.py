"""The restriction-site inputs of tests/test_high_positions.py: an enzyme set of eight, the flanks, and the reference's
columns of a placement (tests/site_reference.py over the letters moved down by Placed.base: the masks do not depend on where
the arena begins, and a byte string of 2 GB is not to be built).

ENZYMES   poly_a      AAAA: occurs at every position of the filler, so an enzyme's rank rows reach about 2^30 at `straddle` and
                      about 2^31 at `top`, and every trip of the scan over the chunk sums starts from a non-zero carry
          span16      ANNNNNNNNNNNNNNA: the longest motif there is, in the filler and in the case contigs -- the planes' halo
          AluI        AGCT, a palindrome of four;  MnlI  CCTC, four letters and no palindrome
          BstNI       CCWGG and HinfI GANTC: palindromes of five with an IUPAC letter
          cut_plus, cut_minus   the eight letters around the cut of the first-copy row of the middle pair of hp_tie's block, one
                      per strand (cut_out_motifs): each occurs once in either copy and nowhere else, so an amplicon that holds
                      one copy counts exactly 1 and one that holds both counts 2
FLANKS    16 (the longest motif), 64, 300 (the default), 1000 -- the copies lie 1 422 apart, so at `straddle` an amplicon of
          half-width 1000 around a cut in either copy crosses arena position 2^30 and holds one copy only -- and 100000 (the
          largest: every amplicon is its whole text)
On the device the filler is text 0 with bounds [64, 64 + n); no row's cut lies in it, a separator word of 64 void positions
lies behind it, and a motif has at most 16 letters: it is simply absent from the local statement."""
import numpy as np

import high_position_cases as hp
import site_reference as ref

L = 20
FLANKS = (16, 64, 300, 1000, 100000)
CROSSING_FLANK = 1000
FIXED = [("poly_a", "AAAA"), ("span16", "A" + "N" * 14 + "A"), ("AluI", "AGCT"), ("MnlI", "CCTC"), ("BstNI", "CCWGG"), ("HinfI", "GANTC")]
FOUR_CUTTERS = ("AluI", "MnlI")
CUT_OUT = ("cut_plus", "cut_minus")


def cut_of(pos, minus):
    """The cut boundary of the site column's definition: i - 3 of a '+' row, j + 6 of a '-' row."""
    return int(pos) + 6 if minus else int(pos) - 3


def cut_out_rows(hits):
    """Per strand the first-copy row of the middle pair of the tie block (an index into hp_tie's table of that strand)."""
    out = {}
    for strand in ("plus", "minus"):
        pairs = hp.tie_pairs(hits, strand)
        out[strand] = pairs[len(pairs) // 2][0]
    return out


def cut_out_motifs(contigs, hits):
    """(the '+' motif, the '-' motif): the letters contig[c - 4 : c + 4] around the cut c of cut_out_rows' rows."""
    text = contigs[hp.TIE]
    out = []
    for strand, row in cut_out_rows(hits).items():
        c = cut_of(hits[hp.TIE]["pos_" + strand][row], strand == "minus")
        out.append(text[c - 4:c + 4].decode())
    return tuple(out)


def enzymes(contigs, hits):
    """[(name, motif)] of the set, the two cut-out motifs last."""
    return FIXED + list(zip(CUT_OUT, cut_out_motifs(contigs, hits)))


def mask(names, some):
    return sum(1 << names.index(n) for n in some)


def count_in(text, motif):
    """Occurrences of the motif on either strand of one text, by site_reference's own statement."""
    return int(ref.occurrences_numpy(text, motif).sum())


def local_bounds(placed):
    """[(t0, t1)] of the case contigs in the letters moved down by placed.base."""
    return [(o - placed.base, o - placed.base + n) for o, n in zip(placed.offsets, placed.case.lengths)]


def columns(placed, motifs, flank, bounds=None, arena=None, shift=0):
    """dict(plus, minus) of site_reference.columns_numpy over placed.local_arena and placed.local_tables.  bounds, arena, shift:
    another statement of the texts' bounds, other letters, and what to add to the local positions for them."""
    arena = placed.local_arena if arena is None else arena
    bounds = local_bounds(placed) if bounds is None else bounds
    t = placed.local_tables
    return {s: ref.columns_numpy(arena, bounds, t["pos_" + s].astype(np.int64) + shift, s == "minus", L, flank, motifs) for s in ("plus", "minus")}


def amplicon(placed, strand, flank, m):
    """(a_lo, last start a_hi - m, cut) per row of one strand's table, in ARENA positions: the amplicon clipped to the row's text."""
    pos = placed.tables["pos_" + strand].astype(np.int64)
    c = pos + 6 if strand == "minus" else pos - 3
    starts = np.array(placed.offsets, np.int64)
    ends = starts + np.array(placed.case.lengths, np.int64)
    k = np.searchsorted(starts, c, "right") - 1
    assert (k >= 0).all() and (c < ends[k]).all()  # every row's cut lies in its own text
    return np.maximum(c - flank, starts[k]), np.minimum(c + flank, ends[k]) - m, c


def index_bytes(n_enzymes, n_words):
    """The bytes of an arena's site index: per enzyme an occurrence plane of 8 B a word, a rank row of 4 B a word and one more
    element for the total, and a chunk sum of 4 B per 1 024 words."""
    return n_enzymes * (8 * n_words + 4 * (n_words + 1) + 4 * ((n_words + 1023) // 1024))
