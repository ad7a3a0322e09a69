"""Inputs of the self-selection tests (test_select_self.py): the patterns, a ~80 kb genome in four texts with soft-masked
stretches, N runs, a tandem repeat per strand and a planted pair of sites that share a cut letter, the saturation texts, and
the builders that choose genes ON THE ROWS a search fetched.  Every builder returns what it claims together with the genes, and
the tests prove the claim on the reference before a GPU result is compared."""
import numpy as np

import select_self_reference as ref

# id -> (candidate pattern, guide pattern or None, PAM letters, PAM on the 3' side, cut offset or None for the default)
PATTERNS = {
    "ngg": ("N" * 20 + "NRG", "N" * 20 + "NGG", 3, True, 17),
    "cas12a": ("TTTV" + "N" * 23, None, 4, False, 22),
    "t32": ("N" * 29 + "NGG", None, 3, True, None),
    "tiny": ("NNNNNGG", None, 3, True, None),
}
UNIT = b"ATTATAATATTAATTTATAAAGG"  # 20 letters of A / T, then AGG: one '+' NGG site per copy, no CC, no other GG
REPEATS = 70                      # copies of the unit, and of its reverse complement: at least 65 equal rows per strand
SHARED_AT = 3000                  # text 1: a '+' site here and a '-' site 11 letters on cut before the same letter (c = 17)


def revcomp(b):
    return b.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


def genome(seed=5):
    """Four texts, ~80 kb: random letters, lower-case stretches, N runs, the two tandem repeats and the shared-cut plant."""
    rng = np.random.default_rng(seed)
    texts = []
    for n in (30011, 20000, 24989, 5003):
        t = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())
        for _ in range(n // 4000):
            a = int(rng.integers(0, n - 300))
            t[a:a + 200] = bytes(t[a:a + 200]).lower()
        texts.append(t)
    for t in texts:  # N runs of 1 .. 39 letters, two of them soft-masked 'n'
        n = len(t)
        for j in range(max(1, n // 9000)):
            a = 500 + j * 7001 % (n - 600)
            ln = 1 + (a * 7) % 39
            t[a:a + ln] = (b"n" if j % 2 else b"N") * ln
    texts[0][9000:9000 + len(UNIT) * REPEATS] = UNIT * REPEATS
    texts[2][10000:10000 + len(UNIT) * REPEATS] = revcomp(UNIT) * REPEATS
    w = bytearray(b"ATTAATATAATTATATTAATATA")
    w[11:13], w[21:23] = b"CC", b"GG"
    texts[1][SHARED_AT:SHARED_AT + 23] = w
    texts[1][SHARED_AT + 23:SHARED_AT + 40] = b"ATATTATAATATTAATA"  # (bases under the '-' site's window)
    return [bytes(t) for t in texts]


SMALL_COPIES = 41  # the small family of saturation_c0: 40 other perfect copies each


def saturation_c0():
    """counts[0] above 65 535 in two classes with different raw counts, under ...NGG: a repeat family of 65 700 identical '+'
    sites FIRST in the text, then a small family of 41, then a poly-G run of just over 65 536 + 20 letters (about 65 540 sites of
    one guide).  Raw counts order the poly-G sites before the repeat family; saturated they tie at the top field and the
    later fields and the cut letter decide.  A field that merely truncated to 16 bits would put both classes (163 and about 5)
    around the small family's 40."""
    big, small = b"ATTATAATATTAATTTATAAAGG", b"TTATTATATAATTTAATAATAGG"
    return [b"ACGTTTACGTAAACGT" + big * 65700 + b"ACAT" + small * SMALL_COPIES + b"ACAT" + b"G" * (65536 + 20 + 8) + b"TACGTAAACGT"]


def saturation_c1():
    """Two families of identical '+' sites, 4 200 and 4 100 copies (the larger one FIRST in the text), and behind each family one
    site that differs from its family's guide in one letter: those two sites have no perfect copy and 4 200 and 4 100 hits of
    one mismatch.  Raw counts order the second before the first; saturated at 4 095 they tie, and the cut letter decides."""
    u1, u2 = b"ATTATAATATTAATTTATAAAGG", b"TTATTATATAATTTAATAATAGG"
    v1, v2 = bytearray(u1), bytearray(u2)
    v1[5], v2[7] = ord("C"), ord("C")
    return [b"ACGT" + u1 * 4200 + bytes(v1) + b"ACAT" + u2 * 4100 + bytes(v2) + b"ACGTACAT"]


IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT",
         "H": "ACT", "V": "ACG", "N": "ACGT"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def candidates(texts, offsets, pattern):
    """(arena start, strand) of every candidate of an arena's texts in extraction order, stated on the letters: a window is a
    '+' candidate when every non-N pattern position holds a base of its set (an N position holds anything, a non-base too), a
    '-' candidate when its reverse complement does.  Order: by (64-position word, strand, position)."""
    T = len(pattern)
    pos, strand = [], []
    for text, off in zip(texts, offsets):
        u = np.frombuffer(text.upper(), np.uint8)
        n = u.size - T + 1
        if n <= 0:
            continue
        plus, minus = np.ones(n, bool), np.ones(n, bool)
        for p, ch in enumerate(pattern):
            if ch == "N":
                continue
            plus &= np.isin(u[p:p + n], np.frombuffer(IUPAC[ch].encode(), np.uint8))
            comp = "".join(COMP[b] for b in IUPAC[ch])
            minus &= np.isin(u[T - 1 - p:T - 1 - p + n], np.frombuffer(comp.encode(), np.uint8))
        for st, m in ((0, plus), (1, minus)):
            at = np.nonzero(m)[0] + int(off)
            pos.append(at)
            strand.append(np.full(at.size, st, np.int64))
    pos, strand = np.concatenate(pos), np.concatenate(strand)
    order = np.argsort(((pos >> 6) << 7) | (strand << 6) | (pos & 63), kind="stable")
    return pos[order], strand[order]


# ---- genes chosen on fetched rows --------------------------------------------------------------------------------------------

def sorted_cuts(rows, T, c):
    """The guide sites' cut letters, ascending, with the row behind each."""
    cut = ref.cut_letters(rows["pos"], rows["strand"], T, c)
    order = np.argsort(cut, kind="stable")
    return cut[order], order


def gene_holding(cuts, n, start=0):
    """[lo, hi] that holds exactly n of the ascending cut letters `cuts`, the first such window at or after index `start`."""
    m = len(cuts)
    if n == 0:
        for i in range(start, m - 1):
            if cuts[i + 1] - cuts[i] >= 2:
                return int(cuts[i]) + 1, int(cuts[i + 1]) - 1
        raise AssertionError("no gap")
    for i in range(max(start, 1), m - n):
        if cuts[i - 1] < cuts[i] and cuts[i + n - 1] < cuts[i + n]:
            return int(cuts[i]), int(cuts[i + n - 1])
    raise AssertionError("no window of %d sites" % n)


def size_genes(rows, T, c, sizes):
    """One gene per size in `sizes`, spread over the arena: (lo, hi) arrays."""
    cuts, _ = sorted_cuts(rows, T, c)
    lo, hi = [], []
    for j, n in enumerate(sizes):
        a, b = gene_holding(cuts, n, (j * 97) % max(1, len(cuts) - max(sizes) - 2))
        lo.append(a)
        hi.append(b)
    return np.array(lo, np.uint32), np.array(hi, np.uint32)


def edge_genes(rows, T, c, text_offsets, text_lengths):
    """Genes at the edges the kernels can get wrong; {name: index} and the (lo, hi) arrays."""
    cuts, order = sorted_cuts(rows, T, c)
    strand = np.asarray(rows["strand"])[order]
    names, lo, hi = {}, [], []

    def add(name, a, b):
        names[name] = len(lo)
        lo.append(int(a))
        hi.append(int(b))

    # a one-letter gene on a '+' site's cut whose neighbour in cut order is a '-' site one letter off, and the reverse
    for want, name in ((0, "plus-in-minus-out"), (1, "minus-in-plus-out")):
        for i in range(1, len(cuts) - 1):
            alone = cuts[i - 1] < cuts[i] < cuts[i + 1]
            if alone and strand[i] == want and ((strand[i + 1] != want and cuts[i + 1] - cuts[i] <= 3) or
                                                (strand[i - 1] != want and cuts[i] - cuts[i - 1] <= 3)):
                add(name, cuts[i], cuts[i])
                break
    mid = int(cuts[len(cuts) // 2])
    add("lo-0-mod-64", mid // 64 * 64, mid // 64 * 64 + 300)
    add("lo-63-mod-64", mid // 64 * 64 + 63, mid // 64 * 64 + 300)
    add("hi-0-mod-64", mid // 64 * 64 - 290, mid // 64 * 64)
    add("hi-63-mod-64", mid // 64 * 64 - 290, mid // 64 * 64 + 63)
    add("lo-below-T", 3, T + 40)
    add("lo-zero", 0, T - 1)
    add("first-candidate", 0, cuts[0])
    end = int(text_offsets[-1] + text_lengths[-1]) - 1
    add("last-candidate", cuts[-1], end)
    t = min(1, len(text_offsets) - 1)
    add("whole-contig", text_offsets[t], text_offsets[t] + text_lengths[t] - 1)
    add("whole-arena", 0, end)
    # nested, overlapping and duplicate genes
    add("outer", max(0, mid - 2000), mid + 2000)
    add("nested", mid - 100, mid + 100)
    add("overlap", mid, mid + 3000)
    add("duplicate", mid - 100, mid + 100)
    # one-strand genes: a run of neighbouring sites of one strand
    for want, name in ((0, "plus-only"), (1, "minus-only")):
        for i in range(1, len(cuts) - 3):
            if (strand[i:i + 2] == want).all() and cuts[i - 1] < cuts[i] and cuts[i + 1] < cuts[i + 2]:
                add(name, cuts[i], cuts[i + 1])
                break
    return names, np.array(lo, np.uint32), np.array(hi, np.uint32)


def random_rows(rng, n, M, scored, T=23, span=5000):
    """Rows of made-up guide sites, in extraction order, for the tests that need no GPU: many equal counts, so ties abound."""
    pos = np.sort(rng.integers(0, span, n)).astype(np.uint32)
    strand = rng.integers(0, 2, n).astype(np.uint8)
    key = ((pos.astype(np.int64) >> 6) << 7) | (strand.astype(np.int64) << 6) | (pos & 63)
    order = np.argsort(key, kind="stable")
    pos, strand = pos[order], strand[order]
    counts = rng.integers(0, 3, (n, M + 1)).astype(np.uint32)
    return dict(pos=pos, strand=strand, hi=rng.integers(0, 1 << T, n).astype(np.uint32), lo=rng.integers(0, 1 << T, n).astype(np.uint32),
                counts=counts, hit_sum=(rng.integers(0, 4, n).astype(np.uint64) << np.uint64(28)) if scored else None,
                cand=np.arange(n, dtype=np.uint32) * 2 + 1)
