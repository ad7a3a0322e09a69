"""The genomes of tests/test_guide_properties.py: about 80 kb in four contigs with every window the property kernel can
get wrong built in, and four small texts whose '+' table has an exact number of rows and whose '-' table is empty.  The
tests check on the reference's side that the cases are really there before they look at the device."""
import numpy as np

LENGTHS = (1, 20, 32, 33, 50)
NAMES = ["c0", "c1", "c2", "c3"]
SIZES = (30000, 6000, 20000, 24000)  # three arenas at 600 words each, one at the default
TABLE_ROWS = (64, 65, 256, 257)
TAIL = b"C" * 70 + b"A"  # '-' hits at every j of the last 70 characters but two: windows the contig end cuts by 1 .. 10
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(b):
    return bytes(b).translate(COMP)[::-1]


def hairpin(rng, l, loop):
    """A window of l letters: arm + loop + revcomp(arm), the arm as long as l and the loop allow (padded in front by one
    letter where l - loop is odd).  loop >= 3: stem = len(arm), the most a window of l letters can hold when loop is 3 or 4."""
    s = (l - loop) // 2
    rand = lambda n: rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()
    arm = rand(s)
    w = b"A" * (l - loop - 2 * s) + arm + b"ATTA"[:loop] + revcomp(arm)
    assert len(w) == l
    return w


def palindrome(rng, l):
    """A reverse palindrome of l letters (l even)."""
    half = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), l // 2).tobytes()
    return half + revcomp(half)


def designed(l):
    """{name: window} of the designed '+' windows of guide length l (each is followed by AGG in the genome)."""
    rng = np.random.default_rng(1000 + l)
    out = {"poly_t": b"T" * l, "poly_a": b"A" * l, "no_base": b"N" * l}
    if l >= 5:
        out["hairpin"] = hairpin(rng, l, 3 + (l - 3) % 2)
        out["hairpin_loop2"] = hairpin(rng, l, 2)
    if l >= 4 and l % 2 == 0:
        out["palindrome"] = palindrome(rng, l)
    return out


def contigs():
    rng = np.random.default_rng(1717)
    rand = lambda n: rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()
    texts = [bytearray(rand(n)) for n in SIZES]
    c0 = texts[0]
    # '+' rows with i - l = 5: GG at i + 1, i + 2 for i = l + 5
    c0[0:64] = b"AT" * 32
    for l in LENGTHS:
        c0[l + 6:l + 8] = b"GG"
    # the designed windows, each as a '+' window (window + AGG) and, reverse-complemented, as a '-' window (CCT + ...)
    at = 1000
    for l in LENGTHS:
        for name, w in sorted(designed(l).items()):
            c0[at:at + l + 3] = w + b"AGG"
            at += l + 40
            c0[at:at + l + 3] = b"CCT" + (w if name == "no_base" else revcomp(w))
            at += l + 40
    assert at < 9000
    c0[10000:10012] = b"N" * 12                         # an N run
    for k, ch in enumerate(b"RYSWKMBDHVZun"):           # single IUPAC letters, Z, lower-case u and n
        c0[10500 + 37 * k] = ch
    c0[11200:11400] = bytes(c0[11200:11400]).lower()    # a soft-masked stretch
    c0[11500:11530] = bytes(c0[11500:11530]).replace(b"A", b"U")
    texts[2][5000:5300] = bytes(texts[2][5000:5300]).lower()
    texts[3][100:130] = b"N" * 30
    for t in texts:                                     # every contig ends in the tail: the last contig of every arena does
        t[-len(TAIL):] = TAIL
    return [bytes(t) for t in texts]


def exact_table(n_rows):
    """A text whose '+' table has n_rows rows at every guide length up to 50 and whose '-' table is empty."""
    return b"AT" * 32 + b"ATATATATATATATATATATATATAAGG" * n_rows + b"ATAT"


def kept(text, l):
    """The scan's keep-filter restated (CROPSR.py:419 / :430): match indices of (?=.GG) and (?=CC.) that stay."""
    import re
    n = len(text)
    plus = [m.start() for m in re.finditer(rb"(?=.GG)", text)]
    minus = [m.start() for m in re.finditer(rb"(?=CC.)", text)]
    ok = lambda a, b: a >= 5 and a + 5 <= n + 10 and b >= 5 and b <= n + 10
    return (np.array([i for i in plus if ok(i - l, i)], np.uint32), np.array([j for j in minus if ok(j + 3, j + 3 + l)], np.uint32))
