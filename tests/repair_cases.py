"""The genome of tests/test_repair_outcome.py: about 80 kb in four contigs with every window the repair kernel can get
wrong built in.  The tests check on the reference's side that the cases are really there before they look at the device.

A planted segment has 140 letters and its cut at index 70: as a '+' row (GG at 74, 75: match index 73) and, reverse
complemented, as a '-' row (CC at 64, 65: match index 64).  The PAM lies inside the window from a flank of 5 on, so only
poly-G is one letter throughout at every flank; the other segments are what they are called up to the PAM."""
import numpy as np

FLANKS = (2, 3, 16, 30, 31, 32)
NAMES = ["c0", "c1", "c2", "c3"]
SIZES = (30000, 6000, 20000, 24000)  # three arenas at 600 words each, one at the default
TAIL = b"C" * 70 + b"A"  # '-' hits at every j of the last characters: windows the contig end cuts by 1 .. F letters (scan at -l 1)
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
SEG, CUT = 140, 70
PLANT_AT, PLANT_STEP = 1000, 200
TWOMER_D = (3, 4, 8)  # one of each residue mod 3
MASK_AT, MASK_LEN, MASK_COPY = 12000, 400, 13000  # a stretch and its copy with lower-case flanks around an upper-case core


def revcomp(b):
    return bytes(b).translate(COMP)[::-1]


def _background(fill):
    seg = bytearray(fill * SEG)
    seg[74:76] = b"GG"
    return seg


def plants():
    """{name: 140-letter segment whose '+' row has match index 73 (cut at 70)}, in planting order."""
    out = {}
    out["poly_g"] = b"G" * SEG
    out["poly_a"] = bytes(_background(b"A"))                 # A x 74, GG, A x 64
    out["no_base"] = bytes(_background(b"N"))                # the PAM is the only base text: no left partner, the score is 0
    seg = bytearray((b"AT" * SEG)[:SEG])
    seg[74:76] = b"GG"
    out["unit2"] = bytes(seg)
    out["unit3"] = (b"GGA" * 50)[1:1 + SEG]                  # G, G at 74, 75
    out["unit4"] = (b"AGGT" * 40)[3:3 + SEG]
    for d in TWOMER_D:                                       # AC at p = F - 2, F - 1 and again d further on, nothing else but the PAM
        seg = _background(b"N")
        seg[68:70] = b"AC"
        seg[68 + d:70 + d] = b"AC"
        assert seg[74:76] == b"GG"
        out["twomer_d%d" % d] = bytes(seg)
    seg = _background(b"N")                                  # ACT in tandem across the cut: on d = 3 the run goes on past p = F - 1
    seg[61:74] = b"ACTACTACTACTA"
    out["across_cut"] = bytes(seg)
    seg = _background(b"N")                                  # d = 10 at F = 30: TCA at p = 20 .. 22 = max(0, F - d) on, and one more
    seg[59:63] = b"TTCA"                                     # matching pair in front of the range (p = 19, p + d = 29 < F)
    seg[69:73] = b"TTCA"
    out["range_start"] = bytes(seg)
    seg = _background(b"N")                                  # an IUPAC letter inside a run: ACGTRCA / ACGTACA on d = 8 ...
    seg[62:69] = b"ACGRACG"
    seg[76:83] = b"ACGAACG"
    out["split_run"] = bytes(seg)
    seg = _background(b"N")                                  # ... and one that leaves a piece of length 1: AC R G
    seg[62:66] = b"ACRG"
    seg[76:80] = b"ACAG"
    out["piece_of_one"] = bytes(seg)
    return out


def plant_positions():
    """{name: (match index of the '+' row, match index of the '-' row)} in contig c0."""
    out, at = {}, PLANT_AT
    for name in plants():
        out[name] = (at + 73, at + PLANT_STEP + 64)
        at += 2 * PLANT_STEP
    return out


def contigs():
    rng = np.random.default_rng(2014)
    rand = lambda n: rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()
    texts = [bytearray(rand(n)) for n in SIZES]
    c0 = texts[0]
    c0[0:64] = b"AT" * 32
    c0[2:4] = b"CC"      # the first '-' row a scan can keep: j = 2, cut at 8
    c0[7:9] = b"GG"      # the first '+' row a scan at -l 1 keeps: i = 6, cut at 3 -- the window reaches into the arena's leading void
    c0[26:28] = b"GG"    # and the first one a scan at -l 20 keeps: i = 25
    at = PLANT_AT
    for name, seg in plants().items():
        c0[at:at + SEG] = seg
        c0[at + PLANT_STEP:at + PLANT_STEP + SEG] = revcomp(seg)
        at += 2 * PLANT_STEP
    assert at < 9000
    c0[10000:10012] = b"N" * 12                         # an N run
    for k, ch in enumerate(b"RYSWKMBDHVZun"):           # single IUPAC letters, Z, lower-case u and n
        c0[10500 + 37 * k] = ch
    c0[11500:11530] = bytes(c0[11500:11530]).replace(b"A", b"U")
    # soft-masking: the copy has lower-case flanks around an upper-case core (the scan's PAM match is case-sensitive, so the
    # rows compared are the core's)
    stretch = bytes(c0[MASK_AT:MASK_AT + MASK_LEN])
    c0[MASK_COPY:MASK_COPY + MASK_LEN] = stretch[:150].lower() + stretch[150:250] + stretch[250:].lower()
    texts[2][5000:5300] = bytes(texts[2][5000:5300]).lower()
    texts[3][100:130] = b"N" * 30
    for t in texts:                                     # every contig ends in the tail: the last contig of every arena does
        t[-len(TAIL):] = TAIL
    return [bytes(t) for t in texts]


def kept(text, l):
    """The scan's keep-filter restated (CROPSR.py:419 / :430): match indices of (?=.GG) and (?=CC.) that stay."""
    import re
    n = len(text)
    plus = [m.start() for m in re.finditer(rb"(?=.GG)", text)]
    minus = [m.start() for m in re.finditer(rb"(?=CC.)", text)]
    ok = lambda a, b: a >= 5 and a + 5 <= n + 10 and b >= 5 and b <= n + 10
    return (np.array([i for i in plus if ok(i - l, i)], np.uint32), np.array([j for j in minus if ok(j + 3, j + 3 + l)], np.uint32))
