"""The case genome, GFF and family file of tests/test_family_sets.py: 38 kb over six contigs, one family per case of the
greedy family sets (cropsr_amd/family_sets.py); the test checks on the reference's rows that every case occurs before it
looks at the device.  Gene coordinates here are string indices (dec = 0): the GFF holds index + 1.

  one      three exact copies of one block (the third reverse-complemented): one guide suffices
  gain     X1 = U1 + P, X2 = P + U2, X3 = U3: the shared piece P is short, so the best score lies in a unique piece (gain 1)
           and a lower one in P (gain 2); two steps
  twin     W2 (first in the file, so the lower member and layout row) holds block B once, at the HIGHER position; W1 holds
           it twice: three bit-equal rows tie on gain and score, two of them inside one gene; the smallest cut wins
  strands  TS2 (first in the file) holds the reverse complement of a block at the higher position, TS1 the block
  apart    TA1 on c1 and TA2 on c2 hold one block: with MAX_WORDS the two contigs lie in different arenas
  three    three unrelated genes: incomplete at S = 1 and S = 2
  stuck    K2 lies where there is no G or C: the set ends on gain 0 before S
  none     no member has a row: no pick
  tiny     64 unrelated small genes: 64 steps, and bits 32 .. 63 decide picks
  trips    members with 0, 1, 63, 64 and 65 rows (the wave's trips of 64)
  lap      O1 and O2 overlap: a row of the overlap is a candidate of both; for O2 both bits are in its cover word
  z, v     V1 lies inside Z1, a gene of another family that comes first in the file and owns V1's sites: V1's candidates cover
           V1 alone although V2 holds a copy of its block
  lim      L1 and L2 hold one block whose first 200 letters are copied to a place in no gene: with max_perfect_outside = 0
           the rows inside the copy fail
"""
import numpy as np

import search_self_reference as selfref

PATTERN, GUIDE_PATTERN, PAM_LEN = "N" * 20 + "NRG", "N" * 20 + "NGG", 3
T = len(PATTERN)
NAMES = ["c0", "c1", "c2", "runs", "tiny", "at"]
TRIP_ROWS = (63, 64, 65)
N_TINY, TINY_STEP, TINY_LEN = 64, 80, 70
MAX_WORDS = 300                                       # three arenas: c0 + c1 | c2 + runs + tiny | at
ARENAS_OF_THREE = [[0, 1], [2, 3, 4], [5]]
SEED = 2424


def revcomp(b):
    return bytes(b).translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def contigs():
    rng = np.random.default_rng(SEED)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rand = lambda n: rng.choice(acgt, n).tobytes()
    at = lambda n: rng.choice(np.frombuffer(b"AT", dtype=np.uint8), n).tobytes()
    c0, c1, c2 = bytearray(rand(9000)), bytearray(rand(8000)), bytearray(rand(6000))
    one, piece, twin, strands, apart, inner, lim = rand(260), rand(120), rand(200), rand(200), rand(200), rand(200), rand(300)
    c0[500:760], c1[400:660], c2[300:560] = one, one, revcomp(one)
    c0[1800:1920] = piece                                # X1 = [1500, 1919]: U1 then P
    c1[1200:1320] = piece                                # X2 = [1200, 1619]: P then U2
    c0[2500:2700] = c0[2800:3000] = c0[4000:4200] = twin  # W1 = [2480, 3020] twice, W2 = [3990, 4210] once
    c0[4800:5000], c0[5500:5700] = strands, revcomp(strands)
    c1[5200:5400] = c2[2000:2200] = apart
    c0[7120:7320] = c1[2400:2600] = inner                # V1 inside Z1 = [7000, 7500]; V2
    c0[8000:8300] = c1[3200:3500] = lim
    c1[4200:4400] = lim[:200]                            # in no gene
    runs = bytearray(rand(7000))
    tiny = bytearray(rand(N_TINY * TINY_STEP + 100))
    spare = bytearray(at(3000))                          # no G or C: no site but the planted one
    spare[1500:1523] = at(20) + b"TGG"
    return [bytes(c) for c in (c0, c1, c2, runs, tiny, spare)]


def _trip_genes(texts):
    """[(lo, hi)] on `runs`: consecutive ranges that hold exactly TRIP_ROWS guide sites each, by the reference's rows."""
    k = NAMES.index("runs")
    (ck, pos, strand, _), g = selfref.guide_sites(texts, PATTERN, PAM_LEN, GUIDE_PATTERN)
    mine = g & (ck == k)
    cuts = np.sort(np.where(strand[mine] == 0, pos[mine] + T - 6, pos[mine]))
    out, i = [], 5
    for n in TRIP_ROWS:
        while cuts[i - 1] == cuts[i] or cuts[i + n - 1] == cuts[i + n]:  # the range's ends split no pair of sites at one cut
            i += 1
        out.append((int(cuts[i]), int(cuts[i + n - 1])))
        i += n + 2
    return out


def build():
    """dict(contigs, names, gff (text), families (text), genes [(ident, contig, lo, hi)] in GFF order, family_of {ident:
    token})."""
    texts = contigs()
    genes, fam = [], {}

    def gene(ident, contig, lo, hi, family=None):
        genes.append((ident, NAMES.index(contig), lo, hi))
        if family:
            fam[ident] = family

    gene("one1", "c0", 500, 759, "one")
    gene("X1", "c0", 1500, 1919, "gain")
    gene("W2", "c0", 3990, 4210, "twin")                 # first in the file, at the higher position
    gene("W1", "c0", 2480, 3020, "twin")
    gene("TS2", "c0", 5490, 5710, "strands")
    gene("TS1", "c0", 4790, 5010, "strands")
    gene("O1", "c0", 6000, 6400, "lap")
    gene("O2", "c0", 6200, 6600, "lap")
    gene("Z1", "c0", 7000, 7500, "z")
    gene("V1", "c0", 7100, 7350, "v")
    gene("L1", "c0", 8000, 8299, "lim")
    gene("free", "c0", 8500, 8800)                       # a gene in no family
    gene("one2", "c1", 400, 659, "one")
    gene("X2", "c1", 1200, 1619, "gain")
    gene("V2", "c1", 2390, 2610, "v")
    gene("L2", "c1", 3200, 3499, "lim")
    gene("TA1", "c1", 5190, 5410, "apart")
    gene("D1", "c1", 6000, 6300, "three")
    gene("K1", "c1", 6800, 7100, "stuck")
    gene("one3", "c2", 300, 559, "one")
    gene("X3", "c2", 1000, 1299, "gain")
    gene("TA2", "c2", 1990, 2210, "apart")
    gene("D2", "c2", 3000, 3300, "three")
    gene("D3", "c2", 3700, 4000, "three")
    gene("E0", "at", 100, 900, "trips")                  # no row
    gene("E1", "at", 1400, 1600, "trips")                # one row
    for n, (lo, hi) in zip(TRIP_ROWS, _trip_genes(texts)):
        gene("E%d" % n, "runs", lo, hi, "trips")
    gene("K2", "at", 2000, 2400, "stuck")
    gene("N1", "at", 2500, 2700, "none")
    gene("N2", "at", 2750, 2950, "none")
    for j in range(N_TINY):
        gene("T%d" % j, "tiny", 50 + TINY_STEP * j, 50 + TINY_STEP * j + TINY_LEN - 1, "tiny")
    gff = ["##gff-version 3"]
    for ident, k, lo, hi in genes:
        gff.append("%s\ttest\tgene\t%d\t%d\t.\t+\t.\tID=%s" % (NAMES[k], lo + 1, hi + 1, ident))
    lines = ["# gene\tfamily"] + ["%s\t%s" % kv for kv in fam.items()]
    return dict(contigs=texts, names=list(NAMES), gff="\n".join(gff) + "\n", families="\n".join(lines) + "\n", genes=genes, family_of=fam)
