"""The case genome, GFF and family file of tests/test_families.py: 61 kb over eight contigs, built so that every
case the family kernels can get wrong is present; the test checks that on the reference's rows before it looks at the
device.  Gene coordinates here are string indices (dec = 0): the GFF holds index + 1."""
import numpy as np

import search_self_reference as selfref

PATTERN, GUIDE_PATTERN, PAM_LEN = "N" * 20 + "NRG", "N" * 20 + "NGG", 3
T = len(PATTERN)
NAMES = ["chrA", "chrB", "chrD", "rep", "edge", "runs", "tiny", "spare"]
RUN_GUIDES = (255, 256, 257)  # a tile of queries - 1, one tile, one tile + 1
TINY = 65                     # tiny genes on `tiny`: 64 of them make the largest family, 65 are refused
A_LEN = 1203                  # the homeolog's length: no multiple of 64


def revcomp(b):
    return bytes(b).translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def _plant_edge(text, x):
    """'+' sites that cut at x and x + 1 (starts x - 17, x - 16: NGG at x + 4 and at x + 5) and '-' sites that cut at x and
    x + 1 (forward starts x, x + 1: CCN there)."""
    text[x:x + 3] = b"CCC"
    text[x + 4:x + 7] = b"GGG"


def contigs():
    rng = np.random.default_rng(2323)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rand = lambda n: rng.choice(acgt, n).tobytes()
    at = lambda n: rng.choice(np.frombuffer(b"AT", dtype=np.uint8), n).tobytes()
    homeolog = rand(A_LEN)
    mutated = bytearray(homeolog)
    for p in np.nonzero(rng.random(A_LEN) < 0.03)[0].tolist():
        mutated[p] = int(rng.choice(acgt))
    chrA = bytearray(rand(14000))
    chrA[1001:1001 + A_LEN] = homeolog                   # A1
    chrA[9000:9400] = homeolog[300:700]                  # a copy of a piece in no gene: what lies outside the family
    _plant_edge(chrA, 4999)                              # F1 = [5000, 5777]: cuts at lo - 1, lo
    _plant_edge(chrA, 5777)                              # ... and at hi, hi + 1
    chrB = bytearray(rand(12000))
    chrB[2010:2010 + A_LEN] = mutated                    # A2: ~3 % substitutions
    chrB[2500] = ord("N")                                # a non-base inside a member
    chrB[2700:2760] = bytes(chrB[2700:2760]).lower()
    piece = rand(120)                                    # S1: every window has a copy outside every gene at 1 .. 3 mismatches
    drifted, last = bytearray(piece), -8
    for p in range(120):                                 # A <-> T only (no PAM changes), 8 or a few more letters apart
        if p >= last + 8 and piece[p:p + 1] in (b"A", b"T"):
            drifted[p], last = (ord("T") if piece[p:p + 1] == b"A" else ord("A")), p
    chrB[9000:9120] = piece
    chrB[9500:9620] = drifted
    chrD = bytearray(rand(11000))
    chrD[3333:3333 + A_LEN] = revcomp(homeolog)          # A3: its sites match on the opposite strand
    rep = bytearray(rand(6000))
    unit = rand(151)
    rep[1000:1000 + 2 * 151] = unit * 2                  # E1: an internal tandem repeat, two exact units ...
    for j in (2, 3):                                     # ... and two that have drifted (~8 %): 1 .. 4 mismatches
        drift = bytearray(unit)
        for p in np.nonzero(rng.random(151) < 0.08)[0].tolist():
            drift[p] = int(rng.choice(acgt))
        rep[1000 + j * 151:1000 + (j + 1) * 151] = drift
    edge = bytearray(rand(3000))
    edge[2990:3000] = b"TTCCATTTTT"                      # CCA at 2992: a '-' window that the contig's end cuts (no candidate)
    runs = bytearray(rand(9000))
    tiny = bytearray(rand(TINY * 40 + 100))
    spare = bytearray(at(3000))                          # no G or C: no site but the planted one
    spare[1500:1523] = at(20) + b"TGG"                   # H1: exactly one guide site, H0: none
    return [bytes(c) for c in (chrA, chrB, chrD, rep, edge, runs, tiny, spare)]


def _run_genes(texts):
    """[(lo, hi)] on `runs`: consecutive ranges that hold exactly RUN_GUIDES guide sites each, by the reference's rows."""
    k = NAMES.index("runs")
    (ck, pos, strand, _), g = selfref.guide_sites(texts, PATTERN, PAM_LEN, GUIDE_PATTERN)
    mine = g & (ck == k)
    cuts = np.sort(np.where(strand[mine] == 0, pos[mine] + T - 6, pos[mine]))
    out, i = [], 3
    for n in RUN_GUIDES:
        while cuts[i - 1] == cuts[i] or cuts[i + n - 1] == cuts[i + n]:  # the range's ends split no pair of sites at one cut
            i += 1
        out.append((int(cuts[i]), int(cuts[i + n - 1])))
        i += n + 2
    return out


def build():
    """dict(contigs, names, gff (text), families (text), too_many (a family file of 65 members), genes [(ident, contig,
    lo, hi)] in GFF order, family_of {ident: token}, unknown (names of the file that the GFF lacks))."""
    texts = contigs()
    genes, fam = [], {}

    def gene(ident, contig, lo, hi, family=None):
        genes.append((ident, NAMES.index(contig), lo, hi))
        if family:
            fam[ident] = family

    gene("A1", "chrA", 1001, 1001 + A_LEN - 1, "homeo")
    gene("B_inner", "chrA", 3100, 3391, "nest")          # nested in B_outer and first in the file: it owns its part
    gene("B_outer", "chrA", 2801, 3790, "nest")
    gene("F1", "chrA", 5000, 5777, "edges")
    gene("C1", "chrA", 7003, 7900, "over")
    gene("D1", "chrA", 7500, 8400, "other")              # overlaps C1: the cuts in [7500, 7900] are C1's
    gene("lonely", "chrA", 11000, 11500)                 # a gene in no family
    gene("A2", "chrB", 2010, 2010 + A_LEN - 1, "homeo")
    gene("D2", "chrB", 6001, 6650, "other")
    gene("S1", "chrB", 9017, 9097, "solo")               # (the cuts whose windows lie inside the copied piece)
    gene("A3", "chrD", 3333, 3333 + A_LEN - 1, "homeo")
    gene("E1", "rep", 990, 1000 + 4 * 151 + 13, "single")
    gene("G_first", "edge", 0, 301, "ends")
    gene("G_last", "edge", 2700, 2999, "ends")
    for n, (lo, hi) in zip(RUN_GUIDES, _run_genes(texts)):
        gene("R%d" % n, "runs", lo, hi, "runs")
    gene("H0", "spare", 100, 900, "runs")                # no guide site
    gene("H1", "spare", 1400, 1600, "runs")              # one guide site
    for j in range(TINY):
        gene("T%d" % j, "tiny", 50 + 40 * j, 50 + 40 * j + 30, "tiny" if j < 64 else None)
    gff = ["##gff-version 3"]
    for ident, k, lo, hi in genes:
        gff.append("%s\ttest\tgene\t%d\t%d\t.\t+\t.\tID=%s" % (NAMES[k], lo + 1, hi + 1, ident))
    unknown = ["ghost1", "ghost2"]
    lines = ["# gene\tfamily", ""] + ["%s\t%s" % kv for kv in fam.items()] + ["ghost1\thomeo", "ghost2\tnowhere", "A1\thomeo"]
    too_many = ["T%d\ttiny" % j for j in range(TINY)]
    return dict(contigs=texts, names=list(NAMES), gff="\n".join(gff) + "\n", families="\n".join(lines) + "\n",
                too_many="\n".join(too_many) + "\n", genes=genes, family_of=fam, unknown=unknown)
