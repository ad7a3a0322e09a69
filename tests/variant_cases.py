"""Inputs of tests/test_variants.py, shared by its CPU and GPU tests: small genomes with planted variants, so that every rule
and edge of the variant counts (cropsr_amd/variants.py) is met -- the CPU tests check that on the reference's columns before
the GPU tests look at the device.

A case is dict(name, texts, l, S, variants): variants are (text index, s, e) in 0-based STRING indices of that text, closed
ends, e >= s - 1 (an insertion is (p, p - 1)).  arena(case) lays the texts out as an arena does (64-aligned, one separator
word between texts, the first at 64) and gives the kept positions and the variants in arena positions."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
BUCKET = 2048


def rand(rng, n):
    return rng.choice(ACGT, n).tobytes()


def kept(text, l):
    """The scan's keep-filter restated (CROPSR.py:419 / :430) in numpy: match indices of (?=.GG) and (?=CC.) that stay."""
    b = np.frombuffer(bytes(text), dtype=np.uint8)
    n = b.size
    if n < 3:
        return np.empty(0, np.uint32), np.empty(0, np.uint32)
    i = np.flatnonzero((b[1:n - 1] == ord("G")) & (b[2:n] == ord("G")) & (b[0:n - 2] != ord("\n")))
    j = np.flatnonzero((b[0:n - 2] == ord("C")) & (b[1:n - 1] == ord("C")) & (b[2:n] != ord("\n")))
    i = i[(i - l >= 5) & (i - l + 5 <= n + 10) & (i <= n + 10)]
    j = j[(j + 3 >= 5) & (j + 8 <= n + 10) & (j + 3 + l <= n + 10)]
    return i.astype(np.uint32), j.astype(np.uint32)


def offsets(texts):
    out, off = [], 64
    for t in texts:
        out.append(off)
        off += ((len(t) + 63) // 64 + 1) * 64
    return out


def arena(case):
    """dict(offsets, pos_plus, pos_minus (arena positions, uint32), intervals [(s, e)] distinct, in arena positions)."""
    offs = offsets(case["texts"])
    per = [kept(t, case["l"]) for t in case["texts"]]
    cat = lambda k: np.concatenate([p[k].astype(np.int64) + o for p, o in zip(per, offs)]).astype(np.uint32)
    iv = sorted(set((offs[t] + s, offs[t] + e) for t, s, e in case["variants"]))
    return dict(offsets=offs, pos_plus=cat(0), pos_minus=cat(1), intervals=iv)


def _windows(pos, minus, l, S):
    p = int(pos)
    if minus:
        return [(p, p + 2 + l), (p + 3, p + 2 + l), (p + 3, p + 2 + S), (p, p + 1)]
    return [(p - l, p + 2), (p - l, p - 1), (p - S, p - 1), (p + 1, p + 2)]


# ---------------------------------------------------------------------------------------------- the boundary sweep
SWEEP_L, SWEEP_S = 20, 12


def sweep_text():
    return rand(np.random.default_rng(4101), 4000)


def sweep_targets():
    """(i of a '+' hit, j of a '-' hit) of sweep_text(), each well inside the text and 600 letters from the other."""
    plus, minus = kept(sweep_text(), SWEEP_L)
    i = int(plus[np.searchsorted(plus, 1200)])
    j = int(minus[np.searchsorted(minus, 2400)])
    return i, j


def sweep_variants():
    """[(what, strand, (s, e))] in string indices of sweep_text(): for the '+' target and the '-' target one SNP at a - 1, a,
    b, b + 1 of each window, one insertion at every junction from a - 1 | a to b | b + 1 of the site, a deletion that starts
    before the site and ends inside it, one that covers it whole, and one inside the PAM's N."""
    out = []
    for strand, pos in zip("+-", sweep_targets()):
        minus = strand == "-"
        names = ("site", "guide", "seed", "pam")
        for name, (a, b) in zip(names, _windows(pos, minus, SWEEP_L, SWEEP_S)):
            for tag, x in (("a-1", a - 1), ("a", a), ("b", b), ("b+1", b + 1)):
                out.append(("snp %s %s" % (name, tag), strand, (x, x)))
        a, b = _windows(pos, minus, SWEEP_L, SWEEP_S)[0]
        for p in range(a, b + 2):  # the junction p - 1 | p
            out.append(("ins %d" % (p - a), strand, (p, p - 1)))
        out.append(("del into", strand, (a - 7, a + 4)))
        out.append(("del over", strand, (a - 3, b + 3)))
        n_at = pos + 2 if minus else pos  # the PAM's N: the '.' of .GG at i, of CC. at j + 2
        out.append(("del N", strand, (n_at, n_at)))
    return out


def sweep_cases():
    """One case per planted variant, and one with all of them."""
    text = sweep_text()
    singles = [dict(name="sweep %s %s" % (strand, what), texts=[text], l=SWEEP_L, S=SWEEP_S, variants=[(0, s, e)], strand=strand, what=what)
               for what, strand, (s, e) in sweep_variants()]
    together = dict(name="sweep all", texts=[text], l=SWEEP_L, S=SWEEP_S, variants=[(0, s, e) for _, _, (s, e) in sweep_variants()])
    return singles, together


# ---------------------------------------------------------------------------------------------- bucket edges
def bucket_edges_case():
    """Hits and variants at arena positions 2047, 2048, 2049 ('+') and 4095, 4096, 4097 ('-'); sites that straddle a bucket
    border; intervals whose start and end lie in different buckets; an insertion on the border itself."""
    text = bytearray(rand(np.random.default_rng(4102), 6000))
    at = lambda arena_pos: arena_pos - 64
    text[at(2048):at(2048) + 4] = b"GGGG"   # .GG at 2047, 2048, 2049
    text[at(4095):at(4095) + 4] = b"CCCC"   # CC. at 4095, 4096, 4097
    v = [(0, at(p), at(p)) for p in (2047, 2048, 2049, 4095, 4096, 4097)]
    v += [(0, at(2040), at(2060)), (0, at(4090), at(4100)), (0, at(2048), at(2047)), (0, at(4096), at(4095)), (0, at(2030), at(2047)),
          (0, at(2048), at(2055)), (0, at(4000), at(4096))]
    return dict(name="bucket edges", texts=[bytes(text)], l=20, S=12, variants=v)


# ---------------------------------------------------------------------------------------------- bucket fill
FILL_BUCKET = 3  # arena positions 6144 .. 8191


def bucket_fill_case():
    """One bucket with more than 5 000 distinct intervals (overlapping deletions), empty buckets on both sides: 255 intervals
    under the seed of one '+' hit, 256 under the seed of another, and 5 000 more away from both (counts far above 255)."""
    text = rand(np.random.default_rng(4103), 12000)
    base = FILL_BUCKET * BUCKET - 64  # string index of the bucket's first position
    plus, _ = kept(text, 20)
    h1 = int(plus[np.searchsorted(plus, base + 300)])
    h2 = int(plus[np.searchsorted(plus, base + 700)])
    v = []
    for h, n in ((h1, 255), (h2, 256)):
        p = h - 5  # inside the seed
        combos = [(p - k, p + m) for k in range(16) for m in range(16)]
        v += [(0, s, e) for s, e in combos[:n]]
    v += [(0, base + 1000 + s, base + 1000 + s + d) for s in range(250) for d in range(20)]
    return dict(name="bucket fill", texts=[text], l=20, S=12, variants=v, rows_255_256=(h1, h2))


# ---------------------------------------------------------------------------------------------- extremes
LENGTHS = [(1, 1), (20, 1), (20, 12), (20, 20), (50, 1), (50, 12), (50, 50)]


def extreme_texts():
    rng = np.random.default_rng(4104)
    a = rand(rng, 3000) + b"CCT" + b"A" * 10   # a '-' row whose window runs 10 letters past the end (l = 20)
    b = rand(rng, 2500) + b"TGG"                # a '+' row in the last word of the last text
    return [a, b]


def extreme_cases():
    texts = extreme_texts()
    rng = np.random.default_rng(4105)
    out = [dict(name="empty track", texts=texts, l=20, S=12, variants=[]),
           dict(name="all before the first hit", texts=texts, l=20, S=12, variants=[(0, 0, 0), (0, 1, 1), (0, 0, 1)]),
           # (a text of A's has no hit: everything in it lies behind the last row)
           dict(name="all after the last hit", texts=texts + [b"A" * 300], l=20, S=12, variants=[(2, 10, 10), (2, 50, 80), (2, 299, 299)])]
    n0, n1 = len(texts[0]), len(texts[1])
    ends = [(0, n0 - 1, n0 - 1), (0, n0 - 11, n0 - 10), (0, n0 - 4, n0 - 5), (1, n1 - 1, n1 - 1), (1, n1 - 3, n1 - 3), (1, n1 - 2, n1 - 3),
            (1, n1 - 30, n1 - 1), (1, n1, n1 - 1)]
    for l, S in LENGTHS:
        v = list(ends)
        for t, n in ((0, n0), (1, n1)):
            for s in rng.integers(0, n - 40, 150).tolist():
                kind = int(rng.integers(0, 3))
                v.append((t, s, s) if kind == 0 else (t, s, s - 1) if kind == 1 else (t, s, s + int(rng.integers(1, 30))))
        out.append(dict(name="ends l=%d S=%d" % (l, S), texts=texts, l=l, S=S, variants=v))
    return out


# ---------------------------------------------------------------------------------------------- several contigs and arenas, through a VCF
VCF_NAMES = ["chrA", "chrB", "scaffold_3", "chrD"]


def vcf_case(dec):
    """Four contigs (dec = 1: in the re-formatted path's decoration, one character before the first base) and VCF bytes whose
    records name them, a CHROM no contig names among them; REF is the genome's own letters at POS, which the test checks
    against the texts.  Returns dict(texts, names, dec, vcf, l, S)."""
    rng = np.random.default_rng(4106 + dec)
    seqs = [rand(rng, n) for n in (5000, 900, 7000, 3100)]
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    other = {ord("A"): "C", ord("C"): "G", ord("G"): "T", ord("T"): "A"}
    for name, seq in zip(VCF_NAMES, seqs):
        at = np.unique(rng.integers(1, len(seq) - 40, len(seq) // 60))
        for c in at.tolist():  # 1-based coordinate
            kind = int(rng.integers(0, 4))
            ref1 = chr(seq[c - 1])
            if kind == 0:
                ref, alt = ref1, other[seq[c - 1]]
            elif kind == 1:
                ref, alt = ref1, ref1 + "ACG"[:int(rng.integers(1, 4))]
            elif kind == 2:
                ref, alt = seq[c - 1:c + int(rng.integers(1, 25))].decode(), ref1
            else:
                ref, alt = ref1, other[seq[c - 1]] + "," + other[ord(other[seq[c - 1]])]  # multi-allelic SNP: one variant
            lines.append("%s\t%d\t.\t%s\t%s\t50\tPASS\t." % (name, c, ref, alt))
        lines.append("%s\t1\t.\t%s\t%s\t50\tPASS\t." % (name, chr(seq[0]), other[seq[0]]))                       # the first base
        lines.append("%s\t%d\t.\t%s\t%s\t50\tPASS\t." % (name, len(seq), chr(seq[-1]), other[seq[-1]]))           # the last base
        lines.append("%s\t%d\t.\t%s\t%s\t50\tPASS\t." % (name, len(seq) - 2, seq[-3:].decode() + "AC", chr(seq[-3])))  # REF runs past the end
    lines.append("nowhere\t100\t.\tA\tG\t50\tPASS\t.")
    texts = [b"'" + s + b"')," for s in seqs] if dec else list(seqs)
    return dict(texts=texts, seqs=seqs, names=list(VCF_NAMES), dec=dec, vcf=("\n".join(lines) + "\n").encode(), l=20, S=12)


# ---------------------------------------------------------------------------------------------- the random case
def random_genome():
    """The 2.4 Mb genome of tests/test_specificity_join.py's two-hundred-thousand-hit test (the same seed)."""
    rng = np.random.default_rng(78)
    first = rng.choice(ACGT, 1_200_000)
    second = first.copy()
    at = np.nonzero(rng.random(second.size) < 0.03)[0]
    second[at] = rng.choice(ACGT, at.size)
    n_run = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), 30_001)
    return [first.tobytes(), second.tobytes(), n_run.tobytes()]


def random_case():
    """3 x 10^4 seeded variants of all kinds over the 2.4 Mb genome: 45 % SNPs, 15 % insertions, 40 % deletions of 1..400
    letters (long ones, so that intervals span buckets and fewer than half of the rows stay untouched)."""
    texts = random_genome()
    rng = np.random.default_rng(4107)
    sizes = np.array([len(t) for t in texts])
    t = rng.choice(3, 30_000, p=sizes / sizes.sum())
    s = (rng.random(30_000) * (sizes[t] - 401)).astype(np.int64)
    u = rng.random(30_000)
    length = rng.integers(1, 401, 30_000)
    e = np.where(u < 0.45, s, np.where(u < 0.60, s - 1, s + length - 1))
    return dict(name="random", texts=texts, l=20, S=12, variants=list(zip(t.tolist(), s.tolist(), e.tolist())))
