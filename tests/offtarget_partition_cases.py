"""Genomes and expected numbers for tests/test_offtarget_partition.py: the off-target seed scan (crp_offtarget.hip) on
inputs whose row counts, site counts and seed distributions are PRESCRIBED instead of drawn from a uniform genome.

Planted genomes.  The background is random over ATat: bases, but no PAM.  A site with a prescribed seed is one plant
(tests/test_sparse_genomes.py::_no_site_genome does the same):
  AGGA at p   one '+' row at p; its 12 seed letters are p - 12 .. p - 1 (seed character k, k = 0 next to the PAM, is
              the COMPLEMENT of the letter at p - 1 - k: `sequence` is the reverse complement of the protospacer)
  TCCT at p   one '-' row at p + 1; its seed letters are p + 4 .. p + 15 (seed character k is the letter at p + 4 + k)
Codes are the header's: A=0 T=1 C=2 G=3, character k at bits 2k.  A seed is plantable iff it holds no GG and no CC (its
complement then holds none either), so a plant adds exactly one row.  An N among the seed letters keeps the row and
makes it a non-site.  A plant fills letters 2 .. 17 of its slot; slots are 40 letters apart.  Case B alone puts them 20
apart (16 letters of plant, 4 of background): its 2 * (2C + 5) rows would otherwise take 2.6 Mb, and no genome here is
longer than 1.7 Mb.

S = OT_STAGE and C = OT_CHUNK, the units of the partition, and OT_BUCKETS and BLOCK are read from the kernel sources
and asserted to be 8192 / 16384 / 4096 / 256: if they move, the cases below have to move with them.

This module does not load the GPU library.  Functions that need the CPU oracle take it as an argument.
"""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

NOT_A_SITE = 0xFFFFFFFF
NOT_OWNED = 0xFFFFFFFE
N_SEEDS = 1 << 24
SEED_LEN = 12
STRIDE = 40
LEAD = TAIL = 64
PAIRS_LIMIT = 40000  # the definition (all pairs) is the reference as well up to this many codes
BALL_SIZE = 6571     # seeds within distance 3 of a seed: 1 + 36 + 594 + 5940


def kernel_constants():
    """dict(stage, chunk, buckets, block) from crp_offtarget.hip and crp_kernels.h"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cropsr_amd", "csrc")
    with open(os.path.join(src, "crp_offtarget.hip")) as f:
        ot = f.read()
    with open(os.path.join(src, "crp_kernels.h")) as f:
        kh = f.read()
    find = lambda pattern, text: int(re.search(pattern, text).group(1))
    return dict(stage=find(r"constexpr uint32_t OT_STAGE = (\d+);", ot), chunk=find(r"#define CRP_OT_CHUNK (\d+)", ot),
                buckets=find(r"constexpr uint32_t OT_BUCKETS = (\d+);", ot), block=find(r"constexpr int BLOCK = (\d+);", kh))


_K = kernel_constants()
assert _K == dict(stage=8192, chunk=16384, buckets=4096, block=256), _K
S, C, BUCKETS, BLOCK = _K["stage"], _K["chunk"], _K["buckets"], _K["block"]

# ---- seeds and letters
_SEQ = np.frombuffer(b"ATCG", dtype=np.uint8)   # the letter of a code digit in `sequence`
_COMP = np.frombuffer(b"TAGC", dtype=np.uint8)  # its complement: what a '+' row's protospacer holds in the genome


def _digits(codes):
    """(n, 12) code digits, column k = seed character k"""
    codes = np.asarray(codes, dtype=np.uint32).reshape(-1)
    return (codes[:, None] >> (2 * np.arange(SEED_LEN, dtype=np.uint32))) & 3


def _genome_letters(codes, minus):
    """(n, 12) letters in GENOME order: p - 12 .. p - 1 of a '+' plant, p + 4 .. p + 15 of a '-' plant"""
    d = _digits(codes)
    return _SEQ[d] if minus else _COMP[d[:, ::-1]]


def letters_for(code, strand):
    """the 12 genome letters (bytes, ascending genome position) that give the row of a `strand` plant the seed `code`"""
    assert strand in ("+", "-") and 0 <= code < N_SEEDS
    return _genome_letters([code], strand == "-")[0].tobytes()


def plantable_mask(codes):
    d = _digits(codes)
    return ~((d[:, :-1] == d[:, 1:]) & (d[:, :-1] >= 2)).any(axis=1)


def plantable(code):
    """no GG and no CC among the 12 seed letters: the plant adds one row and no other"""
    return bool(plantable_mask([code])[0])


def seed_distance(a, b):
    return sum(((a ^ b) >> (2 * k)) & 3 != 0 for k in range(SEED_LEN))


def random_plantable(rng, n):
    out = np.empty(0, dtype=np.uint32)
    while out.size < n:
        c = rng.integers(0, N_SEEDS, 2 * n + 16, dtype=np.uint32)
        out = np.concatenate([out, c[plantable_mask(c)]])
    return out[:n]


def code_of(digits):
    return sum(int(d) << (2 * k) for k, d in enumerate(digits))


PLANTABLE_12 = np.flatnonzero(plantable_mask(np.arange(4096))).astype(np.uint32)  # plantable strings of 6 characters
LOWS = PLANTABLE_12[(PLANTABLE_12 >> 10) < 2]  # ... whose last character is A or T: any plantable bucket may follow them
LOWEST, HIGHEST = 0, code_of([2, 3] * 6)  # A x 12; G C G C ... from character 11 down (the CPU tests check that none is higher)


# ---- genomes
class Case:
    """contigs: bytes per contig; l: guide length; plan_plus / plan_minus: the planted code of every row in table order
    (contig after contig, ascending position; NOT_A_SITE where the plant carries an N); at_plus / at_minus: (contig,
    position in the contig) of those rows; max_words: arena size that spreads the contigs over three arenas"""

    def __init__(self, name, strands, codes, n_at=None, seed=0, stride=STRIDE, n_contigs=1, l=20):
        rng = np.random.default_rng(seed)
        strands = np.asarray(strands, dtype=np.uint8)
        codes = np.asarray(codes, dtype=np.uint32)
        n_at = np.full(strands.size, -1, dtype=np.int64) if n_at is None else np.asarray(n_at, dtype=np.int64)
        assert strands.shape == codes.shape == n_at.shape and plantable_mask(codes).all() and stride >= 20
        self.name, self.l, self.stride = name, l, stride
        self.contigs, plan, at = [], ([], []), ([], [])
        cuts = [strands.size * k // n_contigs for k in range(n_contigs + 1)]
        for k in range(n_contigs):
            sl = slice(cuts[k], cuts[k + 1])
            text, pos = _contig(rng, strands[sl], codes[sl], n_at[sl], stride, k == n_contigs - 1)
            self.contigs.append(text)
            for s in (0, 1):
                pick = strands[sl] == s
                plan[s].append(np.where(n_at[sl][pick] >= 0, np.uint32(NOT_A_SITE), codes[sl][pick]))
                at[s].append(np.stack([np.full(int(pick.sum()), k, dtype=np.int64), pos[pick]], axis=1))
        self.plan_plus, self.plan_minus = (np.concatenate(p).astype(np.uint32) for p in plan)
        self.at_plus, self.at_minus = (np.concatenate(a) for a in at)
        self.n_chars = sum(len(c) for c in self.contigs)
        assert self.n_chars <= 1_700_000, (name, self.n_chars)
        words = [(len(c) + 63) // 64 + 1 for c in self.contigs]  # a contig starts on a word boundary, one separator word behind it
        self.max_words = 2 + max(sum(words[i] for i in g) for g in _thirds(n_contigs)) if n_contigs >= 3 else None
        self._rows, self._expected = {}, {}

    def rows(self, oracle, l=None):
        """the ORACLE's rows: dict(pos_plus, pos_minus: per contig; seed_plus, seed_minus: one array per strand, in table order)"""
        l = self.l if l is None else l
        if l not in self._rows:
            pp, pm, sp, sm = [], [], [], []
            for c in self.contigs:
                plus, minus = oracle.scan(c, l)
                pp.append(plus)
                pm.append(minus)
                sp.append(oracle.seed_codes(c, plus, False, l))
                sm.append(oracle.seed_codes(c, minus, True, l))
            self._rows[l] = dict(pos_plus=pp, pos_minus=pm, seed_plus=np.concatenate(sp), seed_minus=np.concatenate(sm))
        return self._rows[l]

    def expected(self, oracle, l=None):
        """reference() of the oracle's own seeds (computed once, shared, read-only)"""
        l = self.l if l is None else l
        if l not in self._expected:
            r = self.rows(oracle, l)
            self._expected[l] = reference(oracle, r["seed_plus"], r["seed_minus"])
        return self._expected[l]


def _thirds(n):
    return [list(range(n * k // 3, n * (k + 1) // 3)) for k in range(3)]


def _contig(rng, strands, codes, n_at, stride, last):
    n = strands.size
    a = rng.choice(np.frombuffer(b"ATat", dtype=np.uint8), LEAD + n * stride + TAIL)
    base = LEAD + stride * np.arange(n, dtype=np.int64)
    plus = strands == 0
    b = base[plus]
    a[b[:, None] + 2 + np.arange(12)] = _genome_letters(codes[plus], False)
    a[b[:, None] + 14 + np.arange(4)] = np.frombuffer(b"AGGA", dtype=np.uint8)
    b = base[~plus]
    a[b[:, None] + 2 + np.arange(4)] = np.frombuffer(b"TCCT", dtype=np.uint8)
    a[b[:, None] + 6 + np.arange(12)] = _genome_letters(codes[~plus], True)
    holed = n_at >= 0
    assert (n_at < SEED_LEN).all()
    a[base[holed] + np.where(plus[holed], 2, 6) + n_at[holed]] = ord("N")
    a[0] = ord("'")
    a[-3:] = np.frombuffer(b"')]" if last else b"'),", dtype=np.uint8)
    return a.tobytes(), np.where(plus, base + 14, base + 3)


def _shuffled_strands(rng, n_plus, n_minus):
    s = np.concatenate([np.zeros(n_plus, dtype=np.uint8), np.ones(n_minus, dtype=np.uint8)])
    rng.shuffle(s)
    return s


# ---- the reference
def _enum(oracle, codes, hist, threads=8):
    """oracle.offtarget_enum of every code, evaluated once per DISTINCT code (the counts of a site are a function of its
    seed and the histogram) on a few threads"""
    codes = np.ascontiguousarray(codes, dtype=np.uint32)
    uniq, inverse = np.unique(codes, return_inverse=True)
    parts = np.array_split(uniq, max(1, min(4 * threads, uniq.size // 256)))
    with ThreadPoolExecutor(threads) as pool:
        table = np.concatenate(list(pool.map(lambda c: oracle.offtarget_enum(c, hist), parts)))
    return table[inverse.reshape(-1)]


def reference(oracle, seed_plus, seed_minus, hist=None):
    """dict(sites, hist, ot_plus, ot_minus) for the seed columns given (NOT_A_SITE / NOT_OWNED rows are no sites): the
    histogram of the sites (or `hist`, an arbitrary one), offtarget_enum of every row against it and, up to PAIRS_LIMIT
    codes and with the sites' own histogram, the definition (offtarget_pairs) as well: the two have to agree."""
    n_plus = seed_plus.size
    codes = np.concatenate([seed_plus, seed_minus]).astype(np.uint32)
    codes[codes == NOT_OWNED] = NOT_A_SITE  # (the oracle knows one kind of non-site)
    own_hist = hist is None
    if own_hist:
        hist = oracle.offtarget_hist([codes])
    counts = _enum(oracle, codes, hist)
    if own_hist and codes.size <= PAIRS_LIMIT:
        assert (oracle.offtarget_pairs(codes) == counts).all()
    return dict(sites=int((codes != NOT_A_SITE).sum()), hist=hist, ot_plus=counts[:n_plus], ot_minus=counts[n_plus:])


_BUILT = {}


def _once(key, make):
    if key not in _BUILT:
        _BUILT[key] = make()
    return _BUILT[key]


# ---- A. row counts on the edges of the partition units, every row a site
# (the last one mirrors (C + 2, 3): without it no '-' table has 2 rows over a multiple of 4)
EDGE_ROWS = [(S - 1, S + 1), (S, C), (C - 1, C + 1), (C + 2, 3), (2 * C + S + 3, 1), (0, C + 1), (5, 0), (3, C + 2)]
LARGEST = (2 * C + S + 3, 1)
PROBE = (C - 1, C + 1)  # case E's probe arena


def edge_rows(n_plus, n_minus):
    def make():
        rng = np.random.default_rng(1000 + 7 * n_plus + n_minus)
        return Case("rows_%d_%d" % (n_plus, n_minus), _shuffled_strands(rng, n_plus, n_minus), random_plantable(rng, n_plus + n_minus),
                    seed=n_plus + 3 * n_minus)
    return _once(("A", n_plus, n_minus), make)


# ---- B. site counts on the edges, fewer sites than rows
SITE_ROWS = 2 * C + 5
SITE_COUNTS = [1, 3, S, C - 1, C, C + 1]
OWNED_SITE_COUNTS = [C, C + 1]


def edge_sites(m):
    """SITE_ROWS rows on each strand, m of them sites, the others with an N among their seed letters, scattered"""
    def make():
        rng = np.random.default_rng(2000 + m)
        strands = np.tile(np.array([0, 1], dtype=np.uint8), SITE_ROWS)  # '+' and '-' plants take turns
        n_at = rng.integers(0, SEED_LEN, strands.size)
        for s in (0, 1):
            keep = rng.choice(SITE_ROWS, m, replace=False)
            n_at[2 * keep + s] = -1
        return Case("sites_%d" % m, strands, random_plantable(rng, strands.size), n_at, seed=m, stride=20)
    return _once(("B", m), make)


def edge_sites_owned(m):
    """(case, ranges): SITE_ROWS rows on each strand, all of them sites; five ranges (positions in the contig) own m of
    each strand -- stretches of whole ('+', '-') slot pairs, cut out of the table's beginning, middle and end"""
    def make():
        rng = np.random.default_rng(2500 + m)
        strands = np.tile(np.array([0, 1], dtype=np.uint8), SITE_ROWS)
        case = Case("owned_sites_%d" % m, strands, random_plantable(rng, strands.size), seed=50 + m, stride=20)
        rest = SITE_ROWS - m
        pairs = [1, m // 3, 7, m // 2, m - 1 - m // 3 - 7 - m // 2]                # slot pairs per range ...
        gaps = [0, rest // 4, 3, rest // 2, rest - rest // 4 - 3 - rest // 2]      # ... and unowned ones in front of it
        ranges, at = [], 0
        for gap, n in zip(gaps, pairs):
            at += gap
            ranges.append((LEAD + 40 * at, LEAD + 40 * (at + n)))  # a pair of slots is 40 letters
            at += n
        assert at == SITE_ROWS and sum(pairs) == m and min(pairs) > 0
        return case, np.array(ranges, dtype=np.int64)
    return _once(("B_owned", m), make)


# ---- C. skewed seed distributions
ONE_SEED = int(PLANTABLE_12[1500]) << 12 | int(LOWS[300])
ONE_SEED_ROWS = (C + S + 5, S + 1)
TWO_SEED_ROWS = (S + 2, S + 7)
LADDER_BUCKETS = 324
LADDER_MINUS_SHIFT = 5


def one_seed():
    def make():
        assert plantable(ONE_SEED)
        rng = np.random.default_rng(31)
        strands = _shuffled_strands(rng, *ONE_SEED_ROWS)
        return Case("one_seed", strands, np.full(strands.size, ONE_SEED, dtype=np.uint32), seed=31)
    return _once("C1", make)


def two_seeds():
    def make():
        rng = np.random.default_rng(32)
        strands = _shuffled_strands(rng, *TWO_SEED_ROWS)
        codes = np.where(rng.random(strands.size) < 0.7, np.uint32(LOWEST), np.uint32(HIGHEST))
        return Case("two_seeds", strands, codes, seed=32)
    return _once("C2", make)


def ladder_plan():
    """(buckets, counts_plus, counts_minus): LADDER_BUCKETS plantable buckets in ascending order, every sixth of the
    plantable ones; bucket j holds j % 18 entries on '+' and (j + LADDER_MINUS_SHIFT) % 18 on '-'"""
    buckets = PLANTABLE_12[1::6][:LADDER_BUCKETS]
    assert buckets.size == LADDER_BUCKETS and (np.diff(buckets.astype(np.int64)) > 1).any()
    j = np.arange(LADDER_BUCKETS)
    return buckets, j % 18, (j + LADDER_MINUS_SHIFT) % 18


def ladder(n_contigs=6):
    """the ladder_plan() as a genome; inside a bucket the low 12 bits take up to five values, each twice in a row"""
    def make():
        rng = np.random.default_rng(33)
        buckets, cp, cm = ladder_plan()
        strands, codes = [], []
        for s, cnt in ((0, cp), (1, cm)):
            for j, (b, n) in enumerate(zip(buckets.tolist(), cnt.tolist())):
                for i in range(n):
                    strands.append(s)
                    codes.append(b << 12 | int(LOWS[(37 * j + (i // 2) % 5 + 101 * s) % LOWS.size]))
        order = rng.permutation(len(codes))  # table order has nothing to do with bucket order
        return Case("ladder", np.array(strands, dtype=np.uint8)[order], np.array(codes, dtype=np.uint32)[order], seed=33, n_contigs=n_contigs)
    return _once(("C3", n_contigs), make)


# ---- D. Hamming families
PRIMES = [7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97]
CENTRE_COPIES = 5000
CHANGED = [(1,), (5,), (10,),                                                   # one position, in each pass
           (0, 2), (4, 7), (9, 11), (3, 4), (7, 8), (0, 11),                    # two: inside a pass, across two
           (1, 2, 3), (4, 5, 6), (8, 10, 11), (3, 4, 8), (0, 5, 11),            # three
           (0, 1, 2, 3), (4, 5, 6, 7), (8, 9, 10, 11), (2, 5, 7, 9)]            # four: never counted
CENTRES = [code_of([0, 1] * 3 + [0] * 6), code_of([1, 3, 1, 2, 1, 3, 1, 3, 1, 2, 1, 3])]  # in bucket 0; 12 characters away


def family_plan():
    """[(centre, [(neighbour, changed positions, multiplicity)])] for the two centres"""
    out = []
    for f, centre in enumerate(CENTRES):
        members, taken = [], {centre}
        for j, where in enumerate(CHANGED):
            for trial in range(3 ** len(where)):
                x = centre
                for i, k in enumerate(where):
                    x ^= (1 + (trial // 3 ** i + j + i) % 3) << (2 * k)
                if plantable(x) and x not in taken:
                    break
            else:
                raise AssertionError((centre, where))
            taken.add(x)
            members.append((x, where, PRIMES[(j + 4 * f) % len(PRIMES)]))
        out.append((centre, members))
    return out


def family_counts(multiplicity):
    """{code: [c0, c1, c2, c3]} from {code: copies}, by comparing the seeds character by character"""
    out = {}
    for a in multiplicity:
        c = [0, 0, 0, 0]
        for b, copies in multiplicity.items():
            d = seed_distance(a, b)
            if d <= 3:
                c[d] += copies
        c[0] -= 1
        out[a] = c
    return out


def family_multiplicity():
    mult = {}
    for centre, members in family_plan():
        mult[centre] = CENTRE_COPIES
        for x, _, copies in members:
            mult[x] = copies
    return mult


def families():
    def make():
        rng = np.random.default_rng(41)
        codes = np.concatenate([np.full(n, c, dtype=np.uint32) for c, n in family_multiplicity().items()])
        rng.shuffle(codes)
        assert codes.size <= PAIRS_LIMIT
        return Case("families", (rng.random(codes.size) < 0.4).astype(np.uint8), codes, seed=41)
    return _once("D", make)


# ---- E. an arbitrary histogram
HOT_ENTRIES, HOT_VALUE, UNIFORM_BELOW = 10, 600_000, 256
assert BALL_SIZE * (UNIFORM_BELOW - 1) + HOT_ENTRIES * HOT_VALUE < 1 << 32  # no ball sum can wrap


def arbitrary_hist(probe_codes):
    """uniform over 0 .. 255 on all 4^12 seeds, at least 1 on every probe seed (a probe counts itself out of c0), and ten
    entries of 600 000: on probe seeds, at distance 1, 2, 3 and 4 of probe seeds and anywhere"""
    def make():
        rng = np.random.default_rng(51)
        h = rng.integers(0, UNIFORM_BELOW, N_SEEDS, dtype=np.uint32)
        probes = np.unique(probe_codes[probe_codes < N_SEEDS])
        h[probes] = np.maximum(h[probes], 1)
        hot = [int(probes[0]), int(probes[-1])]
        for d in (1, 2, 3, 4):
            x = int(probes[probes.size * d // 5])
            for k in rng.choice(SEED_LEN, d, replace=False).tolist():
                x ^= int(rng.integers(1, 4)) << (2 * k)
            hot.append(x)
        hot += [0, N_SEEDS - 1] + rng.integers(0, N_SEEDS, HOT_ENTRIES).tolist()
        hot = list(dict.fromkeys(hot))[:HOT_ENTRIES]
        h[hot] = HOT_VALUE
        assert int((h == HOT_VALUE).sum()) == HOT_ENTRIES and int(h[h != HOT_VALUE].max()) == UNIFORM_BELOW - 1
        return h
    return _once("E", make)


def probe_reference(oracle):
    """(case, its oracle rows, the histogram, reference() of the rows against that histogram)"""
    case = edge_rows(*PROBE)
    r = case.rows(oracle)
    h = arbitrary_hist(np.concatenate([r["seed_plus"], r["seed_minus"]]))
    return case, r, h, _once("E_reference", lambda: reference(oracle, r["seed_plus"], r["seed_minus"], hist=h))


# ---- F. ownership ranges
OWN_PLANTS = 3000


def owned_genome():
    def make():
        rng = np.random.default_rng(61)
        pool = random_plantable(rng, 50)
        near = []
        for c in pool.tolist():  # two seeds one character away from each, so that c1 depends on who is owned
            for k in rng.choice(SEED_LEN, 2, replace=False).tolist():
                x = c ^ (1 << (2 * k))  # A <-> T, C <-> G: G next to G only where c held C G or G C there
                if plantable(x):
                    near.append(x)
        pool = np.concatenate([pool, np.array(near, dtype=np.uint32)])
        strands = _shuffled_strands(rng, OWN_PLANTS, OWN_PLANTS)
        n_at = np.where(rng.random(strands.size) < 0.03, rng.integers(0, SEED_LEN, strands.size), -1)
        return Case("owned", strands, pool[rng.integers(0, pool.size, strands.size)], n_at, seed=61)
    return _once("F", make)


def ownership_sets(rows):
    """{name: (k, 2) ranges} over `rows`, the ascending positions of all rows of the contig (both strands)"""
    r = lambda k: int(rows[k])
    many = [(r(3 * i), r(3 * i + 3) if i % 5 == 0 and i < 1999 else r(3 * i + 2)) for i in range(2000)]
    sets = {
        "tight_1": [(r(1000), r(1000) + 1)],
        "end_begin_2": [(r(200) + 1, r(700)), (r(900), r(1500) + 1)],
        "adjacent_3": [(r(100), r(400)), (r(400), r(401)), (r(401), r(2500))],
        "empty_4": [(r(50), r(60)), (r(60), r(60)), (r(61), r(61)), (r(3000), r(3100))],
        "mixed_5": [(r(10), r(10) + 1), (r(20) + 1, r(30)), (r(30), r(40)), (r(45), r(45)), (r(5000), r(5990))],
        "many_2000": many,
        "empty_alone": [(r(3000), r(3000))],
    }
    return {k: np.array(v, dtype=np.int64) for k, v in sets.items()}


OWNERSHIP_SETS = ["tight_1", "end_begin_2", "adjacent_3", "empty_4", "mixed_5", "many_2000", "empty_alone"]
EDGE_KINDS = ["tight", "at_end", "at_begin", "at_joint", "at_empty", "before_first", "after_last"]


def owned_mask(pos, ranges):
    """the definition: p is owned iff begin <= p < end for one of the ranges"""
    p = np.asarray(pos, dtype=np.int64)[:, None]
    return ((p >= ranges[None, :, 0]) & (p < ranges[None, :, 1])).any(axis=1)


def edge_kinds(rows, ranges):
    """{kind: rows of it}: in a range [p, p + 1); exactly at the end of a range that holds something (and not owned); exactly
    at the begin of one; where one range ends and the next begins; at an empty range [p, p) (and not owned); before the
    first range; at or behind the last one's end"""
    rows = np.asarray(rows, dtype=np.int64)
    own = owned_mask(rows, ranges)
    b, e = ranges[:, 0], ranges[:, 1]
    full = e > b
    joint = np.concatenate([(e[:-1] == b[1:]) & full[:-1] & full[1:], [False]])
    return {"tight": int(np.isin(rows, b[e == b + 1]).sum()),
            "at_end": int((np.isin(rows, e[full]) & ~own).sum()),
            "at_begin": int((np.isin(rows, b[full]) & own).sum()),
            "at_joint": int((np.isin(rows, e[joint]) & own).sum()),
            "at_empty": int((np.isin(rows, b[~full]) & ~own).sum()),
            "before_first": int((rows < b[0]).sum()),
            "after_last": int((rows >= e[-1]).sum())}


def owned_columns(seeds, own):
    """the seed column with ownership applied: a site that is not owned reads NOT_OWNED, a non-site stays one"""
    return np.where(own | (seeds == NOT_A_SITE), seeds, np.uint32(NOT_OWNED)).astype(np.uint32)
