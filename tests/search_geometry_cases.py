"""The case table and the planted genomes of tests/test_search_geometry.py: pattern geometries at the limits of the
off-target search (T = 32, T = 31, tiny guide regions, a PAM on either side, no PAM at all).

Random sequence gives no hit at G = 28..31, so every case's genome carries, per query, copies of the query on both
strands with mismatches at the first and the last compared position, non-bases there, and copies at the starts where the
device's extraction changes word or workgroup.  The PAM's length is part of the case: nothing here guesses it."""
import numpy as np

import search_pair_reference as pref
import search_reference as ref
import search_score_reference as sref
import search_self_reference as selfref

WORD = 64             # characters per plane word
GROUP = 256 * WORD    # characters one workgroup of the extraction covers
# 76 letters, 3 of them no base (U reads as A): a 29-letter window of it is all bases three times in ten
ALPHA = np.frombuffer(b"ACGT" * 12 + b"acgt" * 6 + b"NRYU", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


class Case:
    """One row of the table.  pam_len None: no guide region (a plain search only); then every position of a query may
    hold a base and `gpos` is all of them."""

    def __init__(self, cid, pattern, pam_len=None, alpha=ALPHA):
        self.id, self.pattern, self.P, self.T, self.alpha = cid, pattern, pam_len, len(pattern), alpha
        T, P = self.T, pam_len
        if P is None:
            self.pam3, self.gpos = None, list(range(T))
        elif set(pattern[:T - P]) <= {"N"}:
            self.pam3, self.gpos = True, list(range(T - P))
        else:
            assert set(pattern[P:]) <= {"N"}
            self.pam3, self.gpos = False, list(range(T - 1, P - 1, -1))
        self.G = len(self.gpos)  # (g = 0 is gpos[0], the PAM-distal end)

    def __repr__(self):
        return self.id


def _rich(letters):
    return np.frombuffer(letters * 10 + b"ACGT" * 4 + b"acgt" * 2 + b"NRYU", dtype=np.uint8)


L3 = Case("L3", "N" * 29 + "NGG", 3)
L5 = Case("L5", "TTTV" + "N" * 28, 4)
W3 = Case("W3", "N" * 31 + "G", 1)
W5 = Case("W5", "G" + "N" * 30, 1)
S5 = Case("S5", "NNNGG", 2, _rich(b"GGC"))     # rich in GG and CC: a quarter of its positions are candidates
S5P = Case("S5'", "TTNNN", 2, _rich(b"TTA"))
S3 = Case("S3", "NGG", 2)
S2 = Case("S2", "NG", 1)
S1G = Case("S1-G", "G")
S1N = Case("S1-N", "N")
A32 = Case("A32", "N" * 32)
E32 = Case("E32", "R" + "N" * 30 + "Y")
ALL = [L3, L5, W3, W5, S5, S5P, S3, S2, S1G, S1N, A32, E32]
SCORED = [L3, L5, W3, W5, S5, S5P]
# the PAM offsets of the pair-table runs: on the PAM's letters other than N
PAM_OFFSETS = {"L3": (1, 2), "L5": (3,), "W3": (0,), "W5": (0,), "S5": (0, 1), "S5'": (0, 1)}
# characters of the long contig: given-guides runs (past one workgroup of the extraction), self searches
CHARS = {"L3": 24_000, "L5": 24_000, "W3": 17_500, "W5": 17_500, "S5": 24_000, "S5'": 24_000, "S3": 20_000, "S2": 17_500,
         "S1-G": 17_000, "S1-N": 17_000, "A32": 17_500, "E32": 20_000}
SELF_CHARS = {"L3": 24_000, "L5": 24_000, "W3": 6_000, "W5": 6_000, "S5": 40_000, "S5'": 40_000, "S3": 20_000, "S2": 6_000}
# bulge cases: (case of the unbulged pattern, D, R)
B27 = Case("B27", "N" * 27 + "NGG", 3)
B26 = Case("B26", "TTTV" + "N" * 26, 4)
B28 = Case("B28", "N" * 28 + "NGG", 3)
BULGES = [(B27, 2, 2), (B26, 2, 2), (B28, 1, 2), (L3, 0, 2), (L5, 0, 2)]


def letters_of(c):
    return ref.IUPAC_SETS.get(c, "ACGT")


def make_queries(case, rng, n=3):
    """n queries of T letters.  With a PAM: guides in the guide region, N at the PAM positions, the last one (n >= 3,
    G >= 6) two letters short at the PAM-distal end.  Without: a letter of the pattern's set everywhere, the last one
    (n >= 2, T >= 3) with N at both ends."""
    out = []
    for k in range(n):
        q = ["N"] * case.T
        for p in case.gpos:
            q[p] = str(rng.choice(list(letters_of(case.pattern[p]))))
        if case.P is not None and k == n - 1 and n >= 3 and case.G >= 6:
            q[case.gpos[0]] = q[case.gpos[1]] = "N"
        if case.P is None and k == n - 1 and n >= 2 and case.T >= 3:
            q[0] = q[-1] = "N"
        out.append("".join(q))
    return list(dict.fromkeys(out))  # (a one-letter pattern has few queries to choose from)


def compared(case, query):
    """The pattern positions a query compares, in g order."""
    return [p for p in case.gpos if query[p] in "ACGT"]


def variants(case, query, rng, counts=(3, 4, 8)):
    """[(tag, oriented site)] of one query: an exact copy, one mismatch at the first compared g and one at the last, both,
    n mismatches including both (n of `counts`), and a non-base at either end.  A variant the pattern cannot hold (a
    substitution inside a one-letter set, a non-base under a PAM letter) is left out."""
    cmp_ = compared(case, query)
    base = [query[p] if query[p] in "ACGT" else str(rng.choice(list(letters_of(case.pattern[p])))) for p in range(case.T)]

    def made(tag, subs, non_base=()):
        site = list(base)
        for p in subs:
            other = [b for b in letters_of(case.pattern[p]) if b != site[p]]
            if not other:
                return []
            site[p] = str(rng.choice(other))
        for p in non_base:
            if case.pattern[p] != "N":
                return []
            site[p] = "N"
        return [(tag, "".join(site))]

    out = made("exact", [])
    if cmp_:
        first, last = cmp_[0], cmp_[-1]
        out += made("first", [first]) + made("last", [last]) + made("n-first", [], [first]) + made("n-last", [], [last])
        if len(cmp_) >= 2:
            out += made("ends", [first, last])
        for n in sorted(set(min(c, len(cmp_)) for c in counts)):
            if n >= 3:
                mid = [cmp_[int(i)] for i in rng.choice(np.arange(1, len(cmp_) - 1), n - 2, replace=False)]
                out += made("ends+%d" % (n - 2), [first, last] + mid)
    return out


def rc(site):
    return site.encode().translate(_COMP)[::-1].decode()


class _Contig:
    def __init__(self, rng, n, alpha):
        self.text = bytearray(rng.choice(alpha, n).tobytes())
        self.taken = []
        self.cursor = 0

    def put(self, at, s):
        assert 0 <= at and at + len(s) <= len(self.text), (at, len(s), len(self.text))
        assert all(at + len(s) <= a or b <= at for a, b in self.taken), "plants overlap"
        self.text[at:at + len(s)] = s.encode()
        self.taken.append((at, at + len(s)))

    def put_next(self, s):
        while any(self.cursor < b + 1 and a < self.cursor + len(s) + 1 for a, b in self.taken):
            self.cursor += 1
        self.put(self.cursor, s)
        self.cursor += len(s) + 1


def build_genome(case, queries, n_chars, rng, sites_of=None):
    """(contigs, plants).  Contig q holds query q's copies: every variant on both strands (every third copy in lower
    case), an exact copy at position 0, one at the last possible start, and a one-mismatch copy astride a word boundary.
    Contig 0 has n_chars characters (or what its copies need); where it is long enough it also holds query 0's copies
    astride the workgroup boundaries of the extraction (the arena's first word is taken, so a contig position of GROUP -
    WORD is an arena position of GROUP: both are planted).  Then come a contig of T - 1 characters, one of T / 2, and one
    with a run of N.  sites_of(query) -> [(tag, oriented window)] replaces `variants` (windows of any length).
    plants: [(query, tag, contig, position, strand)]."""
    T = case.T
    contigs, plants, n_put = [], [], 0
    for q, query in enumerate(queries):
        vs = sites_of(query) if sites_of else variants(case, query, rng)
        longest = max(len(s) for _, s in vs)
        need = 4 * WORD + (2 * len(vs) + 4) * (longest + 2)
        c = _Contig(rng, max(n_chars, need) if q == 0 else need, case.alpha)
        exact, one = vs[0][1], vs[min(1, len(vs) - 1)][1]
        special = [("at-0", 0, exact, 0), ("at-end", len(c.text) - len(exact), exact, 1), ("word", 3 * WORD - len(one) // 2, one, 0)]
        if q == 0:
            for b in range(GROUP, len(c.text), GROUP):
                for shift, strand in ((WORD, 0), (0, 1)):
                    at = b - shift - len(one) // 2
                    if at + len(one) <= len(c.text) - len(exact):
                        special.append(("group", at, one, strand))
        for tag, at, s, strand in special:
            c.put(at, rc(s) if strand else s)
            plants.append((q, tag, q, at, strand))
        c.cursor = WORD + 3
        for tag, s in vs:
            for strand in (0, 1):
                o = rc(s) if strand else s
                n_put += 1
                c.put_next(o.lower() if n_put % 3 == 0 else o)
                plants.append((q, tag, q, c.taken[-1][0], strand))
        contigs.append(bytes(c.text))
    contigs.append(rng.choice(case.alpha, T - 1).tobytes())
    contigs.append(rng.choice(case.alpha, T // 2).tobytes())
    contigs.append(rng.choice(case.alpha, 300).tobytes() + b"N" * 50 + b"n" * 20 + rng.choice(case.alpha, 300).tobytes())
    return contigs, plants


def rows_of(s, fields=ref.SITE_FIELDS):
    """A reference's site dictionary as a sorted list of tuples."""
    return sorted(zip(*[s[f].tolist() for f in fields]))


def straddles(start, length, offset, every):
    """Whether the window [start, start + length) of a contig at arena offset `offset` has a multiple of `every` inside."""
    a = start + offset
    return (a + length - 1) // every > a // every


def buckets(contigs, case):
    """[(candidates, guide sites)] per guide-region position and letter: the buckets of a self search whose segments are
    one letter long."""
    (k, pos, strand, O), g = selfref.guide_sites(contigs, case.pattern, case.P)
    return [(int((O[:, p] == c).sum()), int((O[g][:, p] == c).sum())) for p in sorted(case.gpos) for c in range(4)]


def self_reference(contigs, case, max_mm, weights=None):
    """search_self_reference.search_self, with the given-guides reference run once per distinct query: a guide region of
    3 letters has 64 of them among ten thousand guide sites.  The CPU tests hold the two against each other."""
    (k, pos, strand, O), g = selfref.guide_sites(contigs, case.pattern, case.P)
    queries = selfref.queries_of(O[g], case.pattern, case.P)
    distinct = list(dict.fromkeys(queries))
    if weights is None:
        counts, hit_sum = ref.search(contigs, case.pattern, distinct, max_mm)[0], None
    else:
        factor, shape = sref.tables(weights)
        counts, _, sums = sref.search(contigs, case.pattern, distinct, max_mm, case.P, factor, shape)
    row = {q: i for i, q in enumerate(distinct)}
    at = [row[q] for q in queries]
    counts = counts.astype(np.int64).reshape(len(distinct), max_mm + 1)[at]
    counts[:, 0] -= 1  # the site itself
    assert (counts >= 0).all()
    if weights is not None:
        hit_sum = [sums[i] for i in at]
    sites = list(zip(k[g].tolist(), pos[g].tolist(), strand[g].tolist()))
    return sites, selfref.guide_letters(queries, case.pattern, case.P), counts, hit_sum


def self_pair_reference(contigs, case, max_mm, pair, pam_offsets, pam):
    """The self search under a pair table: (sites, guides, counts (n, M + 1) int64, hit_sum [int]), rows in the order of
    search_self_reference.search_self.  Row s is the given-guides definition of s's own query with 1 taken off
    counts[0]; every value is search_pair_reference.value_loop's.  Equal windows are valued once and weighed by how often
    they occur, which is what lets a guide region of 3 letters, where every candidate is a hit, be summed at all."""
    (k, pos, strand, O), g = selfref.guide_sites(contigs, case.pattern, case.P)
    gpos = np.array(case.gpos, dtype=np.int64)
    classes, n_of = np.unique(O, axis=0, return_counts=True)
    strings = ["".join("ACGT?"[c] for c in row) for row in classes.tolist()]
    queries = selfref.queries_of(O[g], case.pattern, case.P)
    counts = np.zeros((len(queries), max_mm + 1), dtype=np.int64)
    hit_sum, done = [], {}
    for r, query in enumerate(queries):
        if query not in done:
            qc = np.array(["ACGTN".index(ch) for ch in query], dtype=np.uint8)
            mm = (classes[:, gpos] != qc[gpos][None, :]).sum(axis=1)
            sel = np.nonzero(mm <= max_mm)[0]
            c = np.bincount(mm[sel], weights=n_of[sel], minlength=max_mm + 1)[:max_mm + 1].astype(np.int64)
            total = sum(int(n_of[i]) * pref.value_loop(query, strings[i], case.pattern, case.P, pair, pam_offsets, pam)
                        for i in sel.tolist() if mm[i])
            done[query] = (c, total)
        counts[r], total = done[query]
        hit_sum.append(total)
    counts[:, 0] -= 1  # the site itself
    assert (counts >= 0).all()
    sites = list(zip(k[g].tolist(), pos[g].tolist(), strand[g].tolist()))
    return sites, selfref.guide_letters(queries, case.pattern, case.P), counts, hit_sum


def weights_for(case, rng):
    """G random weights of three decimals with an exact 0 and an exact 1 among them (both, from G = 2 on)."""
    w = np.round(rng.random(case.G), 3)
    w[case.G // 2] = 0.0
    if case.G >= 2:
        w[case.G - 2 if case.G >= 4 else 0] = 1.0
    return w.tolist()


def table_for(case, rng):
    """(pair, offsets, pam) of a scored case: search_pair_reference.random_table (G >= 3).  The PAM letters of these
    patterns are nearly all fixed, so few entries of pam can be met: one of them at least is not the table's exact 0."""
    offsets = PAM_OFFSETS[case.id]
    pair, pam = pref.random_table(rng, case.pattern, case.P, offsets)
    pam_at = case.T - case.P if case.pam3 else 0
    met = [0]
    for o in offsets:
        met = [4 * i + "ACGT".index(b) for i in met for b in letters_of(case.pattern[pam_at + o])]
    if not pam[met].any():
        pam[met[0]] = 0.625
    return pair, offsets, pam


def write_fasta(path, names, contigs, width=61):
    with open(path, "wb") as f:
        for n, c in zip(names, contigs):
            f.write(b">" + n.encode() + b" x\n")
            for i in range(0, len(c), width):
                f.write(c[i:i + width] + b"\n")
