"""The CSV join of the self search's rows onto the guide table's hits (cropsr_amd/search.py and DESIGN.md section 15, CSV
join, state the definition), in numpy, and the small genome the tests run it on.

    rows       the CPU references' self-search rows as a dict (contig, forward start, strand) -> (counts, hit_sum)
    join       per contig, the columns a scan's hits get from that dict: '+' hit i -> (k, i - l, 0), '-' hit j -> (k, j, 1);
               a hit without an entry gets all-ones
    join_fast  the same join for 10^5 hits, by searchsorted over the sorted site keys (checked against `join`)

genome() builds three contigs, some 6 kb, with planted copies of three guides on both strands and the edge cases the join
must get right; WHERE names their places."""
import numpy as np

import search_pair_reference as pref
import search_reference as ref
import search_score_reference as sref
import search_self_reference as selfref

L = 20
NO_COUNT, NO_SUM = 0xFFFFFFFF, (1 << 64) - 1
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(b):
    return bytes(b).translate(_COMP)[::-1]


def patterns(l, pam="NRG"):
    return "N" * l + pam, "N" * l + "NGG"


def _mut(g, at):
    g = bytearray(g)
    for p in at:
        g[p] = b"CGTA"[b"ACGT".index(g[p])]
    return bytes(g)


# places of the edge cases in genome(): (contig, local position)
WHERE = dict(
    plus_first_kept=(0, 25),       # '+' match index with i - l == 5
    plus_not_kept=(0, 24),         # i - l == 4: the reference drops it
    plus_straddles_word=(0, 147),  # site start 127: the window crosses a 64-position word
    plus_at_word_start=(0, 212),   # site start 192
    minus_before_word=(0, 447),    # '-' site start 63 mod 64
    minus_at_word_start=(0, 512),
    nag_copy=(1, 300),             # site start of a copy with a TAG PAM: a candidate only
    lower_gg_copy=(1, 400),        # site start of a copy with a Tgg PAM: a guide site of the search, no hit of the scan
    proper_copy=(1, 520),          # '+' match index of the same guide with TGG
    plus_n_in_guide=(1, 620),      # '+' match index, an N inside its guide
    minus_n_in_guide=(1, 700),     # '-' match index, an N inside its guide
)


def genome():
    """(contigs as bytes, the three planted guides)."""
    rng = np.random.default_rng(20261)
    acgt, at = np.frombuffer(b"ACGT", dtype=np.uint8), np.frombuffer(b"AT", dtype=np.uint8)
    contigs = [bytearray(rng.choice(acgt, n).tobytes()) for n in (3001, 2050, 977)]
    g0, g1, g2 = (rng.choice(acgt, L).tobytes() for _ in range(3))

    def put(k, where, seq):
        contigs[k][where:where + len(seq)] = seq

    c0, c1, c2 = contigs
    put(0, 0, rng.choice(at, 40).tobytes())
    put(0, 25, b"GGG")                       # .GG at 24 (start 4: not kept) and at 25 (start 5: the first kept)
    put(0, 127, g0 + b"TGG")
    put(0, 192, g0 + b"AGG")
    put(0, 300, revcomp(g0 + b"CGG"))
    put(0, 447, revcomp(g1 + b"TGG"))
    put(0, 512, revcomp(g1 + b"TGG"))
    put(0, 600, _mut(g0, [3]) + b"TGG")
    put(0, 700, _mut(g0, [3, 11, 17]) + b"CGG")
    put(0, 800, revcomp(_mut(g1, [0, 19]) + b"AGG"))
    put(0, 900, revcomp(_mut(g2, [5, 6, 7, 8]) + b"TGG"))
    n = len(c0)
    put(0, n - 40, rng.choice(at, 40).tobytes())
    put(0, n - 23, b"CCC")                   # CC. at n - 23 (its window ends with the contig) and at n - 22 (cut by 1)
    put(1, 100, g0 + b"TGG")
    put(1, 200, revcomp(_mut(g0, [0, 19]) + b"AGG"))
    put(1, 300, g1 + b"TAGT")
    put(1, 400, g1 + b"TggT")
    put(1, 500, g1 + b"TGG")
    put(1, 600, g2[:7] + b"N" + g2[8:] + b"TGG")
    put(1, 700, revcomp(g2 + b"TGG"))
    c1[708] = ord("N")
    put(1, 800, g2 + b"TGG")
    put(1, 900, _mut(g2, [10]) + b"GGG")
    n = len(c1)
    put(1, n - 40, rng.choice(at, 40).tobytes())
    put(1, n - 13, b"CC")                    # CC. at n - 13: the window is cut by 10, the reference still keeps the hit
    put(2, 50, g0 + b"TGG")
    put(2, 150, revcomp(g1 + b"TGG"))
    put(2, 250, revcomp(_mut(g2, [1]) + b"TGG"))
    put(2, 350, _mut(g1, [2, 9]) + b"CGG")
    return [bytes(c) for c in contigs], (g0, g1, g2)


def pair_table(l, seed=5):
    """(pair (l, 4, 4), PAM offsets, pam) for N * l + NRG: random, asymmetric, with exact 0 and 1 entries."""
    pattern, _ = patterns(l)
    pair, pam = pref.random_table(np.random.default_rng(900 + seed), pattern, 3, (1, 2))
    return pair, (1, 2), pam


def rows(contigs, l, max_mm, pam="NRG", score=None):
    """The self-search rows of the CPU references: {(contig, start, strand): (counts (M + 1,) int64, hit_sum int or None)}.
    score: None, "hsu2013", a list of l weights, or (pair, offsets, pam) of a pair table."""
    pattern, gp = patterns(l, pam)
    if isinstance(score, tuple):
        (k, pos, strand, O), g = selfref.guide_sites(contigs, pattern, 3, gp)
        queries = selfref.queries_of(O[g], pattern, 3)
        counts, _, hit_sum = pref.search(contigs, pattern, queries, max_mm, 3, *score)
        counts = counts.astype(np.int64).reshape(len(queries), max_mm + 1)
        counts[:, 0] -= 1  # the site itself (its value is 0: no mismatch)
        sites = list(zip(k[g].tolist(), pos[g].tolist(), strand[g].tolist()))
    else:
        w = sref.W_HSU if score == "hsu2013" else score
        sites, _, counts, hit_sum = selfref.search_self(contigs, pattern, max_mm, 3, gp, w)
    assert (counts >= 0).all() and len(set(sites)) == len(sites)
    return {s: (counts[i], None if hit_sum is None else int(hit_sum[i])) for i, s in enumerate(sites)}


def join(hits, table, l, max_mm):
    """Per contig (hits[k]: the scan's pos_plus / pos_minus, local match indices) the joined columns, as
    search.specificity_columns returns them."""
    out = []
    for k, h in enumerate(hits):
        cols = {}
        for name, strand, shift in (("plus", 0, -l), ("minus", 1, 0)):
            pos = np.asarray(h["pos_" + name]).astype(np.int64)
            counts = np.full((pos.size, max_mm + 1), NO_COUNT, dtype=np.uint32)
            sums = np.full(pos.size, NO_SUM, dtype=np.uint64)
            for r, p in enumerate(pos.tolist()):
                row = table.get((k, p + shift, strand))
                if row is not None:
                    counts[r] = row[0]
                    if row[1] is not None:
                        sums[r] = row[1]
            cols["self_counts_" + name], cols["self_sum_" + name] = counts, sums
        out.append(cols)
    return out


def join_fast(hits, sites, counts, hit_sum, l):
    """`join` over arrays: sites (search.SELF_SITE_DTYPE, sorted by contig, position, strand) with their counts and sums."""
    key = (sites["contig"].astype(np.int64) << 33) | (sites["position"].astype(np.int64) << 1) | (sites["strand"] == b"-")
    assert (np.diff(key) > 0).all()
    out = []
    for k, h in enumerate(hits):
        cols = {}
        for name, strand, shift in (("plus", 0, -l), ("minus", 1, 0)):
            pos = np.asarray(h["pos_" + name]).astype(np.int64) + shift
            want = (np.int64(k) << 33) | (pos << 1) | strand
            at = np.minimum(np.searchsorted(key, want), max(key.size - 1, 0))
            found = (key[at] == want) & (pos >= 0) if key.size else np.zeros(pos.size, bool)
            c = np.full((pos.size, counts.shape[1]), NO_COUNT, dtype=np.uint32)
            s = np.full(pos.size, NO_SUM, dtype=np.uint64)
            c[found] = counts[at[found]]
            if hit_sum is not None:
                s[found] = hit_sum[at[found]]
            cols["self_counts_" + name], cols["self_sum_" + name] = c, s
        out.append(cols)
    return out


def specificity_of(hit_sum):
    """The CSV's specificity field of one hit_sum (a Python int below 2^64 - 1), as text."""
    return repr(1.0 / (1.0 + float(np.float64(np.uint64(hit_sum))) / float(1 << 30)))


def expected_fields(cols, n_plus, row):
    """The added CSV fields of row `row` of a contig ('+' rows first) from its joined columns."""
    name, r = ("plus", row) if row < n_plus else ("minus", row - n_plus)
    out = ["-1" if int(v) == NO_COUNT else str(int(v)) for v in cols["self_counts_" + name][r]]
    hs = int(cols["self_sum_" + name][r])
    return out + (["-1", "-1"] if hs == NO_SUM else [str(hs), specificity_of(hs)])
