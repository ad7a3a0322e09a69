"""The distinct pair selection's definition (cropsr_amd/select.py), stated twice for the tests: in
numpy by rounds (distinct_numpy: all qualifying pairs of a gene in the pairs' order, then round after round the first pair
without a row among the earlier picks) and as the plain walk with a set of taken rows (distinct_walk).

Everything of tests/select_pairs_reference.py stands: eligible rows, the boundary c, qualifying pairs, the order, n_pass and
n_pairs.  New, per arena text and per gene g:
  distinct   walk the qualifying pairs of g in that order; take a pair iff neither of its two rows is a row of a pair
             already taken; stop at KP taken.  A row is a table row of one strand, packed row | strand << 31: two rows with
             equal boundaries on the two strands are different guides; a row taken as a shuts out pairs that offer it as
             b, and the other way round
  by rounds  round t takes the first qualifying pair in the order that has no row among the picks of rounds < t
  result     n_pass[g], n_pairs[g] as the pair selection's; n_distinct[g], the pairs taken; pairs[g][0..KP) in pick order,
             each as (row_a | sa << 31, row_b | sb << 31), else 0xFFFFFFFF
"""
import struct

import numpy as np

import select_pairs_reference as pref

NONE = 0xFFFFFFFF
SHARED_A, SHARED_B, B_AS_A, A_AS_B = "shared a", "shared b", "a taken as b offered as a", "a taken as a offered as b"


def ordered_pairs(tables, lo, hi, dmin, dmax, mask=pref.ANY, frameshift=False, min_score=0.0, spec=None, cds=None, also=None):
    """Per gene (n_pass, A, B): every qualifying pair in the pairs' order, as two arrays of packed rows."""
    ok = pref.eligible_numpy(tables, min_score, spec, cds, also)
    n_plus, n_minus = len(tables["pos_plus"]), len(tables["pos_minus"])
    site = np.concatenate([np.asarray(tables["pos_plus"], np.int64) - 3, np.asarray(tables["pos_minus"], np.int64)])
    c_all = np.concatenate([np.asarray(tables["pos_plus"], np.int64) - 3, np.asarray(tables["pos_minus"], np.int64) + 6])
    strand = np.concatenate([np.zeros(n_plus, np.int64), np.ones(n_minus, np.int64)])
    packed = (np.concatenate([np.arange(n_plus), np.arange(n_minus)]).astype(np.int64) | strand << 31).astype(np.uint32)
    key = np.concatenate([tables["score_plus"], tables["score_minus"]]).astype(np.float64).view(np.uint64)
    passing = np.concatenate([ok["plus"], ok["minus"]])
    big = np.iinfo(np.uint64).max
    out = []
    for g in range(len(lo)):
        e = np.flatnonzero(passing & (site >= int(lo[g])) & (site <= int(hi[g])))
        n_pass = e.size
        e = e[np.argsort(c_all[e], kind="stable")]
        c = c_all[e]
        first, last = np.searchsorted(c, c + dmin, "left"), np.searchsorted(c, c + dmax, "right")
        count = last - first
        a = np.repeat(np.arange(e.size), count)
        b = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count) + np.repeat(first, count)
        sbits = strand[e][a] * 2 + strand[e][b]
        good = ((mask >> sbits) & 1).astype(bool)
        if frameshift:
            good &= (c[b] - c[a]) % 3 != 0
        a, b, sbits = a[good], b[good], sbits[good]
        ka, kb = key[e][a], key[e][b]
        order = np.lexsort((sbits, c[b], c[a], big - np.maximum(ka, kb), big - np.minimum(ka, kb)))
        out.append((n_pass, packed[e[a[order]]], packed[e[b[order]]]))
    return out


def rounds_of(A, B, KP):
    """The picks of one gene by rounds: the plain ranks (indices into A, B) of the pairs taken."""
    free = np.ones(A.size, bool)
    ranks = []
    for _ in range(KP):
        if not free.any():
            break
        i = int(np.argmax(free))  # the first pair in the order without a row among the earlier picks
        ranks.append(i)
        for x in (A[i], B[i]):
            free &= (A != x) & (B != x)
    return ranks


def distinct_numpy(tables, lo, hi, KP, dmin, dmax, mask=pref.ANY, frameshift=False, min_score=0.0, spec=None, cds=None, also=None, ranks=None):
    """(n_pass, n_pairs, n_distinct, pairs).  ranks: a list that receives, per gene, the plain ranks of its picks."""
    G = len(lo)
    n_pass, n_pairs, n_distinct = np.zeros(G, np.uint32), np.zeros(G, np.uint64), np.zeros(G, np.uint32)
    pairs = np.full((G, KP, 2), NONE, np.uint32)
    for g, (n, A, B) in enumerate(ordered_pairs(tables, lo, hi, dmin, dmax, mask, frameshift, min_score, spec, cds, also)):
        n_pass[g], n_pairs[g] = n, A.size
        r = rounds_of(A, B, KP)
        n_distinct[g] = len(r)
        pairs[g, :len(r), 0], pairs[g, :len(r), 1] = A[r], B[r]
        if ranks is not None:
            ranks.append(r)
    return n_pass, n_pairs, n_distinct, pairs


def distinct_walk(tables, lo, hi, KP, dmin, dmax, mask=pref.ANY, frameshift=False, min_score=0.0, spec=None, cds=None, also=None):
    """Row by row and pair by pair, in plain Python, then one walk down the sorted pairs with a set of taken rows."""
    G = len(lo)
    n_pass, n_pairs, n_distinct, pairs = [0] * G, [0] * G, [0] * G, [[[NONE, NONE] for _ in range(KP)] for _ in range(G)]
    for g in range(G):
        rows = []  # (c, strand, score bits, row)
        for s, name in enumerate(("plus", "minus")):
            pos, score = tables["pos_" + name], tables["score_" + name]
            for r in range(len(pos)):
                x = float(score[r])
                site = int(pos[r]) - 3 if s == 0 else int(pos[r])
                if x == -1.0 or not int(lo[g]) <= site <= int(hi[g]) or not x >= float(min_score):
                    continue
                if spec is not None:
                    c0 = int(np.asarray(spec["counts_" + name]).reshape(len(pos), -1)[r, 0])
                    if c0 == NONE or c0 > int(spec["max_mm0"]) or int(spec["sum_" + name][r]) > int(spec["max_hit_sum"]):
                        continue
                if cds is not None:
                    i = int(cds["feat_" + name][r])
                    if i == NONE or not cds["flags"][i]:
                        continue
                if also is not None and not also[name][r]:
                    continue
                rows.append((pref.boundary(int(pos[r]), s == 1), s, struct.unpack("<Q", struct.pack("<d", x))[0], r))
        n_pass[g] = len(rows)
        found = []
        for ca, sa, ka, ra in rows:
            for cb, sb, kb, rb in rows:
                D = cb - ca
                if dmin <= D <= dmax and not (frameshift and D % 3 == 0) and mask >> (sa * 2 + sb) & 1:
                    found.append((-min(ka, kb), -max(ka, kb), ca, cb, sa * 2 + sb, ra | sa << 31, rb | sb << 31))
        n_pairs[g] = len(found)
        taken = set()
        for f in sorted(found):
            if n_distinct[g] == KP:
                break
            if f[5] in taken or f[6] in taken:
                continue
            pairs[g][n_distinct[g]] = [f[5], f[6]]
            n_distinct[g] += 1
            taken.update(f[5:7])
    return (np.array(n_pass, np.uint32), np.array(n_pairs, np.uint64), np.array(n_distinct, np.uint32),
            np.array(pairs, np.uint32).reshape(G, KP, 2))


def rejections(A, B, ranks):
    """Of one gene's walk down to its last pick: how often each kind of rejection occurs (a pair may count under two kinds,
    and `both` counts the pairs rejected on both of their rows)."""
    out = {SHARED_A: 0, SHARED_B: 0, B_AS_A: 0, A_AS_B: 0, "both": 0}
    taken_a, taken_b = set(), set()
    picks = set(ranks)
    for i in range(ranks[-1] + 1 if ranks else 0):
        a, b = int(A[i]), int(B[i])
        if i in picks:
            taken_a.add(a)
            taken_b.add(b)
            continue
        kinds = [k for k, hit in ((SHARED_A, a in taken_a), (SHARED_B, b in taken_b), (B_AS_A, a in taken_b), (A_AS_B, b in taken_a)) if hit]
        for k in kinds:
            out[k] += 1
        if ({SHARED_A, B_AS_A} & set(kinds)) and ({SHARED_B, A_AS_B} & set(kinds)):
            out["both"] += 1
    return out
