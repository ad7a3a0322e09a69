"""The guide pairs' definition (cropsr_amd/select.py), stated twice for the tests: in numpy
(pairs_numpy: searchsorted windows plus one lexsort per gene) and as a plain double loop over a gene's rows (pairs_loop).

Per arena, after a scan at guide length 20.  tables: dict(pos_plus, score_plus, pos_minus, score_minus), positions
ascending.  Gene g is the closed range [lo[g], hi[g]] of arena positions.
  eligible   the rows that PASS for gene g as the selection has it (tests/select_reference.py): the row has a score other
             than -1, its cut site -- i - 3 of a '+' row, j of a '-' row -- lies in [lo, hi], score >= min_score, and
             the joined columns (spec), the CDS flag (cds) and any further per-row verdict (also = dict(plus, minus) of
             booleans: the property and repair limits) hold
  boundary   c = i - 3 of a '+' row, c = j + 6 of a '-' row: the cut boundary of repair.py, not the cut site above
  pair       (a, b): two eligible rows of one gene with c_a < c_b; D = c_b - c_a is the deletion's length
  qualifies  dmin <= D <= dmax; with frameshift D mod 3 != 0; bit sa * 2 + sb of the mask is set (0 for '+', 1 for '-')
  order      higher min(score_a, score_b) (the doubles' bits as unsigned 64-bit integers), then higher max, then smaller
             c_a, then smaller c_b, then smaller sa * 2 + sb
  result     n_pass[g], n_pairs[g] (all qualifying pairs) and pairs[g][0..KP): the first min(KP, n_pairs) pairs, each as
             (row_a | sa << 31, row_b | sb << 31), else 0xFFFFFFFF
"""
import struct

import numpy as np

NONE = 0xFFFFFFFF
ANY, PAM_OUT, PAM_IN = 0xF, 0x4, 0x2


def boundary(pos, minus):
    return pos + 6 if minus else pos - 3


def eligible_numpy(tables, min_score=0.0, spec=None, cds=None, also=None):
    """Per strand a boolean array: the row passes everything but "in the gene"."""
    out = {}
    for s in ("plus", "minus"):
        score = np.asarray(tables["score_" + s], np.float64)
        n = score.size
        ok = (score != -1.0) & (score >= np.float64(min_score))
        if spec is not None:
            c0 = np.asarray(spec["counts_" + s], np.uint32).reshape(n, -1)[:, 0].astype(np.uint64)
            hs = np.asarray(spec["sum_" + s]).astype(np.uint64)
            ok &= (c0 != NONE) & (c0 <= np.uint64(spec["max_mm0"])) & (hs <= np.uint64(spec["max_hit_sum"]))
        if cds is not None:
            ids = np.asarray(cds["feat_" + s]).astype(np.int64)
            flags = np.asarray(cds["flags"], np.uint8)
            ok &= (ids != NONE) & (np.concatenate([flags, [0]])[np.where(ids == NONE, flags.size, ids)] != 0)
        if also is not None:
            ok &= np.asarray(also[s], bool)
        out[s] = ok
    return out


def pairs_numpy(tables, lo, hi, KP, dmin, dmax, mask=ANY, frameshift=False, min_score=0.0, spec=None, cds=None, also=None):
    G = len(lo)
    n_pass, n_pairs = np.zeros(G, np.uint32), np.zeros(G, np.uint64)
    pairs = np.full((G, KP, 2), NONE, np.uint32)
    ok = eligible_numpy(tables, min_score, spec, cds, also)
    n_plus, n_minus = len(tables["pos_plus"]), len(tables["pos_minus"])
    site = np.concatenate([np.asarray(tables["pos_plus"], np.int64) - 3, np.asarray(tables["pos_minus"], np.int64)])
    c_all = np.concatenate([np.asarray(tables["pos_plus"], np.int64) - 3, np.asarray(tables["pos_minus"], np.int64) + 6])
    strand = np.concatenate([np.zeros(n_plus, np.int64), np.ones(n_minus, np.int64)])
    row = np.concatenate([np.arange(n_plus), np.arange(n_minus)]).astype(np.int64)
    key = np.concatenate([tables["score_plus"], tables["score_minus"]]).astype(np.float64).view(np.uint64)
    passing = np.concatenate([ok["plus"], ok["minus"]])
    big = np.iinfo(np.uint64).max
    for g in range(G):
        e = np.flatnonzero(passing & (site >= int(lo[g])) & (site <= int(hi[g])))
        n_pass[g] = e.size
        e = e[np.argsort(c_all[e], kind="stable")]
        c = c_all[e]
        first, last = np.searchsorted(c, c + dmin, "left"), np.searchsorted(c, c + dmax, "right")
        count = last - first
        a = np.repeat(np.arange(e.size), count)
        b = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count) + np.repeat(first, count)
        D = c[b] - c[a]
        sbits = strand[e][a] * 2 + strand[e][b]
        good = ((mask >> sbits) & 1).astype(bool)
        if frameshift:
            good &= D % 3 != 0
        a, b, sbits = a[good], b[good], sbits[good]
        n_pairs[g] = a.size
        ka, kb = key[e][a], key[e][b]
        order = np.lexsort((sbits, c[b], c[a], big - np.maximum(ka, kb), big - np.minimum(ka, kb)))[:KP]
        ea, eb = e[a[order]], e[b[order]]
        pairs[g, :order.size, 0] = (row[ea] | strand[ea] << 31).astype(np.uint32)
        pairs[g, :order.size, 1] = (row[eb] | strand[eb] << 31).astype(np.uint32)
    return n_pass, n_pairs, pairs


def pairs_loop(tables, lo, hi, KP, dmin, dmax, mask=ANY, frameshift=False, min_score=0.0, spec=None, cds=None, also=None):
    """Row by row and pair by pair, in plain Python: quadratic in a gene's rows."""
    G = len(lo)
    n_pass, n_pairs, pairs = [0] * G, [0] * G, [[[NONE, NONE] for _ in range(KP)] for _ in range(G)]
    for g in range(G):
        rows = []  # (c, strand, score bits, row)
        for s, name in enumerate(("plus", "minus")):
            pos, score = tables["pos_" + name], tables["score_" + name]
            for r in range(len(pos)):
                x = float(score[r])
                if x == -1.0:
                    continue
                site = int(pos[r]) - 3 if s == 0 else int(pos[r])
                if not int(lo[g]) <= site <= int(hi[g]):
                    continue
                if not x >= float(min_score):
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
                rows.append((boundary(int(pos[r]), s == 1), s, struct.unpack("<Q", struct.pack("<d", x))[0], r))
        n_pass[g] = len(rows)
        found = []
        for ca, sa, ka, ra in rows:
            for cb, sb, kb, rb in rows:
                D = cb - ca
                if not dmin <= D <= dmax:
                    continue
                if frameshift and D % 3 == 0:
                    continue
                if not mask >> (sa * 2 + sb) & 1:
                    continue
                found.append((-min(ka, kb), -max(ka, kb), ca, cb, sa * 2 + sb, ra | sa << 31, rb | sb << 31))
        n_pairs[g] = len(found)
        for rank, f in enumerate(sorted(found)[:KP]):
            pairs[g][rank] = [f[5], f[6]]
    return np.array(n_pass, np.uint32), np.array(n_pairs, np.uint64), np.array(pairs, np.uint32).reshape(G, KP, 2)
