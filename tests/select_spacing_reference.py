"""The spaced selection's definition (cropsr_amd/select.py), stated twice for the tests: in numpy
by rounds (spaced_numpy) and as a plain walk over the sorted rows (spaced_loop).

Per arena, after a scan at guide length 20.  tables, genes, the predicate and the order are select_reference's:
  cut site  i - 3 of a '+' row, j of a '-' row (NOT the pairs' cut boundary); only rows whose score is not -1 have one
  passes    in the gene [lo, hi] by its cut site; score >= min_score; with spec / cds the joined columns and the CDS flag
  order     higher score first (the doubles' bits as unsigned 64-bit integers), then smaller cut site, then '+' first
Spaced selection with minimum distance D (0 <= D <= 2^31 - 1):
  walk      the passing rows of the gene in that order; take a row iff |cut - cut(p)| >= D for EVERY row p already taken;
            stop at K taken
  rounds    the same thing: round t takes the best passing row, not taken yet, that is not within D - 1 of any earlier pick
  result    n_pass[g] (unchanged by D), n_spaced[g] (the rows taken) and sel[g][0..K): the rows taken as row | strand << 31
            in pick order, 0xFFFFFFFF beyond n_spaced
"""
import struct

import numpy as np

NONE = 0xFFFFFFFF
MAX_SPACING = (1 << 31) - 1


def _columns(tables, min_score, spec, cds):
    """(score, cut, strand, row, has_cut, ok) over the '+' rows, then the '-' rows."""
    n_plus, n_minus = len(tables["pos_plus"]), len(tables["pos_minus"])
    score = np.concatenate([tables["score_plus"], tables["score_minus"]]).astype(np.float64)
    cut = np.concatenate([np.asarray(tables["pos_plus"], np.int64) - 3, np.asarray(tables["pos_minus"], np.int64)])
    strand = np.concatenate([np.zeros(n_plus, np.int64), np.ones(n_minus, np.int64)])
    row = np.concatenate([np.arange(n_plus), np.arange(n_minus)]).astype(np.int64)
    ok = score >= np.float64(min_score)
    if spec is not None:
        c0 = np.concatenate([np.asarray(spec["counts_plus"], np.uint32).reshape(n_plus, -1)[:, 0],
                             np.asarray(spec["counts_minus"], np.uint32).reshape(n_minus, -1)[:, 0]]).astype(np.uint64)
        hs = np.concatenate([spec["sum_plus"], spec["sum_minus"]]).astype(np.uint64)
        ok &= (c0 != NONE) & (c0 <= np.uint64(spec["max_mm0"])) & (hs <= np.uint64(spec["max_hit_sum"]))
    if cds is not None:
        ids = np.concatenate([cds["feat_plus"], cds["feat_minus"]]).astype(np.int64)
        flags = np.asarray(cds["flags"], np.uint8)
        ok &= (ids != NONE) & (np.concatenate([flags, [0]])[np.where(ids == NONE, flags.size, ids)] != 0)
    return score, cut, strand, row, score != -1.0, ok


def spaced_numpy(tables, lo, hi, K, D, min_score=0.0, spec=None, cds=None):
    """By rounds: (n_pass, n_spaced, sel)."""
    G, D = len(lo), int(D)
    assert 0 <= D <= MAX_SPACING
    n_pass, n_spaced, sel = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.full((G, K), NONE, np.uint32)
    score, cut, strand, row, has_cut, ok = _columns(tables, min_score, spec, cds)
    key = score.view(np.uint64)
    for g in range(G):
        passing = np.flatnonzero(has_cut & ok & (cut >= int(lo[g])) & (cut <= int(hi[g])))
        n_pass[g] = passing.size
        passing = passing[np.lexsort((strand[passing], cut[passing], np.iinfo(np.uint64).max - key[passing]))]
        c = cut[passing]
        open_ = np.ones(passing.size, bool)  # not taken and clear of every pick so far
        for t in range(K):
            left = np.flatnonzero(open_)
            if not left.size:
                break
            j = left[0]
            sel[g, t] = np.uint32(int(row[passing[j]]) | int(strand[passing[j]]) << 31)
            open_[j] = False
            open_ &= np.abs(c - c[j]) >= D
            n_spaced[g] = t + 1
    return n_pass, n_spaced, sel


def spaced_loop(tables, lo, hi, K, D, min_score=0.0, spec=None, cds=None):
    """By the walk, with plain loops: (n_pass, n_spaced, sel)."""
    G, D = len(lo), int(D)
    n_pass, n_spaced, sel = [0] * G, [0] * G, [[NONE] * K for _ in range(G)]
    for g in range(G):
        passing = []
        for s, name in enumerate(("plus", "minus")):
            pos, score = tables["pos_" + name], tables["score_" + name]
            for r in range(len(pos)):
                x = float(score[r])
                if x == -1.0:
                    continue
                cut = int(pos[r]) - 3 if s == 0 else int(pos[r])
                if not int(lo[g]) <= cut <= int(hi[g]) or not x >= float(min_score):
                    continue
                if spec is not None:
                    c0 = int(np.asarray(spec["counts_" + name]).reshape(len(pos), -1)[r, 0])
                    if c0 == NONE or c0 > int(spec["max_mm0"]) or int(spec["sum_" + name][r]) > int(spec["max_hit_sum"]):
                        continue
                if cds is not None:
                    i = int(cds["feat_" + name][r])
                    if i == NONE or not cds["flags"][i]:
                        continue
                bits = struct.unpack("<Q", struct.pack("<d", x))[0]
                passing.append((-bits, cut, s, r))
        n_pass[g] = len(passing)
        taken = []
        for _, cut, s, r in sorted(passing):
            if len(taken) == K:
                break
            if all(abs(cut - p) >= D for p in taken):
                sel[g][len(taken)] = r | s << 31
                taken.append(cut)
        n_spaced[g] = len(taken)
    return np.array(n_pass, np.uint32), np.array(n_spaced, np.uint32), np.array(sel, np.uint32).reshape(G, K)


def walk(tables, lo, hi, K, D, min_score=0.0):
    """The walk over one gene [lo, hi] with its trace, for the tests that look at single decisions: a list of (cut, strand,
    row, taken, distance to the nearest pick taken before it or None), in the order, up to the K-th pick."""
    score, cut, strand, row, has_cut, ok = _columns(tables, min_score, None, None)
    key = score.view(np.uint64)
    passing = np.flatnonzero(has_cut & ok & (cut >= int(lo)) & (cut <= int(hi)))
    passing = passing[np.lexsort((strand[passing], cut[passing], np.iinfo(np.uint64).max - key[passing]))]
    out, taken = [], []
    for j in passing:
        if len(taken) == K:
            break
        near = min((abs(int(cut[j]) - p) for p in taken), default=None)
        take = near is None or near >= int(D)
        out.append((int(cut[j]), int(strand[j]), int(row[j]), take, near))
        if take:
            taken.append(int(cut[j]))
    return out
