"""The guide selection's definition (cropsr_amd/select.py), stated twice for the tests: in numpy (select_numpy) and as
a plain loop over genes and rows (select_loop).  Plus direct restatements of what the native host code does with the
GFF's gene rows: which lines are genes (gff_genes), where they lie in an arena (layout), which label sets hold a CDS
(cds_flags).

Per arena, after a scan at guide length 20.  tables: dict(pos_plus, score_plus, pos_minus, score_minus), positions
ascending.  Gene g is the closed range [lo[g], hi[g]] of arena positions.
  cut site  i - 3 of a '+' row, j of a '-' row; only rows whose score is not -1 have one
  in        the row has a cut site and lo <= cut site <= hi
  passes    in; score >= min_score (float64); with spec = dict(counts_plus, sum_plus, counts_minus, sum_minus, max_mm0,
            max_hit_sum): counts[0] != 0xFFFFFFFF, counts[0] <= max_mm0 and hit_sum <= max_hit_sum (integers); with cds =
            dict(feat_plus, feat_minus, flags): the row's id is not 0xFFFFFFFF and flags[id] != 0
  order     higher score first (the doubles' bits as unsigned 64-bit integers), then smaller cut site, then '+' first
  result    n_in[g], n_pass[g], sel[g][0..K): the first min(K, n_pass) passing rows as row | strand << 31, else 0xFFFFFFFF
"""
import numpy as np

NONE = 0xFFFFFFFF


def select_numpy(tables, lo, hi, K, min_score=0.0, spec=None, cds=None):
    G = len(lo)
    n_in, n_pass, sel = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.full((G, K), NONE, np.uint32)
    n_plus = len(tables["pos_plus"])
    score = np.concatenate([tables["score_plus"], tables["score_minus"]]).astype(np.float64)
    cut = np.concatenate([np.asarray(tables["pos_plus"], np.int64) - 3, np.asarray(tables["pos_minus"], np.int64)])
    strand = np.concatenate([np.zeros(n_plus, np.int64), np.ones(len(tables["pos_minus"]), np.int64)])
    row = np.concatenate([np.arange(n_plus), np.arange(len(tables["pos_minus"]))]).astype(np.int64)
    has_cut = score != -1.0
    ok = score >= np.float64(min_score)
    if spec is not None:
        c0 = np.concatenate([np.asarray(spec["counts_plus"], np.uint32).reshape(n_plus, -1)[:, 0],
                             np.asarray(spec["counts_minus"], np.uint32).reshape(len(tables["pos_minus"]), -1)[:, 0]]).astype(np.uint64)
        hs = np.concatenate([spec["sum_plus"], spec["sum_minus"]]).astype(np.uint64)
        ok &= (c0 != NONE) & (c0 <= np.uint64(spec["max_mm0"])) & (hs <= np.uint64(spec["max_hit_sum"]))
    if cds is not None:
        ids = np.concatenate([cds["feat_plus"], cds["feat_minus"]]).astype(np.int64)
        flags = np.asarray(cds["flags"], np.uint8)
        ok &= (ids != NONE) & (np.concatenate([flags, [0]])[np.where(ids == NONE, flags.size, ids)] != 0)
    key = score.view(np.uint64)
    for g in range(G):
        inside = has_cut & (cut >= int(lo[g])) & (cut <= int(hi[g]))
        passing = np.flatnonzero(inside & ok)
        n_in[g], n_pass[g] = inside.sum(), passing.size
        order = np.lexsort((strand[passing], cut[passing], np.iinfo(np.uint64).max - key[passing]))[:K]
        best = passing[order]
        sel[g, :best.size] = (row[best] | (strand[best] << 31)).astype(np.uint32)
    return n_in, n_pass, sel


def select_loop(tables, lo, hi, K, min_score=0.0, spec=None, cds=None):
    import struct
    G = len(lo)
    n_in, n_pass, sel = [0] * G, [0] * G, [[NONE] * K for _ in range(G)]
    for g in range(G):
        passing = []
        for s, name in enumerate(("plus", "minus")):
            pos, score = tables["pos_" + name], tables["score_" + name]
            for r in range(len(pos)):
                x = float(score[r])
                if x == -1.0:
                    continue
                cut = int(pos[r]) - 3 if s == 0 else int(pos[r])
                if not int(lo[g]) <= cut <= int(hi[g]):
                    continue
                n_in[g] += 1
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
                bits = struct.unpack("<Q", struct.pack("<d", x))[0]
                passing.append((-bits, cut, s, r))
        n_pass[g] = len(passing)
        for rank, (_, _, s, r) in enumerate(sorted(passing)[:K]):
            sel[g][rank] = r | s << 31
    return np.array(n_in, np.uint32), np.array(n_pass, np.uint32), np.array(sel, np.uint32).reshape(G, K)


def gff_genes(text):
    """[(seqid, start, end, label)] of the lines the native parser takes for genes, in file order."""
    out = []
    for line in text.split("\n"):
        if not line or line[0] == "#":
            continue
        cols = line.split("\t")
        if len(cols) < 9 or cols[2] != "gene":
            continue
        if not all(c and len(c) <= 18 and all(ch in "0123456789" for ch in c) for c in cols[3:5]):
            continue
        attrs = {}
        for part in cols[8].split(";"):
            part = part.strip(" \t\n\r\v\f")
            key, _, val = part.partition("=")
            attrs.setdefault(key, val)
        ident = attrs.get("ID") or attrs.get("Name") or attrs.get("Parent") or "."
        out.append((cols[0], int(cols[3]), int(cols[4]), "gene:" + ident))
    return out


def layout(genes, entries, dec):
    """entries: [(seqid name, index of the text's first character in its contig string, length, arena offset)] in arena
    order -> (lo, hi, gene index) rows: string index = coordinate + dec - 1 - first, clipped to the text."""
    lo, hi, idx = [], [], []
    for name, first, length, base in entries:
        for g, (seqid, start, end, _) in enumerate(genes):
            if seqid != name or start > end or length == 0:
                continue
            a, b = max(start + dec - 1 - first, 0), min(end + dec - 1 - first, length - 1)
            if a > b:
                continue
            lo.append(base + a)
            hi.append(base + b)
            idx.append(g)
    return np.array(lo, np.uint32), np.array(hi, np.uint32), np.array(idx, np.uint64)


def cds_flags(strings):
    """1 for a label-set string (labels joined with ';') that holds a `CDS:` label."""
    return np.array([1 if any(lab.startswith("CDS:") for lab in s.split(";")) else 0 for s in strings], np.uint8)
