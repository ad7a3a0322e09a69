"""The coding position's definition (cropsr_amd/coding.py), stated twice for the tests: as a plain loop over GFF lines
and sets of coordinates (model_loop, position_loop, select_loop) and in numpy over merged segments (model_numpy,
position_numpy, select_numpy).  Only the splitting of a line into its fields is shared.

A MODEL is a list with one dict per `gene` row of the GFF, in file order: strand ('+', '-' or '.'), model (bool), n_tx,
length (L_P; both 0 without a model), and the coding transcripts in file order with the primary one's index -- as sets of
1-based coordinates in the loop statement, as (start, end) arrays of merged closed segments in the numpy one.

A layout ROW places a gene in an arena text: (gene index, shift, text_lo, text_hi) with arena index = coordinate + shift and
the text's letters at arena indices text_lo .. text_hi.  The cut boundary c lies between the letters c - 1 and c.
"""
import numpy as np

NONE = 0xFFFFFFFF
NOT_INSIDE = 0xFFFFFFFF
TRANSCRIPT_TYPES = ("mRNA", "transcript")


def gff_rows(text):
    """[(type, seqid, start, end, strand, attrs)] of the lines the native parser reads, in file order."""
    out = []
    for line in text.split("\n"):
        if not line or line[0] == "#":
            continue
        cols = line.split("\t")
        if len(cols) < 9 or cols[2] not in ("gene", "CDS") + TRANSCRIPT_TYPES:
            continue
        if not all(c and len(c) <= 18 and all(ch in "0123456789" for ch in c) for c in cols[3:5]):
            continue
        attrs = {}
        for part in cols[8].split(";"):
            part = part.strip(" \t\n\r\v\f")
            key, _, val = part.partition("=")
            attrs.setdefault(key, val)
        out.append((cols[2], cols[0], int(cols[3]), int(cols[4]), cols[6], attrs))
    return out


def _parents(attrs):
    return [v for v in attrs.get("Parent", "").split(",") if v]


def _no_model(strand):
    return dict(strand=strand if strand in ("+", "-") else ".", model=False, n_tx=0, length=0, transcripts=[], primary=None)


# ------------------------------------------------------------------------------------------------ the plain loop
def model_loop(text):
    rows = gff_rows(text)
    out = []
    for gi, (typ, seqid, _, _, strand, attrs) in enumerate(rows):
        if typ != "gene":
            continue
        m = _no_model(strand)
        out.append(m)
        gid = attrs.get("ID", "")
        if strand not in ("+", "-") or not gid:
            continue
        if any(r[0] == "gene" and r[1] == seqid and r[5].get("ID", "") == gid for r in rows[:gi]):
            continue  # a later gene row of the same ID: the first one owns the children

        def letters(ident):
            s = set()
            for typ2, seq2, a, b, _, at2 in rows:
                if typ2 == "CDS" and seq2 == seqid and ident in _parents(at2) and a <= b:
                    s.update(range(a, b + 1))
            return s

        coding = []
        for ti, (typ2, seq2, _, _, _, at2) in enumerate(rows):
            if ti == gi:
                s = letters(gid)  # the implicit transcript stands at the gene row
            elif typ2 in TRANSCRIPT_TYPES and seq2 == seqid and gid in _parents(at2):
                tid = at2.get("ID", "")
                first = tid and not any(r[0] in TRANSCRIPT_TYPES and r[1] == seqid and r[5].get("ID", "") == tid for r in rows[:ti])
                s = letters(tid) if first else set()
            else:
                continue
            if s:
                coding.append(s)
        if not coding:
            continue
        best = max(len(s) for s in coding)
        if best > 0xFFFFFFFF:
            continue
        m.update(model=True, n_tx=len(coding), length=best, transcripts=coding, primary=[len(s) for s in coding].index(best))
    return out


def position_loop(m, row, c):
    """(off, cover) of boundary c for a layout row of gene model m: off NOT_INSIDE where the cut is not inside P."""
    _, shift, text_lo, text_hi = row
    if not m["model"] or c - 1 < text_lo or c > text_hi:
        return NOT_INSIDE, 0
    cover = sum(1 for T in m["transcripts"] if (c - 1 - shift) in T and (c - shift) in T)
    P = m["transcripts"][m["primary"]]
    if not ((c - 1 - shift) in P and (c - shift) in P):
        return NOT_INSIDE, cover
    before = sum(1 for p in P if p + shift < c)
    return (before if m["strand"] == "+" else m["length"] - before), cover


# ------------------------------------------------------------------------------------------------ numpy
def _merge(ranges):
    arr = np.array(sorted(ranges), dtype=np.int64).reshape(-1, 2)
    reach = np.maximum.accumulate(arr[:, 1])
    new = np.concatenate([[True], arr[1:, 0] > reach[:-1] + 1])
    at = np.flatnonzero(new)
    return arr[at, 0], np.maximum.reduceat(arr[:, 1], at)


def model_numpy(text):
    rows = gff_rows(text)
    gene_of, tx_of = {}, {}
    for i, (typ, seqid, _, _, _, attrs) in enumerate(rows):
        ident = attrs.get("ID", "")
        if ident:
            if typ == "gene":
                gene_of.setdefault((seqid, ident), i)
            elif typ in TRANSCRIPT_TYPES:
                tx_of.setdefault((seqid, ident), i)
    ranges = {}   # row index of the owner (a gene row: its implicit transcript) -> [(start, end)]
    members = {}  # row index of a gene -> row indices of its transcript rows
    for i, (typ, seqid, a, b, _, attrs) in enumerate(rows):
        for v in dict.fromkeys(_parents(attrs)):
            if typ == "CDS" and a <= b:
                for owner in (gene_of.get((seqid, v)), tx_of.get((seqid, v))):
                    if owner is not None:
                        ranges.setdefault(owner, []).append((a, b))
            elif typ in TRANSCRIPT_TYPES and (seqid, v) in gene_of:
                members.setdefault(gene_of[(seqid, v)], []).append(i)
    out = []
    for i, (typ, seqid, _, _, strand, attrs) in enumerate(rows):
        if typ != "gene":
            continue
        m = _no_model(strand)
        out.append(m)
        if strand not in ("+", "-") or gene_of.get((seqid, attrs.get("ID", ""))) != i:
            continue
        order = sorted(set(members.get(i, []) + [i]))
        coding = [_merge(ranges[t]) for t in order if ranges.get(t)]
        if not coding:
            continue
        lengths = np.array([int((e - s + 1).sum()) for s, e in coding], dtype=object)
        best = max(lengths)
        if best > 0xFFFFFFFF:
            continue
        m.update(model=True, n_tx=len(coding), length=int(best), transcripts=coding, primary=int(list(lengths).index(best)))
    return out


def position_numpy(m, row, c):
    """(off uint32, cover uint32) arrays for an array of boundaries c."""
    _, shift, text_lo, text_hi = row
    c = np.asarray(c, dtype=np.int64)
    off, cover = np.full(c.shape, NOT_INSIDE, np.uint32), np.zeros(c.shape, np.uint32)
    if not m["model"]:
        return off, cover
    in_text = (c - 1 >= text_lo) & (c <= text_hi)
    for t, (s, e) in enumerate(m["transcripts"]):
        a, b = s + shift, e + shift  # letters a .. b: the boundaries a + 1 .. b are inside
        k = np.searchsorted(a, c - 1, "right") - 1
        inside = in_text & (k >= 0) & (c <= b[np.maximum(k, 0)])
        cover += inside.astype(np.uint32)
        if t == m["primary"]:
            before = np.clip(c[:, None] - a[None, :], 0, (e - s + 1)[None, :]).sum(axis=1)
            value = before if m["strand"] == "+" else m["length"] - before
            off[inside] = value[inside].astype(np.uint32)
    return off, cover


def passes(limits, m, off, cover):
    """The limits of the definition in Python's exact integers: limits = (min_pct, max_pct, min_transcripts_pct)."""
    lo, hi, tx = limits
    return (m["model"] and off != NOT_INSIDE and lo * m["length"] <= 100 * int(off) <= hi * m["length"]
            and 100 * int(cover) >= tx * m["n_tx"])


# ------------------------------------------------------------------------------------------------ the layout
def layout_rows(text, entries, dec):
    """The rows of select_reference.layout, as (gene index, shift, text_lo, text_hi): the same rows in the same order."""
    genes = [r for r in gff_rows(text) if r[0] == "gene"]
    out = []
    for name, first, length, base in entries:
        for g, (_, seqid, start, end, _, _) in enumerate(genes):
            if seqid != name or start > end or length == 0:
                continue
            if max(start + dec - 1 - first, 0) > min(end + dec - 1 - first, length - 1):
                continue
            out.append((g, dec - 1 - first + base, base, base + length - 1))
    return out


def steps_position(model, r, c):
    """(off, cover) arrays that a native layout (the dict of Annotation.coding_layout) gives for row r at boundaries c: the
    step function read as include/cropsr_hip.h describes it."""
    c = np.asarray(c, dtype=np.int64)
    a, b = int(model["first"][r]), int(model["first"][r + 1])
    at, word, cum = (np.asarray(model[key][a:b]).astype(np.int64) for key in ("at", "word", "cum"))
    info, L = int(model["info"][r]), int(model["length"][r])
    off, cover = np.full(c.shape, NOT_INSIDE, np.uint32), np.zeros(c.shape, np.uint32)
    if not info >> 17 & 1 or not at.size:
        return off, cover
    k = np.searchsorted(at, c, "right") - 1
    has = k >= 0
    k = np.maximum(k, 0)
    cover[has] = (word[k] & 0xFFFF)[has].astype(np.uint32)
    inside = has & ((word[k] >> 16 & 1) == 1)
    before = cum[k] + (word[k] >> 17 & 1) * (c - at[k])
    value = L - before if info >> 16 & 1 else before
    off[inside] = value[inside].astype(np.uint32)
    return off, cover


# ------------------------------------------------------------------------------------------------ the selection
def _rows_of(tables):
    n_plus, n_minus = len(tables["pos_plus"]), len(tables["pos_minus"])
    score = np.concatenate([tables["score_plus"], tables["score_minus"]]).astype(np.float64)
    pos = np.concatenate([np.asarray(tables["pos_plus"], np.int64), np.asarray(tables["pos_minus"], np.int64)])
    strand = np.concatenate([np.zeros(n_plus, np.int64), np.ones(n_minus, np.int64)])
    row = np.concatenate([np.arange(n_plus), np.arange(n_minus)]).astype(np.int64)
    return score, pos, strand, row


def positions_numpy(tables, models, rows):
    """(off, cover), each (layout rows, rows of both tables -- '+' rows, then '-' rows): the coding position of EVERY table
    row's cut boundary for every layout row."""
    _, pos, strand, _ = _rows_of(tables)
    c = pos + np.where(strand == 0, -3, 6)
    both = [position_numpy(models[r[0]], r, c) for r in rows]
    return np.array([b[0] for b in both], np.uint32).reshape(len(rows), c.size), np.array([b[1] for b in both], np.uint32).reshape(len(rows), c.size)


def membership(tables, lo, hi):
    """Boolean (genes, rows of both tables): the row has a cut site and it lies in the gene."""
    score, pos, strand, _ = _rows_of(tables)
    cut = pos - np.where(strand == 0, 3, 0)
    return (score != -1.0)[None, :] & (cut[None, :] >= np.asarray(lo, np.int64)[:, None]) & (cut[None, :] <= np.asarray(hi, np.int64)[:, None])


def select_numpy(tables, lo, hi, models, rows, K, limits=None, ok=None, positions=None):
    """(n_in, n_pass, sel) per layout row.  models: a MODEL (numpy form); rows: layout_rows; limits: None or the three
    percentages; ok: None or a boolean per table row ('+' rows, then '-' rows) -- everything else the predicate asks;
    positions: positions_numpy's result when the caller has it."""
    G = len(lo)
    score, pos, strand, row = _rows_of(tables)
    cut = pos - np.where(strand == 0, 3, 0)       # the cut site that decides membership
    base_ok = np.ones(score.size, bool) if ok is None else np.asarray(ok, bool)
    key = score.view(np.uint64)
    n_in, n_pass, sel = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.full((G, K), NONE, np.uint32)
    offs, covers = positions if positions is not None else positions_numpy(tables, models, rows)
    member = membership(tables, lo, hi)
    for g in range(G):
        m = models[rows[g][0]]
        inside = member[g]
        good = base_ok
        if limits is not None:
            at = np.flatnonzero(inside)
            coded = np.zeros(score.size, bool)
            coded[at] = [passes(limits, m, int(o), int(c)) for o, c in zip(offs[g][at], covers[g][at])]
            good = good & coded
        passing = np.flatnonzero(inside & good)
        n_in[g], n_pass[g] = inside.sum(), passing.size
        order = np.lexsort((strand[passing], cut[passing], np.iinfo(np.uint64).max - key[passing]))[:K]
        best = passing[order]
        sel[g, :best.size] = (row[best] | (strand[best] << 31)).astype(np.uint32)
    return n_in, n_pass, sel


def select_loop(tables, lo, hi, models, rows, K, limits=None, ok=None):
    """(n_in, n_pass, sel) by the plain loop; models in the loop form."""
    import struct
    G = len(lo)
    n_in, n_pass, sel = [0] * G, [0] * G, [[NONE] * K for _ in range(G)]
    n_plus = len(tables["pos_plus"])
    for g in range(G):
        m = models[rows[g][0]]
        passing = []
        for s, name in enumerate(("plus", "minus")):
            pos, score = tables["pos_" + name], tables["score_" + name]
            for r in range(len(pos)):
                x = float(score[r])
                cut = int(pos[r]) - 3 if s == 0 else int(pos[r])
                if x == -1.0 or not int(lo[g]) <= cut <= int(hi[g]):
                    continue
                n_in[g] += 1
                if ok is not None and not ok[r + s * n_plus]:
                    continue
                if limits is not None:
                    off, cover = position_loop(m, rows[g], int(pos[r]) - 3 if s == 0 else int(pos[r]) + 6)
                    if not passes(limits, m, off, cover):
                        continue
                passing.append((-struct.unpack("<Q", struct.pack("<d", x))[0], cut, s, r))
        n_pass[g] = len(passing)
        for rank, (_, _, s, r) in enumerate(sorted(passing)[:K]):
            sel[g][rank] = r | s << 31
    return np.array(n_in, np.uint32), np.array(n_pass, np.uint32), np.array(sel, np.uint32).reshape(G, K)
