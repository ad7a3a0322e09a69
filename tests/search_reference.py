"""CPU reference of the off-target search of given guides (cropsr_amd/search.py states the definition).

Vectorised over window starts with stride tricks: every contig's characters become codes (0..3 = A C G T, U read as A;
4 = not a base), the T-character windows are a strided view, the '-' windows their reversed complement; the pattern
keeps the windows whose letters are in its sets, and each query's mismatches are counted on those.  `search_slow`
states the same definition character by character; the CPU tests hold the two against each other.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

IUPAC_SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
              "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG"}
CODE = np.full(256, 4, dtype=np.uint8)
for _c, _v in zip(b"ACGTUacgt", (0, 1, 2, 3, 0, 0, 1, 2, 3)):
    CODE[_c] = _v
COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
SITE_FIELDS = ("query", "contig", "position", "strand", "mismatches")


def _allowed(pattern):
    """(T, 5) bool: which codes each pattern position accepts (N: all five)."""
    T = len(pattern)
    ok = np.zeros((T, 5), dtype=bool)
    for p, c in enumerate(pattern.upper()):
        if c == "N":
            ok[p, :] = True
        else:
            for b in IUPAC_SETS[c]:
                ok[p, "ACGT".index(b)] = True
    return ok


def _as_bytes(c):
    return c.encode() if isinstance(c, str) else bytes(c)


def candidates(contigs, pattern):
    """[(contig, position, strand 0/1, oriented codes (T,))...] as arrays: contig, position, strand, windows (m, T)."""
    T = len(pattern)
    ok = _allowed(pattern)
    cols = ([], [], [], [])
    for k, c in enumerate(contigs):
        codes = CODE[np.frombuffer(_as_bytes(c), dtype=np.uint8)]
        if codes.size < T:
            continue
        W = sliding_window_view(codes, T)
        for strand, O in ((0, W), (1, COMP[W[:, ::-1]])):
            keep = ok[np.arange(T), O].all(axis=1)
            idx = np.nonzero(keep)[0]
            cols[0].append(np.full(idx.size, k, dtype=np.int64))
            cols[1].append(idx.astype(np.int64))
            cols[2].append(np.full(idx.size, strand, dtype=np.int64))
            cols[3].append(O[idx])
    if not cols[0]:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, T), np.uint8)
    return tuple(np.concatenate(x) for x in cols)


def _pack(codes):
    """(m, T) codes -> three uint32 fields, bit p = position p: code bit 1, code bit 0, not a base."""
    w = (np.uint64(1) << np.arange(codes.shape[1], dtype=np.uint64))
    hi = (((codes >> 1) & 1).astype(np.uint64) * w).sum(axis=1, dtype=np.uint64)
    lo = ((codes & 1).astype(np.uint64) * w).sum(axis=1, dtype=np.uint64)
    nb = ((codes == 4).astype(np.uint64) * w).sum(axis=1, dtype=np.uint64)
    return hi, lo, nb


def search(contigs, pattern, queries, max_mm):
    """(counts (Q, M + 1) uint32, sites: dict of arrays in SITE_FIELDS, ordered by query, contig, position, strand)."""
    k, pos, strand, O = candidates(contigs, pattern)
    order = np.lexsort((strand, pos, k))
    k, pos, strand, O = k[order], pos[order], strand[order], O[order]
    hi, lo, nb = _pack(O)
    qc = np.array([[CODE[ord(ch)] for ch in q.upper()] for q in queries], dtype=np.uint8).reshape(len(queries), len(pattern))
    qmask = (qc != 4).astype(np.uint64) @ (np.uint64(1) << np.arange(len(pattern), dtype=np.uint64)) if len(queries) else []
    qh, ql, _ = _pack(np.where(qc == 4, 0, qc)) if len(queries) else ([], [], [])
    counts = np.zeros((len(queries), max_mm + 1), dtype=np.uint32)
    out = {f: [] for f in SITE_FIELDS}
    for q in range(len(queries)):
        mm = np.bitwise_count(((hi ^ qh[q]) | (lo ^ ql[q]) | nb) & qmask[q]).astype(np.int64)
        sel = np.nonzero(mm <= max_mm)[0]
        counts[q] = np.bincount(mm[sel], minlength=max_mm + 1)[:max_mm + 1]
        out["query"].append(np.full(sel.size, q, dtype=np.int64))
        out["contig"].append(k[sel])
        out["position"].append(pos[sel])
        out["strand"].append(strand[sel])
        out["mismatches"].append(mm[sel])
    sites = {f: (np.concatenate(v) if v else np.zeros(0, np.int64)) for f, v in out.items()}
    return counts, sites


def search_slow(contigs, pattern, queries, max_mm):
    """The definition character by character, in plain Python: sorted list of (query, contig, position, strand, mm)."""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    pattern = pattern.upper()
    T = len(pattern)

    def base(ch):  # the arena alphabet: acgtACGT, U read as A
        return "A" if ch == "U" else (ch.upper() if ch in "ACGTacgt" else None)

    out = []
    for q, query in enumerate(queries):
        query = query.upper()
        for k, c in enumerate(contigs):
            s = _as_bytes(c).decode("latin-1")
            for i in range(len(s) - T + 1):
                fwd = [base(ch) for ch in s[i:i + T]]
                for strand, win in ((0, fwd), (1, [None if b is None else comp[b] for b in reversed(fwd)])):
                    if any(pattern[p] != "N" and (win[p] is None or win[p] not in IUPAC_SETS[pattern[p]]) for p in range(T)):
                        continue
                    mm = sum(1 for p in range(T) if query[p] != "N" and win[p] != query[p])
                    if mm <= max_mm:
                        out.append((q, k, i, strand, mm))
    return sorted(out)
