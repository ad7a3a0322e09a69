"""The restriction-site definition (cropsr_amd/sites.py, include/cropsr_hip.h), stated twice for the tests: as a plain loop
over strings (column_loop) and in numpy (column_numpy).  Neither calls the other or the package's sites.py.

The arena is a byte string: the texts' own characters at their arena positions, chr(0) (void) everywhere else; bounds is
[(t0, t1)] of the texts, ascending.  Enzymes are motifs, strings over the 15 IUPAC letters.

  base        A C G T a c g t, and U (packed as A); everything else -- N, IUPAC letters, u, Z, decoration, void, a position
              outside the string -- is a non-base and matches nothing, not even a motif N
  occurrence  of enzyme e at q: every letter of s[q : q + m] is a base in the motif letter's set, for M or for rc(M); once for a
              palindrome
  per row     c = i - 3 ('+') / j + 6 ('-'); g0 = i - l / j + 3; [t0, t1) the text that contains c
              in_guide bit e: an occurrence with g0 <= q and q + m <= g0 + l
              span_e: occurrences with c - m + 1 <= q <= c - 1;  amp_e: occurrences with max(c - A, t0) <= q, q + m <= min(c + A, t1)
              assay bit e: span_e >= 1 and amp_e == 1
              value = in_guide | assay << 32
"""
import numpy as np

IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT",
         "H": "ACT", "V": "ACG", "N": "ACGT"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
BASE_OF = {"A": "A", "C": "C", "G": "G", "T": "T", "a": "A", "c": "C", "g": "G", "t": "T", "U": "A"}


def clean(motif):
    return motif.upper().replace("U", "T")


def rc_loop(motif):
    """rc(M), letter by letter: the letter whose set is the complement of the letter's set, last letter first."""
    out = []
    for ch in reversed(clean(motif)):
        want = sorted(COMPLEMENT[b] for b in IUPAC[ch])
        out.append([k for k, v in IUPAC.items() if sorted(v) == want][0])
    return "".join(out)


# ------------------------------------------------------------------------------------------------------------- the loop
def _matches(arena, q, motif):
    for k, ch in enumerate(motif):
        p = q + k
        if p < 0 or p >= len(arena):
            return False
        b = BASE_OF.get(chr(arena[p]))
        if b is None or b not in IUPAC[ch]:
            return False
    return True


def occurs_loop(arena, q, motif):
    m = clean(motif)
    return _matches(arena, q, m) or _matches(arena, q, rc_loop(m))


def occurrences_loop(arena, motifs):
    """Per motif the list of flags: an occurrence starts at q, for every q of the arena."""
    out = []
    for motif in motifs:
        m = clean(motif)
        both = [m] if rc_loop(m) == m else [m, rc_loop(m)]  # (a palindrome occurring at q is one occurrence)
        out.append([any(_matches(arena, q, x) for x in both) for q in range(len(arena))])
    return out


def row_loop(occ, bounds, pos, minus, l, A, motifs):
    """(in_guide, assay, span [per enzyme], amp [per enzyme]) of one row; occ: occurrences_loop's lists."""
    p = int(pos)
    c, g0 = (p + 6, p + 3) if minus else (p - 3, p - l)
    text = [(t0, t1) for t0, t1 in bounds if t0 <= c < t1]
    in_guide = assay = 0
    spans, amps = [], []
    for e, motif in enumerate(motifs):
        m = len(motif)
        at = lambda q: 0 <= q < len(occ[e]) and occ[e][q]
        if any(at(q) for q in range(g0, g0 + l - m + 1)):
            in_guide |= 1 << e
        span = sum(1 for q in range(c - m + 1, c) if at(q))
        amp = 0
        if text:
            t0, t1 = text[0]
            amp = sum(1 for q in range(max(c - A, t0), min(c + A, t1) - m + 1) if at(q))
        if span >= 1 and amp == 1:
            assay |= 1 << e
        spans.append(span)
        amps.append(amp)
    return in_guide, assay, spans, amps


def column_loop(arena, bounds, pos, minus, l, A, motifs, occ=None):
    occ = occurrences_loop(arena, motifs) if occ is None else occ
    out = []
    for p in pos:
        in_guide, assay, _, _ = row_loop(occ, bounds, p, minus, l, A, motifs)
        out.append(in_guide | assay << 32)
    return np.array(out, np.uint64)


# ------------------------------------------------------------------------------------------------------------- numpy
_CODE = np.full(256, -1, np.int64)
for _ch, _b in BASE_OF.items():
    _CODE[ord(_ch)] = "ACGT".index(_b)


def occurrences_numpy(arena, motif):
    """Boolean array over the arena's positions: an occurrence of the motif (either strand) starts here."""
    code = _CODE[np.frombuffer(bytes(arena), np.uint8)]
    n = code.size
    m = len(motif)
    fwd = [np.array([b in IUPAC[ch] for b in "ACGT"]) for ch in clean(motif)]
    rev = [np.array([COMPLEMENT[b] in IUPAC[ch] for b in "ACGT"]) for ch in reversed(clean(motif))]
    out = np.zeros(n, bool)
    if n < m:
        return out
    for sets in (fwd, rev):
        ok = np.ones(n - m + 1, bool)
        for k, s in enumerate(sets):
            col = code[k:n - m + 1 + k]
            ok &= (col >= 0) & np.concatenate([s, [False]])[col]
        out[:n - m + 1] |= ok
    return out


def columns_numpy(arena, bounds, pos, minus, l, A, motifs):
    """dict(value (uint64), in_guide, assay (uint32), span, amp ((rows, E) int64)) of a table's rows."""
    p = np.asarray(pos, np.int64)
    n = len(arena)
    c, g0 = (p + 6, p + 3) if minus else (p - 3, p - l)
    starts = np.array([b[0] for b in bounds], np.int64)
    ends = np.array([b[1] for b in bounds], np.int64)
    k = np.searchsorted(starts, c, side="right") - 1
    inside = (k >= 0) & (c < ends[np.maximum(k, 0)]) if len(bounds) else np.zeros(p.size, bool)
    t0 = np.where(inside, starts[np.maximum(k, 0)], 0) if len(bounds) else np.zeros(p.size, np.int64)
    t1 = np.where(inside, ends[np.maximum(k, 0)], 0) if len(bounds) else np.zeros(p.size, np.int64)
    in_guide, assay = np.zeros(p.size, np.uint32), np.zeros(p.size, np.uint32)
    spans, amps = np.zeros((p.size, len(motifs)), np.int64), np.zeros((p.size, len(motifs)), np.int64)
    for e, motif in enumerate(motifs):
        m = len(motif)
        cum = np.concatenate([[0], np.cumsum(occurrences_numpy(arena, motif))])  # cum[x] = occurrences below x
        count = lambda lo, hi: np.where(hi > lo, cum[np.clip(hi, 0, n)] - cum[np.clip(np.minimum(lo, hi), 0, n)], 0)  # q in [lo, hi)
        guide = count(g0, g0 + l - m + 1)
        span = count(c - m + 1, c)
        amp = np.where(inside, count(np.maximum(c - A, t0), np.minimum(c + A, t1) - m + 1), 0)
        in_guide |= np.where(guide > 0, np.uint32(1 << e), np.uint32(0)).astype(np.uint32)
        assay |= np.where((span >= 1) & (amp == 1), np.uint32(1 << e), np.uint32(0)).astype(np.uint32)
        spans[:, e], amps[:, e] = span, amp
    return dict(value=in_guide.astype(np.uint64) | assay.astype(np.uint64) << np.uint64(32), in_guide=in_guide, assay=assay, span=spans, amp=amps)


def column_numpy(arena, bounds, pos, minus, l, A, motifs):
    return columns_numpy(arena, bounds, pos, minus, l, A, motifs)["value"]


# ------------------------------------------------------------------------------------------------------------- selection
def passes_numpy(col, forbid, need):
    col = np.asarray(col, np.uint64)
    in_guide, assay = col & np.uint64(0xFFFFFFFF), col >> np.uint64(32)
    ok = (in_guide & np.uint64(forbid)) == 0
    return ok & ((assay & np.uint64(need)) != 0) if need else ok


def passes_loop(col, forbid, need):
    out = []
    for v in col:
        v = int(v)
        ok = not (v & 0xFFFFFFFF) & forbid
        if need and not (v >> 32) & need:
            ok = False
        out.append(ok)
    return np.array(out, bool)
