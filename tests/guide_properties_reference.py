"""The guide properties' definition (cropsr_amd/properties.py), stated twice for the tests: as a plain Python loop over
strings (window_loop / column_loop) and in numpy (column_numpy).  Plus the selection's reference extended by the five
property limits, again as a numpy statement (select_numpy) and as a plain loop (select_loop).

Per row of a contig's hit tables at guide length l.  The window is l characters of the contig string: s[i - l : i] for a
'+' row with match index i, s[j + 3 : j + 3 + l] for a '-' row with match index j; an index outside the string is a void
position.  A letter is a base when it is one of ACGT in either case, or U (which is A; lower-case u is not a base);
everything else, void included, is a non-base.
  gc     window letters that are C or G
  run    longest run of equal bases (0: no base)
  t_run  longest run of T ('+' row) or of A ('-' row) in the window
  stem   the largest s such that a, b exist with w[a + t] complementary to w[b - t] (A-T, C-G) for t < s and
         (b - s + 1) - (a + s) >= 3
  packed gc | run << 8 | t_run << 16 | stem << 24
"""
import numpy as np

NONE = 0xFFFFFFFF
BASE = {"A": "A", "U": "A", "T": "T", "C": "C", "G": "G", "a": "A", "t": "T", "c": "C", "g": "G"}
PAIR = {("A", "T"), ("T", "A"), ("C", "G"), ("G", "C")}


# ------------------------------------------------------------------------------------------------- the plain loop
def window(text, pos, minus, l):
    """The row's window as a list of l entries: 'A' / 'C' / 'G' / 'T' for a base, None for a non-base."""
    text = text.decode("latin-1") if isinstance(text, (bytes, bytearray)) else text
    start = pos + 3 if minus else pos - l
    return [BASE.get(text[k]) if 0 <= k < len(text) else None for k in range(start, start + l)]


def longest_run(w, of=None):
    """Longest run of equal bases in w (of: only runs of that base)."""
    best = cur = 0
    prev = None
    for ch in w:
        if ch is None or (of is not None and ch != of):
            cur, prev = 0, None
            continue
        cur = cur + 1 if ch == prev else 1
        prev = ch
        best = max(best, cur)
    return best


def stem_by_definition(w):
    """The definition itself: every a, b, s."""
    l = len(w)
    best = 0
    for a in range(l):
        for b in range(a, l):
            s = 0
            while a + s < l and b - s >= 0 and (w[a + s], w[b - s]) in PAIR and (b - (s + 1) + 1) - (a + (s + 1)) >= 3:
                s += 1
            best = max(best, s)
    return best


def stem_by_diagonals(w):
    """The equivalent form: over every anti-diagonal c = p + q the longest run in p of complementary (p, q), q - p >= 4."""
    l = len(w)
    best = 0
    for c in range(2 * l - 1):
        cur = 0
        for p in range(l):
            q = c - p
            cur = cur + 1 if 0 <= q < l and q - p >= 4 and (w[p], w[q]) in PAIR else 0
            best = max(best, cur)
    return best


def window_loop(w, minus):
    """(gc, run, t_run, stem) of one window (a list as window() returns it)."""
    return (sum(1 for ch in w if ch in ("C", "G")), longest_run(w), longest_run(w, "A" if minus else "T"), stem_by_definition(w))


def pack(values):
    gc, run, t_run, stem = values
    return gc | run << 8 | t_run << 16 | stem << 24


def column_loop(text, pos, minus, l):
    return np.array([pack(window_loop(window(text, int(p), minus, l), minus)) for p in pos], dtype=np.uint32)


# ------------------------------------------------------------------------------------------------- numpy
_CODE = np.full(256, 4, np.int8)  # 0 A, 1 T, 2 C, 3 G (the planes' codes), 4: non-base
for _ch, _b in BASE.items():
    _CODE[ord(_ch)] = "ATCG".index(_b)


def windows_numpy(text, pos, minus, l):
    """(n, l) int8 codes of the rows' windows; 4 marks a non-base (void positions too)."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    start = np.asarray(pos, np.int64) + 3 if minus else np.asarray(pos, np.int64) - l
    idx = start[:, None] + np.arange(l)[None, :]
    inside = (idx >= 0) & (idx < t.size)
    codes = _CODE[t[np.clip(idx, 0, max(t.size - 1, 0))]] if t.size else np.full(idx.shape, 4, np.int8)
    return np.where(inside, codes, np.int8(4))


def _longest_true_run(m):
    """Row-wise longest run of True of a 2-d boolean array."""
    n, l = m.shape
    best, cur = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for k in range(l):
        cur = np.where(m[:, k], cur + 1, 0)
        best = np.maximum(best, cur)
    return best


def column_numpy(text, pos, minus, l):
    w = windows_numpy(text, pos, minus, l)
    n = w.shape[0]
    base = w < 4
    gc = ((w == 2) | (w == 3)).sum(axis=1)
    run = np.zeros(n, np.int64)
    for code in range(4):
        run = np.maximum(run, _longest_true_run(w == code))
    t_run = _longest_true_run(w == (0 if minus else 1))
    stem = np.zeros(n, np.int64)
    comp = w ^ 1  # A <-> T, C <-> G: flip the low bit
    for c in range(4, 2 * l - 1):
        p = np.arange(l)
        q = c - p
        ok = (q < l) & (q - p >= 4)
        if not ok.any():
            continue
        p, q = p[ok], q[ok]  # (consecutive p: a run along the diagonal is a run of these columns)
        stem = np.maximum(stem, _longest_true_run(base[:, p] & base[:, q] & (comp[:, p] == w[:, q])))
    return (gc | run << 8 | t_run << 16 | stem << 24).astype(np.uint32)


# ------------------------------------------------------------------------------------------------- selection with limits
def limits_pass(packed, limits):
    """limits: (gc_min, gc_max, max_run, max_t_run, max_stem)."""
    p = np.asarray(packed, np.uint32).astype(np.int64)
    gc, run, t_run, stem = p & 255, p >> 8 & 255, p >> 16 & 255, p >> 24
    return (gc >= limits[0]) & (gc <= limits[1]) & (run <= limits[2]) & (t_run <= limits[3]) & (stem <= limits[4])


def select_numpy(tables, lo, hi, K, min_score=0.0, spec=None, cds=None, props=None, limits=None):
    """tests/select_reference.py's select_numpy with `passes` extended: props = dict(props_plus, props_minus) and limits
    given, a row passes only if limits_pass holds for it.  The property test is folded into the label-set test of the
    base statement: a row that fails it gets no label set."""
    import select_reference as base
    if limits is None:
        return base.select_numpy(tables, lo, hi, K, min_score, spec, cds)
    if cds is None:
        cds = dict(feat_plus=np.zeros(len(tables["pos_plus"]), np.uint32), feat_minus=np.zeros(len(tables["pos_minus"]), np.uint32),
                   flags=np.ones(1, np.uint8))
    folded = dict(flags=cds["flags"])
    for s in ("plus", "minus"):
        folded["feat_" + s] = np.where(limits_pass(props["props_" + s], limits), np.asarray(cds["feat_" + s], np.uint32), np.uint32(NONE))
    return base.select_numpy(tables, lo, hi, K, min_score, spec, folded)


def select_loop(tables, lo, hi, K, min_score=0.0, spec=None, cds=None, props=None, limits=None):
    """The whole definition as one plain loop over genes and rows."""
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
                if limits is not None:
                    v = int(props["props_" + name][r])
                    gc, run, t_run, stem = v & 255, v >> 8 & 255, v >> 16 & 255, v >> 24
                    if not (limits[0] <= gc <= limits[1] and run <= limits[2] and t_run <= limits[3] and stem <= limits[4]):
                        continue
                bits = struct.unpack("<Q", struct.pack("<d", x))[0]
                passing.append((-bits, cut, s, r))
        n_pass[g] = len(passing)
        for rank, (_, _, s, r) in enumerate(sorted(passing)[:K]):
            sel[g][rank] = r | s << 31
    return np.array(n_in, np.uint32), np.array(n_pass, np.uint32), np.array(sel, np.uint32).reshape(G, K)
