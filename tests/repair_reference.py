"""The repair scores' definition (cropsr_amd/repair.py), stated twice for the tests: as an enumerate-and-drop loop over
strings (score_enumerate / column_loop) and in the diagonal form, on Python integers the way the kernel computes it
(score_diagonals) and vectorised in numpy (column_numpy).  Plus the selection's reference extended by the two repair
limits, again as a numpy statement (select_numpy) and as a plain loop (select_loop).

Per row of a contig's hit tables; the guide length is not used.  F is the flank, 2 <= F <= 32.
  cut      the boundary c between s[c - 1] and s[c]: c = i - 3 for a '+' row with match index i, c = j + 6 for a '-' row
  window   w[p] = s[c - F + p], p = 0 .. 2 F - 1; an index outside the string is a void position.  A letter is a base when
           it is one of ACGT in either case, or U (which is A; lower-case u is not a base); everything else is a non-base
  pattern  (k >= 2, i, j) with w[i : i + k] == w[j : j + k], all bases, i + k <= F, j >= F, j + k <= 2 F; longest first,
           a pattern nested in a kept one with the same j - i is dropped; a kept one adds W[j - i] (k + its C and G)
  result   mh = the sum; oof = the sum over patterns whose j - i is no multiple of 3; packed mh | oof << 32
The weights W[d] are written out here from the formula floor(1000 exp(-d / 20) + 1/2); the test holds the library's
committed table to them.
"""
import math

import numpy as np

NONE = 0xFFFFFFFF
BASE = {"A": "A", "U": "A", "T": "T", "C": "C", "G": "G", "a": "A", "t": "T", "c": "C", "g": "G"}
W = [0] + [int(math.floor(1000.0 * math.exp(-d / 20.0) + 0.5)) for d in range(1, 64)]  # W[d]


def cut(pos, minus):
    return pos + 6 if minus else pos - 3


def window(text, pos, minus, F):
    """The row's window as a list of 2 F entries: 'A' / 'C' / 'G' / 'T' for a base, None for a non-base."""
    text = text.decode("latin-1") if isinstance(text, (bytes, bytearray)) else text
    start = cut(pos, minus) - F
    return [BASE.get(text[k]) if 0 <= k < len(text) else None for k in range(start, start + 2 * F)]


def as_window(text):
    return [BASE.get(ch) for ch in text]


# ------------------------------------------------------------------------------------------------- enumerate and drop
def score_enumerate(w, F):
    """(mh, oof) of one window (a list of 2 F entries) by the pattern statement."""
    assert len(w) == 2 * F
    kept = []
    for k in range(F, 1, -1):  # longest first
        for i in range(0, F - k + 1):
            if any(ch is None for ch in w[i:i + k]):
                continue
            for j in range(F, 2 * F - k + 1):
                if w[i:i + k] != w[j:j + k]:
                    continue
                if any(j - i == J - I and I <= i and i + k <= I + K for K, I, J in kept):
                    continue  # nested in a kept pattern on the same diagonal
                kept.append((k, i, j))
    mh = oof = 0
    for k, i, j in kept:
        v = W[j - i] * (k + sum(1 for ch in w[i:i + k] if ch in ("C", "G")))
        mh += v
        if (j - i) % 3:
            oof += v
    return mh, oof


def column_loop(text, pos, minus, F):
    out = []
    for p in pos:
        mh, oof = score_enumerate(window(text, int(p), minus, F), F)
        out.append(mh | oof << 32)
    return np.array(out, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------- diagonals, on integers
def planes_of(w):
    """(AC, H, L) of a window as integers, bit p = letter p; codes A=00 T=01 C=10 G=11, H and L masked by AC."""
    ac = h = l = 0
    for p, ch in enumerate(w):
        if ch is None:
            continue
        code = "ATCG".index(ch)
        ac |= 1 << p
        h |= (code >> 1) << p
        l |= (code & 1) << p
    return ac, h, l


def score_diagonals(w, F):
    """(mh, oof) by the diagonal form: per d, M = ~(H ^ H >> d) & ~(L ^ L >> d) & AC & AC >> d & range_d, the letters of
    runs of two and more R = M & (M >> 1 | M << 1), n_d = popcount(R) + popcount(R & H)."""
    ac, h, l = planes_of(w)
    full = (1 << 64) - 1
    mh = oof = 0
    for d in range(1, 2 * F):
        lo, hi = max(0, F - d), min(F, 2 * F - d)
        rng = ((1 << hi) - 1) & ~((1 << lo) - 1)
        m = (~(h ^ h >> d) & ~(l ^ l >> d) & ac & ac >> d & rng) & full
        r = m & (m >> 1 | m << 1)
        n = bin(r).count("1") + bin(r & h).count("1")
        mh += W[d] * n
        if d % 3:
            oof += W[d] * n
    return mh, oof


# ------------------------------------------------------------------------------------------------- numpy
_CODE = np.full(256, 4, np.int8)  # 0 A, 1 T, 2 C, 3 G (the planes' codes), 4: non-base
for _ch, _b in BASE.items():
    _CODE[ord(_ch)] = "ATCG".index(_b)


def windows_numpy(text, pos, minus, F):
    """(n, 2 F) int8 codes of the rows' windows; 4 marks a non-base (void positions too)."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    c = np.asarray(pos, np.int64) + (6 if minus else -3)
    idx = c[:, None] - F + np.arange(2 * F)[None, :]
    inside = (idx >= 0) & (idx < t.size)
    codes = _CODE[t[np.clip(idx, 0, max(t.size - 1, 0))]] if t.size else np.full(idx.shape, 4, np.int8)
    return np.where(inside, codes, np.int8(4))


def column_numpy(text, pos, minus, F):
    w = windows_numpy(text, pos, minus, F)
    n = w.shape[0]
    mh, oof = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for d in range(1, 2 * F):
        lo, hi = max(0, F - d), min(F, 2 * F - d)
        a, b = w[:, lo:hi], w[:, lo + d:hi + d]
        m = (a == b) & (a < 4)
        pad = np.zeros((n, 1), bool)
        r = m & (np.concatenate([pad, m[:, :-1]], axis=1) | np.concatenate([m[:, 1:], pad], axis=1))
        n_d = r.sum(axis=1) + (r & (a >= 2)).sum(axis=1)
        mh += W[d] * n_d
        if d % 3:
            oof += W[d] * n_d
    return mh.astype(np.uint64) | oof.astype(np.uint64) << np.uint64(32)


# ------------------------------------------------------------------------------------------------- selection with limits
def limits_pass(col, limits):
    """limits: (min_mh in tenths, min_oof in percent)."""
    c = np.asarray(col, np.uint64)
    mh, oof = (c & np.uint64(0xFFFFFFFF)).astype(np.int64), (c >> np.uint64(32)).astype(np.int64)
    return (mh >= limits[0]) & (100 * oof >= limits[1] * mh) & ((mh > 0) | (limits[1] == 0))


def select_numpy(tables, lo, hi, K, min_score=0.0, spec=None, cds=None, repair=None, limits=None, also=None):
    """tests/select_reference.py's select_numpy with `passes` extended: repair = dict(repair_plus, repair_minus) and
    limits given, a row passes only if limits_pass holds for it; also = dict(plus, minus) of boolean arrays: further
    conditions per row (the property limits).  The tests are folded into the label-set test of the base statement: a
    row that fails one gets no label set."""
    import select_reference as base
    if limits is None and also is None:
        return base.select_numpy(tables, lo, hi, K, min_score, spec, cds)
    if cds is None:
        cds = dict(feat_plus=np.zeros(len(tables["pos_plus"]), np.uint32), feat_minus=np.zeros(len(tables["pos_minus"]), np.uint32),
                   flags=np.ones(1, np.uint8))
    folded = dict(flags=cds["flags"])
    for s in ("plus", "minus"):
        ok = np.ones(len(tables["pos_" + s]), bool)
        if limits is not None:
            ok &= limits_pass(repair["repair_" + s], limits)
        if also is not None:
            ok &= np.asarray(also[s], bool)
        folded["feat_" + s] = np.where(ok, np.asarray(cds["feat_" + s], np.uint32), np.uint32(NONE))
    return base.select_numpy(tables, lo, hi, K, min_score, spec, folded)


def select_loop(tables, lo, hi, K, min_score=0.0, repair=None, limits=None):
    """The definition with repair limits as one plain loop over genes and rows (no joined columns, no CDS filter)."""
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
                c = int(pos[r]) - 3 if s == 0 else int(pos[r])
                if not int(lo[g]) <= c <= int(hi[g]):
                    continue
                n_in[g] += 1
                if not x >= float(min_score):
                    continue
                if limits is not None:
                    v = int(repair["repair_" + name][r])
                    mh, oof = v & 0xFFFFFFFF, v >> 32
                    if mh < limits[0] or 100 * oof < limits[1] * mh or (limits[1] > 0 and mh == 0):
                        continue
                bits = struct.unpack("<Q", struct.pack("<d", x))[0]
                passing.append((-bits, c, s, r))
        n_pass[g] = len(passing)
        for rank, (_, _, s, r) in enumerate(sorted(passing)[:K]):
            sel[g][rank] = r | s << 31
    return np.array(n_in, np.uint32), np.array(n_pass, np.uint32), np.array(sel, np.uint32).reshape(G, K)
