"""The base-editing definition (cropsr_amd/baseedit.py), stated three times for the tests:

  outcome_loop    at the level of strings: the spliced coding string of the primary transcript P in the gene's orientation
                  with a letter-to-position map (sets of coordinates, select_coding_reference.model_loop), edited at the
                  targets and translated codon by codon;
  outcome_closed  the closed form over merged segments (model_numpy): where the edit reads C -> T in the gene's orientation,
                  CAA / CAG / CGA whose first letter is a window letter; where it reads G -> A, TGG with its second or third
                  letter in the window;
  outcome_subset  over the same segments: an evaluated codon that is no stop and becomes one when SOME non-empty subset of
                  its targets is converted.

An ARENA is a bytes object indexed by arena position (void positions hold a zero byte); a layout ROW is
select_coding_reference's (gene index, shift, text_lo, text_hi).  The selection with edit limits follows, as a plain loop
and in numpy.
"""
import itertools
import struct

import numpy as np

NONE = 0xFFFFFFFF
NO_STOP = 0xFFFFFFFF
STOPS = ("TAA", "TAG", "TGA")
BASE = {ord(c): b for c, b in zip("ACGTUacgtu", "ACGTAACGTA")}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
WINDOWS = ((4, 8), (1, 20), (1, 1), (20, 20), (13, 17))


def make_arena(texts, offsets):
    """The letters by arena position: every text at its offset, zero bytes elsewhere, one separator word behind the last."""
    out = bytearray(max(o + len(t) for t, o in zip(texts, offsets)) + 64)
    for t, o in zip(texts, offsets):
        out[o:o + len(t)] = bytes(t)
    return bytes(out)


def base(arena, x):
    return BASE.get(arena[x]) if 0 <= x < len(arena) else None


def window_positions(pos, minus, window):
    """Arena positions of the window's letters p = lo .. hi: i - 21 + p on a '+' row, j + 23 - p on a '-' row."""
    lo, hi = window
    return [int(pos) + 23 - p if minus else int(pos) - 21 + p for p in range(lo, hi + 1)]


def targets_of(arena, pos, minus, window):
    return [x for x in window_positions(pos, minus, window) if base(arena, x) == ("G" if minus else "C")]


# ------------------------------------------------------------------------------------------------ strings
_SPLICED = {}


def spliced(m, row, arena):
    """(P's coding string in the gene's orientation, '.' for a letter outside the row's text or a non-base; the arena
    position of every letter)."""
    key = (id(m), row, id(arena))
    if key not in _SPLICED:
        _, shift, lo, hi = row
        xs = sorted(p + shift for p in m["transcripts"][m["primary"]])
        if m["strand"] == "-":
            xs.reverse()
        letters = []
        for x in xs:
            b = base(arena, x) if lo <= x <= hi else None
            letters.append("." if b is None else (COMP[b] if m["strand"] == "-" else b))
        _SPLICED[key] = ("".join(letters), xs, {x: i for i, x in enumerate(xs)}, m, arena)  # (m and arena kept alive: their ids are the key)
    return _SPLICED[key][:3]


def outcome_loop(m, row, arena, pos, minus, window):
    """(targets, stops, stop_off); m in select_coding_reference's loop form."""
    targets = targets_of(arena, pos, minus, window)
    if not m["model"]:
        return len(targets), 0, NO_STOP
    s, xs, where = spliced(m, row, arena)
    edited = list(s)
    to = "A" if minus else "T"
    for x in targets:
        if x in where and s[where[x]] != ".":
            edited[where[x]] = COMP[to] if m["strand"] == "-" else to
    found = []
    for q in sorted({where[x] // 3 for x in targets if x in where}):  # (a codon without a target stays what it is)
        if 3 * q + 2 >= len(s):
            continue
        step = xs[3 * q + 1] - xs[3 * q]
        if abs(step) != 1 or xs[3 * q + 2] - xs[3 * q + 1] != step:
            continue
        before, after = s[3 * q:3 * q + 3], "".join(edited[3 * q:3 * q + 3])
        if "." not in before and before not in STOPS and after in STOPS:
            found.append(3 * q)
    return len(targets), len(found), min(found, default=NO_STOP)


# ------------------------------------------------------------------------------------------------ segments
def _index(m, row):
    """x -> the coding index of letter x in the gene's orientation, or None: over the merged segments of P."""
    _, shift, lo, hi = row
    start, end = m["transcripts"][m["primary"]]
    a, b = start + shift, end + shift
    below = np.concatenate([[0], np.cumsum(end - start + 1)])

    def index(x):
        if not lo <= x <= hi:
            return None
        k = int(np.searchsorted(a, x, "right")) - 1
        if k < 0 or x > b[k]:
            return None
        c = int(below[k]) + x - int(a[k])
        return m["length"] - 1 - c if m["strand"] == "-" else c
    return index


def _codon(m, row, arena, index, x):
    """The evaluated codon whose first letter (in the gene's orientation) is x: (3 q, its letters' positions, its string), or
    None."""
    i = index(x)
    if i is None or i % 3 or i + 2 >= m["length"]:
        return None
    step = -1 if m["strand"] == "-" else 1
    xs = [x, x + step, x + 2 * step]
    if [index(y) for y in xs] != [i, i + 1, i + 2] or any(base(arena, y) is None for y in xs):
        return None
    read = (lambda c: COMP[c]) if m["strand"] == "-" else (lambda c: c)
    return i, xs, "".join(read(base(arena, y)) for y in xs)


def outcome_closed(m, row, arena, pos, minus, window):
    """(targets, stops, stop_off) by the closed form; m in the numpy form."""
    targets = targets_of(arena, pos, minus, window)
    if not m["model"]:
        return len(targets), 0, NO_STOP
    index = _index(m, row)
    letters = window_positions(pos, minus, window)
    step = -1 if m["strand"] == "-" else 1
    found = set()
    if (m["strand"] == "-") == bool(minus):  # the edit reads C -> T in the gene's orientation
        for x in letters:
            c = _codon(m, row, arena, index, x)
            if c is not None and c[2] in ("CAA", "CAG", "CGA"):
                found.add(c[0])
    else:                                    # it reads G -> A
        for x in sorted({w - step for w in letters} | {w - 2 * step for w in letters}):
            c = _codon(m, row, arena, index, x)
            if c is not None and c[2] == "TGG" and (c[1][1] in letters or c[1][2] in letters):
                found.add(c[0])
    return len(targets), len(found), min(found, default=NO_STOP)


def outcome_subset(m, row, arena, pos, minus, window):
    """(targets, stops, stop_off): a codon counts when some non-empty subset of its targets, converted, makes it a stop."""
    targets = targets_of(arena, pos, minus, window)
    if not m["model"]:
        return len(targets), 0, NO_STOP
    index = _index(m, row)
    letters = window_positions(pos, minus, window)
    to = "A" if minus else "T"
    to = COMP[to] if m["strand"] == "-" else to
    found = set()
    for x in range(min(letters) - 2, max(letters) + 3):
        c = _codon(m, row, arena, index, x)
        if c is None or c[2] in STOPS:
            continue
        mine = [j for j, y in enumerate(c[1]) if y in targets]
        for n in range(1, len(mine) + 1):
            for subset in itertools.combinations(mine, n):
                if "".join(to if j in subset else ch for j, ch in enumerate(c[2])) in STOPS:
                    found.add(c[0])
    return len(targets), len(found), min(found, default=NO_STOP)


# ------------------------------------------------------------------------------------------------ the selection
def passes(limits, targets, stop_off, length):
    """The edit limits in Python's exact integers: limits = (min_pct, max_pct, max_targets)."""
    lo, hi, most = limits
    return stop_off != NO_STOP and lo * int(length) <= 100 * int(stop_off) <= hi * int(length) and int(targets) <= most


def rows_of(tables):
    """(pos, strand) of both tables' rows: '+' rows, then '-' rows."""
    n_plus, n_minus = len(tables["pos_plus"]), len(tables["pos_minus"])
    pos = np.concatenate([np.asarray(tables["pos_plus"], np.int64), np.asarray(tables["pos_minus"], np.int64)])
    return pos, np.concatenate([np.zeros(n_plus, np.int64), np.ones(n_minus, np.int64)])


def outcomes(tables, member, models, rows, arena, window, statement=outcome_closed):
    """Per layout row g: (at, targets, stops, stop_off) -- at: the rows of both tables IN the gene ('+' rows, then '-' rows),
    the three others their outcomes for that gene."""
    pos, strand = rows_of(tables)
    out = []
    for g, row in enumerate(rows):
        at = np.flatnonzero(member[g])
        res = [statement(models[row[0]], row, arena, int(pos[r]), bool(strand[r]), window) for r in at]
        out.append((at,) + tuple(np.array([v[j] for v in res], np.uint32) for j in range(3)))
    return out


def select_numpy(tables, member, models, rows, K, per_gene, limits=None, ok=None):
    """(n_in, n_pass, sel) per layout row.  member: select_coding_reference.membership; per_gene: outcomes(); limits: None or
    the three bounds; ok: None or a boolean per table row -- everything else the predicate asks."""
    G = len(rows)
    score = np.concatenate([tables["score_plus"], tables["score_minus"]]).astype(np.float64)
    pos, strand = rows_of(tables)
    n_plus = len(tables["pos_plus"])
    row = np.where(strand == 0, np.arange(pos.size), np.arange(pos.size) - n_plus)
    cut = pos - np.where(strand == 0, 3, 0)
    key = score.view(np.uint64)
    n_in, n_pass, sel = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.full((G, K), NONE, np.uint32)
    for g in range(G):
        at, targets, _, off = per_gene[g]
        good = np.ones(at.size, bool) if ok is None else np.asarray(ok, bool)[at]
        if limits is not None:
            L = int(models[rows[g][0]]["length"])
            off64 = off.astype(np.uint64)  # (100 off < 2^39)
            good = good & (off != NO_STOP) & (np.uint64(limits[0] * L) <= np.uint64(100) * off64) & (np.uint64(100) * off64 <= np.uint64(limits[1] * L)) \
                & (targets <= limits[2])
        passing = at[good]
        n_in[g], n_pass[g] = at.size, passing.size
        order = np.lexsort((strand[passing], cut[passing], np.iinfo(np.uint64).max - key[passing]))[:K]
        best = passing[order]
        sel[g, :best.size] = (row[best] | (strand[best] << 31)).astype(np.uint32)
    return n_in, n_pass, sel


def select_loop(tables, lo, hi, models, rows, arena, window, K, limits=None, ok=None):
    """(n_in, n_pass, sel) by the plain loop; models in the loop form, outcomes by the string statement."""
    G = len(rows)
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
                    targets, _, off = outcome_loop(m, rows[g], arena, int(pos[r]), bool(s), window)
                    if not passes(limits, targets, off, m["length"]):
                        continue
                passing.append((-struct.unpack("<Q", struct.pack("<d", x))[0], cut, s, r))
        n_pass[g] = len(passing)
        for rank, (_, _, s, r) in enumerate(sorted(passing)[:K]):
            sel[g][rank] = r | s << 31
    return np.array(n_in, np.uint32), np.array(n_pass, np.uint32), np.array(sel, np.uint32).reshape(G, K)
