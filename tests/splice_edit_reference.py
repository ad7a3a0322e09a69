"""The splice-site definition (cropsr_amd/baseedit.py), stated for the tests from GFF lines, not from
the step function:

  outcome_loop    at the level of strings: the spliced coding string of the primary transcript P in the gene's orientation
                  with a letter-to-position map (sets of coordinates, select_coding_reference.model_loop).  Two neighbours of
                  that string whose positions are not adjacent have an intron between them; its donor is the two letters 3'
                  of the first, its acceptor the two letters 5' of the second, read in the gene's orientation;
  outcome_masks   the closed form over merged segments (model_numpy) as boolean arrays over the arena: coding, its shifts,
                  cum_P as a running sum, the letters as codes; `sites` holds what they give per layout row;
  outcomes        outcome_masks for all rows of a gene at once.

An ARENA is a bytes object indexed by arena position (void positions hold a zero byte); a layout ROW is
select_coding_reference's (gene index, shift, text_lo, text_hi); an EDITOR is "cbe" or "abe".  The selection with splice
limits -- alone or as the alternative to the stop limits -- follows, as a plain loop and in numpy.
"""
import struct

import numpy as np

import base_edit_reference as eref

NONE = 0xFFFFFFFF
NO_SITE = 0xFFFFFFFF
WINDOWS = eref.WINDOWS
EDITORS = ("cbe", "abe")
KINDS = {"donor": (0,), "acceptor": (1,), "any": (0, 1)}
SOURCE = {("cbe", False): "C", ("cbe", True): "G", ("abe", False): "A", ("abe", True): "T"}  # (editor, '-' row) -> the forward letter converted
base = eref.base
window_positions = eref.window_positions


def targets_of(arena, pos, minus, window, editor):
    return [x for x in window_positions(pos, minus, window) if base(arena, x) == SOURCE[editor, bool(minus)]]


# ------------------------------------------------------------------------------------------------ strings
_INTRONS = {}


def introns(m, row, arena):
    """[(coding letters 5' of the intron, donor or None, acceptor or None)] of P in the gene's orientation; a site is (the
    positions of its two letters, its two letters read in the gene's orientation), None where the exon letter next to it
    lies outside the row's text or one of its letters is a coding letter of P."""
    key = (id(m), row, id(arena))
    if key not in _INTRONS:
        _, shift, lo, hi = row
        s, xs, where = eref.spliced(m, row, arena)
        d = -1 if m["strand"] == "-" else 1

        def read(x):
            b = base(arena, x) if lo <= x <= hi else None
            return "." if b is None else (eref.COMP[b] if m["strand"] == "-" else b)

        out = []
        for i in range(len(xs) - 1):
            if xs[i + 1] - xs[i] == d:
                continue
            sites = []
            for exon_letter, pair in ((xs[i], (xs[i] + d, xs[i] + 2 * d)), (xs[i + 1], (xs[i + 1] - 2 * d, xs[i + 1] - d))):
                ok = lo <= exon_letter <= hi and pair[0] not in where and pair[1] not in where
                sites.append((pair, read(pair[0]) + read(pair[1])) if ok else None)
            out.append((i + 1, sites[0], sites[1]))
        _INTRONS[key] = (out, m, arena)  # (m and arena kept alive: their ids are the key)
    return _INTRONS[key][0]


def outcome_loop(m, row, arena, pos, minus, window, editor):
    """(targets, donors, acceptors, donor_off, acceptor_off); m in select_coding_reference's loop form."""
    targets = targets_of(arena, pos, minus, window, editor)
    if not m["model"] or not targets:
        return len(targets), 0, 0, NO_SITE, NO_SITE
    found = ([], [])
    for before, donor, acceptor in introns(m, row, arena):
        for kind, site, canon in ((0, donor, "GT"), (1, acceptor, "AG")):
            if site is not None and site[1] == canon and (site[0][0] in targets or site[0][1] in targets):
                found[kind].append(before)
    return len(targets), len(found[0]), len(found[1]), min(found[0], default=NO_SITE), min(found[1], default=NO_SITE)


# ------------------------------------------------------------------------------------------------ masks
_CODES, _SITES = {}, {}
_CODE = np.full(256, 4, np.int8)
for _c, _v in zip(b"ACGTUacgtu", (0, 1, 2, 3, 0, 0, 1, 2, 3, 0)):
    _CODE[_c] = _v


def codes(arena):
    """The letters as codes A 0, C 1, G 2, T 3, non-base 4, with 4 non-bases in front and behind: index = position + 4."""
    if id(arena) not in _CODES:
        _CODES[id(arena)] = (np.concatenate([np.full(4, 4, np.int8), _CODE[np.frombuffer(arena, np.uint8)], np.full(4, 4, np.int8)]), arena)
    return _CODES[id(arena)][0]


def sites(m, row, arena):
    """(lower letter, kind 0 donor / 1 acceptor, off) arrays of the EVALUATED sites of P inside the row's text, whatever the
    editor: the closed-form masks over the text's positions; m in the numpy form."""
    key = (id(m), row, id(arena))
    if key not in _SITES:
        _, shift, lo, hi = row
        empty = (np.empty(0, np.int64),) * 3
        if not m["model"]:
            _SITES[key] = (empty, m, arena)
            return empty
        start, end = m["transcripts"][m["primary"]]
        a, b, L = start + shift, end + shift, int(m["length"])
        # positions lo - 3 .. hi + 3, index = position - lo + 3; outside the text nothing is a coding letter
        n = hi - lo + 7
        coding = np.zeros(n, bool)
        for x, y in zip(a.tolist(), b.tolist()):
            x, y = max(x, lo), min(y, hi)
            if x <= y:
                coding[x - lo + 3:y - lo + 4] = True
        before = int(np.clip(lo - a, 0, b - a + 1).sum())  # P's letters below the text
        cum = before + np.concatenate([[0], np.cumsum(coding)[:-1]])  # cum_P at the boundary below each position
        full, idx = codes(arena), np.arange(lo - 3, hi + 4) + 4
        code = np.where((idx >= lo + 4) & (idx <= hi + 4) & (idx < len(full)), full[np.clip(idx, 0, len(full) - 1)], 4)  # a letter outside the text is no base
        minus = m["strand"] == "-"
        sh = lambda v, k: np.concatenate([v[k:], np.zeros(k, v.dtype)]) if k >= 0 else np.concatenate([np.zeros(-k, v.dtype), v[:k]])  # v at position + k
        starts = sh(coding, -1) & ~coding & (cum < L)
        ends = ~sh(coding, -1) & coding & (cum > 0)
        first, second = ((1, 3) if minus else (2, 3)), ((0, 1) if minus else (0, 2))  # forward CT / GT opens, AC / AG closes
        start_site = starts & ~sh(coding, 1) & (code == first[0]) & (sh(code, 1) == first[1])
        end_site = sh(ends, 2) & ~coding & ~sh(coding, 1) & (code == second[0]) & (sh(code, 1) == second[1])
        lower = np.concatenate([np.flatnonzero(start_site), np.flatnonzero(end_site)])
        kind = np.concatenate([np.full(int(start_site.sum()), int(minus)), np.full(int(end_site.sum()), int(not minus))])
        at_boundary = np.concatenate([cum[start_site], sh(cum, 2)[end_site]])
        off = L - at_boundary if minus else at_boundary
        _SITES[key] = ((lower + lo - 3, kind.astype(np.int64), off.astype(np.int64)), m, arena)
    return _SITES[key][0]


def outcomes_of(m, row, arena, pos, minus, window, editor):
    """The five outcome arrays (uint32) of rows with match indices pos and strands minus (arrays) for one gene's layout row."""
    pos, minus = np.asarray(pos, np.int64), np.asarray(minus, bool)
    lo, hi = window
    wlo, whi = np.where(minus, pos + 23 - hi, pos - 21 + lo), np.where(minus, pos + 23 - lo, pos - 21 + hi)
    code = codes(arena)
    n = len(code)
    want = {"cbe": (1, 2), "abe": (0, 3)}[editor]  # the code converted on a '+' row, on a '-' row
    src = np.where(minus, want[1], want[0])
    count = {c: np.concatenate([[0], np.cumsum(code == c)]) for c in want}
    clip = lambda v: np.clip(v + 4, 0, n)
    targets = np.where(minus, count[want[1]][clip(whi + 1)] - count[want[1]][clip(wlo)], count[want[0]][clip(whi + 1)] - count[want[0]][clip(wlo)])
    lower, kind, off = sites(m, row, arena)
    num = [np.zeros(pos.size, np.int64), np.zeros(pos.size, np.int64)]
    best = [np.full(pos.size, NO_SITE, np.int64), np.full(pos.size, NO_SITE, np.int64)]
    for a, k, o in zip(lower.tolist(), kind.tolist(), off.tolist()):
        hit = np.zeros(pos.size, bool)
        for x in (a, a + 1):
            hit |= (wlo <= x) & (x <= whi) & (code[x + 4] == src)
        num[k] += hit
        best[k] = np.where(hit, np.minimum(best[k], o), best[k])
    return tuple(v.astype(np.uint32) for v in (targets, num[0], num[1], best[0], best[1]))


def outcome_masks(m, row, arena, pos, minus, window, editor):
    return tuple(int(v[0]) for v in outcomes_of(m, row, arena, [pos], [minus], window, editor))


# ------------------------------------------------------------------------------------------------ the selection
def passes(limits, out, length):
    """The splice limits in Python's exact integers: limits = (min_pct, max_pct, max_targets, kinds' name); out: the five."""
    lo, hi, most, kinds = limits
    return int(out[0]) <= most and any(int(out[3 + k]) != NO_SITE and lo * int(length) <= 100 * int(out[3 + k]) <= hi * int(length) for k in KINDS[kinds])


def passes_numpy(limits, out, length):
    lo, hi, most, kinds = limits
    L = int(length)
    ok = np.zeros(out[0].shape, bool)
    for k in KINDS[kinds]:
        off = out[3 + k].astype(np.uint64)  # (100 off < 2^39)
        ok |= (out[3 + k] != NO_SITE) & (np.uint64(lo * L) <= np.uint64(100) * off) & (np.uint64(100) * off <= np.uint64(hi * L))
    return ok & (out[0] <= most)


def outcomes(tables, member, models, rows, arena, window, editor):
    """Per layout row g: (at, the five outcome arrays) -- at: the rows of both tables IN the gene ('+' rows, then '-' rows)."""
    pos, strand = eref.rows_of(tables)
    out = []
    for g, row in enumerate(rows):
        at = np.flatnonzero(member[g])
        out.append((at,) + outcomes_of(models[row[0]], row, arena, pos[at], strand[at] != 0, window, editor))
    return out


def select_numpy(tables, member, models, rows, K, per_gene, limits=None, ok=None, stop=None):
    """(n_in, n_pass, sel) per layout row.  per_gene: outcomes() over `member`; limits: None or the four bounds; ok: None or a
    boolean per table row -- everything else the predicate asks; stop: None, or (per-gene outcomes of
    base_edit_reference.outcomes over the same member, the three stop limits): the alternative."""
    G = len(rows)
    score = np.concatenate([tables["score_plus"], tables["score_minus"]]).astype(np.float64)
    pos, strand = eref.rows_of(tables)
    n_plus = len(tables["pos_plus"])
    row = np.where(strand == 0, np.arange(pos.size), np.arange(pos.size) - n_plus)
    cut = pos - np.where(strand == 0, 3, 0)
    key = score.view(np.uint64)
    n_in, n_pass, sel = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.full((G, K), NONE, np.uint32)
    for g in range(G):
        at = per_gene[g][0]
        good = np.ones(at.size, bool) if ok is None else np.asarray(ok, bool)[at]
        if limits is not None:
            L = int(models[rows[g][0]]["length"])
            test = passes_numpy(limits, per_gene[g][1:], L)
            if stop is not None:
                s_at, s_targets, _, s_off = stop[0][g]
                assert np.array_equal(s_at, at)
                off64 = s_off.astype(np.uint64)
                test = test | ((s_off != eref.NO_STOP) & (np.uint64(stop[1][0] * L) <= np.uint64(100) * off64)
                               & (np.uint64(100) * off64 <= np.uint64(stop[1][1] * L)) & (s_targets <= stop[1][2]))
            good = good & test
        passing = at[good]
        n_in[g], n_pass[g] = at.size, passing.size
        order = np.lexsort((strand[passing], cut[passing], np.iinfo(np.uint64).max - key[passing]))[:K]
        best = passing[order]
        sel[g, :best.size] = (row[best] | (strand[best] << 31)).astype(np.uint32)
    return n_in, n_pass, sel


def select_loop(tables, lo, hi, models, rows, arena, window, editor, K, limits=None, ok=None, stop=None):
    """(n_in, n_pass, sel) by the plain loop; models in the loop form, outcomes by the string statements; stop: None or the
    three stop limits."""
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
                    good = passes(limits, outcome_loop(m, rows[g], arena, int(pos[r]), bool(s), window, editor), m["length"])
                    if not good and stop is not None:
                        targets, _, off = eref.outcome_loop(m, rows[g], arena, int(pos[r]), bool(s), window)
                        good = eref.passes(stop, targets, off, m["length"])
                    if not good:
                        continue
                passing.append((-struct.unpack("<Q", struct.pack("<d", x))[0], cut, s, r))
        n_pass[g] = len(passing)
        for rank, (_, _, s, r) in enumerate(sorted(passing)[:K]):
            sel[g][rank] = r | s << 31
    return np.array(n_in, np.uint32), np.array(n_pass, np.uint32), np.array(sel, np.uint32).reshape(G, K)
