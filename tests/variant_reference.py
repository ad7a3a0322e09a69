"""The variant counts' definition (cropsr_amd/variants.py, include/cropsr_hip.h), stated twice for the tests -- a brute-force
loop over hits x variants with the touch rule (column_loop) and the rank-difference form in numpy (column_numpy) -- plus a
pure-Python VCF reader (read_vcf) and the arena layout (layout) that restate the native host code.

Intervals are (s, e) pairs of closed ends, e >= s - 1 (an insertion is (p, p - 1)).  Windows of a row with match index pos at
guide length l and seed length S, closed ranges [a, b]:

              '+' row               '-' row
  site        [i - l, i + 2]        [j, j + 2 + l]
  guide       [i - l, i - 1]        [j + 3, j + 2 + l]
  seed        [i - S, i - 1]        [j + 3, j + 2 + S]
  pam         [i + 1, i + 2]        [j, j + 1]

A variant touches a window when s <= b and e >= a.  Packed: site | guide << 8 | seed << 16 | pam << 24, each min(count, 255).
"""
import re

import numpy as np

LETTERS = set("ACGTNacgtn")


def windows(pos, minus, l, S):
    """[(a, b)] for site, guide, seed, pam of one row."""
    p = int(pos)
    if minus:
        return [(p, p + 2 + l), (p + 3, p + 2 + l), (p + 3, p + 2 + S), (p, p + 1)]
    return [(p - l, p + 2), (p - l, p - 1), (p - S, p - 1), (p + 1, p + 2)]


def pack(counts):
    site, guide, seed, pam = (min(int(c), 255) for c in counts)
    return site | guide << 8 | seed << 16 | pam << 24


def column_loop(pos, minus, l, S, intervals):
    """The packed column of the rows `pos` of one strand by the touch rule, variant by variant."""
    out = np.zeros(len(pos), np.uint32)
    for r, p in enumerate(pos):
        counts = []
        for a, b in windows(p, minus, l, S):
            counts.append(sum(1 for s, e in intervals if s <= b and e >= a))
        out[r] = pack(counts)
    return out


def column_numpy(pos, minus, l, S, starts, ends1):
    """The same from the track's two sorted arrays: #(starts <= b) - #(ends1 <= a) per window."""
    p = np.asarray(pos, np.int64)
    starts, ends1 = np.asarray(starts, np.int64), np.asarray(ends1, np.int64)
    if minus:
        wins = [(p, p + 2 + l), (p + 3, p + 2 + l), (p + 3, p + 2 + S), (p, p + 1)]
    else:
        wins = [(p - l, p + 2), (p - l, p - 1), (p - S, p - 1), (p + 1, p + 2)]
    out = np.zeros(p.size, np.uint32)
    for k, (a, b) in enumerate(wins):
        n = np.searchsorted(starts, b, "right") - np.searchsorted(ends1, a, "right")
        assert (n >= 0).all()
        out |= np.minimum(n, 255).astype(np.uint32) << np.uint32(8 * k)
    return out


def track(intervals):
    """(starts, ends1) uint32 of a list of distinct (s, e) intervals in arena positions: each array sorted on its own."""
    iv = sorted(set((int(s), int(e)) for s, e in intervals))
    return (np.array(sorted(s for s, _ in iv), np.uint32), np.array(sorted(e + 1 for _, e in iv), np.uint32))


class VcfError(ValueError):
    def __init__(self, line_no, what):
        ValueError.__init__(self, "line %d: %s" % (line_no, what))
        self.line_no = line_no


def _alt_kind(a):
    if a in (".", "*") or "[" in a or "]" in a or (len(a) >= 2 and a[0] == "<" and a[-1] == ">"):
        return 1
    return 0 if a and set(a) <= LETTERS else -1


def allele_interval(pos, ref, alt):
    """(s, e) of one sequence allele, or None when REF' and ALT' are both empty."""
    R, A = ref.upper(), alt.upper()
    pre = 0
    while pre < len(R) and pre < len(A) and R[pre] == A[pre]:
        pre += 1
    R, A = R[pre:], A[pre:]
    suf = 0
    while suf < len(R) and suf < len(A) and R[len(R) - 1 - suf] == A[len(A) - 1 - suf]:
        suf += 1
    ref_left, alt_left = len(R) - suf, len(A) - suf
    if not ref_left and not alt_left:
        return None
    s = pos + pre
    return s, s + ref_left - 1


def read_vcf(data, samples=None, pass_only=False):
    """(chroms {name: [(s, e)] sorted, distinct} in order of first appearance, stats dict) of VCF bytes; VcfError names the line."""
    samples = list(samples or [])
    chroms, order = {}, []
    st = dict(lines=0, records=0, filtered=0, alleles=0, skipped_alt=0, not_carried=0, same_as_ref=0)
    pieces = data.split(b"\n")
    if pieces and pieces[-1] == b"":
        pieces.pop()
    sample_col, have_header = [], False
    for no, raw in enumerate(pieces, 1):
        st["lines"] += 1
        if raw.endswith(b"\r"):
            raw = raw[:-1]
        if not raw:
            continue
        line = raw.decode("latin-1")
        if line[0] == "#":
            if line.startswith("#CHROM\t") or line == "#CHROM":
                col = line.split("\t")
                have_header, sample_col = True, []
                for name in samples:
                    at = [c for c in range(9, len(col)) if col[c] == name]
                    if not at:
                        raise VcfError(no, "no sample " + name)
                    sample_col.append(at[0])
            continue
        col = line.split("\t")
        if len(col) < 5 or not col[0]:
            raise VcfError(no, "columns")
        if not (1 <= len(col[1]) <= 15 and all(ch in "0123456789" for ch in col[1])) or int(col[1]) < 1:
            raise VcfError(no, "POS")
        pos, ref = int(col[1]), col[3]
        if not ref or not set(ref) <= LETTERS:
            raise VcfError(no, "REF")
        alts = col[4].split(",")
        kinds = [_alt_kind(a) for a in alts]
        if -1 in kinds:
            raise VcfError(no, "ALT")
        if pass_only and len(col) < 7:
            raise VcfError(no, "FILTER")
        carried = [not samples] * len(alts)
        if samples:
            if not have_header or len(col) < 10:
                raise VcfError(no, "samples")
            fmt = col[8].split(":")
            gt = fmt.index("GT") if "GT" in fmt else None
            for c in sample_col:
                if c >= len(col):
                    raise VcfError(no, "sample columns")
                if gt is None:
                    continue
                parts = col[c].split(":")
                if gt >= len(parts):
                    continue
                for tok in re.split(r"[/|]", parts[gt]):
                    if tok == ".":
                        continue
                    if not tok or len(tok) > 6 or not all(ch in "0123456789" for ch in tok) or int(tok) > len(alts):
                        raise VcfError(no, "GT")
                    if int(tok):
                        carried[int(tok) - 1] = True
        st["records"] += 1
        if pass_only and col[6] not in ("PASS", "."):
            st["filtered"] += 1
            continue
        for a, kind, has in zip(alts, kinds, carried):
            if kind == 1:
                st["skipped_alt"] += 1
            elif not has:
                st["not_carried"] += 1
            else:
                iv = allele_interval(pos, ref, a)
                if iv is None:
                    st["same_as_ref"] += 1
                else:
                    if col[0] not in chroms:
                        chroms[col[0]] = set()
                        order.append(col[0])
                    chroms[col[0]].add(iv)
                    st["alleles"] += 1
    st["chroms"] = len(order)
    return {name: sorted(chroms[name]) for name in order}, st


def layout(chroms, entries, dec):
    """The arena's distinct intervals [(s', e')] in arena positions: entries = [(FASTA name, first, length, offset)]; string
    index = coordinate + dec - 1, clipped to [first, first + length - 1], kept when e' >= s' - 1."""
    out = set()
    for name, first, length, offset in entries:
        if not length:
            continue
        for s, e in chroms.get(name, ()):
            a, b = max(s + dec - 1, first), min(e + dec - 1, first + length - 1)
            if b >= a - 1:
                out.add((a - first + offset, b - first + offset))
    return sorted(out)
