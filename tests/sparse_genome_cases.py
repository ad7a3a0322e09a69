"""Genomes for tests/test_sparse_genomes.py: long stretches without a PAM site (N runs, AT-only sequence), stretches
with sites on one strand only, and tiles that hold a handful of rows -- the inputs on which a tile of the scan has no
hit, a bucket of the exchange no row and a chunk of the search no candidate.

A genome is a list of contigs, a contig a list of segments (kind, n_chars[, sites]):
  "dense"     random over ACGTACGTacgtN                       rows on both strands
  "nrun"      N, one in eight of them n                       no row
  "at"        random over ATat                                no row (bases, but no PAM)
  "plus"      random over AGGT                                '+' rows only
  "minus"     random over ACCT                                '-' rows only
  "isolated"  "at" with AGGA / TCCT planted at `sites`: (offset in the segment, "plus" | "minus"), one row each
Contigs carry the reference's decoration (a quote in front, "')]" or "')," behind, written over the first character of
the first segment and the last three of the last one).  Every segment but a contig's first begins with T: a '+' row sits
one character BEFORE its GG, so without that a gap's last character could carry a row of the segment that follows it.

The arena layout is the one tests/scan_edge_cases.py states (word 0 void, a contig starts on a word boundary and is
followed by one separator word); a tile is `tile_words` words, and the row at arena position p belongs to tile
p // (64 * tile_words), whichever strand it is on.  Lengths below are in tiles of the geometry a case is built for.
"""
import os
import re

import numpy as np

from scan_edge_cases import TILE_L, TILE_S, WAVE  # noqa: F401  (the CPU checks take the geometry from there)

GUIDE_LENGTHS = (20, 23)
GAP_KINDS = ("nrun", "at")
BUCKET = 65536  # arena positions per bucket of the 16-bit position exchange

_ALPHA = {"dense": b"ACGTACGTacgtN", "at": b"ATat", "plus": b"AGGT", "minus": b"ACCT", "isolated": b"ATat"}


def emit_geometries():
    """{"large" | "small": dict(block, words, list)} read from the geometry lines of crp_kernels.h
    (TileGeo<BLOCK, WORDS, WPT, LIST, ...>): threads of the emit workgroup, words per tile, hit-list entries per round"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cropsr_amd", "csrc", "crp_kernels.h")
    with open(path) as f:
        text = f.read()
    large = re.search(r"using GeoLarge = TileGeo<(\d+), (\d+), (\d+), (\d+),", text)
    small = re.search(r"#define CRP_GEO_SMALL (\d+), (\d+), (\d+), (\d+),", text)
    return {name: dict(block=int(m.group(1)), words=int(m.group(2)), list=int(m.group(4)))
            for name, m in (("large", large), ("small", small))}


def emit_block_sizes():
    """{tile words: threads of the emit workgroup} from emit_geometries()"""
    out = {geo["words"]: geo["block"] for geo in emit_geometries().values()}
    assert set(out) == {TILE_S, TILE_L}, out
    return out


def _segment(rng, kind, n, sites=()):
    if kind == "nrun":
        a = np.where(rng.random(n) < 0.125, np.uint8(ord("n")), np.uint8(ord("N")))
    else:
        a = rng.choice(np.frombuffer(_ALPHA[kind], dtype=np.uint8), n)
    for at, strand in sites:
        assert 0 < at and at + 4 < n, (kind, n, at)
        a[at:at + 4] = np.frombuffer(b"AGGA" if strand == "plus" else b"TCCT", dtype=np.uint8)
    return a


def spread(n_chars, n_plus, n_minus, lo=64, hi=None):
    """sites of an isolated segment: n_plus + n_minus of them evenly over [lo, hi), strands interleaved"""
    hi = n_chars - 64 if hi is None else hi
    n = n_plus + n_minus
    if n == 0:
        return []
    step = (hi - lo) // n
    assert step >= 40, (n_chars, n, step)  # well apart: no site inside another one's 30-character window
    return [(lo + k * step, "plus" if (k + 1) * n_plus // n > k * n_plus // n else "minus") for k in range(n)]


class Case:
    """contigs: bytes per contig; offsets: arena position of each; segments: (contig, kind, begin, end) in contig-local
    positions; used: arena words; tile_words: the geometry it was laid out for"""

    def __init__(self, name, tile_words, spec, seed):
        rng = np.random.default_rng(seed)
        self.name, self.tile_words = name, tile_words
        self.contigs, self.offsets, self.segments = [], [], []
        cur = 1
        for k, segs in enumerate(spec):
            parts, at = [], 0
            for j, seg in enumerate(segs):
                kind, n = seg[0], int(seg[1])
                a = _segment(rng, kind, n, seg[2] if len(seg) > 2 else ())
                if j:
                    a[0] = ord("T")
                parts.append(a)
                self.segments.append((k, kind, at, at + n))
                at += n
            a = np.concatenate(parts)
            a[0] = ord("'")
            a[at - 3:] = np.frombuffer(b"')]" if k == len(spec) - 1 else b"'),", dtype=np.uint8)
            self.contigs.append(a.tobytes())
            self.offsets.append(64 * cur)
            cur += (at + 63) // 64 + 1
        self.used = cur
        self.n_tiles = -(-cur // tile_words)

    def tile_counts(self, rows):
        """(plus, minus) rows per tile, from the oracle's rows per contig"""
        tc = 64 * self.tile_words
        out = []
        for strand in ("plus", "minus"):
            t = [(rows[k]["pos_" + strand].astype(np.int64) + off) // tc for k, off in enumerate(self.offsets)]
            out.append(np.bincount(np.concatenate(t), minlength=self.n_tiles))
        assert out[0].size == out[1].size == self.n_tiles
        return out

    def rows_inside(self, rows, seg):
        k, _, a, b = seg
        return sum(int(np.searchsorted(rows[k]["pos_" + s], b) - np.searchsorted(rows[k]["pos_" + s], a)) for s in ("plus", "minus"))

    def gap_segments(self):
        return [s for s in self.segments if s[1] in GAP_KINDS]


def empty_runs(plus, minus):
    """[(first tile, length)] of the maximal runs of tiles without a row"""
    empty = (plus + minus) == 0
    runs, t = [], 0
    while t < empty.size:
        if empty[t]:
            u = t
            while u < empty.size and empty[u]:
                u += 1
            runs.append((t, u - t))
            t = u
        else:
            t += 1
    return runs


def _tiles(tile_words, x):
    return int(round(x * tile_words * 64))


def few_rows_targets(block):
    """rows per tile (strands together) that case few_rows holds, besides its three single-row tiles"""
    return [63, 64, 65, block - 64, block - 63, block, block + 1]


def _spec(name, tw, block):
    T = lambda x: _tiles(tw, x)
    if name.startswith("gap_mid_"):
        return [[("dense", T(1.5)), (name[8:], T(3.25)), ("dense", T(1.5))]]
    if name.startswith("gap_first_"):
        return [[(name[10:], T(2.5)), ("dense", T(1.5))], [("dense", T(0.4))]]
    if name.startswith("gap_last_"):
        return [[("dense", T(1.2))], [("dense", T(1.3)), (name[9:], T(2.5))]]
    if name.startswith("lookback_"):
        n = int(name.split("_")[1])
        return [[("dense", T(1.5)), ("at" if n == 130 else "nrun", T(n + 0.5)), ("dense", T(1.25))]]
    if name == "one_strand":
        big = _tiles(TILE_L, 2.5)
        first_word = 1 + 2 * ((big + 63) // 64 + 1)            # where the third contig starts
        lead = (-first_word) % TILE_S                          # words up to the next SMALL tile boundary
        if lead < 8:
            lead += TILE_S
        alt = [("plus", 64 * lead)] + [("minus" if j % 2 == 0 else "plus", 64 * TILE_S) for j in range(5)]
        return [[("plus", big)], [("minus", big)], alt]
    if name == "few_rows":
        tc = 64 * tw
        one = lambda sites: ("isolated", tc, sites)
        segs = [("isolated", tc - 64, [(tc // 2, "plus")]),           # tile 0 (the arena's word 0 is void): one '+' row
                one([(tc // 3, "minus")]),                            # one '-' row
                one([]),                                              # a tile without a row between them
                one([(tc - tc // 16, "plus")])]                       # one row, in the tile's last owner wave (the last eighth)
        for j, n in enumerate(few_rows_targets(block)):
            n_plus = n // 2 if j % 2 == 0 else n - n // 3
            segs.append(one(spread(tc, n_plus, n - n_plus)))
        segs.append(("dense", tc // 4))
        return [segs]
    raise KeyError(name)


GAP_CASES = ["gap_%s_%s" % (where, kind) for where in ("mid", "first", "last") for kind in GAP_KINDS]
LOOKBACK_CASES = ["lookback_70", "lookback_130", "lookback_260"]
CASES = GAP_CASES + LOOKBACK_CASES + ["one_strand", "few_rows"]
_BUILT = {}


def build(name, tile_words, block=None):
    """the Case `name` laid out for tiles of `tile_words` words (built once, shared, read-only); block: threads of that
    geometry's emit workgroup (default: from crp_kernels.h)"""
    key = (name, tile_words)
    if key not in _BUILT:
        if block is None:
            block = emit_block_sizes()[tile_words]
        _BUILT[key] = Case(name, tile_words, _spec(name, tile_words, block), sum(name.encode()) * 7 + tile_words)
    return _BUILT[key]


# ---- the node handle's exchange: shares without a hit and 65 536-position buckets without a row
def node_genome():
    """One contig of 28 units of three buckets: gap, a little dense sequence, a gap of a unit, dense, a gap of 2.6 units,
    dense, and gaps to the end -- cut into 2, 4 or 7 equal shares, the later shares have no hit at all and the first
    one begins and ends in a gap and has empty buckets in its middle."""
    u = 3 * BUCKET
    spec = [[("nrun", u), ("dense", u // 5), ("at", u), ("dense", u // 5), ("nrun", 2 * u + 3 * u // 5), ("dense", u // 2),
             ("at", 8 * u + u // 2), ("nrun", 14 * u)]]
    key = ("node_genome", 0)
    if key not in _BUILT:
        _BUILT[key] = Case("node_genome", TILE_L, spec, 4242)
    return _BUILT[key]


def share_conditions(plan, rows, world):
    """Which of the conditions of the 16-bit position exchange each device's share shows, from the cut (node.plan()) and
    the oracle's rows: {"no_hit", "empty_middle", "starts_in_gap", "ends_in_gap"} -> devices.  Positions are those of
    the DEVICE's arena: arena_offset + halo_before + (position in the contig - start)."""
    out = {"no_hit": [], "empty_middle": [], "starts_in_gap": [], "ends_in_gap": []}
    for d in range(world):
        pieces = [p for p in plan if p["device"] == d and p["end"] > p["start"]]
        if not pieces:
            continue
        at = lambda p, x: p["arena_offset"] + p["halo_before"] + (x - p["start"])
        first, last = at(pieces[0], pieces[0]["start"]), at(pieces[-1], pieces[-1]["end"])
        n_rows = 0
        for strand in ("plus", "minus"):
            pos = []
            for p in pieces:
                r = rows[p["contig"]]["pos_" + strand].astype(np.int64)
                r = r[(r >= p["start"]) & (r < p["end"])]
                pos.append(r - p["start"] + p["arena_offset"] + p["halo_before"])
            pos = np.concatenate(pos)
            n_rows += pos.size
            if not pos.size:
                continue
            b = pos // BUCKET
            if (np.diff(b) >= 3).any():
                out["empty_middle"].append(d)
            if b[0] - first // BUCKET >= 2:
                out["starts_in_gap"].append(d)
            if (last - 1) // BUCKET - b[-1] >= 2:
                out["ends_in_gap"].append(d)
        if n_rows == 0:
            out["no_hit"].append(d)
    return {k: sorted(set(v)) for k, v in out.items()}
