"""Cases for tests/test_emit_round_edges.py: tiles whose kept '+' and '-' row counts (p, m) sit exactly on the capacity
of the emit kernel's per-round hit list (C = LIST of a geometry), and a plain restatement of the kernel's round plan.

A G-rich text over GAT has '+' rows and no '-' row, a C-rich text over CAT the opposite.  A case's text is
    64 A, the '+' part, 64 A, the '-' part, 64 A
so that no row lies within a guide's reach of either end and the counts stay what they are wherever the text is embedded
in poly-A.  The parts are prefixes of two seeded random strings, cut IN CONTEXT from the oracle's own positions: the '+'
part with the separator already behind it, the '-' part as a prefix of the whole text; a strand's count grows by at most
one per character, so every count is met exactly, and the builder asserts both from the oracle's rows of the final text.
One oracle pass serves the '+' part of every case.
"""
import os

import numpy as np

from sparse_genome_cases import emit_geometries  # noqa: F401  (the header's TileGeo lines, read in one place)
from test_emit_row_strands import LIST, TILE_CHARS, _draw, arena_offsets

SEP = b"A" * 64
# round sizes at which a wave gains its first row (1, 63 -> 64 -> 65), the prefetching waves 1 ... 4 are complete
# (256 -> 257), wave 0 gets its chunk (448 -> 449) and a lane starts a second trip (511 -> 512 -> 513)
R = (1, 63, 64, 65, 256, 257, 448, 449, 511, 512, 513)
SEAMS = (1, 63, 64, 65)  # rows between a later window's first rank and the first '-' row
GROUPS = "ABCDEFGH"
_STREAM_CHARS = 16000    # either strand's longest part has 2 C + 1 = 10 033 rows, ~0.72 per character
_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cropsr_amd", "csrc")


def rounds(p, m, C):
    """the emit kernel's round plan of a tile with p '+' and m '-' rows: [(lo rank, hi rank, kind)], ranks counting the '+'
    rows first; kind "single" (everything fits), "by_strand" (each strand fits: one round each) or "window" (C ranks each)"""
    n_all = p + m
    if n_all == 0:
        return []
    if n_all <= C:
        return [(0, n_all, "single")]
    if p <= C and m <= C:
        return [(0, p, "by_strand"), (p, n_all, "by_strand")]
    return [(lo, min(lo + C, n_all), "window") for lo in range(0, n_all, C)]


def groups(C):
    """{group: [(p, m)]} for a list of C entries"""
    h = C // 2
    h0 = h - h % 64
    return {
        # one round, exactly full (the seam in the middle of it, 0, 1 and 63 rows into a chunk)
        "A": [(C, 0), (0, C), (C - 1, 1), (1, C - 1)] + [(q, C - q) for q in (h0, h0 + 1, h0 + 63)],
        # one row over: windowed with a last round of one row, or by strand
        "B": [(C + 1, 0), (0, C + 1), (C, 1), (1, C), (h, C + 1 - h)],
        # by strand with a full strand
        "C": [(C, C)] + [(C, r) for r in R] + [(r, C) for r in R],
        # one strand over by one: windowed with both strands present
        "D": [(C + 1, C), (C, C + 1), (C + 1, 1), (1, C + 1), (C + 1, C + 1)],
        # a window edge on or next to the seam; the seam at a chunk edge inside a later window
        "E": [(C, C + 1), (2 * C, 1), (C - 1, C + 1)] + [(C + s, 200) for s in SEAMS],
        # exact multiples of C, and one row past two full windows
        "F": [(2 * C, 0), (0, 2 * C), (C + 64, C - 64), (2 * C + 1, 0), (0, 2 * C + 1)],
        # windowed, every last-round size
        "G": [(C + r, 0) for r in R] + [(0, C + r) for r in R],
        # three rounds or more on both strands
        "H": [(2 * C + 1, 2 * C + 1)],
    }


def pick(C):
    """{group: (p, m)}: the case of each group that also runs on the generic window path (l = 23), through the kernel with
    both extra columns and between neighbouring tiles"""
    g = groups(C)
    return {"A": g["A"][5], "B": (C + 1, 0), "C": (C, C), "D": (C + 1, C), "E": (2 * C, 1), "F": (C + 64, C - 64),
            "G": (0, C + 65), "H": g["H"][0]}


def cases(geometry):
    """[(p, m)] of a geometry, every pair once, in group order"""
    out = []
    for group in groups(LIST[geometry]).values():
        out += [pm for pm in group if pm not in out]
    return out


def runs(geometry):
    """[(p, m, l)]: every case at l = 20; one of each group, and every last-round size of group G, also at l = 23 (the
    generic window path)"""
    return [(p, m, 20) for p, m in cases(geometry)] + [(p, m, 23) for p, m in both_columns_cases(geometry)]


def both_columns_cases(geometry):
    """[(p, m)]: one case of each group and all of group G"""
    C = LIST[geometry]
    out = list(pick(C).values())
    return out + [pm for pm in groups(C)["G"] if pm not in out]


def case_id(pm):
    return "%d+%d" % tuple(pm[:2]) + ("-l%d" % pm[2] if len(pm) > 2 else "")


# ---------------------------------------------------------------------------------------------------------- texts
_STREAMS, _PLUS_POS, _TEXT, _ROWS = {}, {}, {}, {}


def _stream(strand):
    if strand not in _STREAMS:
        rng = np.random.default_rng(71 if strand == "plus" else 72)
        _STREAMS[strand] = _draw(rng, _STREAM_CHARS, "GAT" if strand == "plus" else "CAT", [0.85, 0.075, 0.075])
    return _STREAMS[strand]


def text_of(oracle, p, m):
    """the text with exactly p '+' and m '-' rows (built once, shared, read-only)"""
    if (p, m) in _TEXT:
        return _TEXT[p, m]
    head = SEP
    if p:
        if "pos" not in _PLUS_POS:  # one pass: the '+' rows of the whole G-rich string, separators on both sides
            _PLUS_POS["pos"] = oracle.scan(SEP + _stream("plus") + SEP, 20)[0]
        pos = _PLUS_POS["pos"]
        assert pos.size >= p, (p, pos.size)
        head = (SEP + _stream("plus"))[:int(pos[p - 1]) + 3]  # the p-th row sits one character before its GG
    head += SEP
    text = head
    if m:
        whole = head + _stream("minus") + SEP
        pos = oracle.scan(whole, 20)[1]
        assert pos.size >= m, (m, pos.size)
        text = whole[:int(pos[m - 1]) + 2]  # the m-th row sits on its CC
    text += SEP
    got = oracle.scan(text, 20)
    assert (got[0].size, got[1].size) == (p, m), ((p, m), got[0].size, got[1].size)
    _TEXT[p, m] = text
    return text


def rows_of(oracle, p, m, l):
    """the oracle's rows of a case's text as one contig, computed once and shared (read-only)"""
    if (p, m, l) not in _ROWS:
        _ROWS[p, m, l] = oracle.scan_score(text_of(oracle, p, m), l)
    return _ROWS[p, m, l]


# ------------------------------------------------------------------------------------------------- with neighbours
EDGE_WORDS = 64           # an island keeps at least this many words from either end of its tile
RANDOM_ISLAND_CHARS = 1600
LAYOUTS = ("between", "last", "adjacent")
FOLLOWED = "followed"     # the exact tile first, a populated tile behind it: every case has a successor to ask for
PREFETCH_DISTANCES = (-1, 0, 1)  # the arena's default (3/8 of the CUs' tiles: past every grid here), off, the tile behind
_NEIGHBOURS = {}


def grid_tiles(geometry, contigs):
    """tiles of the kernel's grid over an arena of these contigs: its used words in whole tiles (Arena.tiles()["n_tiles"])"""
    return -(-arena_offsets(contigs)[1] // TILE_CHARS[geometry])


def prefetch_issued(tile, distance, n_tiles):
    """whether tile `tile` of a grid of n_tiles asks for a successor's planes in its last round (prefetch_successor_plane:
    the distance is not 0 and the target is a tile of the grid).  distance: > 0, as configured"""
    return 0 < distance < n_tiles - tile


def neighbour_cases(geometry):
    """[(layout, (p, m))]: one case of each of groups B ... H in every layout"""
    picked = pick(LIST[geometry])
    return [(layout, picked[g]) for layout in LAYOUTS for g in "BCDEFGH"]


def _layout(geometry, layout, pm):
    """what each tile holds: "random", None (no row) or an exact (p, m)"""
    if layout == "between":
        return ["random", pm, "random"]
    if layout == "last":
        return [None, pm]
    if layout == FOLLOWED:
        return [pm, "random"]
    order = [pick(LIST[geometry])[g] for g in "BCDEFGH"]
    return [pm, order[(order.index(pm) + 1) % len(order)], "random"]  # two multi-round tiles side by side


def neighbour_contig(oracle, geometry, layout, pm):
    """(contigs, plan): ONE contig of poly-A with an island per populated tile, its rows EDGE_WORDS words or more from
    either end of the tile; plan: _layout()'s list.  The contig ends EDGE_WORDS words or more before the end of its last tile."""
    key = (geometry, layout, pm)
    if key not in _NEIGHBOURS:
        tile_chars, plan = TILE_CHARS[geometry], _layout(geometry, layout, pm)
        rng = np.random.default_rng([tile_chars, (LAYOUTS + (FOLLOWED,)).index(layout), pm[0], pm[1]])
        text = bytearray(b"A" * (len(plan) * tile_chars - 64 * (EDGE_WORDS + 2)))
        for t, what in enumerate(plan):
            if what is None:
                continue
            island = (_draw(rng, RANDOM_ISLAND_CHARS, "ACGTacgt", [0.125] * 8) if what == "random" else text_of(oracle, *what))
            # (the contig begins at character 64 of the arena; a random island's first row can sit on the A in front of it)
            at = t * tile_chars + 64 * EDGE_WORDS
            assert at + len(island) <= min((t + 1) * tile_chars - 64 * EDGE_WORDS - 64, len(text)), (key, t, len(island))
            text[at:at + len(island)] = island
        _NEIGHBOURS[key] = ([bytes(text)], plan)
    return _NEIGHBOURS[key]


def neighbour_rows(oracle, geometry, layout, pm, l=20):
    key = ("rows", geometry, layout, pm, l)
    if key not in _NEIGHBOURS:
        _NEIGHBOURS[key] = [oracle.scan_score(c, l) for c in neighbour_contig(oracle, geometry, layout, pm)[0]]
    return _NEIGHBOURS[key]


# ---------------------------------------------------------------------------- the first scan's tables exactly full
TABLE_CHARS = 20000  # characters of a table-edge arena: one tile in both geometries
TABLE_EDGE_CASES = [(s, d) for s in ("plus", "minus") for d in (-1, 0, 1)] + [("plus_over_minus_fits", 1)]
FIRST_ROWS = r"n_chars / 8 \+ 1024"         # crp_api.cpp, scan_begin: rows per strand a first single-launch scan asks for
GROW_ROWS = r"need \+ need / 16, 64\)"     # crp_api.cpp, grow: what it allocates for `need` rows


def first_capacity(n_chars):
    """rows per strand that the tables of an arena's first single-launch scan hold (crp_api.cpp: scan_begin asks for
    n_chars / 8 + 1024 rows, grow allocates a sixteenth more)"""
    need = n_chars // 8 + 1024
    return max(need + need // 16, 64)


def api_source():
    with open(os.path.join(_SOURCE, "crp_api.cpp")) as f:
        return f.read()


def table_edge_counts(kind, d):
    cap0 = first_capacity(TABLE_CHARS)
    return {"plus": (cap0 + d, 0), "minus": (0, cap0 + d), "plus_over_minus_fits": (cap0 + d, 500)}[kind]


def table_edge_contig(oracle, kind, d):
    """one contig of TABLE_CHARS characters: the island with table_edge_counts() rows, then poly-A filler"""
    island = text_of(oracle, *table_edge_counts(kind, d))
    assert len(island) <= TABLE_CHARS and arena_offsets([b"A" * TABLE_CHARS])[1] <= min(TILE_CHARS.values())
    return [island + b"A" * (TABLE_CHARS - len(island))]


def table_edge_rows(oracle, kind, d):
    key = ("table", kind, d)
    if key not in _ROWS:
        _ROWS[key] = [oracle.scan_score(c, 20) for c in table_edge_contig(oracle, kind, d)]
    return _ROWS[key]
