"""The genome of tests/test_long_contigs.py and what the reference gives for it (no GPU here).

The genome is [S, b"", T].  S is ONE contig string of `length` characters (2^31 + 2^20 at full scale): upper-case A -- which gives
no row on either strand -- between the decoration ("'" in front, "')]" behind) and a few ISLANDS of 3 000 random letters.
Every island is centred on a boundary of the piece path (crp_plan.cpp: plan_shares, pack_pieces; crp_gather.hip), derived from
the plans themselves -- the cut restated in test_node._pack_share and crp_plan_shares -- never from literals:

    B0  the start of S                                    B4  the cut at which an empty arena of arena_words ends its piece
    B1  the first cut of the default slices               B5  contig position `high` (2^31)
    B2  arena position `mid` (2^30) in an arena S opens   B6  arena position `mid` on device 1 of two
    B3  the world-2 share cut inside S                    B7  the end of S

The first and last islands lie flush inside the decoration; islands closer than 1 024 letters become one longer island.

S is too large for the oracle, so the expected rows are COMPOSED: per island the oracle's rows of the island with 256 characters
of its real surroundings either side (filler, or the decoration where the contig ends sooner), shifted to the island's place.
Everything the reference looks at lies within 58 characters of a match (CROPSR.py:418-434), and filler alone gives no row.  At a
small scale (length about 2^21, every limit scaled with it) the same builder's composition is held against the oracle's scan of
the whole contig (test_long_contigs.test_composition_equals_oracle_at_small_scale).  Positions are int64 throughout.
"""
import numpy as np

from test_node import ALPHA, _genome, _pack_share

HALO = 128           # CRP_HALO
ARENA_OFF = 64       # an arena's first text begins at word 1
ISLAND = 3000
PAD = 256
MIN_GAP = 1024
T_LETTERS = 40_000
FILLER = ord("A")
KEYS = ("pos_plus", "pre_plus", "score_plus", "pos_minus", "pre_minus", "score_minus")


class Scale:
    """The sizes a layout follows from: S's length, the words of the largest arena and of a default slice, and the two
    positions (arena `mid`, contig `high`) that islands are put on."""

    def __init__(self, length, arena_words, slice_words, mid, high):
        self.length, self.arena_words, self.slice_words, self.mid, self.high = int(length), int(arena_words), int(slice_words), int(mid), int(high)


def full_scale():
    from cropsr_amd import _native as nat
    return Scale((1 << 31) + (1 << 20), nat.lib().crp_arena_max_words(), (64 << 20) // 64 + 2, 1 << 30, 1 << 31)


def small_scale(merged):
    """2^-10 of the full scale (S a little longer in proportion, so that B6 still falls inside it).  merged: the arena limit
    scaled exactly, which brings B4 within 384 characters of B5 -- one island over both; else B4 lies 4 480 characters below."""
    return Scale((1 << 21) + (1 << 16), (1 << 15) - (2 if merged else 66), (1 << 16) // 64 + 2, 1 << 20, 1 << 21)


class Layout:
    def __init__(self, scale, seed=20261021):
        from cropsr_amd import node as nd
        self.scale = scale
        rng = np.random.default_rng(seed)
        self.T = _genome(rng, [T_LETTERS])[0]
        L = self.L = scale.length
        self.lengths = [L, 0, len(self.T)]
        whole = [(k, 0, n) for k, n in enumerate(self.lengths)]
        # the three plans, restated
        self.slices = _pack_share(whole, self.lengths, scale.slice_words, HALO)            # [(contig, start, end, slice)]
        self.arenas = _pack_share(whole, self.lengths, scale.arena_words, HALO)            # Node([0]): [(contig, start, end, arena)]
        self.shares = nd.plan_shares(self.lengths, 2)                                      # [(contig, start, end, device)]
        self.node2 = []                                                                    # [(contig, start, end, device, arena)]
        for device in (0, 1):
            share = [(c, s, e) for c, s, e, d in self.shares if d == device]
            self.node2 += [(c, s, e, device, a) for c, s, e, a in _pack_share(share, self.lengths, scale.arena_words, HALO)]
        b3 = [e for c, s, e, d in self.shares if c == 0 and d == 0][0]
        self.boundaries = {
            "B0": 0,
            "B1": self.slices[0][2],
            "B2": scale.mid - ARENA_OFF,
            "B3": b3,
            "B4": self.arenas[0][2],
            "B5": scale.high,
            "B6": b3 - HALO + scale.mid - ARENA_OFF,
            "B7": L,
        }
        spans = []
        for name, b in self.boundaries.items():
            lo, hi = (1, 1 + ISLAND) if name == "B0" else (L - 3 - ISLAND, L - 3) if name == "B7" else (b - ISLAND // 2, b + ISLAND // 2)
            spans.append([lo, hi, [name]])
        spans.sort(key=lambda s: s[0])
        merged = [spans[0]]
        for lo, hi, names in spans[1:]:
            if lo - merged[-1][1] < MIN_GAP:  # too close: one longer island over both boundaries
                merged[-1][1] = max(merged[-1][1], hi)
                merged[-1][2] += names
            else:
                merged.append([lo, hi, names])
        assert merged[0][2] == ["B0"] and merged[-1][2] == ["B7"] and merged[0][0] == 1 and merged[-1][1] == L - 3
        self.islands = [(lo, hi, tuple(names), rng.choice(ALPHA, hi - lo)) for lo, hi, names in merged]
        self._expected = {}

    def island_of(self, name):
        return [i for i in self.islands if name in i[2]][0]

    def arena_position(self, pos, piece_start):
        """Arena position of contig position `pos` of S in an arena whose FIRST piece is S from piece_start on."""
        return ARENA_OFF + pos - max(0, piece_start - HALO)

    def surroundings(self, a, b):
        """Characters [a, b) of S as they are where no island lies: filler and the decoration."""
        out = np.full(b - a, FILLER, dtype=np.uint8)
        for pos, ch in ((0, b"'"), (self.L - 3, b"'"), (self.L - 2, b")"), (self.L - 1, b"]")):
            if a <= pos < b:
                out[pos - a] = ch[0]
        return out

    def build_contig(self):
        """S itself, a uint8 array of L characters."""
        s = np.full(self.L, FILLER, dtype=np.uint8)
        s[0] = ord("'")
        s[-3:] = np.frombuffer(b"')]", dtype=np.uint8)
        for lo, hi, _, text in self.islands:
            s[lo:hi] = text
        return s

    def expected(self, oracle, l):
        """The composed rows of S for guide length l: dict of KEYS, positions int64."""
        if l not in self._expected:
            parts = {key: [] for key in KEYS}
            for lo, hi, _, text in self.islands:
                a, b = max(0, lo - PAD), min(self.L, hi + PAD)
                rows = oracle.scan_score(np.concatenate([self.surroundings(a, lo), text, self.surroundings(hi, b)]), l)
                for key in KEYS:
                    parts[key].append(rows[key].astype(np.int64) + a if key.startswith("pos_") else rows[key])
            self._expected[l] = {key: np.concatenate(parts[key]) for key in KEYS}
        return self._expected[l]

    def expected_genome(self, oracle, l):
        """[rows of S, rows of b"", rows of T], each a dict of KEYS."""
        key = ("genome", l)
        if key not in self._expected:
            rest = [oracle.scan_score(c, l) for c in (b"", self.T)]
            self._expected[key] = [self.expected(oracle, l)] + [{k: (v.astype(np.int64) if k.startswith("pos_") else v) for k, v in r.items()} for r in rest]
        return self._expected[key]
