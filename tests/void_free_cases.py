"""Arenas for tests/test_emit_void_free.py: three tiles whose middle tile holds ONE word that is not plain sequence -- a void
word (the separator between two contigs), a word of N, or a word of lower-case bases -- at the places where a wave of the
scan kernels meets it differently: the last word of a wave (one lane's last word, and the left edge word of the next wave),
the first word of a wave (the right edge word of the wave before), the word after it, and the same three around the seam
between two tiles.  A wave whose own words and two edge words hold no void bit skips the void terms of its hit masks, so these
are the places where the only void bit within a wave's reach sits in its left edge word, in its right edge word, in one
lane's first word or in one lane's second word (LARGE geometry: two words per lane; SMALL: one).

Layout and constants are those of tests/scan_edge_cases.py (word 0 void, a contig per run of whole words, one void separator
word behind each).  Contigs are bare sequence of whole words unless `decorated`, so that in the "void" cases the void word is
the only thing in its neighbourhood that is not a base: no quote or bracket stands in for it.  (scan_edge_cases._contig draws
N into every wave; here N appears only where a case puts it.)

Sites planted around the marked word W (first character b0 = 64 W, first character behind it b1 = b0 + 64), so that each
void test's distance crosses from plain sequence into W and back:
  GGG at b1+l+5   '+' sites at b1+l+4 and b1+l+5: their i - l - 5 look-behind (25 for l = 20) reads b1-1 and b1
  CCC at b1+1     '-' sites at b1+1 and b1+2: their j - 2 look-behind reads b1-1 and b1
  CCC at b0-3     '-' sites at b0-3 and b0-2: their j + 2 look-ahead reads b0-1 and b0
  CCC at b0-l+7   '-' sites at b0-l+7 and b0-l+8: their j + l - 8 look-ahead (12 for l = 20) reads b0-1 and b0
and GGG / CCC astride every other wave boundary of the arena.  Whether the reference keeps a site follows from its contig's
start and end alone (CROPSR.py:419, :430), as in scan_edge_cases."""
import numpy as np

import scan_edge_cases as edge

GEOMETRY = {"large": (edge.TILE_L, 2 * edge.WAVE), "small": (edge.TILE_S, edge.WAVE)}  # words per tile, per wave
KINDS = ("void", "void_decorated", "N", "lower")
GUIDE_LENGTHS = edge.GUIDE_LENGTHS
VALID = np.zeros(256, dtype=bool)
VALID[list(b"ACGTUacgtZ")] = True  # characters with the `up` or the `ac` bit (crp_kernels.hip, classify_char)


def places(geometry):
    """words of the middle tile that a case marks, by name; None = nothing marked"""
    tile, wave = GEOMETRY[geometry]
    return {"lane_last": wave - 1, "wave_first": wave, "lane_second": wave + 1,
            "tile_last": tile - 1, "next_tile_first": tile, "next_tile_second": tile + 1, "none": None}


def used_words(geometry):
    return 2 * GEOMETRY[geometry][0] + 200  # the third tile holds sequence too; the rest of it is padding


def _sequence(rng, n, decorated, k):
    if decorated:
        a = edge._contig(rng, n, k)
        a[a == ord("N")] = ord("A")
        return a
    return rng.choice(np.frombuffer(b"ACGTACGTacgt", dtype=np.uint8), n)


def build(geometry, place, kind, l):
    """(contigs as bytes, offsets in arena positions, planted, dropped, marked word or None) of one case"""
    tile, wave = GEOMETRY[geometry]
    used, rel = used_words(geometry), places(geometry)[place]
    W = None if rel is None else tile + rel
    rng = np.random.default_rng([sum(place.encode()), KINDS.index(kind), tile, l])
    split = W is not None and kind.startswith("void")
    decorated = kind == "void_decorated"
    if split:
        lengths, offsets = [64 * (W - 1), 64 * (used - 2 - W)], [64, 64 * (W + 1)]
    else:
        lengths, offsets = [64 * (used - 2)], [64]
    assert 1 + sum(n // 64 + 1 for n in lengths) == used
    contigs = [_sequence(rng, n, decorated, k) for k, n in enumerate(lengths)]
    if W is not None and not split:
        p = 64 * W - offsets[0]
        contigs[0][p:p + 64] = ord("N") if kind == "N" else rng.choice(np.frombuffer(b"acgt", dtype=np.uint8), 64)
    planted, dropped = [], []

    def plant(first, base, strand):
        for k, (off, n) in enumerate(zip(offsets, lengths)):
            lo, hi = (off + 1, off + n - 3) if decorated else (off, off + n)
            if lo <= first and first + 3 <= hi:
                break
        else:
            return 0
        p = first - off
        contigs[k][p:p + 3] = ord(base)
        for s in ((p - 1, p) if strand == "plus" else (p, p + 1)):
            if strand == "plus":
                kept = s - l >= 5 and s >= 0
            else:
                kept = s + 3 >= 5 and s + 3 + l <= n + 10 and s + 2 < n
            (planted if kept else dropped).append((k, strand, s))
        return 1

    near = 0
    if W is not None:
        b0, b1 = 64 * W, 64 * W + 64
        near = (plant(b1 + l + 5, "G", "plus") + plant(b1 + 1, "C", "minus") + plant(b0 - 3, "C", "minus") +
                plant(b0 - l + 7, "C", "minus"))
        assert near >= 3, (geometry, place, kind, l)  # (a decorated contig's last three characters take no C)
    for idx, w in enumerate(range(edge.WAVE, used - 1, edge.WAVE)):
        if W is not None and abs(w - W) <= 2:
            continue
        plant(64 * w - 1, "G" if idx % 2 == 0 else "C", "plus" if idx % 2 == 0 else "minus")
    return [c.tobytes() for c in contigs], offsets, planted, dropped, W


def waves(geometry, contigs, offsets):
    """Per wave of the padded arena, from the layout alone: (no void bit in its own words and its two edge words, every
    character of those words has the `up` or the `ac` bit).  The first is what allows a wave to skip the void terms, the
    second the kernels' cheaper test, which implies the first."""
    tile, wave = GEOMETRY[geometry]
    used = 1 + sum((len(c) + 63) // 64 + 1 for c in contigs)
    n_words = -(-used // tile) * tile
    inside = np.zeros(64 * (n_words + 2), dtype=bool)  # (one word of void on either side of the arena)
    valid = np.zeros(64 * (n_words + 2), dtype=bool)
    for c, off in zip(contigs, offsets):
        a = np.frombuffer(c, dtype=np.uint8)
        inside[64 + off:64 + off + a.size] = True
        valid[64 + off:64 + off + a.size] = VALID[a]
    reach = [(64 * w0, 64 * (w0 + wave + 2)) for w0 in range(0, n_words, wave)]  # shifted by the leading word
    return [(bool(inside[lo:hi].all()), bool(valid[lo:hi].all())) for lo, hi in reach]
