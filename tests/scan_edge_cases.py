"""Arenas for tests/test_scan_edges.py: contigs laid out so that PAM sites, their look-behind / look-ahead tests and contig
ends fall on the boundaries where the scan kernels take a word from outside a lane, a wave or a tile.

Arena layout (crp_api.cpp): word 0 is void, contig k starts at a word boundary and takes ceil(len / 64) words plus one void
separator word; the arena has `used` = 1 + sum(ceil(len_k / 64) + 1) words and the kernels see it rounded up to whole
tiles.  A wave covers 128 words (LARGE geometry) or 64 (SMALL), a tile 1 024 or 512, so the multiples of 64 words are the
wave boundaries of both geometries and the multiples of 512 / 1 024 their tile boundaries.

A case is built from its number of used words and a list of events (word W, kind):
  "start"  a contig starts at word W (the word before it is a separator: void)
  "end"    a contig's last character is the last bit of word W - 1 (word W is its separator)
  "end+1"  a contig's last character is the first bit of word W
Contigs carry the reference's decoration (a quote in front, "')]" or "')," behind) and a seeded ACGT background.  At every
multiple of 64 words B (and a few plain word boundaries) that lies inside a contig, sites are planted:
  GGG at B-1..B+1          '+' sites at B-2 and B-1 (the PAM itself astride B) -- or CCC: '-' sites at B-1 and B
  GGG at B+l+5..B+l+7      '+' sites at B+l+4 and B+l+5: their i - l - 5 look-behind tests B-1 and B
  CCC at B-l+7..B-l+9      '-' sites at B-l+7 and B-l+8: their j + l - 8 look-ahead tests B-1 and B
For every planted site the generator says, from the contig's own start and end alone, whether the reference keeps it
(CROPSR.py:419, :430); `planted` lists the kept ones, `dropped` the others, as (contig, strand, position in the contig).
"""
import numpy as np

WAVE = 64      # words: a wave of the SMALL geometry; two of them are a wave of the LARGE one
TILE_S, TILE_L = 512, 1024

# used words -> events.  Every case ends with a contig whose last word is full, so sites reach the arena's last used word.
CASES = {
    # a single tile in both geometries; contig boundaries at a plain word boundary and at wave boundaries of each geometry
    "single_tile_300": (300, [(37, "start"), (128, "end"), (192, "start")]),
    # ends exactly at a wave's last word inside a tile / one word past it (the tile's later waves lie beyond the arena)
    "wave_end_640": (640, [(128, "start"), (256, "end"), (384, "end+1")]),
    "wave_end_641": (641, [(64, "end"), (128, "end+1"), (576, "start")]),
    # ends exactly at a SMALL tile's last word (a LARGE wave's) and one word past it
    "tile_end_512": (512, [(64, "start"), (256, "end+1"), (448, "start")]),
    "tile_end_513": (513, [(128, "end"), (320, "start")]),
    # ends exactly at a tile's last word in both geometries: the last owner wave's right edge is the end of the planes
    "tile_end_1024": (1024, [(256, "start"), (640, "end"), (896, "start")]),
    # one word past it: the last tile holds one used word, its other waves lie wholly beyond the arena
    "tile_end_1025": (1025, [(512, "end"), (768, "end+1")]),
    # contig boundaries on the tile boundaries themselves, several tiles
    "tiles_2200": (2200, [(512, "end+1"), (1024, "start"), (2048, "end")]),
    "tiles_2049": (2049, [(512, "start"), (1024, "end"), (1536, "end+1")]),
    # no contig boundary at the tile boundaries: sites and windows astride them inside one contig
    "one_contig_1100": (1100, []),
}
GUIDE_LENGTHS = (20, 23)


def _contig(rng, n_chars, k):
    a = rng.choice(np.frombuffer(b"ACGTACGTacgtN", dtype=np.uint8), n_chars)
    a[0] = ord("'")
    tail = b"')," if k % 2 else b"')]"
    a[n_chars - 3:] = np.frombuffer(tail, dtype=np.uint8)
    return a


def build(name, l):
    """(contigs as bytes, offsets in arena positions, planted, dropped, used words) of one case at guide length l"""
    used, events = CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 100 + l)
    lengths, cur = [], 1  # cur: first word of the next contig
    for w, kind in events:
        if kind == "start":
            body, n = w - 1 - cur, 64 * (w - 1 - cur) - int(rng.integers(0, 60))
            nxt = w
        elif kind == "end":
            body, n = w - cur, 64 * (w - cur)
            nxt = w + 1
        else:
            body, n = w - cur + 1, 64 * (w - cur) + 1
            nxt = w + 2
        assert body >= 2, (name, w, kind)
        lengths.append(n)
        cur = nxt
    body = used - cur - 1
    assert body >= 2, name
    lengths.append(64 * body)
    offsets, cur = [], 1
    for n in lengths:
        offsets.append(64 * cur)
        cur += (n + 63) // 64 + 1
    assert cur == used, (name, cur, used)

    contigs = [_contig(rng, n, k) for k, n in enumerate(lengths)]
    planted, dropped = [], []

    def contig_of(lo, hi):  # the contig that holds arena positions lo..hi-1 clear of its decoration, or None
        for k, (off, n) in enumerate(zip(offsets, lengths)):
            if off + 1 <= lo and hi <= off + n - 3:
                return k
        return None

    def plant(first, base, strand):
        k = contig_of(first, first + 3)
        if k is None:
            return
        off, n = offsets[k], lengths[k]
        p = first - off
        contigs[k][p:p + 3] = ord(base)
        for s in ((p - 1, p) if strand == "plus" else (p, p + 1)):
            if strand == "plus":
                kept = s - l >= 5                       # i - l >= 5
            else:
                kept = s + 3 >= 5 and s + 3 + l <= n + 10  # j + 3 >= 5 and j + 3 + l <= len + 10
            (planted if kept else dropped).append((k, strand, s))

    bounds = list(range(WAVE, used, WAVE)) + [w for w, _ in events] + [w + 1 for w, _ in events] + [3, 7, used - 2, used - 1]
    for idx, w in enumerate(sorted(set(bounds))):
        b = 64 * w
        # the three plants of one boundary never overlap: they start at b - 1, b + l + 5 and b - l + 7 (l >= 12)
        plant(b - 1, "G" if idx % 2 == 0 else "C", "plus" if idx % 2 == 0 else "minus")
        plant(b + l + 5, "G", "plus")
        plant(b - l + 7, "C", "minus")
    return [c.tobytes() for c in contigs], offsets, planted, dropped, used


def boundary_kinds(name, l):
    """how many planted sites, kept or dropped, have their PAM, look-behind or look-ahead astride a word / wave / tile
    boundary (a case generator that planted nothing at the edges must not pass)"""
    _, offsets, planted, dropped, _ = build(name, l)
    kinds = {"word": 0, "wave_small": 0, "wave_large": 0, "tile_small": 0, "tile_large": 0}
    for k, strand, s in planted + dropped:
        p = offsets[k] + s
        # positions the site's mask reads: the PAM and the void tests
        reach = (p - l - 5, p + 2) if strand == "plus" else (p - 2, max(p + 2, p + l - 8))
        for kind, words in (("word", 1), ("wave_small", WAVE), ("wave_large", 2 * WAVE), ("tile_small", TILE_S), ("tile_large", TILE_L)):
            if reach[0] // (64 * words) != reach[1] // (64 * words):
                kinds[kind] += 1
    return kinds
