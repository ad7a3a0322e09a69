"""Inputs of the on-target model tests (test_ontarget.py): seeded random models, the window-edge genome and the scan genome.
Every builder returns what it claims, and the tests prove the claims on the reference before a GPU result is compared."""
import numpy as np

from cropsr_amd import ontarget

# id -> (select_self_cases pattern id, W, left, with a gc table)
MODEL_CASES = {
    "ngg-w30": ("ngg", 30, 5, True),
    "ngg-w64": ("ngg", 64, 20, False),
    "ngg-w1": ("ngg", 1, 0, True),
    "ngg-inside": ("ngg", 10, 0, False),      # the window ends inside the pattern
    "cas12a-w34": ("cas12a", 34, 4, True),
    "t32-w64": ("t32", 64, 16, False),
    "tiny-w9": ("tiny", 9, 1, True),
}


def random_model(seed, W, left, G, gc=True, link="identity", scale=1.0, intercept=None):
    """A model whose every term is set: normal weights (sums straddle zero), an intercept, gc[0 .. G] when asked."""
    rng = np.random.default_rng([77, seed, W, left])
    return ontarget.Model(W, left, float(rng.normal()) if intercept is None else intercept, rng.normal(size=(W, 4)) * scale,
                          rng.normal(size=(max(W - 1, 0), 16)) * scale, rng.normal(size=G + 1) * scale if gc else None, link)


def zero_model(W, left, link="identity"):
    """Every weight 0.0: every sum is +0.0, the order is the tie order alone."""
    return ontarget.Model(W, left, 0.0, None, None, None, link)


def gc_only_model(W, left, G):
    """The sum is the guide's GC count minus G / 2: many equal sums on either side of zero, and exact in f64."""
    return ontarget.Model(W, left, -G / 2.0, None, None, np.arange(G + 1, dtype=np.float64))


def _acgt(rng, n):
    return bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())


def edge_genome(W, left, T=23, seed=3):
    """Three upper-case texts for ...NGG sites and a model window (W, left), with planted sites; returns (texts, planted):
    planted maps a name to (text index, local start, strand, whether the site has a sum).  The '+' site at start s has GG at
    s + 21, the '-' site CC at s.  Planted: sites whose window reaches the text's first / last letter exactly and one letter
    past it, on both strands where the geometry allows; an N and a lower-case letter in the left flank, the right flank and
    the PAM's N position; the last text ends with a site, so its right flank lies in the arena's last words and beyond."""
    rng = np.random.default_rng(seed)
    texts = [_acgt(rng, n) for n in (6000, 4931, 3700)]  # (about 900 sites a strand: every start offset modulo 64)
    planted = {}

    def plant(name, k, s, strand, has):
        t = texts[k]
        assert 0 <= s <= len(t) - T, name
        if strand:
            t[s:s + 2] = b"CC"
        else:
            t[s + T - 2:s + T] = b"GG"
        planted[name] = (k, s, strand, has)

    right = W - left  # window letters from pattern position 0 on
    for k in (0, 1):
        n = len(texts[k])
        if left <= n - T:
            plant("plus-first-exact-%d" % k, k, left, 0, right <= n - left)
        if left >= 1:
            plant("plus-first-past-%d" % k, k, left - 1, 0, False)
        if right >= T:
            plant("plus-last-exact-%d" % k, k, n - right, 0, True)
            if right > T:
                plant("plus-last-past-%d" % k, k, n - right + 1, 0, False)
        # '-': the window is forward [s + T + left - W, s + T - 1 + left]
        if W - T - left >= 0:
            plant("minus-first-exact-%d" % k, k, W - T - left, 1, True)
            if W - T - left >= 1:
                plant("minus-first-past-%d" % k, k, W - T - left - 1, 1, False)
        plant("minus-last-exact-%d" % k, k, n - T - left, 1, W - T - left <= n - T - left)
        if left >= 1:
            plant("minus-last-past-%d" % k, k, n - T - left + 1, 1, False)
    # letters inside the window, in the middle of text 0 (apart from each other and from the ends)
    at = 600
    for where, off in (("left", -min(2, left)), ("right", min(T + 1, right - 1)), ("pam-n", T - 3)):
        if not -left <= off < right or (where == "left" and left == 0) or (where == "right" and right <= T):
            continue
        for kind in ("n", "lower"):
            for strand in (0, 1):
                s = at
                at += 150
                plant("%s-%s-%s" % (where, kind, "m" if strand else "p"), 0, s, strand, kind == "lower")
                f = s + T - 1 - off if strand else s + off  # the forward position of oriented pattern position `off`
                t = texts[0]
                t[f] = ord("N") if kind == "n" else ord(chr(t[f]).lower())
    # the genome's last letters are a '+' site: its right flank (if any) lies beyond the last text
    k = 2
    texts[k][len(texts[k]) - 2:] = b"GG"
    planted["plus-at-end"] = (k, len(texts[k]) - T, 0, right <= T)
    return [bytes(t) for t in texts], planted


def scan_genome(seed=9):
    """Four upper-case ACGT contigs for the comparison with the scan; their lengths put sites next to both ends of each, so
    rows with clipped windows exist, and one contig is shorter than the 30-letter window."""
    rng = np.random.default_rng(seed)
    texts = [_acgt(rng, n) for n in (4001, 2500, 29, 1203)]
    for t in texts:  # a '+' and a '-' site hard on each end: their windows are clipped
        if len(t) >= 60:
            t[21:23] = b"GG"
            t[0:2] = b"CC"
            t[len(t) - 2:] = b"GG"
            t[len(t) - 23:len(t) - 21] = b"CC"
    texts[2][20:23] = b"AGG"
    return [bytes(t) for t in texts]
