"""On-target models for any nuclease: a position-specific linear model, evaluated on the GPU for every guide site of a self
search (csrc/crp_ontarget.hip).

Not in the reference, opt-in.  Published activity models outside SpCas9's -- Doench 2014, CRISPRscan, SSC, the Cas12a position
matrices -- are linear models over the site and a few letters around it.  The user brings the published numbers in a file
(as with --weights and --score-table); the built-in model `rs1` is the scan's own, read from csrc/doench_weights.def.

Definition.  A model belongs to a pattern geometry: T pattern letters, a PAM of P on either side, a guide region of
G = T - P.  It has

  window     W letters, 1 <= W <= 64, and `left`, the number of window letters before pattern position 0 of the ORIENTED site:
             window position w is pattern position w - left.  0 <= left < W (the window holds at least pattern position 0; it
             need not hold the whole pattern).
  terms      intercept (f64); single[w][b], W x 4; pair[w][b1][b2], (W - 1) x 16, for window letters w and w + 1; optionally
             gc[0 .. G], one weight per GC count of the guide region.  Letters in the project's order A T C G (codes 00 01 10
             11).  Terms not named are 0.0.
  link       identity or logistic.

  oriented window   a '+' site with forward start s reads forward positions s - left .. s - left + W - 1.  A '-' site with
             forward start s reads forward positions s + T - 1 + left down to s + T + left - W, each complemented.
  has a sum  only if every window position is a base: A, C, G, T, in either case (case is ignored), U read as A's packed code
             (the arena packs U as A).  N, IUPAC letters, decoration, the void between contigs (at least 64 positions: a window
             that leaves its contig always meets it) and positions outside the arena are non-bases.  A window with a non-base
             has NO SUM: a quiet NaN.
  the sum    s = ((intercept + gc[GC]) + single[0] + .. + single[W - 1]) + pair[0] + .. + pair[W - 2], accumulated in f64
             strictly left to right as written, one add per term, zero terms included, no fused multiply-add, no
             reassociation.  Without a gc table the first add is intercept + 0.0.  GC is the number of C and G letters of the
             guide region (the popcount of its high code bits, as in select_self.py).
  the value  s under identity, 1 / (1 + exp(-s)) under logistic, computed on the host from the fetched s (value()).  Ranking
             and thresholds work on s, which is monotone in the value.

File format (text; '#' starts a comment; one statement per line; parse_model):

  window W | left L | link identity|logistic | intercept X | single POS LETTER X | pair POS LETTERS X | gc COUNT X

POS is a 0-based window position.  A malformed statement raises ValueError with a one-line message that names the line.

Limits: linear models only (no boosted trees, no networks); adjacent pairs only; one window of at most 64 letters; one
cut-independent model per run.
"""
import importlib.util
import math
import os

import numpy as np

MAX_W = 64
LETTERS = "ATCG"  # code = index: A=00 T=01 C=10 G=11
LINKS = ("identity", "logistic")
RS1_GEOMETRY = (23, 3, True)  # N20 NGG: T, P, PAM on the 3' side


class Model:
    """W, left, intercept, single (W, 4), pair (W - 1, 16), gc (n,) or None -- gc[c] for c = 0 .. n - 1, counts above are 0.0 --
    link, and geometry: None, or the (T, P, pam3) the model is valid for alone."""

    def __init__(self, window, left, intercept=0.0, single=None, pair=None, gc=None, link="identity", geometry=None, name=None):
        W = window
        if isinstance(W, bool) or not isinstance(W, (int, np.integer)) or not 1 <= int(W) <= MAX_W:
            raise ValueError("a model's window is 1..%d letters, not %r" % (MAX_W, W))
        W = int(W)
        if isinstance(left, bool) or not isinstance(left, (int, np.integer)) or not 0 <= int(left) < W:
            raise ValueError("left must be 0..%d (the window holds at least pattern position 0), not %r" % (W - 1, left))
        if link not in LINKS:
            raise ValueError("the link is identity or logistic, not %r" % (link,))
        self.window, self.left, self.link, self.geometry, self.name = W, int(left), link, geometry, name
        self.intercept = float(intercept)
        self.single = np.zeros((W, 4)) if single is None else np.array(single, dtype=np.float64).reshape(W, 4)
        self.pair = np.zeros((W - 1, 16)) if pair is None else np.array(pair, dtype=np.float64).reshape(W - 1, 16)
        self.gc = None if gc is None else np.array(gc, dtype=np.float64).reshape(-1)
        for what, v in (("intercept", self.intercept), ("single", self.single), ("pair", self.pair), ("gc", self.gc)):
            if v is not None and not np.isfinite(v).all():
                raise ValueError("a model's %s weights must be finite numbers" % what)

    def check_geometry(self, pattern_len, pam_len, pam3):
        """ValueError unless the model fits a pattern of T letters with a PAM of P on the 3' (pam3) or 5' side."""
        T, P = int(pattern_len), int(pam_len)
        if self.geometry is not None and tuple(self.geometry) != (T, P, bool(pam3)):
            gT, gP, g3 = self.geometry
            raise ValueError("the model %s is valid for a pattern of %d letters with a PAM of %d on the %s side only" % (
                self.name or "given", gT, gP, "3'" if g3 else "5'"))
        if self.gc is not None and self.gc.size > T - P + 1:
            raise ValueError("the model has a gc weight for count %d: above the guide region's %d letters" % (self.gc.size - 1, T - P))

    def gc_table(self, guide_letters):
        """gc[0 .. G] as (G + 1,) float64, or None without a gc table."""
        if self.gc is None:
            return None
        out = np.zeros(int(guide_letters) + 1)
        out[:self.gc.size] = self.gc
        return out

    def terms(self):
        """How many adds a sum takes: intercept + gc, W singles, W - 1 pairs."""
        return 1 + self.window + (self.window - 1)

    def abs_weight(self):
        """The sum of the absolute values of all the model's weights: a bound on every partial sum of every site."""
        a = abs(self.intercept) + np.abs(self.single).sum() + np.abs(self.pair).sum()
        return float(a + (np.abs(self.gc).sum() if self.gc is not None else 0.0))


def _number(tok, n, line):
    try:
        v = float(tok)
    except ValueError:
        raise ValueError("line %d: %r is not a number: %s" % (n, tok, line))
    if not math.isfinite(v):
        raise ValueError("line %d: %r is not a finite number: %s" % (n, tok, line))
    return v


def _count(tok, n, line, what):
    try:
        v = int(tok)
    except ValueError:
        raise ValueError("line %d: %s %r is not an integer: %s" % (n, what, tok, line))
    return v


def parse_model(text, guide_letters=None):
    """The Model of a model file's text (str or bytes).  guide_letters: G of the pattern the model is for -- a gc COUNT above
    it is refused here, with its line; without it Model.check_geometry refuses it later.  ValueError, one line, naming the
    line: an unknown statement, a POS out of range, a letter outside ACGT, a repeated term, a COUNT above G, a number that
    is not finite, a missing window."""
    if isinstance(text, bytes):
        text = text.decode("ascii", "replace")
    head, single, pair, gc = {}, {}, {}, {}
    rows = []
    for n, raw in enumerate(text.splitlines(), 1):
        line = raw.split("#", 1)[0].strip()
        if line:
            rows.append((n, line, line.split()))
    for n, line, f in rows:  # the header first: POS is checked against the window wherever `window` stands
        key = f[0].lower()
        if key in ("window", "left", "link", "intercept"):
            if len(f) != 2:
                raise ValueError("line %d: `%s` takes one value: %s" % (n, key, line))
            if key in head:
                raise ValueError("line %d: `%s` is given twice: %s" % (n, key, line))
            if key == "link":
                if f[1].lower() not in LINKS:
                    raise ValueError("line %d: the link is identity or logistic: %s" % (n, line))
                head[key] = f[1].lower()
            elif key == "intercept":
                head[key] = _number(f[1], n, line)
            else:
                head[key] = _count(f[1], n, line, key)
    if "window" not in head:
        raise ValueError("line %d: the model has no `window` statement" % (rows[-1][0] if rows else 0))
    W, left = head["window"], head.get("left", 0)
    wl = [n for n, _, f in rows if f[0].lower() == "window"][0]
    if not 1 <= W <= MAX_W:
        raise ValueError("line %d: the window is 1..%d letters, not %d" % (wl, MAX_W, W))
    if not 0 <= left < W:
        ll = [n for n, _, f in rows if f[0].lower() == "left"][0]
        raise ValueError("line %d: left must be 0..%d, not %d" % (ll, W - 1, left))
    for n, line, f in rows:
        key = f[0].lower()
        if key in ("window", "left", "link", "intercept"):
            continue
        if key == "single" and len(f) == 4:
            pos, letters, last = _count(f[1], n, line, "POS"), f[2].upper(), W - 1
        elif key == "pair" and len(f) == 4:
            pos, letters, last = _count(f[1], n, line, "POS"), f[2].upper(), W - 2
        elif key == "gc" and len(f) == 3:
            c = _count(f[1], n, line, "COUNT")
            if c < 0 or (guide_letters is not None and c > int(guide_letters)):
                raise ValueError("line %d: COUNT %d is outside 0..%s (the guide region's letters): %s" % (
                    n, c, "G" if guide_letters is None else int(guide_letters), line))
            if c > 32:
                raise ValueError("line %d: COUNT %d is above 32, the longest guide region: %s" % (n, c, line))
            if c in gc:
                raise ValueError("line %d: gc %d is given twice: %s" % (n, c, line))
            gc[c] = _number(f[2], n, line)
            continue
        else:
            raise ValueError("line %d: unknown statement: %s" % (n, line))
        if not 0 <= pos <= last:
            raise ValueError("line %d: POS %d is outside 0..%d: %s" % (n, pos, last, line))
        want = 1 if key == "single" else 2
        if len(letters) != want or any(ch not in LETTERS for ch in letters):
            raise ValueError("line %d: %r is not %d of the letters A C G T: %s" % (n, f[2], want, line))
        store = single if key == "single" else pair
        if (pos, letters) in store:
            raise ValueError("line %d: %s %d %s is given twice: %s" % (n, key, pos, letters, line))
        store[(pos, letters)] = _number(f[3], n, line)
    s1, s2 = np.zeros((W, 4)), np.zeros((max(W - 1, 0), 16))
    for (pos, b), v in single.items():
        s1[pos, LETTERS.index(b)] = v
    for (pos, bb), v in pair.items():
        s2[pos, LETTERS.index(bb[0]) * 4 + LETTERS.index(bb[1])] = v
    g = None
    if gc:
        g = np.zeros(max(gc) + 1)
        for c, v in gc.items():
            g[c] = v
    return Model(W, left, head.get("intercept", 0.0), s1, s2, g, head.get("link", "identity"))


def format_model(model):
    """The model as a file's text: parse_model(format_model(m)) has m's terms (zero terms are not written)."""
    out = ["window %d" % model.window, "left %d" % model.left, "link %s" % model.link, "intercept %r" % float(model.intercept)]
    for w in range(model.window):
        for b in range(4):
            if model.single[w, b] != 0.0:
                out.append("single %d %s %r" % (w, LETTERS[b], float(model.single[w, b])))
    for w in range(model.window - 1):
        for b in range(16):
            if model.pair[w, b] != 0.0:
                out.append("pair %d %s%s %r" % (w, LETTERS[b >> 2], LETTERS[b & 3], float(model.pair[w, b])))
    if model.gc is not None:
        for c, v in enumerate(model.gc):
            out.append("gc %d %r" % (c, float(v)))
    return "\n".join(out) + "\n"


def _weights_def():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    spec = importlib.util.spec_from_file_location("cropsr_amd_gen_score_terms", os.path.join(here, "gen_score_terms.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen.parse(os.path.join(here, "doench_weights.def"))


def rs1():
    """The scan's own model, built from csrc/doench_weights.def (the project's one copy of those weights): W = 30, left = 5
    for N20 NGG, single from FIRST, pair from SECOND, intercept = intersect + low_gc (added in f64 in that order), no gc
    table, link logistic.  Valid for T = 23, P = 3 on the 3' side only.

    The window: for a '+' scan row with match index i it is forward [i - 25, i + 5); for a '-' row with match index j it is
    forward [j - 2, j + 28), reverse-complemented -- the oriented window of this module with left = 5.  The reference does not
    score that string, though: it passes every slice through its guide-RNA conversion (complement and reverse) first, so the
    30-mer it scores is the REVERSE COMPLEMENT of the oriented window, on both strands.  As a model over the oriented window
    that is FIRST and SECOND read from the far end with complemented letters:
        single[w][b]      = FIRST[position 30 - w][complement b]                  (FIRST's positions are 1-based)
        pair[w][b1][b2]   = SECOND[position 29 - w][complement b2][complement b1]
    Placed without the mirror the model would be another one than the scan's, and its values would not be the scan's scores."""
    consts, first, second = _weights_def()
    s1, s2 = np.zeros((30, 4)), np.zeros((29, 16))
    comp = {"A": "T", "T": "A", "C": "G", "G": "C"}
    for b, pos, w, _ in first:
        s1[30 - pos, LETTERS.index(comp[b])] = w
    for b1, b2, pos, w, _ in second:
        s2[29 - pos, LETTERS.index(comp[b2]) * 4 + LETTERS.index(comp[b1])] = w
    return Model(30, 5, consts["intersect"] + consts["low_gc"], s1, s2, None, "logistic", RS1_GEOMETRY, "rs1")


def load(spec, guide_letters=None):
    """--on-target's argument: `rs1`, or the path of a model file."""
    if spec == "rs1":
        return rs1()
    with open(spec, "rb") as f:
        return parse_model(f.read(), guide_letters)


def value(s, link):
    """The value of sums s under the link: s itself, or 1 / (1 + exp(-s)).  NaN (no sum) stays NaN."""
    if link not in LINKS:
        raise ValueError("the link is identity or logistic, not %r" % (link,))
    s = np.asarray(s, dtype=np.float64)
    if link == "identity":
        return s.copy()
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-s))


def min_sum(x, link):
    """A threshold on the value as a threshold on the sum: itself under identity, log(x / (1 - x)) under logistic, where it
    must lie in (0, 1).  ValueError otherwise."""
    x = float(x)
    if link == "identity":
        if not math.isfinite(x):
            raise ValueError("the on-target threshold must be a finite number, not %r" % x)
        return x
    if not 0.0 < x < 1.0:
        raise ValueError("under the logistic link the on-target threshold lies in (0, 1), not %r" % x)
    return math.log(x / (1.0 - x))


def sort_key(s):
    """The selection's list key of sums s (uint64; a larger s is a higher key): with b the bits of s, -0.0 first replaced by
    +0.0, b ^ 2^63 for b >= 0 as a signed value and ~b otherwise."""
    b = np.array(s, dtype=np.float64).reshape(-1).view(np.int64).copy()
    b[b == np.int64(-2 ** 63)] = 0
    u = b.view(np.uint64)
    return np.where(b >= 0, u ^ np.uint64(1 << 63), ~u)


def sums_of_codes(model, codes, gc_count):
    """The sums of windows given as letter codes (n, W) uint8 (0..3; 4 or more: a non-base) and the guide regions' GC counts
    (n,), with numpy in the definition's order of adds -- the host's statement beside the device's."""
    codes = np.asarray(codes)
    n, W = codes.shape
    c = np.minimum(codes, 3).astype(np.int64)
    gc = model.gc_table(32)
    acc = np.full(n, model.intercept) + (gc[np.asarray(gc_count, np.int64)] if gc is not None else 0.0)
    for w in range(W):
        acc = acc + model.single[w][c[:, w]]
    for w in range(W - 1):
        acc = acc + model.pair[w][c[:, w] * 4 + c[:, w + 1]]
    acc[(codes > 3).any(axis=1)] = np.nan
    return acc
