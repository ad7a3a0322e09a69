"""The on-target model (cropsr_amd/ontarget.py) stated twice on the host: as a plain Python loop over
letters, and with numpy in the same left-to-right f64 order.  Both take site rows (forward start in an arena's coordinates,
strand 0 '+' / 1 '-') and the arena's letters as one byte string -- test code only.

model: dict -- W, left, intercept (float), single (W, 4), pair (W - 1, 16), gc (G + 1,) or None; letters in the order A T C G.
geometry: (T, P, pam3)."""
import numpy as np

NAN_BITS = 0x7FF8000000000000
CODE = {"A": 0, "T": 1, "C": 2, "G": 3, "U": 0}  # (U was packed as A)
_CODES = np.full(256, 4, np.uint8)
for _ch, _v in CODE.items():
    _CODES[ord(_ch)] = _v
    _CODES[ord(_ch.lower())] = _v


def as_dict(model, guide_letters):
    """An ontarget.Model as the dict the statements take."""
    return dict(W=model.window, left=model.left, intercept=float(model.intercept), single=np.asarray(model.single, np.float64),
                pair=np.asarray(model.pair, np.float64), gc=model.gc_table(guide_letters))


def arena_text(texts, offsets, tail=64):
    """The letters of an arena as one byte string in arena coordinates: NUL (a void position) wherever no text lies."""
    end = max(int(o) + len(t) for t, o in zip(texts, offsets)) + tail
    out = bytearray(end)
    for t, o in zip(texts, offsets):
        out[int(o):int(o) + len(t)] = t
    return bytes(out)


def region(geometry):
    T, P, pam3 = geometry
    glo = 0 if pam3 else P
    return glo, T - P


def window_forward(model, geometry, s, strand):
    """The forward positions of window positions 0 .. W - 1 of a site."""
    T = geometry[0]
    if strand:
        return [s + T - 1 + model["left"] - w for w in range(model["W"])]
    return [s - model["left"] + w for w in range(model["W"])]


def _letter_code(text, f, strand):
    if f < 0 or f >= len(text):
        return None
    c = CODE.get(chr(text[f]).upper())
    if c is None:
        return None
    return c ^ 1 if strand else c  # the complement flips the low code bit: A <-> T, C <-> G


def sum_loop(model, geometry, text, s, strand):
    """The sum of one site as a plain loop, or NaN; one add per term, left to right."""
    T = geometry[0]
    codes = [_letter_code(text, f, strand) for f in window_forward(model, geometry, s, strand)]
    if any(c is None for c in codes):
        return float("nan")
    glo, G = region(geometry)
    gc = 0
    for p in range(glo, glo + G):
        c = _letter_code(text, s + T - 1 - p if strand else s + p, strand)
        gc += 1 if c is not None and c >= 2 else 0
    acc = float(model["intercept"]) + (float(model["gc"][gc]) if model["gc"] is not None else 0.0)
    for w, c in enumerate(codes):
        acc = acc + float(model["single"][w][c])
    for w in range(len(codes) - 1):
        acc = acc + float(model["pair"][w][codes[w] * 4 + codes[w + 1]])
    return acc


def sums_loop(model, geometry, text, pos, strand):
    return np.array([sum_loop(model, geometry, text, int(s), int(st)) for s, st in zip(pos, strand)], np.float64)


def sums_numpy(model, geometry, text, pos, strand):
    """The same with numpy: a column of adds per term, in the loop's order."""
    T = geometry[0]
    W, left = model["W"], model["left"]
    pos, minus = np.asarray(pos, np.int64), np.asarray(strand).astype(bool)
    letters = np.concatenate([_CODES[np.frombuffer(text, np.uint8)], np.array([4], np.uint8)])  # [-1]: outside the text

    def codes_at(f):  # f: (n, letters) forward positions
        inside = (f >= 0) & (f < len(text))
        c = letters[np.where(inside, f, len(text))]
        return np.where(minus[:, None] & (c < 4), c ^ 1, c)

    w = np.arange(W, dtype=np.int64)[None, :]
    codes = codes_at(np.where(minus[:, None], pos[:, None] + T - 1 + left - w, pos[:, None] - left + w))
    glo, G = region(geometry)
    p = np.arange(glo, glo + G, dtype=np.int64)[None, :]
    gcodes = codes_at(np.where(minus[:, None], pos[:, None] + T - 1 - p, pos[:, None] + p))
    gc = ((gcodes == 2) | (gcodes == 3)).sum(axis=1)
    c = np.minimum(codes, 3).astype(np.int64)
    acc = np.full(pos.size, float(model["intercept"])) + (np.asarray(model["gc"], np.float64)[gc] if model["gc"] is not None else 0.0)
    for k in range(W):
        acc = acc + np.asarray(model["single"], np.float64)[k][c[:, k]]
    for k in range(W - 1):
        acc = acc + np.asarray(model["pair"], np.float64)[k][c[:, k] * 4 + c[:, k + 1]]
    acc[(codes > 3).any(axis=1)] = np.nan
    return acc


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def key_of(s):
    """The selection's list key of one sum, on Python integers."""
    b = int(np.float64(s).view(np.uint64))
    if b == 1 << 63:
        b = 0
    return b ^ (1 << 63) if b < (1 << 63) else (~b) & ((1 << 64) - 1)


# ---- the ranked selection: section 28's statement with the new order and threshold ---------------------------------------

def select_ranked(rows, lo, hi, sp, sums, rank_model, min_sum, base):
    """(n_in, n_pass, sel) of the self selection with a model: `base` is select_self_reference (its row predicate is kept as
    the filter), sums the guide sites' on-target sums.  A site passes only if base's tests hold, with min_sum set its sum is
    not NaN and >= min_sum, and ranked by model it has a sum.  Order by model: larger sum first (-0.0 equals +0.0), then the
    smaller cut letter, then '+' before '-'."""
    NONE = base.NONE
    cut = base.cut_letters(rows["pos"], rows["strand"], sp["T"], sp["c"])
    ok = rows["counts"][:, 0].astype(np.int64) <= sp["max_mm0"]
    if rows["hit_sum"] is not None:
        ok &= rows["hit_sum"] <= np.uint64(sp["max_hit_sum"])
    gc = base._popcount(np.asarray(rows["hi"], np.uint64) & np.uint64(sp["region"]))
    ok &= (gc >= sp["gc_min"]) & (gc <= sp["gc_max"]) & (base._t_runs(rows["hi"], rows["lo"], sp["region"]) <= sp["max_t_run"])
    assert sp["track"] is None
    sums = np.asarray(sums, np.float64)
    has = ~np.isnan(sums)
    if min_sum is not None:
        ok &= has & (np.where(has, sums, 0.0) >= min_sum)
    if rank_model:
        ok &= has
    e = base.row_keys(rows)
    tie = cut * 2 + np.asarray(rows["strand"], np.int64)
    G, k = len(lo), sp["k"]
    n_in, n_pass, sel = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.full((G, k), NONE, np.uint32)
    for g in range(G):
        inside = (cut >= int(lo[g])) & (cut <= int(hi[g]))
        n_in[g] = inside.sum()
        idx = np.nonzero(inside & ok)[0]
        n_pass[g] = idx.size
        if rank_model:
            order = sorted(idx.tolist(), key=lambda i: (-(sums[i] + 0.0), int(tie[i])))[:k]
        else:
            order = sorted(idx.tolist(), key=lambda i: (e[i], int(tie[i])))[:k]
        sel[g, :len(order)] = np.asarray(rows["cand"])[order]
    return n_in, n_pass, sel
