"""The self selection (cropsr_amd/select_self.py) stated twice on the host: with numpy over the rows of the
guide sites, and as a plain loop.  Both take the rows a self search fetched -- test code only.

rows: dict of the guide sites of one arena in extraction order -- pos (forward start), strand (0 '+', 1 '-'), hi, lo (the
oriented window's code bits, A=00 T=01 C=10 G=11), counts (n, M + 1), hit_sum (n,) or None for an unscored search, and cand
(n,): each site's candidate index in extraction order.
spec: dict -- T, c (the cut offset), region (bit mask of the guide region's pattern positions), k, max_mm0, max_hit_sum,
gc_min, gc_max, max_t_run, and track: None or (points, ids, flags) -- ascending arena positions, the label-set id each opens,
one flag byte per id."""
import numpy as np

NONE = 0xFFFFFFFF
NO_MM0, NO_SUM, NO_LIMIT = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF


def spec(T, c, region, k, max_mm0=NO_MM0, max_hit_sum=NO_SUM, gc_min=0, gc_max=NO_LIMIT, max_t_run=NO_LIMIT, track=None):
    return dict(T=T, c=c, region=region, k=k, max_mm0=max_mm0, max_hit_sum=max_hit_sum, gc_min=gc_min, gc_max=gc_max,
                max_t_run=max_t_run, track=track)


def region_mask(T, P, pam3):
    G = T - P
    return ((1 << G) - 1) << (0 if pam3 else P)


def default_cut(T, P, pam3):
    G = T - P
    return G - 3 if pam3 else P + min(18, G - 1)


def cut_letters(pos, strand, T, c):
    pos, strand = np.asarray(pos, np.int64), np.asarray(strand, np.int64)
    return np.where(strand == 1, pos + T - c, pos + c)


def scored_e(c0, hit_sum):
    return int(hit_sum) + (int(c0) << 30)


def packed_e(counts):
    e = min(int(counts[0]), 65535) << 48
    for j in range(1, len(counts)):
        e |= min(int(counts[j]), 4095) << (48 - 12 * j)
    return e


def t_run(hi, lo, region):
    m, r = ~int(hi) & int(lo) & region, 0
    while m:
        m &= m >> 1
        r += 1
    return r


def gc_count(hi, region):
    return bin(int(hi) & region).count("1")


def cds_flag(cut, track):
    points, ids, flags = track
    k = int(np.searchsorted(np.asarray(points, np.int64), int(cut), "right"))
    if k == 0:
        return False
    i = int(ids[k - 1])
    return i < len(flags) and bool(flags[i])


def row_e(rows, i):
    if rows["hit_sum"] is not None:
        return scored_e(rows["counts"][i, 0], rows["hit_sum"][i])
    return packed_e(rows["counts"][i])


def select_loop(rows, lo, hi, sp):
    """The definition as a plain loop: (n_in, n_pass, sel (G, k))."""
    n = len(rows["pos"])
    G, k = len(lo), sp["k"]
    n_in, n_pass, sel = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.full((G, k), NONE, np.uint32)
    for g in range(G):
        keep = []
        for i in range(n):
            s, st = int(rows["pos"][i]), int(rows["strand"][i])
            cut = s + sp["T"] - sp["c"] if st else s + sp["c"]
            if not int(lo[g]) <= cut <= int(hi[g]):
                continue
            n_in[g] += 1
            if int(rows["counts"][i, 0]) > sp["max_mm0"]:
                continue
            if rows["hit_sum"] is not None and int(rows["hit_sum"][i]) > sp["max_hit_sum"]:
                continue
            if sp["track"] is not None and not cds_flag(cut, sp["track"]):
                continue
            if not sp["gc_min"] <= gc_count(rows["hi"][i], sp["region"]) <= sp["gc_max"]:
                continue
            if t_run(rows["hi"][i], rows["lo"][i], sp["region"]) > sp["max_t_run"]:
                continue
            keep.append((row_e(rows, i), cut, st, int(rows["cand"][i])))
        n_pass[g] = len(keep)
        keep.sort()
        for r, entry in enumerate(keep[:k]):
            sel[g, r] = entry[3]
    return n_in, n_pass, sel


def _popcount(v):
    v = np.asarray(v, np.uint64)
    out = np.zeros(v.shape, np.int64)
    for b in range(32):
        out += ((v >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return out


def _t_runs(hi, lo, region):
    m = (~np.asarray(hi, np.uint64)) & np.asarray(lo, np.uint64) & np.uint64(region)
    r = np.zeros(m.shape, np.int64)
    while m.any():
        r += (m != 0)
        m = m & (m >> np.uint64(1))
    return r


def row_keys(rows):
    """e of every row, as Python integers in an object array (a scored e may pass 2^63)."""
    return np.array([row_e(rows, i) for i in range(len(rows["pos"]))], dtype=object)


def select_numpy(rows, lo, hi, sp):
    """The definition with numpy: the row predicate once, then per gene a mask and one sort."""
    cut = cut_letters(rows["pos"], rows["strand"], sp["T"], sp["c"])
    ok = rows["counts"][:, 0].astype(np.int64) <= sp["max_mm0"]
    if rows["hit_sum"] is not None:
        ok &= rows["hit_sum"] <= np.uint64(sp["max_hit_sum"])
    gc = _popcount(np.asarray(rows["hi"], np.uint64) & np.uint64(sp["region"]))
    ok &= (gc >= sp["gc_min"]) & (gc <= sp["gc_max"]) & (_t_runs(rows["hi"], rows["lo"], sp["region"]) <= sp["max_t_run"])
    if sp["track"] is not None:
        points, ids, flags = sp["track"]
        at = np.searchsorted(np.asarray(points, np.int64), cut, "right")
        i = np.asarray(ids, np.int64)[np.maximum(at, 1) - 1] if len(points) else np.zeros(cut.shape, np.int64)
        fl = np.asarray(flags, np.uint8)
        ok &= (at > 0) & (i < fl.size) & (fl[np.minimum(i, max(fl.size - 1, 0))] != 0 if fl.size else False)
    e = row_keys(rows)
    tie = cut * 2 + np.asarray(rows["strand"], np.int64)
    G, k = len(lo), sp["k"]
    n_in, n_pass, sel = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.full((G, k), NONE, np.uint32)
    for g in range(G):
        inside = (cut >= int(lo[g])) & (cut <= int(hi[g]))
        n_in[g] = inside.sum()
        idx = np.nonzero(inside & ok)[0]
        n_pass[g] = idx.size
        order = sorted(idx.tolist(), key=lambda i: (e[i], int(tie[i])))[:k]
        sel[g, :len(order)] = np.asarray(rows["cand"])[order]
    return n_in, n_pass, sel
