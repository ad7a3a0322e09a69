"""Whether a table row PASSES a selection, "in the gene" apart: the tests' one statement of the row predicate that
cropsr_amd/csrc/crp_select_predicate.inc states once for the device (cropsr_amd/select.py has the definition in words).

columns   a dict of arrays over the rows of one arena's two tables, the '+' rows first, then the '-' rows:
            score     float64, -1.0 for a row without a score (such a row has no cut site and passes nowhere)
            counts0   uint32, the joined counts[0]; 0xFFFFFFFF for a row the join did not match
            hit_sum   uint64, the joined hit sum
            feat      uint32, the label-set id of the annotation join; 0xFFFFFFFF: none
            flags     uint8 per label-set id: non-zero where the set holds a CDS label (the one entry that is not per row)
            props     uint32, gc | run << 8 | t_run << 16 | stem << 24   (tests/guide_properties_reference.py)
            repair    uint64, mh | oof << 32                              (tests/repair_reference.py)
            variants  uint32, site | guide << 8 | seed << 16 | pam << 24, each saturated at 255 (tests/variant_reference.py)
          `columns()` builds them from the per-strand columns of the other references.
limits    a dict; a term whose key is absent is not part of the predicate:
            min_score    float: score >= min_score
            joined       True: the selection reads the joined columns -- the row is joined, counts0 <= max_mm0 (absent: no bound)
                         and hit_sum <= max_hit_sum (absent: no bound); a family kernel always reads them
            require_cds  True: feat is an id below len(flags) and flags[feat] != 0; or a tuple of flag bytes to read instead of
                         the columns' flags (the device takes whatever flags the host sets)
            props        (gc_min, gc_max, max_run, max_t_run, max_stem)
            repair       (min_mh, min_oof_pct): mh >= min_mh, 100 oof >= min_oof_pct mh, and mh > 0 where min_oof_pct > 0
            variants     (max_site, max_guide, max_seed, max_pam)

Stated twice: mask_numpy over the arrays, mask_loop row by row with every `if` written out."""
import numpy as np

NONE = 0xFFFFFFFF
NO_BOUND_MM0, NO_BOUND_SUM = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
KEYS = ("min_score", "joined", "max_mm0", "max_hit_sum", "require_cds", "props", "repair", "variants")


def columns(tables, spec, feat, flags, props, repair, variants):
    """spec: dict(counts_plus, sum_plus, counts_minus, sum_minus); feat, props, repair, variants: (plus, minus) pairs."""
    n_plus, n_minus = len(tables["pos_plus"]), len(tables["pos_minus"])
    cat = lambda pair, dt: np.concatenate([np.asarray(pair[0], dt), np.asarray(pair[1], dt)])
    out = dict(score=cat((tables["score_plus"], tables["score_minus"]), np.float64),
               counts0=cat((np.asarray(spec["counts_plus"], np.uint32).reshape(n_plus, -1)[:, 0],
                            np.asarray(spec["counts_minus"], np.uint32).reshape(n_minus, -1)[:, 0]), np.uint32),
               hit_sum=cat((spec["sum_plus"], spec["sum_minus"]), np.uint64), feat=cat(feat, np.uint32), flags=np.asarray(flags, np.uint8),
               props=cat(props, np.uint32), repair=cat(repair, np.uint64), variants=cat(variants, np.uint32))
    assert all(v.shape == (n_plus + n_minus,) for k, v in out.items() if k != "flags")
    return out


def _check(limits):
    assert set(limits) <= set(KEYS), sorted(set(limits) - set(KEYS))
    assert "joined" in limits or not ("max_mm0" in limits or "max_hit_sum" in limits)


def _flags(cols, limits):
    return cols["flags"] if limits["require_cds"] is True else np.array(limits["require_cds"], np.uint8)


def mask_numpy(cols, limits):
    _check(limits)
    score = cols["score"]
    ok = (score != -1.0) & (score >= np.float64(limits.get("min_score", 0.0)))
    if limits.get("joined"):
        c0, hs = cols["counts0"].astype(np.uint64), cols["hit_sum"].astype(np.uint64)
        ok &= (c0 != NONE) & (c0 <= np.uint64(limits.get("max_mm0", NO_BOUND_MM0))) & (hs <= np.uint64(limits.get("max_hit_sum", NO_BOUND_SUM)))
    if limits.get("require_cds"):
        ids, flags = cols["feat"].astype(np.int64), _flags(cols, limits)
        inside = ids < flags.size
        ok &= inside & (np.concatenate([flags, [0]])[np.where(inside, ids, flags.size)] != 0)
    if "props" in limits:
        gc_min, gc_max, max_run, max_t_run, max_stem = limits["props"]
        p = cols["props"].astype(np.int64)
        gc = p & 255
        ok &= (gc >= gc_min) & (gc <= gc_max) & ((p >> 8 & 255) <= max_run) & ((p >> 16 & 255) <= max_t_run) & ((p >> 24) <= max_stem)
    if "repair" in limits:
        min_mh, min_oof = limits["repair"]
        r = cols["repair"]
        mh, oof = (r & np.uint64(0xFFFFFFFF)).astype(np.int64), (r >> np.uint64(32)).astype(np.int64)
        ok &= (mh >= min_mh) & (100 * oof >= min_oof * mh) & ((mh != 0) | (min_oof == 0))
    if "variants" in limits:
        v = cols["variants"].astype(np.int64)
        for k, bound in enumerate(limits["variants"]):
            ok &= (v >> (8 * k) & 255) <= bound
    return ok


def mask_loop(cols, limits):
    _check(limits)
    n = len(cols["score"])
    out = np.zeros(n, bool)
    for r in range(n):
        x = float(cols["score"][r])
        if x == -1.0:
            continue
        if "min_score" in limits and not x >= float(limits["min_score"]):
            continue
        if limits.get("joined"):
            c0, hs = int(cols["counts0"][r]), int(cols["hit_sum"][r])
            if c0 == NONE:
                continue
            if "max_mm0" in limits and c0 > int(limits["max_mm0"]):
                continue
            if "max_hit_sum" in limits and hs > int(limits["max_hit_sum"]):
                continue
        if limits.get("require_cds"):
            i, flags = int(cols["feat"][r]), _flags(cols, limits)
            if i == NONE or i >= len(flags):
                continue
            if not flags[i]:
                continue
        if "props" in limits:
            gc_min, gc_max, max_run, max_t_run, max_stem = limits["props"]
            word = int(cols["props"][r])
            gc, run, t_run, stem = word & 255, word >> 8 & 255, word >> 16 & 255, word >> 24
            if gc < gc_min or gc > gc_max:
                continue
            if run > max_run:
                continue
            if t_run > max_t_run:
                continue
            if stem > max_stem:
                continue
        if "repair" in limits:
            min_mh, min_oof = limits["repair"]
            word = int(cols["repair"][r])
            mh, oof = word & 0xFFFFFFFF, word >> 32
            if mh < min_mh:
                continue
            if min_oof > 0 and mh == 0:
                continue
            if 100 * oof < min_oof * mh:
                continue
        if "variants" in limits:
            max_site, max_guide, max_seed, max_pam = limits["variants"]
            word = int(cols["variants"][r])
            if word & 255 > max_site:
                continue
            if word >> 8 & 255 > max_guide:
                continue
            if word >> 16 & 255 > max_seed:
                continue
            if word >> 24 > max_pam:
                continue
        out[r] = True
    return out


def edge_rows():
    """(columns, [(limits, the expected mask)]) of six hand-made rows that hold the packing's edges: row 0 is plain and passes
    everything here, row 1 has mh = 0 (and so oof = 0), row 2 a site count saturated at 255, row 3 is not joined, row 4 has no
    score, row 5 has a label-set id beyond the flags."""
    cols = dict(score=np.array([0.5, 0.5, 0.5, 0.5, -1.0, 0.5]), counts0=np.array([0, 0, 0, NONE, 0, 0], np.uint32),
                hit_sum=np.array([0, 0, 0, NO_BOUND_SUM, 0, 0], np.uint64), feat=np.array([1, 1, 1, 1, 1, 2], np.uint32),
                flags=np.array([0, 1], np.uint8), props=np.full(6, 10, np.uint32),
                repair=np.array([400 | 300 << 32, 0, 400 | 300 << 32, 400 | 300 << 32, 400 | 300 << 32, 400 | 300 << 32], np.uint64),
                variants=np.array([0, 0, 255 | 3 << 8, 0, 0, 0], np.uint32))
    T, F = True, False
    return cols, [
        ({}, [T, T, T, T, F, T]),
        (dict(repair=(0, 0)), [T, T, T, T, F, T]),             # mh == 0 with min_oof == 0: passes
        (dict(repair=(0, 1)), [T, F, T, T, F, T]),             # ... and with min_oof above 0: fails, although 100 * 0 >= 1 * 0
        (dict(repair=(1, 0)), [T, F, T, T, F, T]),
        (dict(variants=(255, 255, 255, 255)), [T, T, T, T, F, T]),  # a saturated count meets a limit of 255
        (dict(variants=(254, 255, 255, 255)), [T, T, F, T, F, T]),
        (dict(variants=(255, 2, 255, 255)), [T, T, F, T, F, T]),
        (dict(joined=True), [T, T, T, F, F, T]),               # an unjoined row fails with the columns read, whatever the bounds
        (dict(joined=True, max_mm0=NO_BOUND_MM0, max_hit_sum=NO_BOUND_SUM), [T, T, T, F, F, T]),  # (its sentinel meets the bound)
        (dict(require_cds=True), [T, T, T, T, F, F]),
        (dict(require_cds=(1, 0, 1)), [F, F, F, F, F, T]),
        (dict(min_score=0.5), [T, T, T, T, F, T]),
        (dict(min_score=0.5000001), [F] * 6),
    ]
