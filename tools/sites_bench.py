#!/usr/bin/env python3
"""Times the restriction-site kernels on a genome-scale stand-in and prints ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) in one arena, one scan at guide length 20, the built-in 32 enzymes,
amplicon half-width 300.  Reported, each the median of five in one session (HIP events): the plane build, the rank build
and the column kernel, with the bytes each moves; next to them, on the same tables, the two yardsticks: guide_properties_kernel
(VALU-bound) and annot_lookup_kernel (bound by dependent loads, section 14).  Sampled rows are checked
against numpy on the host: occurrences by comparing letters, counts by cumulative sums.

    python tools/sites_bench.py [--workload sorghum|tair10|ecoli] [--flank A] [--genes N] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CODE = np.full(256, -1, np.int8)
for _k, _pair in enumerate(("Aa", "Cc", "Gg", "Tt")):
    for _ch in _pair:
        CODE[ord(_ch)] = _k
CODE[ord("U")] = 0  # packed as A


def host_occurrences(code, sets_fwd, sets_rev):
    """Boolean array over the positions of `code` (base codes, -1: no base): an occurrence of either strand starts here."""
    m, n = len(sets_fwd), code.size
    out = np.zeros(n, bool)
    for sets in (sets_fwd, sets_rev):
        ok = np.ones(n - m + 1, bool)
        for k, s in enumerate(sets):
            col = code[k:n - m + 1 + k]
            ok &= (col >= 0) & ((s >> np.maximum(col, 0).astype(np.uint32)) & 1).astype(bool)
        out[:n - m + 1] |= ok
    return out


def host_rows(text, t0, pos, minus, l, flank, enzymes):
    """The packed values of rows whose cut lies in the text that begins at arena position t0 (sites.py's definition)."""
    from cropsr_amd import sites
    code = CODE[np.frombuffer(text, np.uint8)]
    n = code.size
    p = np.asarray(pos, np.int64) - t0
    c, g0 = (p + 6, p + 3) if minus else (p - 3, p - l)
    in_guide, assay = np.zeros(p.size, np.uint64), np.zeros(p.size, np.uint64)
    for e, motif in enumerate(enzymes.motifs):
        m = len(motif)
        fwd = sites.motif_sets(motif)
        rev = [sites.complement_set(s) for s in reversed(fwd)]
        cum = np.concatenate([[0], np.cumsum(host_occurrences(code, fwd, rev))])
        count = lambda lo, hi: np.where(hi > lo, cum[np.clip(hi, 0, n)] - cum[np.clip(np.minimum(lo, hi), 0, n)], 0)
        inside = (c >= 0) & (c < n)
        amp = np.where(inside, count(np.maximum(c - flank, 0), np.minimum(c + flank, n) - m + 1), 0)
        in_guide |= np.where(count(g0, g0 + l - m + 1) > 0, np.uint64(1 << e), np.uint64(0))
        assay |= np.where((count(c - m + 1, c) >= 1) & (amp == 1), np.uint64(1 << e), np.uint64(0))
    return in_guide | assay << np.uint64(32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["sorghum", "tair10", "ecoli"], default="sorghum")
    ap.add_argument("--flank", type=int, default=300)
    ap.add_argument("--genes", type=int, default=34000)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine, annotate, sites
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
    l = 20
    enzymes = sites.EnzymeSet()
    with tempfile.TemporaryDirectory() as tmp:
        gff = os.path.join(tmp, "genes.gff3")
        bw.synthetic_annotation(wl, gff, None, n_genes=args.genes)
        ann = annotate.Annotation(gff)
    eng = Engine(0)
    try:
        builder = eng.arena_builder([s.length + 4 for s in wl.specs])
        for k in range(len(wl.specs)):
            builder.add(wl.contig_string(k))
        arena = builder.seal()
        n_plus, n_minus = arena.scan_score_device(l)
        rows = n_plus + n_minus
        arena.set_enzymes(enzymes)  # (warm: a kernel's first launch loads its code object)
        planes, ranks = [], []
        for _ in range(5):
            arena.set_enzymes(enzymes)
            st = arena.site_stats()
            planes.append(st["planes_ms"])
            ranks.append(st["rank_ms"])
        arena.site_columns(n_plus, n_minus, args.flank, fetch=False)
        cols_ms = []
        for _ in range(5):
            arena.site_columns(n_plus, n_minus, args.flank, fetch=False)
            cols_ms.append(arena.site_stats()["kernel_ms"])
        st = arena.site_stats()
        words = st["bytes"] // (12 * len(enzymes))  # (about: the ranks' last entry and the chunk sums are in the bytes)
        # the yardsticks on the same tables
        arena.guide_properties(n_plus, n_minus, fetch=False)
        props = []
        for _ in range(5):
            arena.guide_properties(n_plus, n_minus, fetch=False)
            props.append(arena.guide_properties_stats()["kernel_ms"])
        req = annotate.Request(ann, [s.name for s in wl.specs], 1)
        layout = [(k, int(arena.offsets[k]), int(arena.lengths[k])) for k in range(len(wl.specs))]
        points, ids = req.track(layout)
        arena.annotate_set_track(points, ids)
        arena.annotate_lookup(n_plus, n_minus, fetch=False)
        eng.profile(2)
        annot = []
        for _ in range(5):
            eng.profile_read()
            arena.annotate_lookup(n_plus, n_minus, fetch=False)
            annot.append(eng.profile_read()["annotate"]["ms"])
        eng.profile(0)
        med = lambda v: float(np.median(v))
        E = len(enzymes)
        out = dict(workload=wl.name, guide_len=l, flank=args.flank, enzymes=E, rows=int(rows), plane_words=int(words), bytes_held=st["bytes"],
                   planes_ms=med(planes), planes_ms_runs=planes, planes_bytes=int(words * (24 + 8 * E)),
                   planes_GB_per_s=words * (24 + 8 * E) / (med(planes) * 1e-3) / 1e9,
                   rank_ms=med(ranks), rank_ms_runs=ranks, rank_bytes=int(words * E * (8 + 8 + 4)),
                   rank_GB_per_s=words * E * 20 / (med(ranks) * 1e-3) / 1e9,
                   columns_ms=med(cols_ms), columns_ms_runs=cols_ms, columns_table_bytes=int(rows * 12), rows_per_s=rows / (med(cols_ms) * 1e-3),
                   guide_properties_ms=med(props), guide_properties_ms_runs=props, annot_lookup_ms=med(annot), annot_lookup_ms_runs=annot,
                   columns_ms_over_guide_properties_ms=med(cols_ms) / med(props), columns_ms_over_annot_lookup_ms=med(cols_ms) / med(annot))
        # sampled rows against numpy on the host: up to 20 000 rows a strand of three texts
        sp, sm = arena.site_columns(n_plus, n_minus, args.flank)
        tabs = arena.fetch(n_plus, n_minus)
        lengths = np.asarray(arena.lengths)
        order = np.argsort(np.where(lengths >= 100000, lengths, lengths.max() + 1))[:3]  # (the three shortest of 100 kb or more)
        checked = 0
        for k in order.tolist():
            t0, n = int(arena.offsets[k]), int(arena.lengths[k])
            text = bytes(wl.contig_string(k))[:n]
            for pos, got, minus in ((tabs[0], sp, False), (tabs[3], sm, True)):
                cut = pos.astype(np.int64) + (6 if minus else -3)
                pick = np.flatnonzero((cut >= t0) & (cut < t0 + n))[:20000]
                assert np.array_equal(got[pick], host_rows(text, t0, pos[pick], minus, l, args.flank, enzymes)), (k, minus)
                checked += int(pick.size)
        out["rows_checked_against_numpy"] = checked
        g, a = sites.unpack(np.concatenate([sp, sm]))
        out["rows_with_a_site_in_the_guide"] = int(np.count_nonzero(g))
        out["rows_with_a_cloning_site"] = int(np.count_nonzero(g & np.uint32(31)))
        out["rows_with_an_assay"] = int(np.count_nonzero(a))
        arena.close()
    finally:
        eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
