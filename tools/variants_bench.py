#!/usr/bin/env python3
"""Times the variant counts on a genome-scale stand-in and prints ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) with its seeded synthetic GFF in one arena, one scan at guide length
20, and a seeded variant set at about 1 per 100 letters (70 % SNPs, 15 % insertions, 15 % deletions of 1..30 letters), laid
out in arena positions on the host.  Reported: the track build (validation, upload, the two bucket indices), the count
kernel's HIP-event time and rows per second, and the selection at K = 5 without limits and with max_seed = max_pam = 0.  The
yardstick next to the kernel comes from the same run: crp_annotate_lookup on the same tables (16 B per row, ONE rank per row
against the GFF's track) -- the count kernel reads 4 B and writes 4 B per row and takes FIVE ranks.  Sampled rows are checked
against the rank-difference form in numpy on the host.

    python tools/variants_bench.py [--workload sorghum|tair10|ecoli] [--per-letters N] [--genes N] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def seeded_track(offsets, lengths, per_letters, seed=2025):
    """(starts, ends1) uint32 of a seeded variant set over the arena's texts: distinct intervals, each array sorted."""
    rng = np.random.default_rng(seed)
    s_all, e_all = [], []
    for off, n in zip(offsets, lengths):
        m = int(n) // per_letters
        if not m or n < 64:
            continue
        s = rng.integers(0, int(n) - 32, m).astype(np.int64)
        u = rng.random(m)
        e = np.where(u < 0.70, s, np.where(u < 0.85, s - 1, s + rng.integers(1, 31, m) - 1))
        s_all.append(s + int(off))
        e_all.append(e + int(off))
    s, e = np.concatenate(s_all), np.concatenate(e_all)
    key = np.unique(s * 64 + (e - s + 1))  # (e - s + 1 is 0 .. 30: one number per distinct pair)
    s, e1 = key >> 6, (key >> 6) + (key & 63)
    return s.astype(np.uint32), np.sort(e1).astype(np.uint32)


def host_column(pos, minus, l, S, starts, ends1):
    """The packed column by #(starts <= b) - #(ends1 <= a) per window (cropsr_amd/variants.py)."""
    p = np.asarray(pos, np.int64)
    wins = [(p, p + 2 + l), (p + 3, p + 2 + l), (p + 3, p + 2 + S), (p, p + 1)] if minus else \
           [(p - l, p + 2), (p - l, p - 1), (p - S, p - 1), (p + 1, p + 2)]
    out = np.zeros(p.size, np.uint32)
    for k, (a, b) in enumerate(wins):
        n = np.searchsorted(starts, b, "right") - np.searchsorted(ends1, a, "right")
        out |= np.minimum(n, 255).astype(np.uint32) << np.uint32(8 * k)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["sorghum", "tair10", "ecoli"], default="sorghum")
    ap.add_argument("--per-letters", type=int, default=100, help="one variant per this many letters")
    ap.add_argument("--genes", type=int, default=34000)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine, annotate, variants
    from cropsr_amd import select as sel
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
    l, S = 20, 12
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
        t0 = time.perf_counter()
        starts, ends1 = seeded_track(arena.offsets, arena.lengths, args.per_letters)
        layout_s = time.perf_counter() - t0
        arena.variant_set_track(starts, ends1)  # (warm: a kernel's first launch loads its code object)
        t0 = time.perf_counter()
        arena.variant_set_track(starts, ends1)
        track_s = time.perf_counter() - t0
        arena.variant_counts(n_plus, n_minus, S, fetch=False)
        times = []
        for _ in range(5):
            arena.variant_counts(n_plus, n_minus, S, fetch=False)
            times.append(arena.variant_counts_stats()["kernel_ms"])
        ms = float(np.median(times))
        # the yardstick: the annotation look-up over the same tables, against the GFF's track
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
        annot_ms = float(np.median(annot))
        out = dict(workload=wl.name, guide_len=l, seed_len=S, rows=int(rows), variants=int(starts.size), per_letters=args.per_letters,
                   host_layout_s=layout_s, track_build_s=track_s, kernel_ms=ms, kernel_ms_runs=times, rows_per_s=rows / (ms * 1e-3),
                   table_GB_per_s=rows * 8 / (ms * 1e-3) / 1e9, annot_lookup_ms=annot_ms, annot_lookup_ms_runs=annot, annot_points=int(points.size),
                   kernel_ms_over_annot_lookup_ms=ms / annot_ms)
        # the selection at K = 5: without limits, with limits of 255 (the column is read, every row passes), seed and PAM clean
        lo, hi, _ = req.gene_layout(layout)
        handle = sel.ArenaSelect(arena, lo, hi)
        for name, limits in (("no_limits", None), ("limits_255", variants.Limits()), ("clean_seed_and_pam", variants.Limits(max_seed=0, max_pam=0))):
            handle.set_variant_limits(limits)
            handle.run(sel.Params(5))
            runs = []
            for _ in range(3):
                handle.run(sel.Params(5))
                runs.append(handle.stats())
            st = sorted(runs, key=lambda r: r["select_ms"])[1]
            n_pass = handle.fetch()[1]
            out["select_" + name] = dict(select_ms=st["select_ms"], select_ms_runs=[r["select_ms"] for r in runs], bytes_per_row=st["bytes_per_row"],
                                         rows_in_runs=st["rows_in_runs"], passing=int(n_pass.astype(np.int64).sum()))
        handle.close()
        # sampled rows against numpy on the host
        vp, vm = arena.variant_counts(n_plus, n_minus, S)
        cols = arena.fetch(n_plus, n_minus)
        checked = 0
        for pos, got, minus in ((cols[0], vp, False), (cols[3], vm, True)):
            pick = np.unique(np.concatenate([np.arange(0, pos.size, 997), np.arange(min(64, pos.size)), np.arange(max(0, pos.size - 64), pos.size)]))
            assert np.array_equal(got[pick], host_column(pos[pick], minus, l, S, starts, ends1)), minus
            checked += int(pick.size)
        out["rows_checked_against_numpy"] = checked
        out["rows_touched"] = int(np.count_nonzero(vp) + np.count_nonzero(vm))
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
