#!/usr/bin/env python3
"""Times the spaced selection on a genome-scale stand-in and prints ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) with its seeded synthetic Phytozome-style GFF, as
tools/select_bench.py builds them: one arena, one scan at guide length 20, then per parameter set (K, D) --
K = 5 with D = 20, K = 64 with D = 20 and D = 1 000 --

  spaced      crp_select_run_spaced: its parts from the stats (pass key, whole-gene items, the cut genes' step and pick
              launches, host rounds, launches, the longest launch) and the wall time of the call
  plain       crp_select_run at the same K, in the same session: the kernel of the plain selection, not the code under test
  ratio       spaced kernel time / plain kernel time, and the same of the wall times

Every run is warmed once and repeated --repeats times; the figures are medians, with the smallest and the largest beside
them.  64 sampled genes are recomputed on the host in numpy from the fetched columns, by the definition's rounds, and
checked exactly.

    python tools/spacing_bench.py [--workload sorghum|tair10|ecoli] [--genes N] [--repeats R] [--slice-rows N] [--out FILE]
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

SETS = ((5, 20), (64, 20), (64, 1000))
NONE = 0xFFFFFFFF
SAMPLE = 64


def host_spaced(cols, lo, hi, K, D):
    """The definition of cropsr_amd/select.py (spaced selection) in numpy over host copies of the columns, for the genes
    [lo, hi]: (n_pass, n_spaced, sel)."""
    pos_p, sc_p, pos_m, sc_m = cols
    cut_p, cut_m = pos_p.astype(np.int64) - 3, pos_m.astype(np.int64)
    b = [np.searchsorted(cut_p, lo.astype(np.int64), "left"), np.searchsorted(cut_p, hi.astype(np.int64), "right"),
         np.searchsorted(cut_m, lo.astype(np.int64), "left"), np.searchsorted(cut_m, hi.astype(np.int64), "right")]
    G = lo.size
    n_pass, n_spaced, sel = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.full((G, K), NONE, np.uint32)
    for g in range(G):
        p0, p1, m0, m1 = (int(x[g]) for x in b)
        rp, rm = p0 + np.flatnonzero(sc_p[p0:p1] != -1.0), m0 + np.flatnonzero(sc_m[m0:m1] != -1.0)
        n_pass[g] = rp.size + rm.size
        key = np.concatenate([sc_p[rp], sc_m[rm]]).view(np.uint64)
        cut = np.concatenate([cut_p[rp], cut_m[rm]])
        strand = np.concatenate([np.zeros(rp.size, np.int64), np.ones(rm.size, np.int64)])
        order = np.lexsort((strand, cut, np.iinfo(np.uint64).max - key))
        packed = (np.concatenate([rp, rm]) | (strand << 31)).astype(np.uint32)[order]
        cut = cut[order]
        open_ = np.ones(order.size, bool)
        for t in range(K):
            left = np.flatnonzero(open_)
            if not left.size:
                break
            j = left[0]
            sel[g, t] = packed[j]
            open_[j] = False
            open_ &= np.abs(cut - cut[j]) >= D
            n_spaced[g] = t + 1
    return n_pass, n_spaced, sel


def spread(values):
    v = sorted(values)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["sorghum", "tair10", "ecoli"], default="sorghum")
    ap.add_argument("--genes", type=int, default=34000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slice-rows", type=int, default=0, help="crp_select_set_limits (0: the default): smaller slices cut more genes")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine, annotate
    from cropsr_amd import _native as nat
    from cropsr_amd import select as sel
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
    out = dict(workload=wl.name, build_id=nat.lib().crp_build_id().decode(), repeats=args.repeats, slice_rows=args.slice_rows, runs={})
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
        n_plus, n_minus = arena.scan_score_device(20)
        req = annotate.Request(ann, [s.name for s in wl.specs], 1)
        layout = [(k, int(arena.offsets[k]), int(arena.lengths[k])) for k in range(len(wl.specs))]
        lo, hi, gene = req.gene_layout(layout)
        out.update(rows=int(n_plus + n_minus), genes=int(ann.n_genes), genes_with_range=int(lo.size))
        handle = sel.ArenaSelect(arena, lo, hi)
        if args.slice_rows:
            handle.set_limits(args.slice_rows)
        cols = arena.fetch(n_plus, n_minus)
        cols = (cols[0], cols[2], cols[3], cols[5])
        sample = np.sort(np.random.default_rng(26).choice(lo.size, min(SAMPLE, lo.size), replace=False))
        for K, D in SETS:
            params = sel.Params(K)
            handle.run(params)  # (warm: a kernel's first launch loads its code object)
            handle.run_spaced(params, D)
            plain, spaced, plain_wall, spaced_wall, parts = [], [], [], [], []
            for _ in range(args.repeats):  # the two interleaved, so that a drift of the clocks meets both
                t0 = time.perf_counter()
                handle.run(params)
                plain_wall.append((time.perf_counter() - t0) * 1e3)
                st = handle.stats()
                plain.append(st["select_ms"] + st["merge_ms"])
                t0 = time.perf_counter()
                handle.run_spaced(params, D)
                spaced_wall.append((time.perf_counter() - t0) * 1e3)
                sp = handle.spaced_stats()
                spaced.append(sp["spaced_key_ms"] + sp["spaced_items_ms"] + sp["spaced_step_ms"] + sp["spaced_pick_ms"])
                parts.append(sp)
            mid = sorted(range(args.repeats), key=lambda i: spaced[i])[args.repeats // 2]
            run = dict(parts[mid], k=K, min_distance=D, spaced_kernels_ms=spread(spaced), plain_kernels_ms=spread(plain),
                       spaced_wall_ms=spread(spaced_wall), plain_wall_ms=spread(plain_wall), plain_items=st["items"], plain_merged_genes=st["merged_genes"])
            run["ratio_kernels"] = run["spaced_kernels_ms"]["median"] / run["plain_kernels_ms"]["median"]
            run["ratio_wall"] = run["spaced_wall_ms"]["median"] / run["plain_wall_ms"]["median"]
            n_pass, n_spaced, picked = handle.fetch_spaced()
            want = host_spaced(cols, lo[sample], hi[sample], K, D)
            run["equals_host"] = bool(all(np.array_equal(a[sample], b) for a, b in zip((n_pass, n_spaced, picked), want)))
            run["sampled_genes"] = int(sample.size)
            run["rows_selected"] = int((picked != NONE).sum())
            run["rows_selected_plain"] = int((handle.fetch()[2] != NONE).sum())
            run["genes_short_of_k"] = int(((n_spaced < K) & (n_pass >= K)).sum())
            out["runs"]["k%d_d%d" % (K, D)] = run
        handle.close()
        arena.close()
    finally:
        eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["equals_host"] for r in out["runs"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
