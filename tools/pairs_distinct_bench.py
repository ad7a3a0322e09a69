#!/usr/bin/env python3
"""Times the distinct pair selection on a genome-scale stand-in and prints ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) with its seeded synthetic Phytozome-style GFF, as
tools/spacing_bench.py builds them: one arena, one scan at guide length 20, then per parameter set -- KP = 5 and 64 at
50 .. 500 "any", KP = 5 at 30 .. 54 "pam-out" -- and per slicing, the default pair_slice_rows and 64:

  distinct    crp_select_run_pairs_distinct: its parts from the stats (pass key, whole-gene items, the cut genes' step and
              pick launches, host rounds, launches, the longest launch, partner rows streamed over all rounds, pairs taken)
              and the wall time of the call
  plain       crp_select_run_pairs at the same parameters, interleaved in the same session: the kernel of the plain pair
              selection, not the code under test
  round0      crp_select_run_pairs_distinct at KP = 1, which is round 0 alone: what the later rounds cost is the difference,
              and what they stream is the distinct run's partner rows less the plain run's
  ratio       distinct kernel time / plain kernel time, and the same of the wall times

Every run is warmed once and repeated --repeats times; the figures are medians, with the smallest and the largest beside
them.  64 sampled genes are recomputed on the host in numpy from the fetched columns, by the definition's rounds, and
checked exactly in every run.

    python tools/pairs_distinct_bench.py [--workload sorghum|tair10|ecoli] [--genes N] [--repeats R] [--out FILE]
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

# (name, KP, dmin, dmax, orientation)
SETS = (("any_50_500_kp5", 5, 50, 500, "any"), ("any_50_500_kp64", 64, 50, 500, "any"), ("pam_out_30_54_kp5", 5, 30, 54, "pam-out"))
SLICES = (0, 64)
NONE = 0xFFFFFFFF
SAMPLE = 64


def host_distinct(cols, lo, hi, KP, dmin, dmax, mask):
    """The definition of cropsr_amd/select.py (distinct pairs) in numpy over host copies of the columns, for the genes
    [lo, hi] under the plain predicate: (n_pass, n_pairs, n_distinct, pairs)."""
    pos_p, sc_p, pos_m, sc_m = cols
    site_p, site_m = pos_p.astype(np.int64) - 3, pos_m.astype(np.int64)
    b = [np.searchsorted(site_p, lo.astype(np.int64), "left"), np.searchsorted(site_p, hi.astype(np.int64), "right"),
         np.searchsorted(site_m, lo.astype(np.int64), "left"), np.searchsorted(site_m, hi.astype(np.int64), "right")]
    G = lo.size
    n_pass, n_pairs, n_distinct = np.zeros(G, np.uint32), np.zeros(G, np.uint64), np.zeros(G, np.uint32)
    pairs = np.full((G, KP, 2), NONE, np.uint32)
    big = np.iinfo(np.uint64).max
    for g in range(G):
        p0, p1, m0, m1 = (int(x[g]) for x in b)
        rp, rm = p0 + np.flatnonzero(sc_p[p0:p1] != -1.0), m0 + np.flatnonzero(sc_m[m0:m1] != -1.0)
        n_pass[g] = rp.size + rm.size
        key = np.concatenate([sc_p[rp], sc_m[rm]]).view(np.uint64)
        c = np.concatenate([site_p[rp], site_m[rm] + 6])  # the cut boundary: i - 3, j + 6
        strand = np.concatenate([np.zeros(rp.size, np.int64), np.ones(rm.size, np.int64)])
        packed = (np.concatenate([rp, rm]) | (strand << 31)).astype(np.uint32)
        by_c = np.argsort(c, kind="stable")
        key, c, strand, packed = key[by_c], c[by_c], strand[by_c], packed[by_c]
        first, last = np.searchsorted(c, c + dmin, "left"), np.searchsorted(c, c + dmax, "right")
        count = last - first
        ia = np.repeat(np.arange(c.size), count)
        ib = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count) + np.repeat(first, count)
        sbits = strand[ia] * 2 + strand[ib]
        good = ((mask >> sbits) & 1).astype(bool)
        ia, ib, sbits = ia[good], ib[good], sbits[good]
        n_pairs[g] = ia.size
        order = np.lexsort((sbits, c[ib], c[ia], big - np.maximum(key[ia], key[ib]), big - np.minimum(key[ia], key[ib])))
        A, B = packed[ia[order]], packed[ib[order]]
        free = np.ones(A.size, bool)
        for t in range(KP):  # round t: the first pair in the order without a row among the earlier picks
            if not free.any():
                break
            i = int(np.argmax(free))
            pairs[g, t] = A[i], B[i]
            n_distinct[g] = t + 1
            for x in (A[i], B[i]):
                free &= (A != x) & (B != x)
    return n_pass, n_pairs, n_distinct, pairs


def spread(values):
    v = sorted(values)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def distinct_ms(st):
    return st["pass_key_ms"] + st["distinct_items_ms"] + st["distinct_step_ms"] + st["distinct_pick_ms"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["sorghum", "tair10", "ecoli"], default="sorghum")
    ap.add_argument("--genes", type=int, default=34000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine, annotate
    from cropsr_amd import _native as nat
    from cropsr_amd import select as sel
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
    out = dict(workload=wl.name, build_id=nat.lib().crp_build_id().decode(), repeats=args.repeats, runs={})
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
        cols = arena.fetch(n_plus, n_minus)
        cols = (cols[0], cols[2], cols[3], cols[5])
        sample = np.sort(np.random.default_rng(29).choice(lo.size, min(SAMPLE, lo.size), replace=False))
        params = sel.Params(1)
        for slice_rows in SLICES:
            handle = sel.ArenaSelect(arena, lo, hi)
            if slice_rows:
                handle.set_pair_limits(slice_rows)
            for name, KP, dmin, dmax, orientation in SETS:
                q, q1 = sel.PairParams(KP, dmin, dmax, False, orientation), sel.PairParams(1, dmin, dmax, False, orientation)
                handle.run_pairs(params, q)  # (warm: a kernel's first launch loads its code object)
                handle.run_pairs_distinct(params, q)
                handle.run_pairs_distinct(params, q1)
                plain, distinct, round0, plain_wall, distinct_wall, parts = [], [], [], [], [], []
                for _ in range(args.repeats):  # interleaved, so that a drift of the clocks meets all three
                    t0 = time.perf_counter()
                    handle.run_pairs(params, q)
                    plain_wall.append((time.perf_counter() - t0) * 1e3)
                    st = handle.pairs_stats()
                    plain.append(st["pass_key_ms"] + st["pairs_ms"] + st["merge_ms"])
                    handle.run_pairs_distinct(params, q1)
                    round0.append(distinct_ms(handle.pairs_distinct_stats()))
                    t0 = time.perf_counter()
                    handle.run_pairs_distinct(params, q)
                    distinct_wall.append((time.perf_counter() - t0) * 1e3)
                    ds = handle.pairs_distinct_stats()
                    distinct.append(distinct_ms(ds))
                    parts.append(ds)
                mid = sorted(range(args.repeats), key=lambda i: distinct[i])[args.repeats // 2]
                run = dict(parts[mid], kp=KP, dmin=dmin, dmax=dmax, orientation=orientation, pair_slice_rows=slice_rows or 1024,
                           distinct_kernels_ms=spread(distinct), plain_kernels_ms=spread(plain), round0_kernels_ms=spread(round0),
                           distinct_wall_ms=spread(distinct_wall), plain_wall_ms=spread(plain_wall), plain_items=st["items"],
                           plain_pair_evaluations=st["pair_evaluations"])
                run["ratio_kernels"] = run["distinct_kernels_ms"]["median"] / run["plain_kernels_ms"]["median"]
                run["ratio_wall"] = run["distinct_wall_ms"]["median"] / run["plain_wall_ms"]["median"]
                run["later_rounds_kernels_ms"] = run["distinct_kernels_ms"]["median"] - run["round0_kernels_ms"]["median"]
                # round 0 streams what the plain run streams; the rest is the later rounds', after the skips
                run["later_rounds_pair_evaluations"] = run["pair_evaluations"] - st["pair_evaluations"]
                run["later_rounds_share_of_unskipped"] = (run["later_rounds_pair_evaluations"] / (st["pair_evaluations"] * (KP - 1))
                                                          if KP > 1 and st["pair_evaluations"] else 0.0)
                got = handle.fetch_pairs_distinct()
                want = host_distinct(cols, lo[sample], hi[sample], KP, dmin, dmax, q.mask)
                run["equals_host"] = bool(all(np.array_equal(a[sample], b) for a, b in zip(got, want)))
                run["sampled_genes"] = int(sample.size)
                n_pass, n_pairs, n_distinct, _ = got
                run["genes_short_of_kp"] = int((n_distinct < np.minimum(KP, n_pairs)).sum())
                plain_pairs = handle.fetch_pairs()[2]
                run["genes_whose_picks_differ"] = int((plain_pairs != got[3]).any(axis=(1, 2)).sum())
                out["runs"]["%s_slices%d" % (name, slice_rows or 1024)] = run
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
