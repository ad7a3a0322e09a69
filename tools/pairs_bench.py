#!/usr/bin/env python3
"""Times the guide-pair selection on a genome-scale stand-in and prints ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) with its seeded synthetic Phytozome-style GFF, as
tools/select_bench.py builds them: one arena, one scan at guide length 20, the annotation look-up (whose HIP-event time
gives the HBM rate a streaming kernel reaches on these very tables), then crp_select_run_pairs at KP = 5 three times:
50 .. 500 "any", 30 .. 54 "pam-out" and 50 .. 5 000 with frameshift.  Per run: the pass-key, pair and merge times from
HIP events, items, launches, the longest launch, pair evaluations (partner rows streamed), qualifying pairs and pair
evaluations per second.  Two yardsticks from the same run stand next to them:

  host        what a user does today, on a sample of the genes: the columns fetched to the host, then the pairing with
              numpy (searchsorted windows, a lexsort per gene); the run checks the device's result for those genes against
              it, exactly, and scales the time to all genes
  floor_ms    the pair kernel's traffic floor: 12 B x pair evaluations / the annotation look-up's rate

    python tools/pairs_bench.py [--workload sorghum|tair10|ecoli] [--genes N] [--sample N] [--out FILE]
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

KP = 5
NONE = 0xFFFFFFFF
RUNS = [("any_50_500", 50, 500, "any", False), ("pam_out_30_54", 30, 54, "pam-out", False), ("frameshift_50_5000", 50, 5000, "any", True)]


def host_pairs(cols, lo, hi, genes, kp, dmin, dmax, mask, frameshift):
    """The definition of cropsr_amd/select.py's guide pairs in numpy over host copies of the columns, for the genes
    `genes`: (n_pass, n_pairs, pairs).  The plain predicate only (a score other than -1).  A stand-alone restatement so that
    the tool needs nothing from tests/: keep it in step with pairs_numpy in tests/select_pairs_reference.py."""
    pos_p, sc_p, pos_m, sc_m = cols
    site_p, site_m = pos_p.astype(np.int64) - 3, pos_m.astype(np.int64)
    n_pass, n_pairs, pairs = np.zeros(genes.size, np.uint32), np.zeros(genes.size, np.uint64), np.full((genes.size, kp, 2), NONE, np.uint32)
    big = np.iinfo(np.uint64).max
    for at, g in enumerate(genes):
        p0, p1 = np.searchsorted(site_p, [int(lo[g]), int(hi[g]) + 1], "left")
        m0, m1 = np.searchsorted(site_m, [int(lo[g]), int(hi[g]) + 1], "left")
        rp, rm = p0 + np.flatnonzero(sc_p[p0:p1] != -1.0), m0 + np.flatnonzero(sc_m[m0:m1] != -1.0)
        n_pass[at] = rp.size + rm.size
        c = np.concatenate([site_p[rp], site_m[rm] + 6])  # the cut boundaries: i - 3 and j + 6
        strand = np.concatenate([np.zeros(rp.size, np.int64), np.ones(rm.size, np.int64)])
        row = np.concatenate([rp, rm])
        key = np.concatenate([sc_p[rp], sc_m[rm]]).view(np.uint64)
        by_c = np.argsort(c, kind="stable")
        c, strand, row, key = c[by_c], strand[by_c], row[by_c], key[by_c]
        first, last = np.searchsorted(c, c + dmin, "left"), np.searchsorted(c, c + dmax, "right")
        count = last - first
        a = np.repeat(np.arange(c.size), count)
        b = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count) + np.repeat(first, count)
        sbits = strand[a] * 2 + strand[b]
        good = ((mask >> sbits) & 1).astype(bool)
        if frameshift:
            good &= (c[b] - c[a]) % 3 != 0
        a, b, sbits = a[good], b[good], sbits[good]
        n_pairs[at] = a.size
        order = np.lexsort((sbits, c[b], c[a], big - np.maximum(key[a], key[b]), big - np.minimum(key[a], key[b])))[:kp]
        pairs[at, :order.size, 0] = (row[a[order]] | strand[a[order]] << 31).astype(np.uint32)
        pairs[at, :order.size, 1] = (row[b[order]] | strand[b[order]] << 31).astype(np.uint32)
    return n_pass, n_pairs, pairs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["sorghum", "tair10", "ecoli"], default="sorghum")
    ap.add_argument("--genes", type=int, default=34000)
    ap.add_argument("--sample", type=int, default=500, help="genes the host yardstick computes and the device result is checked on")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine, annotate
    from cropsr_amd import select as sel
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
    out = dict(workload=wl.name, kp=KP, runs={})
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
        arena.annotate_set_track(*req.track(layout))
        arena.annotate_lookup(n_plus, n_minus, fetch=False)  # (warm)
        eng.profile(2)
        eng.profile_read()
        arena.annotate_lookup(n_plus, n_minus, fetch=False)
        annot_ms = eng.profile_read()["annotate"]["ms"]
        rate = (n_plus + n_minus) * 16 / (annot_ms * 1e-3)  # 4 B position + 8 B score in, 4 B id out per row
        lo, hi, gene = req.gene_layout(layout)
        out.update(rows=int(n_plus + n_minus), genes=int(ann.n_genes), genes_with_range=int(lo.size), annot_lookup_ms=annot_ms,
                   annot_lookup_bytes_per_s=rate)
        handle = sel.ArenaSelect(arena, lo, hi)
        t0 = time.perf_counter()
        cols = arena.fetch(n_plus, n_minus)
        cols = (cols[0], cols[2], cols[3], cols[5])
        fetch_s = time.perf_counter() - t0
        sample = np.unique(np.linspace(0, lo.size - 1, min(args.sample, lo.size)).astype(np.int64)) if lo.size else np.empty(0, np.int64)
        for name, dmin, dmax, orientation, frameshift in RUNS:
            pp = sel.PairParams(KP, dmin, dmax, frameshift, orientation)
            handle.run_pairs(sel.Params(1), pp)  # (warm: the kernels' first launch loads their code object)
            handle.run_pairs(sel.Params(1), pp)
            st = handle.pairs_stats()
            t0 = time.perf_counter()
            got = handle.fetch_pairs()
            st["fetch_result_s"] = time.perf_counter() - t0
            st["pair_evaluations_per_s"] = st["pair_evaluations"] / (st["pairs_ms"] * 1e-3) if st["pairs_ms"] else None
            st["floor_ms"] = 12.0 * st["pair_evaluations"] / rate * 1e3
            st["pairs_share_of_floor"] = st["floor_ms"] / st["pairs_ms"] if st["pairs_ms"] else None
            t0 = time.perf_counter()
            want = host_pairs(cols, lo, hi, sample, KP, dmin, dmax, pp.mask, frameshift)
            st["host_numpy_sample_s"] = time.perf_counter() - t0
            st["host_sample_genes"] = int(sample.size)
            st["host_numpy_all_genes_s"] = st["host_numpy_sample_s"] * lo.size / max(1, sample.size)
            st["host_fetch_columns_s"] = fetch_s
            st["equals_host"] = bool(all(np.array_equal(np.asarray(a)[sample], b) for a, b in zip(got, want)))
            st["pairs_selected"] = int((got[2][:, :, 0] != NONE).sum())
            out["runs"][name] = st
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
