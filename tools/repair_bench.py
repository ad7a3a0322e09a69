#!/usr/bin/env python3
"""Times the repair outcome kernel on a genome-scale stand-in and prints ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) in one arena, one scan at guide length 20, then crp_repair_scores
on the resident tables at flank 30 and flank 32: rows, the kernel's HIP-event time, rows per second.  Two yardsticks come
from the same run on the same tables: the guide property kernel (crp_guide_properties), the nearest existing kernel of
this shape, and the selection (K = 5 over the seeded synthetic genes of tools/select_bench.py) without and with repair
limits, which read 8 more bytes per row.  A spread of rows is checked against a plain restatement of the definition.

    python tools/repair_bench.py [--workload sorghum|tair10|ecoli] [--genes N] [--out FILE]
"""
import argparse
import json
import math
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BASE = {65: 0, 85: 0, 84: 1, 67: 2, 71: 3, 97: 0, 116: 1, 99: 2, 103: 3}  # A U T C G a t c g -> the planes' codes
W = [0] + [int(math.floor(1000.0 * math.exp(-d / 20.0) + 0.5)) for d in range(1, 64)]
FLANKS = (30, 32)


def host_row(text, pos, minus, F):
    """mh | oof << 32 of one row, by the definition (cropsr_amd/repair.py) as a plain loop over the diagonals."""
    c = pos + 6 if minus else pos - 3
    w = [BASE.get(text[k]) if 0 <= k < len(text) else None for k in range(c - F, c + F)]
    mh = oof = 0
    for d in range(1, 2 * F):
        lo, hi = max(0, F - d), min(F, 2 * F - d)
        n = run = gc = 0
        for p in range(lo, hi + 1):
            if p < hi and w[p] is not None and w[p] == w[p + d]:
                run += 1
                gc += w[p] >= 2
                continue
            if run >= 2:
                n += run + gc
            run = gc = 0
        mh += W[d] * n
        oof += W[d] * n if d % 3 else 0
    return mh | oof << 32


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["sorghum", "tair10", "ecoli"], default="sorghum")
    ap.add_argument("--genes", type=int, default=34000)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine, annotate, repair
    from cropsr_amd import select as sel
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
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
        rows = n_plus + n_minus
        out = dict(workload=wl.name, rows=int(rows), flanks={})
        for F in FLANKS:
            arena.repair_scores(n_plus, n_minus, F, fetch=False)  # (warm: a kernel's first launch loads its code object)
            arena.repair_scores(n_plus, n_minus, F, fetch=False)
            ms = arena.repair_scores_stats()["kernel_ms"]
            out["flanks"][str(F)] = dict(kernel_ms=ms, rows_per_s=rows / (ms * 1e-3), diagonals=2 * F - 1,
                                         ns_per_row_and_diagonal=ms * 1e6 / rows / (2 * F - 1))
        arena.guide_properties(n_plus, n_minus, fetch=False)  # (warm)
        arena.guide_properties(n_plus, n_minus, fetch=False)
        props_ms = arena.guide_properties_stats()["kernel_ms"]
        out.update(properties_kernel_ms=props_ms, kernel_ms_f30_over_properties_ms=out["flanks"]["30"]["kernel_ms"] / props_ms)
        # the selection over the same tables, without and with repair limits (the column of flank 30)
        rp, rm = arena.repair_scores(n_plus, n_minus, 30)
        req = annotate.Request(ann, [s.name for s in wl.specs], 1)
        lo, hi, _ = req.gene_layout([(k, int(arena.offsets[k]), int(arena.lengths[k])) for k in range(len(wl.specs))])
        handle = sel.ArenaSelect(arena, lo, hi)
        runs = {}
        for name, limits in (("plain", None), ("repair_limits", repair.Limits(min_mh=20000, min_oof=60))):
            handle.set_repair_limits(limits)
            handle.run(sel.Params(5))  # (warm)
            handle.run(sel.Params(5))
            st = handle.stats()
            n_in, n_pass, _ = handle.fetch()
            runs[name] = dict(select_ms=st["select_ms"], bounds_ms=st["bounds_ms"], merge_ms=st["merge_ms"], bytes_per_row=st["bytes_per_row"],
                              rows_in_runs=st["rows_in_runs"], rows_in=int(n_in.sum()), rows_passing=int(n_pass.sum()))
        handle.close()
        out.update(genes_with_range=int(lo.size), select_k5=runs)
        # a spread of rows of the first contig against the definition
        cols = arena.fetch(n_plus, n_minus)
        text = bytes(wl.contig_string(0))
        off = int(arena.offsets[0])
        checked = 0
        for pos, col, minus in ((cols[0], rp, False), (cols[3], rm, True)):
            n0 = int(np.searchsorted(pos, np.uint32(off + len(text))))
            for r in list(range(0, n0, max(1, n0 // 200))) + list(range(max(0, n0 - 20), n0)):
                assert int(col[r]) == host_row(text, int(pos[r]) - off, minus, 30), (minus, r)
                checked += 1
        out["rows_checked_against_the_definition"] = checked
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
