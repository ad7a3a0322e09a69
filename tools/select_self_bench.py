#!/usr/bin/env python3
"""Times the self selection on a genome-scale stand-in and prints ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) with its seeded synthetic Phytozome-style GFF, as tools/select_bench.py
builds them: one arena.  Per pattern -- ...NGG (T = 23, c = 17, hsu2013) and TTTV... (T = 27, the default c, unscored) -- one
self search at M = 3, then crp_select_run_self at K = 5 and K = 64: the bounds, items, merge and gather times from the handle's
HIP events, launches, items and candidates streamed.  Next to them, from the same session, the plain selection of section 16
(one scan at guide length 20, crp_select_run at the same K) and, per run, 64 sampled genes checked against numpy over the
fetched rows of the self search, exactly.

    python tools/select_self_bench.py [--workload sorghum|tair10|ecoli] [--genes N] [--out FILE]
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

KS = (5, 64)
NONE = 0xFFFFFFFF
PATTERNS = (("ngg", "N" * 20 + "NGG", 3, 17, "hsu2013"), ("tttv", "TTTV" + "N" * 23, 4, None, None))


def host_select(rows, lo, hi, K, T, c, scored):
    """cropsr_amd/select_self.py's definition in numpy over the fetched rows of the guide sites, for the given genes, without
    thresholds: (n_in, sel as (arena position, strand) pairs)."""
    from cropsr_amd import select_self as ss
    pos, strand, _, _, counts, hs = rows
    cut = ss.cut_letter(pos, strand, T, c)
    e = ss.scored_e(counts[:, 0], hs) if scored else ss.packed_e(counts)
    order = np.argsort(cut, kind="stable")
    cs = cut[order]
    out = []
    for a, b in zip(lo.tolist(), hi.tolist()):
        idx = order[np.searchsorted(cs, a, "left"):np.searchsorted(cs, b, "right")]
        top = idx[np.lexsort((strand[idx], cut[idx], e[idx]))][:K]
        out.append((idx.size, [(int(pos[i]), int(strand[i])) for i in top]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["sorghum", "tair10", "ecoli"], default="sorghum")
    ap.add_argument("--genes", type=int, default=34000)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine, annotate
    from cropsr_amd import search as srch
    from cropsr_amd import select as sel
    from cropsr_amd import select_self as ss
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
    out = dict(workload=wl.name, k=list(KS), runs={})
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
        req = annotate.Request(ann, [s.name for s in wl.specs], 1)
        layout = [(k, int(arena.offsets[k]), int(arena.lengths[k])) for k in range(len(wl.specs))]
        lo, hi, gene = req.gene_layout(layout)
        out.update(genes=int(ann.n_genes), genes_with_range=int(lo.size))
        handle = sel.ArenaSelect(arena, lo, hi)
        # section 16's plain selection of the same session
        n_plus, n_minus = arena.scan_score_device(20)
        out["scan_rows"] = int(n_plus + n_minus)
        for K in KS:
            handle.run(sel.Params(K))  # (warm)
            handle.run(sel.Params(K))
            st = handle.stats()
            out["runs"]["plain-k%d" % K] = dict(bounds_ms=st["bounds_ms"], select_ms=st["select_ms"], merge_ms=st["merge_ms"],
                                                items=st["items"], rows_in_runs=st["rows_in_runs"])
        rng = np.random.default_rng(1)
        sample = np.sort(rng.choice(lo.size, min(64, lo.size), replace=False)) if lo.size else np.zeros(0, np.int64)
        for name, pattern, P, c, score in PATTERNS:
            pattern, gp, M, P, scheme = srch.check_self(pattern, 3, P, None, score)
            _, _, pam3 = srch.guide_region(pattern, P)
            c = ss.check_cut(c, len(pattern), P, pam3)
            t0 = time.perf_counter()
            h = srch.ArenaSelfSearch(arena, pattern, gp, P, M)
            try:
                if scheme is not None:
                    h.set_scheme(scheme)
                srch._self_compare_all([h], M)
                search_s = time.perf_counter() - t0
                rows = h.fetch(scheme is not None)
                for K in KS:
                    params = ss.Params(K, c)
                    handle.run_self(params, h)  # (warm: the kernels' first launch loads their code object)
                    handle.run_self(params, h)
                    st = handle.self_stats()
                    got = handle.fetch_self()
                    want = host_select(rows, lo[sample], hi[sample], K, len(pattern), c, scheme is not None)
                    for g, (n_in, top) in zip(sample.tolist(), want):
                        have = got["sel"][g] != NONE
                        mine = list(zip(got["arena_pos"][g][have].tolist(), got["strand"][g][have].tolist()))
                        if int(got["n_in"][g]) != n_in or mine != top:
                            raise SystemExit("select_self_bench: gene row %d differs from numpy (%s, K = %d)" % (g, name, K))
                    out["runs"]["%s-k%d" % (name, K)] = dict(st, guide_sites=int(rows[0].size), self_search_s=search_s, cut_offset=c,
                                                             genes_checked=int(sample.size))
            finally:
                h.close()
        handle.close()
        arena.close()
    finally:
        eng.close()
        ann.close()
    line = json.dumps(out, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
