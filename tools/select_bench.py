#!/usr/bin/env python3
"""Times the guide selection on a genome-scale stand-in and prints ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) with its seeded synthetic Phytozome-style GFF, as
tests/test_annotate.py::test_gpu_annotate_at_genome_scale builds them: one arena, one scan at guide length 20, the
annotation look-up (whose HIP-event time gives the HBM rate a streaming kernel reaches on these very tables), then
crp_select_run at K = 5 and K = 64, without and -- unless --no-specificity -- with the joined columns of a self search
(M = 3, hsu2013).  Per run: the bounds, select and merge times from HIP events, items, launches, the longest launch,
rows in the genes' runs and bytes read per row.  Two yardsticks from the same run stand next to them:

  host        what a user does today: the same columns fetched to the host, then the selection with numpy (run bounds
              by searchsorted, a lexsort per gene); the run checks the device's result against it, exactly
  floor_ms    the select kernel's traffic floor: rows in runs x bytes read per row / the annotation look-up's rate

    python tools/select_bench.py [--workload sorghum|tair10|ecoli] [--genes N] [--no-specificity] [--out FILE]
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


def host_select(cols, lo, hi, K, spec=None):
    """The definition of cropsr_amd/select.py in numpy over host copies of the columns: (n_in, n_pass, sel)."""
    pos_p, sc_p, pos_m, sc_m = cols
    cut_p = pos_p.astype(np.int64) - 3
    cut_m = pos_m.astype(np.int64)
    b = [np.searchsorted(cut_p, lo.astype(np.int64), "left"), np.searchsorted(cut_p, hi.astype(np.int64), "right"),
         np.searchsorted(cut_m, lo.astype(np.int64), "left"), np.searchsorted(cut_m, hi.astype(np.int64), "right")]
    G = lo.size
    n_in, n_pass, sel = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.full((G, K), NONE, np.uint32)
    ok_p, ok_m = sc_p != -1.0, sc_m != -1.0
    pass_p, pass_m = ok_p.copy(), ok_m.copy()
    if spec is not None:
        cp, sp, cm, sm = spec
        pass_p &= cp[:, 0] != NONE
        pass_m &= cm[:, 0] != NONE
    for g in range(G):
        p0, p1, m0, m1 = (int(x[g]) for x in b)
        n_in[g] = ok_p[p0:p1].sum() + ok_m[m0:m1].sum()
        rp, rm = p0 + np.flatnonzero(pass_p[p0:p1]), m0 + np.flatnonzero(pass_m[m0:m1])
        n_pass[g] = rp.size + rm.size
        key = np.concatenate([sc_p[rp], sc_m[rm]]).view(np.uint64)
        cut = np.concatenate([cut_p[rp], cut_m[rm]])
        strand = np.concatenate([np.zeros(rp.size, np.int64), np.ones(rm.size, np.int64)])
        order = np.lexsort((strand, cut, np.iinfo(np.uint64).max - key))[:K]
        sel[g, :order.size] = (np.concatenate([rp, rm])[order] | (strand[order] << 31)).astype(np.uint32)
    return n_in, n_pass, sel


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["sorghum", "tair10", "ecoli"], default="sorghum")
    ap.add_argument("--genes", type=int, default=34000)
    ap.add_argument("--no-specificity", action="store_true", help="skip the runs that read the self search's joined columns")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine, annotate
    from cropsr_amd import search as srch
    from cropsr_amd import select as sel
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
        variants = [("plain", None)]
        spec_handle, spec_cols = None, None
        if not args.no_specificity:
            pattern, gp, M, scheme = srch.check_specificity(20, 3)
            t0 = time.perf_counter()
            spec_handle = srch.ArenaSelfSearch(arena, pattern, gp, srch.SPECIFICITY_PAM_LEN, M)
            spec_handle.set_scheme(scheme)
            srch._self_compare_all([spec_handle], M)
            spec_cols = spec_handle.join_hits(20)
            out["self_search_and_join_s"] = time.perf_counter() - t0
            variants.append(("specificity", spec_handle))
        t0 = time.perf_counter()
        cols = arena.fetch(n_plus, n_minus)
        cols = (cols[0], cols[2], cols[3], cols[5])
        fetch_s = time.perf_counter() - t0
        for name, h in variants:
            for K in KS:
                params = sel.Params(K)
                handle.run(params, h)  # (warm: the kernels' first launch loads their code object)
                handle.run(params, h)
                st = handle.stats()
                t0 = time.perf_counter()
                got = handle.fetch()
                st["fetch_result_s"] = time.perf_counter() - t0
                st["floor_ms"] = st["rows_in_runs"] * st["bytes_per_row"] / rate * 1e3
                st["select_share_of_floor"] = st["floor_ms"] / st["select_ms"] if st["select_ms"] else None
                t0 = time.perf_counter()
                want = host_select(cols, lo, hi, K, spec_cols if h is not None else None)
                st["host_numpy_s"] = time.perf_counter() - t0
                st["host_fetch_columns_s"] = fetch_s
                st["equals_host"] = bool(all(np.array_equal(a, b) for a, b in zip(got, want)))
                st["rows_selected"] = int((got[2] != NONE).sum())
                out["runs"]["%s_k%d" % (name, K)] = st
        handle.close()
        if spec_handle is not None:
            spec_handle.close()
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
