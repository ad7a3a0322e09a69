#!/usr/bin/env python3
"""Times the guide selection with coding limits on a genome-scale stand-in and prints ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) with its seeded synthetic Phytozome-style GFF, as
tools/select_bench.py builds them: one arena, one scan at guide length 20, the genes' coding model laid out on the host
(timed), then at K = 5, each after a warming run and from HIP events:

  plain       crp_select_run without coding limits -- select_items_kernel, whose assembly is the parent commit's
              instruction for instruction (profiles/EXPERIMENTS.md, "Coding position"), so this is the parent's time
  coding      the same selection with --select-coding-min 5 --select-coding-max 65 -- select_items_coding_kernel
  eval        crp_select_coding_eval over the rows the coding run selected

and the ratio coding / plain of the select launches.  The run checks the device against the host: the plain and the
coding selection against numpy over fetched columns, with the coding test read from the laid-out step functions.

    python tools/coding_bench.py [--workload sorghum|tair10|ecoli] [--genes N] [--out FILE]
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

K = 5
LIMITS = (5, 65, 0)
NONE = 0xFFFFFFFF


def host_position(model, g, c):
    """(off, cover) int64 arrays of the boundaries c for layout row g, from the step function (off -1: not inside P)."""
    a, b = int(model["first"][g]), int(model["first"][g + 1])
    off, cover = np.full(c.shape, -1, np.int64), np.zeros(c.shape, np.int64)
    info, L = int(model["info"][g]), int(model["length"][g])
    if not info >> 17 & 1 or a == b:
        return off, cover
    at, word, cum = (model[key][a:b].astype(np.int64) for key in ("at", "word", "cum"))
    k = np.searchsorted(at, c, "right") - 1
    has = k >= 0
    k = np.maximum(k, 0)
    cover[has] = (word[k] & 0xFFFF)[has]
    inside = has & ((word[k] >> 16 & 1) == 1)
    before = cum[k] + (word[k] >> 17 & 1) * (c - at[k])
    off[inside] = (L - before if info >> 16 & 1 else before)[inside]
    return off, cover


def host_select(cols, lo, hi, model, limits):
    """The definition in numpy over host copies of the columns: (n_in, n_pass, sel); limits None: the plain selection."""
    pos_p, sc_p, pos_m, sc_m = cols
    cut_p, cut_m = pos_p.astype(np.int64) - 3, pos_m.astype(np.int64)
    b = [np.searchsorted(cut_p, lo.astype(np.int64), "left"), np.searchsorted(cut_p, hi.astype(np.int64), "right"),
         np.searchsorted(cut_m, lo.astype(np.int64), "left"), np.searchsorted(cut_m, hi.astype(np.int64), "right")]
    G = lo.size
    n_in, n_pass, sel = np.zeros(G, np.uint32), np.zeros(G, np.uint32), np.full((G, K), NONE, np.uint32)
    ok_p, ok_m = sc_p != -1.0, sc_m != -1.0
    for g in range(G):
        p0, p1, m0, m1 = (int(x[g]) for x in b)
        n_in[g] = ok_p[p0:p1].sum() + ok_m[m0:m1].sum()
        rp, rm = p0 + np.flatnonzero(ok_p[p0:p1]), m0 + np.flatnonzero(ok_m[m0:m1])
        if limits is not None:
            L, n_tx = int(model["length"][g]), int(model["info"][g]) & 0xFFFF
            keep = []
            for rows, c in ((rp, cut_p[rp]), (rm, cut_m[rm] + 6)):
                off, cover = host_position(model, g, c)
                keep.append(rows[(off >= 0) & (limits[0] * L <= 100 * off) & (100 * off <= limits[1] * L) & (100 * cover >= limits[2] * n_tx)])
            rp, rm = keep
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
    ap.add_argument("--repeats", type=int, default=5, help="timed runs per variant; the median is reported")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine, annotate, coding
    from cropsr_amd import select as sel
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
    out = dict(workload=wl.name, k=K, limits=list(LIMITS))
    with tempfile.TemporaryDirectory() as tmp:
        gff = os.path.join(tmp, "genes.gff3")
        bw.synthetic_annotation(wl, gff, None, n_genes=args.genes)
        t0 = time.perf_counter()
        ann = annotate.Annotation(gff)
        out["annotation_build_s"] = time.perf_counter() - t0
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
        t0 = time.perf_counter()
        model = req.coding_layout(layout)
        out["coding_layout_s"] = time.perf_counter() - t0
        n_tx = model["info"] & np.uint32(0xFFFF)
        out.update(rows=int(n_plus + n_minus), genes=int(ann.n_genes), genes_with_range=int(lo.size),
                   genes_with_model=int((model["info"] >> np.uint32(17) & np.uint32(1)).sum()), steps=int(model["at"].size),
                   steps_per_gene_max=int(np.diff(model["first"].astype(np.int64)).max()), transcripts_max=int(n_tx.max()))
        handle = sel.ArenaSelect(arena, lo, hi)
        handle.set_coding(model)
        cols = arena.fetch(n_plus, n_minus)
        cols = (cols[0], cols[2], cols[3], cols[5])
        params = sel.Params(K)
        results = {}
        for name, limits in (("plain", None), ("coding", LIMITS)):
            handle.set_coding_limits(None if limits is None else coding.Limits(*limits))
            handle.run(params)  # (warm: the kernels' first launch loads their code object)
            times = []
            for _ in range(args.repeats):
                handle.run(params)
                times.append(handle.stats())
            st = sorted(times, key=lambda t: t["select_ms"])[len(times) // 2]
            st["select_ms_all"] = [t["select_ms"] for t in times]
            got = handle.fetch()
            want = host_select(cols, lo, hi, model, limits)
            st["equals_host"] = bool(all(np.array_equal(a, b) for a, b in zip(got, want)))
            st["rows_selected"] = int((got[2] != NONE).sum())
            st["rows_passing"] = int(got[1].sum())
            results[name] = got
            out[name] = st
        out["coding_over_plain"] = out["coding"]["select_ms"] / out["plain"]["select_ms"] if out["plain"]["select_ms"] else None
        picked = results["coding"][2]
        r, c = np.nonzero(picked != NONE)
        handle.coding_eval(r.astype(np.uint32), picked[r, c])  # (warm)
        evals = []
        for _ in range(args.repeats):
            off, cover = handle.coding_eval(r.astype(np.uint32), picked[r, c])
            evals.append(handle.coding_stats()["coding_eval_ms"])
        L = model["length"][r].astype(np.int64)
        out["eval"] = dict(queries=int(r.size), eval_ms=sorted(evals)[len(evals) // 2], eval_ms_all=evals,
                           all_inside_limits=bool(((off != coding.NOT_INSIDE) & (LIMITS[0] * L <= 100 * off.astype(np.int64))
                                                   & (100 * off.astype(np.int64) <= LIMITS[1] * L)).all()))
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
    return 0 if out["plain"]["equals_host"] and out["coding"]["equals_host"] and out["eval"]["all_inside_limits"] else 1


if __name__ == "__main__":
    sys.exit(main())
