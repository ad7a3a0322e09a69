#!/usr/bin/env python3
"""Times the guide selection with splice limits on a genome-scale stand-in and prints ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) with its seeded synthetic Phytozome-style GFF, as
tools/edit_bench.py builds them: one arena, one scan at guide length 20, the genes' coding model laid out on the host,
then at K = 5, each after a warming run and from HIP events, all in one session:

  plain        crp_select_run without limits -- select_items_kernel, whose assembly is the parent commit's instruction for
               instruction (profiles/EXPERIMENTS.md, "Splice-site editing"), so this is the parent's time
  edit         the same selection with --select-stop --select-stop-min 5 --select-stop-max 65 -- select_items_edit_kernel,
               the nearest existing yardstick, also the parent's assembly
  splice_cbe   the same selection with --select-splice --select-splice-min 5 --select-splice-max 65 --
  splice_abe   select_items_splice_kernel, for either editor
  eval         crp_select_splice_eval over the rows the cbe run selected

and the ratios splice / edit and splice / plain of the select launches.  The run checks the device against the host: the
plain and both splice selections against numpy over fetched columns, the splice test restated over the genome's letters
and the laid-out step functions.

    python tools/splice_bench.py [--workload sorghum|tair10|ecoli] [--genes N] [--out FILE]
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
WINDOW = (4, 8)
LIMITS = (5, 65, 20)
KINDS = "any"
NONE = 0xFFFFFFFF
CODE = np.full(256, 4, np.int8)  # 0 A, 1 T, 2 C, 3 G (the planes' codes), 4: non-base
for _ch, _c in zip(b"AaUuTtCcGg", (0, 0, 0, 0, 1, 1, 2, 2, 3, 3)):
    CODE[_ch] = _c


def host_splice(model, g, letters, pos, minus, editor):
    """(targets, donor_off, acceptor_off) int64 arrays of the rows with match indices pos on one strand for layout row g (an
    off is -1 without a destroyed site of that kind), by the masks over the letters (a uint8 array by arena position) and
    the step function."""
    lo, hi = WINDOW
    wn, ns = hi - lo + 1, hi - lo + 5
    x0 = pos.astype(np.int64) + (21 - hi if minus else lo - 23)
    X = x0[:, None] + np.arange(ns)[None, :]
    code = np.where((X >= 0) & (X < letters.size), CODE[letters[np.clip(X, 0, letters.size - 1)]], 4)
    A, T, C, G = (code == v for v in range(4))
    W = np.zeros(ns, bool)
    W[2:2 + wn] = True
    tg = ((T if minus else A) if editor == "abe" else (G if minus else C)) & W[None, :]
    targets = tg.sum(axis=1)
    none = np.full(pos.size, -1, np.int64)
    a, b = int(model["first"][g]), int(model["first"][g + 1])
    info, L = int(model["info"][g]), int(model["length"][g])
    if not info >> 17 & 1 or a == b or not pos.size:
        return targets, none, none.copy()
    at, word, cum = (model[key][a:b].astype(np.int64) for key in ("at", "word", "cum"))
    k = np.searchsorted(at, X, "right") - 1
    kk = np.maximum(k, 0)
    grow = (k >= 0) & ((word[kk] >> 17 & 1) == 1)
    c = np.where(k >= 0, cum[kk] + np.where(grow, X - at[kk], 0), cum[0])  # cum_P at the boundary below each letter
    gene_minus = bool(info >> 16 & 1)
    s = lambda m, j: m[:, 1 + j:ns - 2 + j]  # column x + j beside column x, x = 1 .. ns - 3: the sites' lower letters
    hit = s(tg, 0) | s(tg, 1)
    clear = ~s(grow, 0) & ~s(grow, 1)
    starts = s(grow, -1) & clear & (s(c, 0) < L) & s(C if gene_minus else G, 0) & s(T, 1) & hit
    ends = clear & s(grow, 2) & (s(c, 2) > 0) & s(A, 0) & s(C if gene_minus else G, 1) & hit
    big = np.iinfo(np.int64).max
    out = []
    for mask, before in ((starts, s(c, 0)), (ends, s(c, 2))):
        off = L - before if gene_minus else before
        best = np.where(mask, off, big).min(axis=1)
        out.append(np.where(mask.any(axis=1), best, -1))
    donor, acceptor = (out[1], out[0]) if gene_minus else (out[0], out[1])
    return targets, donor, acceptor


def host_select(cols, lo, hi, model, letters, limits, editor="cbe"):
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
            L = int(model["length"][g])
            keep = []
            for rows, pos, minus in ((rp, pos_p[rp], False), (rm, pos_m[rm], True)):
                targets, donor, acceptor = host_splice(model, g, letters, pos, minus, editor)
                inside = lambda off: (off >= 0) & (limits[0] * L <= 100 * off) & (100 * off <= limits[1] * L)
                keep.append(rows[(inside(donor) | inside(acceptor)) & (targets <= limits[2])])
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
    from cropsr_amd import Engine, annotate, baseedit
    from cropsr_amd import select as sel
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
    out = dict(workload=wl.name, k=K, window=list(WINDOW), limits=list(LIMITS), kinds=KINDS)
    with tempfile.TemporaryDirectory() as tmp:
        gff = os.path.join(tmp, "genes.gff3")
        bw.synthetic_annotation(wl, gff, None, n_genes=args.genes)
        ann = annotate.Annotation(gff)
    eng = Engine(0)
    try:
        builder = eng.arena_builder([s.length + 4 for s in wl.specs])
        strings = []
        for k in range(len(wl.specs)):
            strings.append(wl.contig_string(k))
            builder.add(strings[-1])
        arena = builder.seal()
        letters = np.zeros(int(arena.offsets[-1]) + int(arena.lengths[-1]) + 64, np.uint8)  # the letters by arena position, for the host's check
        for k, s in enumerate(strings):
            letters[int(arena.offsets[k]):int(arena.offsets[k]) + len(s)] = np.frombuffer(bytes(s), np.uint8)
        del strings
        n_plus, n_minus = arena.scan_score_device(20)
        req = annotate.Request(ann, [s.name for s in wl.specs], 1)
        layout = [(k, int(arena.offsets[k]), int(arena.lengths[k])) for k in range(len(wl.specs))]
        lo, hi, gene = req.gene_layout(layout)
        model = req.coding_layout(layout)
        out.update(rows=int(n_plus + n_minus), genes=int(ann.n_genes), genes_with_range=int(lo.size),
                   genes_with_model=int((model["info"] >> np.uint32(17) & np.uint32(1)).sum()), steps=int(model["at"].size),
                   steps_per_gene_max=int(np.diff(model["first"].astype(np.int64)).max()))
        handle = sel.ArenaSelect(arena, lo, hi)
        handle.set_coding(model)
        cols = arena.fetch(n_plus, n_minus)
        cols = (cols[0], cols[2], cols[3], cols[5])
        params = sel.Params(K)
        window = baseedit.Window(*WINDOW)
        results = {}
        for name in ("plain", "edit", "splice_cbe", "splice_abe"):
            editor = name[-3:] if name.startswith("splice") else "cbe"
            handle.set_edit_limits(window, baseedit.Limits(*LIMITS) if name == "edit" else None)
            handle.set_splice_limits(window, editor, baseedit.SpliceLimits(*LIMITS, kinds=KINDS) if name.startswith("splice") else None)
            handle.run(params)  # (warm: the kernels' first launch loads their code object)
            times = []
            for _ in range(args.repeats):
                handle.run(params)
                times.append(handle.stats())
            st = sorted(times, key=lambda t: t["select_ms"])[len(times) // 2]
            st["select_ms_all"] = [t["select_ms"] for t in times]
            got = handle.fetch()
            if name != "edit":  # (tools/edit_bench.py checks that one)
                t0 = time.perf_counter()
                want = host_select(cols, lo, hi, model, letters, LIMITS if name != "plain" else None, editor)
                st["equals_host"] = bool(all(np.array_equal(a, b) for a, b in zip(got, want)))
                st["host_check_s"] = time.perf_counter() - t0
            st["rows_selected"] = int((got[2] != NONE).sum())
            st["rows_passing"] = int(got[1].sum())
            results[name] = got
            out[name] = st
        for name in ("splice_cbe", "splice_abe"):
            out[name + "_over_edit"] = out[name]["select_ms"] / out["edit"]["select_ms"] if out["edit"]["select_ms"] else None
            out[name + "_over_plain"] = out[name]["select_ms"] / out["plain"]["select_ms"] if out["plain"]["select_ms"] else None
        picked = results["splice_cbe"][2]
        r, c = np.nonzero(picked != NONE)
        handle.splice_eval(window, "cbe", r.astype(np.uint32), picked[r, c])  # (warm)
        evals = []
        for _ in range(args.repeats):
            targets, donors, acceptors, d_off, a_off = handle.splice_eval(window, "cbe", r.astype(np.uint32), picked[r, c])
            evals.append(handle.splice_stats()["splice_eval_ms"])
        L = model["length"][r].astype(np.int64)
        inside = lambda off: (off != baseedit.NO_SITE) & (LIMITS[0] * L <= 100 * off.astype(np.int64)) & (100 * off.astype(np.int64) <= LIMITS[1] * L)
        out["eval"] = dict(queries=int(r.size), eval_ms=sorted(evals)[len(evals) // 2], eval_ms_all=evals,
                           all_inside_limits=bool(((inside(d_off) | inside(a_off)) & (donors + acceptors >= 1) & (targets <= LIMITS[2])).all()))
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
    return 0 if all(out[name]["equals_host"] for name in ("plain", "splice_cbe", "splice_abe")) and out["eval"]["all_inside_limits"] else 1


if __name__ == "__main__":
    sys.exit(main())
