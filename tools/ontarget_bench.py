#!/usr/bin/env python3
"""Times the on-target model kernel and the selection ranked by it on a genome-scale stand-in and prints
ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) with its seeded synthetic Phytozome-style GFF, as tools/select_self_bench.py
builds them: one arena.  Per case -- N20NGG with the built-in rs1 (W = 30), TTTV N23 with a seeded random model at W = 30 and at
W = 64 -- one self search at M = 1, the model kernel (its time and rows from the handle's HIP events), crp_select_run_self at
K = 5 ranked by specificity and ranked by the model (bounds, items, merge and gather times from the select handle's events),
and 4 096 sampled guide sites checked against numpy over the host's letters, bit for bit.  Next to them, from the same
session, the guide-property kernel of section 17 over the rows of one scan at guide length 20: a kernel of the same shape
(one lane per row, two plane words a lane).

    python tools/ontarget_bench.py [--workload sorghum|tair10|ecoli] [--genes N] [--out FILE]
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
SAMPLE = 4096
CASES = (("ngg-rs1", "N" * 20 + "NGG", 3, "rs1", None), ("tttv-w30", "TTTV" + "N" * 23, 4, 30, 3), ("tttv-w64", "TTTV" + "N" * 23, 4, 64, 20))
_CODE = np.full(256, 4, np.uint8)
for _ch, _v in zip(b"ATCGUatcgu", (0, 1, 2, 3, 0) * 2):
    _CODE[_ch] = _v


def random_model(W, left, G, seed=7):
    from cropsr_amd import ontarget
    rng = np.random.default_rng([seed, W])
    return ontarget.Model(W, left, float(rng.normal()), rng.normal(size=(W, 4)), rng.normal(size=(W - 1, 16)), rng.normal(size=G + 1))


def host_sums(model, text, pos, strand, T, glo, G):
    """ontarget.py's definition over the arena's letters (a byte string in arena coordinates) for the given sites."""
    from cropsr_amd import ontarget
    letters = np.concatenate([_CODE[np.frombuffer(text, np.uint8)], np.array([4], np.uint8)])
    minus = strand.astype(bool)[:, None]
    pos = pos.astype(np.int64)[:, None]

    def codes(offsets_plus, offsets_minus):
        f = np.where(minus, pos + offsets_minus, pos + offsets_plus)
        c = letters[np.where((f >= 0) & (f < len(text)), f, len(text))]
        return np.where(minus & (c < 4), c ^ 1, c)

    w = np.arange(model.window, dtype=np.int64)[None, :]
    win = codes(w - model.left, T - 1 + model.left - w)
    p = np.arange(glo, glo + G, dtype=np.int64)[None, :]
    gc = (codes(p, T - 1 - p) >> 1 == 1).sum(axis=1)
    return ontarget.sums_of_codes(model, win, gc)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["sorghum", "tair10", "ecoli"], default="sorghum")
    ap.add_argument("--genes", type=int, default=34000)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine, annotate, ontarget
    from cropsr_amd import search as srch
    from cropsr_amd import select as sel
    from cropsr_amd import select_self as ss
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
    out = dict(workload=wl.name, k=K, sampled=SAMPLE, runs={})
    with tempfile.TemporaryDirectory() as tmp:
        gff = os.path.join(tmp, "genes.gff3")
        bw.synthetic_annotation(wl, gff, None, n_genes=args.genes)
        ann = annotate.Annotation(gff)
    eng = Engine(0)
    try:
        builder = eng.arena_builder([s.length + 4 for s in wl.specs])
        strings = [wl.contig_string(k) for k in range(len(wl.specs))]
        for s in strings:
            builder.add(s)
        arena = builder.seal()
        text = bytearray(int(arena.offsets[-1]) + int(arena.lengths[-1]) + 64)
        for s, o in zip(strings, arena.offsets):
            b = s if isinstance(s, (bytes, bytearray)) else s.encode("ascii", "replace")
            text[int(o):int(o) + len(b)] = b
        text = bytes(text)
        req = annotate.Request(ann, [s.name for s in wl.specs], 1)
        layout = [(k, int(arena.offsets[k]), int(arena.lengths[k])) for k in range(len(wl.specs))]
        lo, hi, _ = req.gene_layout(layout)
        out.update(genes=int(ann.n_genes), genes_with_range=int(lo.size))
        handle = sel.ArenaSelect(arena, lo, hi)
        # section 17's property kernel over one scan's rows, from the same session
        n_plus, n_minus = arena.scan_score_device(20)
        arena.guide_properties(n_plus, n_minus, fetch=False)  # (warm)
        arena.guide_properties(n_plus, n_minus, fetch=False)
        st = arena.guide_properties_stats()
        out["properties"] = dict(kernel_ms=st["kernel_ms"], rows=st["rows"])
        rng = np.random.default_rng(1)
        for name, pattern, P, W, left in CASES:
            pattern, gp, M, P, _ = srch.check_self(pattern, 1, P, None, None)
            glo, ghi, pam3 = srch.guide_region(pattern, P)
            G, T = ghi - glo, len(pattern)
            model = ontarget.rs1() if W == "rs1" else random_model(W, left, G)
            model.check_geometry(T, P, pam3)
            c = ss.check_cut(None, T, P, pam3)
            t0 = time.perf_counter()
            h = srch.ArenaSelfSearch(arena, pattern, gp, P, M)
            try:
                srch._self_compare_all([h], M)
                search_s = time.perf_counter() - t0
                h.set_model(model, G)
                h.run_model()  # (warm: the kernel's first launch loads its code object)
                h.run_model()
                mst = h.model_stats()
                pos, strand, _, _, _, _ = h.fetch(False)
                sums = h.fetch_model()
                pick = np.sort(rng.choice(pos.size, min(SAMPLE, pos.size), replace=False))
                want = host_sums(model, text, pos[pick], strand[pick], T, glo, G)
                if not np.array_equal(sums[pick].view(np.uint64), want.view(np.uint64)):
                    raise SystemExit("ontarget_bench: a sampled site differs from numpy (%s)" % name)
                run = dict(model_ms=mst["model_ms"], model_rows=mst["model_rows"], guide_sites=int(pos.size), window=model.window,
                           sites_checked=int(pick.size), sites_without_sum=int(np.isnan(sums).sum()), self_search_s=search_s)
                for rank in ("specificity", "on-target"):
                    params = ss.Params(K, c, rank=rank).bind_model(model)
                    handle.set_self_model(rank == "on-target", None)
                    handle.run_self(params, h)  # (warm)
                    handle.run_self(params, h)
                    run[rank] = handle.self_stats()
                out["runs"][name] = run
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
