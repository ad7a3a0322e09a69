#!/usr/bin/env python3
"""Times the guide property kernel on a genome-scale stand-in and prints ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) in one arena, one scan at the guide length asked for, then
crp_guide_properties on the resident tables: rows, the kernel's HIP-event time, rows per second, the algorithmic bytes
(4 B position in, 4 B packed word out per row, and the three planes it reads once: hi, lo, ac) and the rate they were
moved at.  The yardstick next to it comes from the same run: the annotation look-up, a streaming kernel over the same
rows (12 B in, 4 B out per row), with a track of one point per contig.  A spread of rows is checked against a plain
restatement of the definition.

    python tools/properties_bench.py [--workload sorghum|tair10|ecoli] [--length L] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BASE = {65: 0, 85: 0, 84: 1, 67: 2, 71: 3, 97: 0, 116: 1, 99: 2, 103: 3}  # A U T C G a t c g -> the planes' codes


def host_row(text, pos, minus, l):
    """The packed word of one row, by the definition (cropsr_amd/properties.py) as a plain loop."""
    start = pos + 3 if minus else pos - l
    w = [BASE.get(text[k]) if 0 <= k < len(text) else None for k in range(start, start + l)]
    gc = sum(1 for c in w if c in (2, 3))
    run = t_run = cur = cur_t = 0
    prev = None
    for c in w:
        cur = 0 if c is None else (cur + 1 if c == prev else 1)
        cur_t = cur_t + 1 if c == (0 if minus else 1) else 0
        prev = c
        run, t_run = max(run, cur), max(t_run, cur_t)
    stem = 0
    for c in range(4, 2 * l - 1):
        cur = 0
        for p in range(l):
            q = c - p
            cur = cur + 1 if 0 <= q < l and q - p >= 4 and w[p] is not None and w[q] is not None and w[p] ^ 1 == w[q] else 0
            stem = max(stem, cur)
    return gc | run << 8 | t_run << 16 | stem << 24


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["sorghum", "tair10", "ecoli"], default="sorghum")
    ap.add_argument("--length", type=int, default=20, help="guide length of the scan (1..50)")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
    l = args.length
    eng = Engine(0)
    try:
        builder = eng.arena_builder([s.length + 4 for s in wl.specs])
        for k in range(len(wl.specs)):
            builder.add(wl.contig_string(k))
        arena = builder.seal()
        n_plus, n_minus = arena.scan_score_device(l)
        rows = n_plus + n_minus
        arena.guide_properties(n_plus, n_minus, fetch=False)  # (warm: a kernel's first launch loads its code object)
        arena.guide_properties(n_plus, n_minus, fetch=False)
        st = arena.guide_properties_stats()
        # the yardstick: the annotation look-up over the same tables
        arena.annotate_set_track(np.asarray(arena.offsets, dtype=np.uint32), np.zeros(len(arena.offsets), dtype=np.uint32))
        arena.annotate_lookup(n_plus, n_minus, fetch=False)
        eng.profile(2)
        eng.profile_read()
        arena.annotate_lookup(n_plus, n_minus, fetch=False)
        annot_ms = eng.profile_read()["annotate"]["ms"]
        eng.profile(0)
        words = arena.stats()["n_words"]
        algo_bytes = rows * 8 + 3 * 8 * words
        ms = st["kernel_ms"]
        out = dict(workload=wl.name, guide_len=l, rows=int(rows), kernel_ms=ms, rows_per_s=rows / (ms * 1e-3), algorithmic_bytes=int(algo_bytes),
                   achieved_GB_per_s=algo_bytes / (ms * 1e-3) / 1e9, annot_lookup_ms=annot_ms, annot_lookup_rows_per_s=rows / (annot_ms * 1e-3),
                   annot_lookup_GB_per_s=rows * 16 / (annot_ms * 1e-3) / 1e9, kernel_ms_over_annot_lookup_ms=ms / annot_ms)
        # a spread of rows of the first contig against the definition
        pp, pm = arena.guide_properties(n_plus, n_minus)
        cols = arena.fetch(n_plus, n_minus)
        text = bytes(wl.contig_string(0))
        end = int(arena.offsets[0]) + len(text)
        checked = 0
        for pos, props, minus in ((cols[0], pp, False), (cols[3], pm, True)):
            n0 = int(np.searchsorted(pos, np.uint32(end)))
            for r in list(range(0, n0, max(1, n0 // 200))) + list(range(max(0, n0 - 20), n0)):
                assert int(props[r]) == host_row(text, int(pos[r]) - int(arena.offsets[0]), minus, l), (minus, r)
                checked += 1
        out["rows_checked_against_the_definition"] = checked
        arena.close()
    finally:
        eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
