#!/usr/bin/env python3
"""Times the greedy family sets on a genome-scale stand-in and prints ONE JSON line.

The workload is tools/family_bench.py's: the sorghum-like genome with its seeded synthetic GFF and families of --family-size
planted as copies of the first member with --substitutions random substitutions per letter, as homeologs are.  Then, in one
session, a scan at guide length 20 and

  family    --specificity --select K --families with --select-min-members all --select-max-perfect-outside 0: the family
            selection, whose launch time is the yardstick -- the PARENT's kernel over the same rows
  sets      --specificity --select K --families --family-sets S: the same and then S greedy steps

a warming run and --repeats timed ones each.  Reported: per step the step kernel's and the pick kernel's time (HIP events,
summed over the arenas; the median over the runs), the family selection's launch time of the same session, and the ratio of
the first step's step_ms to it: a step reads the same columns per row and keeps one entry where that kernel keeps K.

The run checks the device against the host: for --sample families with a pick, the candidates are rebuilt from the fetched
tables (the scored, joined rows that cut inside a member) and the genome's letters (family_bench.host_family_rows gives every
candidate's site_family and fam_cover), the greedy set is recomputed in Python ints (host_family_set below) and compared
with the device's picks field by field.

    python tools/family_sets_bench.py [--workload sorghum|tair10|ecoli] [--genes N] [--family-size 4] [--steps 4] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import family_bench as fb  # noqa: E402

K = 5
GUIDE_LEN = fb.GUIDE_LEN
NONE = fb.NONE


def host_family_set(cands, size, steps):
    """The greedy set over cands [(key, contig, cut << 1 | strand, gene, cover)], all of one family of `size` members: picks
    [(step, index into cands, gain, covered)] by the definition's order -- larger gain, higher key, then (arena positions ascend
    with contig and position) the smaller contig, tie and gene."""
    covered, full, picks = 0, (1 << size) - 1, []
    for step in range(1, steps + 1):
        best, best_rank = None, None
        for i, (key, contig, tie, gene, cover) in enumerate(cands):
            gain = bin(cover & ~covered).count("1")
            if not gain:
                continue
            rank = (-gain, -key, contig, tie, gene)
            if best is None or rank < best_rank:
                best, best_rank = i, rank
        if best is None:
            break
        gain = -best_rank[0]
        covered |= cands[best][4]
        picks.append((step, best, gain, covered))
        if covered == full:
            break
    return picks, covered == full


def family_candidates(f, table, ranges, tables, columns, texts, genes, gene_family, gene_member, max_mm):
    """The candidates of family f from the fetched tables: per member gene the scored, joined rows whose cut lies in its range;
    each row's cover word from the letters (fb.host_family_rows).  Returns (cands for host_family_set, [(gene, contig, position,
    strand)] beside them)."""
    from cropsr_amd import _native as nat
    cands, where = [], []
    for g in table.members(f).tolist():
        k, lo, hi = ranges[g]
        for strand, name in ((0, "plus"), (1, "minus")):
            pos, score = tables[k]["pos_" + name].astype(np.int64), tables[k]["score_" + name]
            cut = pos - 3 if strand == 0 else pos
            c0 = columns[k]["self_counts_" + name][:, 0]
            rows = np.nonzero((cut >= lo) & (cut <= hi) & (score != -1.0) & (c0 != nat.SELF_UNJOINED_COUNT))[0]
            sites = [(k, int(pos[r]) - GUIDE_LEN if strand == 0 else int(pos[r]), strand) for r in rows.tolist()]
            got = fb.host_family_rows(texts, genes, gene_family, gene_member, f, sites, max_mm, 0)
            for r, (site_family, _, _, cover) in zip(rows.tolist(), got):
                c = (cover if site_family == f else 0) | 1 << gene_member[g]
                cands.append((int(np.float64(score[r]).view(np.uint64)), k, int(cut[r]) << 1 | strand, g, c))
                where.append((g, k, int(pos[r]), strand))
    return cands, where


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["sorghum", "tair10", "ecoli"], default="sorghum")
    ap.add_argument("--genes", type=int, default=34000)
    ap.add_argument("--family-size", type=int, default=4)
    ap.add_argument("--substitutions", type=float, default=0.02)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--max-mm", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per variant; the median is reported")
    ap.add_argument("--sample", type=int, default=64, help="families recomputed on the host")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine, annotate, families as fam
    from cropsr_amd import _native as nat
    from cropsr_amd import select as sel
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
    out = dict(workload=wl.name, build_id=nat.lib().crp_build_id().decode(), k=K, steps=args.steps, max_mm=args.max_mm, family_size=args.family_size,
               substitutions=args.substitutions)
    rng = np.random.default_rng(24)
    with tempfile.TemporaryDirectory() as tmp:
        gff = os.path.join(tmp, "genes.gff3")
        bw.synthetic_annotation(wl, gff, None, n_genes=args.genes)
        ann = annotate.Annotation(gff)
    names = [s.name for s in wl.specs]
    labels, seqids, start, end = ann.genes()
    index = {n: k for k, n in enumerate(names)}
    idents = [lb[len(fam.LABEL_PREFIX):] for lb in labels]
    gene_rows = [(i, index[s], int(a), int(b)) for i, s, a, b in zip(idents, seqids, start, end) if s in index and a <= b]
    strings = [bytearray(bytes(wl.contig_string(k))) for k in range(len(wl.specs))]
    pairs = fb.plant_families(strings, gene_rows, args.family_size, args.substitutions, rng)
    table = fam.FamilyTable(pairs, labels)
    out.update(genes=len(labels), families=len(table.names))
    eng = Engine(0)
    g = eng.genome([bytes(s) for s in strings])
    try:
        areq = annotate.Request(ann, names, 1)
        spec = dict(max_mm=args.max_mm)
        requests = dict(family=sel.Request(sel.Params(K), areq, families=table, min_members="all", max_perfect_outside=0),
                        sets=sel.Request(sel.Params(K), areq, families=table, family_sets=args.steps))
        runs = {name: [] for name in requests}
        for r in range(args.repeats + 1):  # (the first run warms: the kernels' first launch loads their code object)
            for name, req in requests.items():
                t0 = time.perf_counter()
                hits = g.scan_score(GUIDE_LEN, specificity=dict(spec), select=req)
                runs[name].append((hits.selection, time.perf_counter() - t0))  # (the tables of the last run only: hits)
        timed = lambda name: [s for s, _ in runs[name][1:]]
        family_ms = float(np.median([s.stats["family_select_ms"] for s in timed("family")]))
        sets = timed("sets")
        n_steps = min(len(s.family_sets_stats["step_ms_per_step"]) for s in sets)
        step_ms = [float(np.median([s.family_sets_stats["step_ms_per_step"][t] for s in sets])) for t in range(n_steps)]
        pick_ms = [float(np.median([s.family_sets_stats["pick_ms_per_step"][t] for s in sets])) for t in range(n_steps)]
        s = hits.selection  # (the last run was a `sets` one)
        st = s.family_sets_stats
        out.update(family_select_ms=round(family_ms, 4), step_ms=[round(v, 4) for v in step_ms], pick_ms=[round(v, 4) for v in pick_ms],
                   step_over_family_select=round(step_ms[0] / family_ms, 4) if family_ms and step_ms else None,
                   items=int(st["items"]), rows_in_runs=int(st["rows_in_runs"]), bytes_per_row=st["bytes_per_row"], plan_builds=int(st["plan_builds"]),
                   arenas=len(g.arenas), picks=int(s.family_sets.size), families_complete=int(np.count_nonzero(s.family_complete)),
                   wall_s=round(float(np.median([w for _, w in runs["sets"][1:]])), 3),
                   family_wall_s=round(float(np.median([w for _, w in runs["family"][1:]])), 3))
        # the device against the host
        t0 = time.perf_counter()
        texts = [fb.CODE[np.frombuffer(bytes(x), np.uint8)] for x in strings]
        ranges, gene_of = [None] * len(labels), {i: n for n, i in enumerate(idents)}
        for i, k, a, b in gene_rows:
            ranges[gene_of[i]] = (k, max(0, a), min(len(strings[k]) - 1, b))  # (dec = 1: the string index is the coordinate)
        genes = [r if r is not None else (0, 1, 0) for r in ranges]
        gene_family, gene_member = [int(x) for x in table.gene_family], [int(x) for x in table.gene_member]
        tables, columns = {}, hits.columns
        picked = np.unique(s.family_sets["family"])
        sample = rng.choice(picked, min(args.sample, picked.size), replace=False).tolist() if picked.size else []
        ok, checked = True, 0
        for f in sample:
            for gi in table.members(f).tolist():
                k = genes[gi][0]
                if k not in tables:
                    tables[k] = hits.contig(k)
            cands, where = family_candidates(f, table, genes, tables, columns, texts, genes, gene_family, gene_member, args.max_mm)
            want, complete = host_family_set(cands, int(table.size[f]), args.steps)
            got = s.family_sets[s.family_sets["family"] == f]
            have = [(int(p["step"]), int(p["gene"]), int(p["contig"]), int(p["position"]), int(p["strand"] == b"-"), int(p["gain"]), int(p["cover"]),
                     int(p["covered"])) for p in got]
            ok = ok and have == [(step,) + where[i] + (gain, cands[i][4], covered) for step, i, gain, covered in want]
            ok = ok and bool(s.family_complete[f]) == complete
            checked += 1
        out.update(families_checked=checked, equals_host=bool(ok), host_check_s=round(time.perf_counter() - t0, 2))
    finally:
        g.close()
        eng.close()
        ann.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if out.get("equals_host") else 1


if __name__ == "__main__":
    sys.exit(main())
