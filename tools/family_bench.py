#!/usr/bin/env python3
"""Times the gene-family steps on a genome-scale stand-in and prints ONE JSON line.

The sorghum-like genome (bench_workload.sorghum_like) with its seeded synthetic Phytozome-style GFF.  The stand-in is
random letters and has no duplicated segments, so the families are planted: the genes are grouped --family-size at a time
(gene i, i + G / size, ...: members far apart, mostly on different contigs), and every member's range is overwritten with a
copy of the first member's letters carrying --substitutions random substitutions per letter, as homeologs are.  Then, in one
session, a scan at guide length 20 and

  plain     --specificity --select K: the self search (extract, order, compare), the join and the plain selection
  family    the same with the family table and --select-min-members all --select-max-perfect-outside 0: also assign, the
            family compare, the family join and the family selection

a warming run and --repeats timed ones each, medians from the handles' HIP events.  Reported next to the times: pairs
compared by the self search and by the family compare, and the family compare's fraction of its issue floor, pairs x VALU
per pair / (256 CU x 128 lanes x 2.4 GHz), with VALU per pair read from the assembly of search_family_compare_kernel (its
no-hit loop, instructions per 8 pairs; FAMILY_VALU_PER_PAIR if no compiler is at hand).

The run checks the device against the host: of --sample selected rows whose site belongs to the gene's family, the joined
site_family, fam_counts, fam_sum and fam_cover are recomputed in numpy from the genome's letters (host_family_rows below:
the family's candidate windows enumerated from the text, owners by the first-owner rule, mismatches counted letter by
letter), and outside_mm0 <= counts[0], outside_hit_sum <= hit_sum are checked on every selected row.

    python tools/family_bench.py [--workload sorghum|tair10|ecoli] [--genes N] [--family-size 4] [--out FILE]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K = 5
GUIDE_LEN = 20
FAMILY_VALU_PER_PAIR = 40 / 8
ISSUE_RATE = 256 * 128 * 2.4e9  # lane-operations per second: 256 CUs x 4 SIMD-32 x 2.4 GHz
NONE = 0xFFFFFFFF
CODE = np.full(256, 4, np.uint8)  # 0 A, 1 C, 2 G, 3 T, 4: no base (U reads as A)
for _ch, _c in zip(b"AaUuCcGgTt", (0, 0, 0, 0, 1, 1, 2, 2, 3, 3)):
    CODE[_ch] = _c


def valu_per_pair():
    """VALU instructions per pair of the family compare's no-hit loop, from its assembly; the constant without a compiler."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import emit_isa_budget as isa
    try:
        hipcc = isa.hipcc()
    except SystemExit:
        return FAMILY_VALU_PER_PAIR, "constant"
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "crp_search_family.s")
        cmd = [hipcc] + isa.makefile_flags() + ["--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                                                os.path.join(isa.CSRC, "crp_search_family.hip"), "-o", out]
        if subprocess.run(cmd, capture_output=True, text=True).returncode != 0:
            return FAMILY_VALU_PER_PAIR, "constant"
        with open(out) as f:
            asm = f.read()
    figures = []
    for m in re.finditer(r"^(_ZN3crp\S*search_family_compare_kernel\S*):", asm, re.M):
        loop = [b for b in isa.blocks_of(asm, m.group(1)) if sum(i.startswith("v_bcnt_u32_b32") for i in b[3]) == 8]
        if len(loop) == 1:
            figures.append(isa.counts(loop[0][3])["valu"] / 8.0)
    return (max(figures), "assembly") if figures else (FAMILY_VALU_PER_PAIR, "constant")


def plant_families(strings, genes, size, rate, rng, dec=1):
    """Overwrites, in the contig strings (bytearrays), the range of every later member of a family with the first member's
    letters carrying `rate` substitutions per letter.  genes: [(ident, contig index, start, end)] with GFF coordinates (string
    index = coordinate + dec - 1).  Returns [(ident, family token)] for the family file."""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    n_fam = len(genes) // size
    pairs = []
    for f in range(n_fam):
        members = [genes[f + j * n_fam] for j in range(size)]
        _, k0, s0, e0 = members[0]
        lo0, hi0 = max(0, s0 + dec - 1), min(len(strings[k0]) - 1, e0 + dec - 1)
        source = np.frombuffer(bytes(strings[k0][lo0:hi0 + 1]), np.uint8)
        pairs.append((members[0][0], "fam%d" % f))
        for ident, k, s, e in members[1:]:
            lo, hi = max(0, s + dec - 1), min(len(strings[k]) - 1, e + dec - 1)
            n = min(source.size, hi - lo + 1)
            if n > 0:
                copy = source[:n].copy()
                at = np.nonzero(rng.random(n) < rate)[0]
                copy[at] = rng.choice(acgt, at.size)
                strings[k][lo:lo + n] = copy.tobytes()
            pairs.append((ident, "fam%d" % f))
    return pairs


def _windows(text, lo, hi, l):
    """The NRG candidates of one contig text (uint8 codes) whose cut lies in [lo, hi]: (start, strand, cut, oriented guide
    codes (n, l), a guide site) -- '+' at start p cuts at p + l - 3, '-' at forward start j cuts at j."""
    T, n = l + 3, text.size
    comp = np.array([3, 2, 1, 0, 4], np.uint8)
    out = []
    p = np.arange(max(0, lo - (l - 3)), min(n - T, hi - (l - 3)) + 1)  # '+': the PAM is text[p + l .. p + l + 2] = N R G
    if p.size:
        p = p[((text[p + l + 1] == 0) | (text[p + l + 1] == 2)) & (text[p + l + 2] == 2)]
        guide = text[p[:, None] + np.arange(l)[None, :]]
        out.append((p, np.zeros(p.size, np.int64), p + l - 3, guide, (text[p + l + 1] == 2) & (guide != 4).all(axis=1)))
    j = np.arange(max(0, lo), min(n - T, hi) + 1)  # '-': forward C Y N at j, the guide is the reverse complement behind it
    if j.size:
        j = j[(text[j] == 1) & ((text[j + 1] == 1) | (text[j + 1] == 3))]
        guide = comp[text[j[:, None] + 3 + np.arange(l - 1, -1, -1)[None, :]]]
        out.append((j, np.ones(j.size, np.int64), j, guide, (text[j + 1] == 1) & (guide != 4).all(axis=1)))
    if not out:
        return (np.zeros(0, np.int64),) * 3 + (np.zeros((0, l), np.uint8), np.zeros(0, bool))
    return tuple(np.concatenate(c) for c in zip(*out))


def host_family_rows(texts, genes, gene_family, gene_member, family, queries, max_mm, cover_mm, scheme=None, l=GUIDE_LEN):
    """The family rows of `queries` [(contig, forward start, strand)], guide sites of family `family`, in numpy from the
    letters.  texts: per contig the uint8 codes (CODE); genes: [(contig, lo, hi)] string indices, closed, clipped, in GFF order;
    gene_family / gene_member per gene (NONE: no family).  Returns per query (site_family or NONE, fam_counts (M + 1,),
    fam_sum, fam_cover); a query that is no guide site owned by the family gets (NONE, zeros, 0, 0)."""
    cands = []  # of the family: (contig, start, strand, guide codes, a guide site, member)
    for g, (k, lo, hi) in enumerate(genes):
        if gene_family[g] != family or lo > hi:
            continue
        start, strand, cut, guide, is_guide = _windows(texts[k], lo, hi, l)
        owner = np.full(start.size, g, np.int64)  # the first family gene of the file that holds the cut
        for g2, (k2, lo2, hi2) in enumerate(genes[:g]):
            if k2 == k and gene_family[g2] != NONE and lo2 <= hi and hi2 >= lo:
                owner[(cut >= lo2) & (cut <= hi2) & (owner == g)] = g2
        keep = owner == g
        cands.append((np.full(int(keep.sum()), k), start[keep], strand[keep], guide[keep], is_guide[keep],
                      np.full(int(keep.sum()), gene_member[g])))
    ck, cs, cst, cg, cguide, cmember = (np.concatenate(c) for c in zip(*cands)) if cands else (np.zeros(0, np.int64),) * 6
    w = np.uint64(1) << np.arange(l, dtype=np.uint64)
    out = []
    for k, start, strand in queries:
        me = np.nonzero((ck == k) & (cs == start) & (cst == strand))[0]
        if me.size != 1 or not cguide[me[0]]:
            out.append((NONE, np.zeros(max_mm + 1, np.int64), 0, 0))
            continue
        others = np.arange(ck.size) != me[0]
        mism = cg[others] != cg[me[0]][None, :]  # (a non-base equals no base of a guide)
        mm = mism.sum(axis=1)
        hit = mm <= max_mm
        total = 0
        if scheme is not None and hit.any():
            from cropsr_amd.search import mask_values
            masks = (mism[hit].astype(np.uint64) * w[None, :]).sum(axis=1, dtype=np.uint64)
            total = int(mask_values(masks, scheme).astype(object).sum())
        cover = 1 << int(cmember[me[0]])
        for m in np.unique(cmember[others][cguide[others] & (mm <= cover_mm)]).tolist():
            cover |= 1 << int(m)
        out.append((family, np.bincount(mm[hit], minlength=max_mm + 1)[:max_mm + 1], total, cover))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=["sorghum", "tair10", "ecoli"], default="sorghum")
    ap.add_argument("--genes", type=int, default=34000)
    ap.add_argument("--family-size", type=int, default=4)
    ap.add_argument("--substitutions", type=float, default=0.02)
    ap.add_argument("--max-mm", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per variant; the median is reported")
    ap.add_argument("--sample", type=int, default=64, help="selected rows recomputed on the host")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    import bench_workload as bw
    from cropsr_amd import Engine, annotate, families as fam
    from cropsr_amd import search as srch
    from cropsr_amd import select as sel
    wl = {"sorghum": bw.sorghum_like, "tair10": bw.tair10_like, "ecoli": bw.ecoli_like}[args.workload]()
    vpp, vpp_source = valu_per_pair()
    out = dict(workload=wl.name, k=K, max_mm=args.max_mm, family_size=args.family_size, substitutions=args.substitutions,
               valu_per_pair=vpp, valu_per_pair_from=vpp_source)
    rng = np.random.default_rng(23)
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
    t0 = time.perf_counter()
    pairs = plant_families(strings, gene_rows, args.family_size, args.substitutions, rng)
    table = fam.FamilyTable(pairs, labels)
    out.update(genes=len(labels), families=len(table.names), plant_s=round(time.perf_counter() - t0, 2))
    eng = Engine(0)
    g = eng.genome([bytes(s) for s in strings])
    try:
        areq = annotate.Request(ann, names, 1)
        spec = dict(max_mm=args.max_mm)
        requests = dict(plain=sel.Request(sel.Params(K), areq),
                        family=sel.Request(sel.Params(K), areq, families=table, min_members="all", max_perfect_outside=0))
        results = {}
        for name, req in requests.items():
            runs = []
            for r in range(args.repeats + 1):  # (the first run warms: the kernels' first launch loads their code object)
                t0 = time.perf_counter()
                hits = g.scan_score(GUIDE_LEN, specificity=dict(spec), select=req)
                runs.append(dict(hits.columns.stats, wall_s=time.perf_counter() - t0, **{"select_" + k: v for k, v in hits.selection.stats.items()
                                                                                          if isinstance(v, float)}))
            med = lambda key: float(np.median([x.get(key, 0.0) for x in runs[1:]]))
            st = {key: round(med(key), 4) for key in ("extract_ms", "order_ms", "compare_ms", "join_ms", "assign_ms", "family_compare_ms",
                                                      "family_join_ms", "select_select_ms", "select_family_select_ms",
                                                      "select_family_eval_ms", "wall_s")}
            st.update(pairs=int(runs[-1].get("pairs", 0)), family_pairs=int(runs[-1].get("family_pairs", 0)),
                      family_compare_launches=int(runs[-1].get("family_compare_launches", 0)), family_bytes=int(runs[-1].get("family_bytes", 0)),
                      rows_selected=int(hits.selection.rows.size), rows_passing=int(hits.selection.n_pass.sum()))
            results[name], out[name] = hits, st
        fs = out["family"]
        if fs["family_compare_ms"]:
            floor_ms = fs["family_pairs"] * vpp / ISSUE_RATE * 1e3
            out.update(family_issue_floor_ms=round(floor_ms, 4), family_fraction_of_issue_floor=round(floor_ms / fs["family_compare_ms"], 3),
                       family_pairs_over_self_pairs=round(fs["family_pairs"] / max(1, fs["pairs"]), 5),
                       family_compare_over_self_compare=round(fs["family_compare_ms"] / fs["compare_ms"], 4) if fs["compare_ms"] else None)
        # the device against the host
        s = results["family"].selection
        ok = bool((s.outside_mm0 <= s.counts[:, 0]).all() and (s.outside_hit_sum <= s.hit_sum).all())
        texts = [CODE[np.frombuffer(bytes(x), np.uint8)] for x in strings]
        ranges, gene_of = [None] * len(labels), {i: n for n, i in enumerate(idents)}
        for i, k, a, b in gene_rows:
            ranges[gene_of[i]] = (k, max(0, a), min(len(strings[k]) - 1, b))  # (dec = 1: the string index is the coordinate)
        genes = [r if r is not None else (0, 1, 0) for r in ranges]
        gene_family = [int(x) for x in table.gene_family]
        scheme = srch.check_specificity(GUIDE_LEN, args.max_mm)[3]
        pick = rng.choice(s.rows.size, min(args.sample, s.rows.size), replace=False) if s.rows.size else []
        t0 = time.perf_counter()
        checked = 0
        for at in pick:
            row = s.rows[at]
            gi, k, minus = int(row["gene"]), int(row["contig"]), row["strand"] == b"-"
            site = (k, int(row["position"]) if minus else int(row["position"]) - GUIDE_LEN, int(minus))
            want = host_family_rows(texts, genes, gene_family, [int(x) for x in table.gene_member], gene_family[gi], [site], args.max_mm, 0, scheme)[0]
            got_cover = int(s.fam_cover[at])
            if want[0] == NONE:  # the row belongs to another family's gene: the plain columns, the gene itself
                ok = ok and got_cover == 0 and int(s.members_hit[at]) == 1 and int(s.outside_mm0[at]) == int(s.counts[at, 0])
            else:
                ok = ok and (got_cover == want[3] and int(s.outside_mm0[at]) == int(s.counts[at, 0]) - int(want[1][0])
                             and int(s.outside_hit_sum[at]) == int(s.hit_sum[at]) - want[2])
            checked += 1
        out.update(rows_checked=checked, equals_host=bool(ok), host_check_s=round(time.perf_counter() - t0, 2))
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
