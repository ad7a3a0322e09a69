"""Times the off-target search of given guides on the 1.13 Gb switchgrass stand-in.

Guides are drawn from real NGG sites of the stand-in (upper- or lower-case, 20 bases followed by NGG); its homeologous
chromosome pairs are 3 %-substituted copies, so every guide has realistic 0..3-mismatch off-targets.  For M = 4 and the
patterns ...NGG and ...NRG it times candidate extraction (count + emit kernels) and the compare kernels separately,
with the library's HIP events (crp_search_stats), for Q = 64, 1 024 and 8 192 guides, and prints one JSON line.

Issue floor of the compare kernel: pairs x VALU per pair / (256 CU x 128 lanes x 2.4 GHz).  VALU_PER_PAIR is read from
the ISA of search_compare_kernel (hipcc -S --offload-arch=gfx950): the no-hit loop body is 41 VALU instructions for
SEARCH_CPL = 8 candidates (9 v_xor_b32, 15 v_bitop3_b32, 1 v_or_b32, 8 v_bcnt_u32_b32, 8 v_cmp_le_i32).

    python tools/search_bench.py [--scale 1.0] [--device 0]

--bulge D,R times the search with bulges instead (Bulges): 1 024 of the same guides against ...NGG
at M = 4, per kind (none, DNA 1..D, RNA 1..R) the extraction and compare times of its own handles, ms per query, the
fraction of the issue floor, and the compare time of the expansion path for the same queries (every query expanded per
bulge placement and run through the no-bulge compare kernel on the same candidates).  BULGE_VALU_PER_PAIR is read from
the ISA of search_bulge_compare_kernel: its no-hit loop body is 72 VALU instructions for 8 candidates (40 v_bitop3_b32,
16 v_bfi_b32, 8 v_bcnt_u32_b32, 8 v_cmp_le_i32).

--score times the specificity score (Specificity score): the 1 024-guide ...NGG M = 4 case run plain
(search_compare_kernel) and scored with hsu2013 (search_score_compare_kernel), interleaved in one process on the same
resident candidates, three rounds each, compare times from crp_search_stats; plus the wall time of the plain run (with
its fetch and sort of the site list) against the score-only run (site_cap 0: no site list at all).

--score --score-table FILE adds the pair-table run (search_pair_compare_kernel; DESIGN.md section 15, Pair tables) to the
same interleaving: FILE is a pair-table file for a 20 + 3 pattern (search.parse_pair_table), set on the same handles in
turn with hsu2013, so all runs use the same resident candidates; pair_over_scored_compare is its compare time over the
hsu2013 scored kernel's.  --self --score-table FILE runs every M under hsu2013 and under the table, and reports the
compare time and the longest launch of both (the hit path is not rare there: a low-complexity bucket is all hits).

--self times the self search (Self search): ...NGG, hsu2013, M = 3 and M = 4, a warm-up and three
rounds each in one process, times from the handles' stats (HIP events): extraction, the M + 1 orderings, the compare
(launches, longest launch), pairs compared against Q x C and the compare's fraction of its issue floor.
SELF_VALU_PER_PAIR is read from the ISA of search_self_compare_kernel (37 VALU instructions per 8 pairs).  In the same
run 8 192 of the guide sites' queries go through search(sites=False, score="hsu2013") and are scaled to all guide
sites: the existing path's figure for the same question.  The run checks itself: 2 048 seeded rows and the 64 rows with
the largest counts against search(), exactly.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench_workload as bw  # noqa: E402
from cropsr_amd import Engine  # noqa: E402
from cropsr_amd import _native as nat  # noqa: E402
from cropsr_amd import search as srch  # noqa: E402

VALU_PER_PAIR = 41 / 8
BULGE_VALU_PER_PAIR = 72 / 8
SELF_VALU_PER_PAIR = 37 / 8
SELF_MMS = (3, 4)
SELF_BRUTE_Q = 8192
BULGE_Q = 1024
ISSUE_RATE = 256 * 128 * 2.4e9  # lane-operations per second: 256 CUs x 4 SIMD-32 x 2.4 GHz
PATTERNS = {"NGG": "N" * 21 + "GG", "NRG": "N" * 21 + "RG"}
QS = (64, 1024, 8192)
MAX_MM = 4


def draw_guides(contigs, n, seed=3):
    """n distinct 20-nt guides from real NGG sites ('+' strand) of the largest contigs."""
    rng = np.random.default_rng(seed)
    code = np.zeros(256, dtype=bool)
    code[list(b"ACGTacgt")] = True
    out = set()
    big = sorted(range(len(contigs)), key=lambda k: -contigs[k].size)[:6]
    while len(out) < n:
        c = contigs[int(rng.choice(big))]
        starts = rng.integers(0, c.size - 23, 4 * n)
        for s in starts.tolist():
            w = c[s:s + 23]
            if code[w].all() and (w[21] | 0x20) == ord("g") and (w[22] | 0x20) == ord("g"):
                out.add(bytes(w[:20]).upper().decode())
                if len(out) == n:
                    break
    return sorted(out)


def bulge_main(args, contigs, guides, out):
    D, R = (int(v) for v in args.bulge.split(","))
    pattern, P = PATTERNS["NGG"], 3
    queries = [srch.check_query(pattern, q, P) for q in guides[:BULGE_Q]]
    spans = srch.query_spans(pattern, P, queries, D, R)
    out.update(bulge_valu_per_pair=BULGE_VALU_PER_PAIR, queries=len(queries), dna_bulge=D, rna_bulge=R, pattern="NGG", kinds={})
    total = 0.0
    with Engine(args.device) as eng:
        out["device"] = eng.device_info()["name"].strip()
        g = eng.genome(contigs)
        for bulge, size in srch.bulge_kinds(D, R):
            kp = srch.kind_pattern(pattern, P, bulge, size)
            searches = [srch.ArenaSearch(a, kp) for a in g.arenas]
            cand = sum(sum(s.candidates()) for s in searches)
            n_sites = 0
            for s in searches:
                st, _, n = s.run(queries, MAX_MM, 1 << 40, (bulge, size), spans)
                nat.check(st, "crp_search_run")
                n_sites += n
            st1 = [s.stats() for s in searches]
            extract_ms = sum(x["extract_ms"] for x in st1)
            compare_ms = sum(x["compare_ms"] for x in st1)
            vpp = BULGE_VALU_PER_PAIR if size else VALU_PER_PAIR
            floor_ms = float(cand) * len(queries) * vpp / ISSUE_RATE * 1e3
            row = dict(window=len(kp), candidates=cand, extract_ms=round(extract_ms, 3), compare_ms=round(compare_ms, 3),
                       compare_launches=int(sum(x["compare_launches"] for x in st1)), ms_per_query=round(compare_ms / len(queries), 5),
                       sites=int(n_sites), issue_floor_ms=round(floor_ms, 3), fraction_of_issue_floor=round(floor_ms / compare_ms, 3),
                       gpu_ms_with_extraction=round(extract_ms + compare_ms, 3))
            total += extract_ms + compare_ms
            if size:  # the expansion path on the same (resident) candidates
                exp = []
                for q, query in enumerate(queries):
                    first, last = (int(v) for v in spans[q])
                    hi = last if bulge == "DNA" else last - size
                    for s_ in range(first + 1, hi + 1):
                        exp.append(query[:s_] + "N" * size + query[s_:] if bulge == "DNA" else query[:s_] + query[s_ + size:])
                n_exp = 0
                for s in searches:
                    st, _, n = s.run(exp, MAX_MM, 1 << 40)
                    nat.check(st, "crp_search_run")
                    n_exp += n
                st2 = [s.stats() for s in searches]
                exp_ms = sum(b["compare_ms"] - a["compare_ms"] for a, b in zip(st1, st2))
                row.update(expansion_queries=len(exp), expansion_compare_ms=round(exp_ms, 3),
                           expansion_launches=int(sum(b["compare_launches"] - a["compare_launches"] for a, b in zip(st1, st2))),
                           expansion_sites=int(n_exp), speedup_vs_expansion=round(exp_ms / compare_ms, 2))
            for s in searches:
                s.close()
            out["kinds"]["%s%d" % (bulge, size) if size else "none"] = row
        g.close()
    out["gpu_ms_all_kinds"] = round(total, 3)
    print(json.dumps(out))


def score_main(args, contigs, guides, out):
    pattern, P, rounds = PATTERNS["NGG"], 3, 3
    queries = [srch.check_query(pattern, q, P) for q in guides[:BULGE_Q]]
    scheme = srch.make_scheme(pattern, P, "hsu2013")
    pair_scheme = None
    if args.score_table:
        with open(args.score_table, "rb") as f:
            pair_scheme = srch.make_scheme(pattern, P, srch.parse_pair_table(f.read()))
    out.update(queries=len(queries), pattern="NGG", scheme="hsu2013", rounds=rounds)
    with Engine(args.device) as eng:
        out["device"] = eng.device_info()["name"].strip()
        g = eng.genome(contigs)
        searches = [srch.ArenaSearch(a, pattern) for a in g.arenas]
        for s in searches:
            s.set_scheme(scheme)
        out["candidates"] = int(sum(sum(s.candidates()) for s in searches))

        def timed(run):
            """(compare ms, wall s, sites, counts, hit sums) of one run over every arena"""
            before = [s.stats()["compare_ms"] for s in searches]
            t = time.perf_counter()
            res = [run(s) for s in searches]
            wall = time.perf_counter() - t
            for r in res:
                if r[0] not in (nat.CRP_OK, nat.CRP_ERR_CAPACITY):
                    nat.check(r[0], "crp_search_run")
            ms = sum(s.stats()["compare_ms"] - b for s, b in zip(searches, before))
            return ms, wall, sum(r[2] for r in res), sum(r[1].astype(np.uint64) for r in res), \
                sum(r[3] for r in res) if len(res[0]) > 3 else None

        def plain(s):
            st, counts, n = s.run(queries, MAX_MM, 1 << 40)
            if st == nat.CRP_OK:
                s.fetch(n)
            return st, counts, n

        def scored(s):
            return s.run_scored(queries, MAX_MM, 1 << 40)

        def score_only(s):
            return s.run_scored(queries, MAX_MM, 0)

        def pair(s):  # (the handle holds one scheme at a time: the upload is outside the compare's events)
            s.set_scheme(pair_scheme)
            try:
                return s.run_scored(queries, MAX_MM, 1 << 40)
            finally:
                s.set_scheme(scheme)

        runs = [("plain", plain), ("scored", scored), ("score_only", score_only)] + ([("pair", pair)] if pair_scheme else [])
        timed(plain)  # warm-up: extraction, the site buffer's growth, the kernels' code objects
        timed(scored)
        if pair_scheme:
            timed(pair)
        rows = {name: [] for name, _ in runs}
        ref_counts = ref_sums = pair_sums = None
        for _ in range(rounds):
            for name, run in runs:
                ms, wall, n_sites, counts, sums = timed(run)
                rows[name].append((ms, wall))
                if ref_counts is None:
                    ref_counts = counts
                assert (counts == ref_counts).all(), name
                if name == "pair":
                    pair_sums = sums if pair_sums is None else pair_sums
                    assert (sums == pair_sums).all(), name
                elif sums is not None:
                    ref_sums = sums if ref_sums is None else ref_sums
                    assert (sums == ref_sums).all(), name
                out["sites"] = int(n_sites)
        for name, r in rows.items():
            out[name] = dict(compare_ms=[round(ms, 3) for ms, _ in r], run_wall_s=[round(w, 4) for _, w in r])
        med = lambda name, k: float(np.median([x[k] for x in rows[name]]))
        out["scored_over_plain_compare"] = round(med("scored", 0) / med("plain", 0), 4)
        out["score_only_over_plain_compare"] = round(med("score_only", 0) / med("plain", 0), 4)
        out["score_only_over_plain_wall"] = round(med("score_only", 1) / med("plain", 1), 4)
        if pair_scheme:
            out["pair_over_scored_compare"] = round(med("pair", 0) / med("scored", 0), 4)
            out["pair_over_plain_compare"] = round(med("pair", 0) / med("plain", 0), 4)
            out["pair_hit_sum_total"] = int(pair_sums.sum())
        out["hit_sum_total"] = int(ref_sums.sum())
        out["guides_with_hits"] = int((ref_sums > 0).sum())
        out["median_specificity"] = round(float(np.median(srch.specificity(ref_sums))), 6)
        for s in searches:
            s.close()
        g.close()
    print(json.dumps(out))


def self_main(args, contigs, out):
    pattern, P, rounds = PATTERNS["NGG"], 3, 3
    out.update(pattern="NGG", scheme="hsu2013", rounds=rounds, self_valu_per_pair=SELF_VALU_PER_PAIR, runs={})
    out.pop("max_mm")
    rng = np.random.default_rng(5)
    with Engine(args.device) as eng:
        out["device"] = eng.device_info()["name"].strip()
        g = eng.genome(contigs)
        table = None
        if args.score_table:
            with open(args.score_table, "rb") as f:
                table = srch.parse_pair_table(f.read())
            srch.make_scheme(pattern, P, table)
        for M in SELF_MMS:
            rows, res, pair_rows = [], None, []
            for r in range(rounds + 1):  # (the first is the warm-up)
                t = time.perf_counter()
                res = srch.search_self(g, pattern, M, P, score="hsu2013")
                wall = time.perf_counter() - t
                if r:
                    rows.append(dict(res.stats, wall_s=wall))
                if table is not None:  # the pair table on the same genome and M, interleaved
                    pres = srch.search_self(g, pattern, M, P, score=table)
                    assert (pres.counts == res.counts).all(), "the counts do not depend on the scheme"
                    if r:
                        pair_rows.append(pres.stats)
            n, cand = len(res.sites), sum(res.candidates)
            med = lambda k: float(np.median([x[k] for x in rows]))
            floor_ms = res.pairs[0] * SELF_VALU_PER_PAIR / ISSUE_RATE * 1e3
            gpu_ms = med("extract_ms") + med("order_ms") + med("compare_ms")
            row = dict(guide_sites=n, candidates=cand, pairs=res.pairs[0], pairs_brute_force=res.pairs[1],
                       pairs_fraction=res.pairs[0] / max(1, res.pairs[1]), device_bytes=int(rows[0]["device_bytes"]),
                       extract_ms=[round(x["extract_ms"], 3) for x in rows], order_ms=[round(x["order_ms"], 3) for x in rows],
                       compare_ms=[round(x["compare_ms"], 3) for x in rows], compare_launches=int(rows[0]["compare_launches"]),
                       longest_launch_ms=[round(x["longest_launch_ms"], 3) for x in rows], gpu_ms=round(gpu_ms, 3),
                       wall_s=[round(x["wall_s"], 2) for x in rows], issue_floor_ms=round(floor_ms, 3),
                       fraction_of_issue_floor=round(floor_ms / med("compare_ms"), 3),
                       median_specificity=round(float(np.median(res.specificity)), 6))
            if pair_rows:
                pm = float(np.median([x["compare_ms"] for x in pair_rows]))
                row.update(pair_compare_ms=[round(x["compare_ms"], 3) for x in pair_rows],
                           pair_longest_launch_ms=[round(x["longest_launch_ms"], 3) for x in pair_rows],
                           pair_over_scored_compare=round(pm / med("compare_ms"), 4))
            # the existing path: a sample of the guide sites' queries through the given-guides compare, scaled to all of them
            pick = np.sort(rng.choice(n, min(n, SELF_BRUTE_Q), replace=False))
            searches = [srch.ArenaSearch(a, pattern) for a in g.arenas]
            scheme = srch.make_scheme(pattern, P, "hsu2013")
            queries = [srch.check_query(pattern, res.guides[i].decode(), P) for i in pick]
            counts = np.zeros((len(queries), M + 1), np.int64)
            sums = np.zeros(len(queries), np.uint64)
            for s in searches:
                s.set_scheme(scheme)
                st, c, _, hs = s.run_scored(queries, M, 0)
                if st not in (nat.CRP_OK, nat.CRP_ERR_CAPACITY):
                    nat.check(st, "crp_search_run_scored")
                counts += c
                sums += hs
            brute_ms = sum(s.stats()["compare_ms"] for s in searches)
            for s in searches:
                s.close()
            counts[:, 0] -= 1
            # the run checks itself: 2 048 of the sampled rows and the 64 rows with the largest counts, exactly
            assert (res.counts[pick[:2048]] == counts[:2048]).all() and (res.hit_sum[pick[:2048]] == sums[:2048]).all(), "sampled rows differ"
            top = np.argsort(res.counts.sum(axis=1), kind="stable")[-64:]
            big = srch.search(g, pattern, [srch.check_query(pattern, res.guides[i].decode(), P) for i in top], M, pam_len=P, score="hsu2013",
                              sites=False)
            bc = big.counts.astype(np.int64)
            bc[:, 0] -= 1
            assert (res.counts[top] == bc).all() and (res.hit_sum[top] == big.hit_sum).all(), "largest rows differ"
            scaled_s = brute_ms * 1e-3 * n / len(queries)
            row.update(brute_queries=len(queries), brute_compare_ms=round(brute_ms, 3), brute_scaled_s=round(scaled_s, 1),
                       speedup_vs_scaled_brute=round(scaled_s / (gpu_ms * 1e-3), 1), rows_checked=int(min(2048, len(queries)) + top.size))
            # the CSV join: the stand-in's hit tables (a scan at l = 20) against the rows of one more search, its own compare_ms
            # next to it
            n_hits = sum(sum(a.scan_score_device(20)) for a in g.arenas)
            cols = srch.specificity_columns(g, 20, max_mm=M, candidate_pam=pattern[20:], score="hsu2013")
            joined = sum(int((c["self_sum_plus"] != nat.SELF_UNJOINED_SUM).sum() + (c["self_sum_minus"] != nat.SELF_UNJOINED_SUM).sum())
                         for c in cols)
            row.update(join_hits=int(n_hits), join_joined=joined, join_ms=round(cols.stats["join_ms"], 3),
                       join_run_compare_ms=round(cols.stats["compare_ms"], 3),
                       join_over_compare=round(cols.stats["join_ms"] / max(1e-9, cols.stats["compare_ms"]), 5))
            out["runs"]["M%d" % M] = row
            print("M = %d: %s" % (M, json.dumps(row)), file=sys.stderr, flush=True)
        g.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--bulge", metavar="D,R", help="time the search with DNA bulges 1..D and RNA bulges 1..R instead")
    ap.add_argument("--score", action="store_true", help="time the scored compare against the plain one instead")
    ap.add_argument("--self", dest="self_search", action="store_true", help="time the self search (every guide site a query) instead")
    ap.add_argument("--score-table", metavar="FILE", help="with --score or --self: also time the pair table of FILE (20 + NGG)")
    args = ap.parse_args()
    if args.score_table and not (args.score or args.self_search):
        ap.error("--score-table goes with --score or --self")
    t0 = time.perf_counter()
    wl = bw.switchgrass_like(0, args.scale)
    contigs = [wl.bases(s) for s in wl.specs]
    if args.self_search:
        return self_main(args, contigs, dict(workload=wl.name, chars=int(sum(c.size for c in contigs)), max_mm=MAX_MM,
                                             generate_s=round(time.perf_counter() - t0, 1)))
    guides = draw_guides(contigs, BULGE_Q if args.bulge or args.score else max(QS))
    gen_s = time.perf_counter() - t0
    if args.score:
        return score_main(args, contigs, guides, dict(workload=wl.name, chars=int(sum(c.size for c in contigs)), max_mm=MAX_MM,
                                                      generate_s=round(gen_s, 1)))
    if args.bulge:
        return bulge_main(args, contigs, guides, dict(workload=wl.name, chars=int(sum(c.size for c in contigs)), max_mm=MAX_MM,
                                                      generate_s=round(gen_s, 1)))
    out = dict(workload=wl.name, chars=int(sum(c.size for c in contigs)), max_mm=MAX_MM, valu_per_pair=VALU_PER_PAIR,
               generate_s=round(gen_s, 1), patterns={})
    with Engine(args.device) as eng:
        out["device"] = eng.device_info()["name"].strip()
        g = eng.genome(contigs)
        for name, pattern in PATTERNS.items():
            queries = [srch.check_query(pattern, q, 3) for q in guides]  # 20-nt guides next to the 3-letter PAM
            searches = [srch.ArenaSearch(a, pattern) for a in g.arenas]
            cand = [sum(s.candidates()[k] for s in searches) for k in (0, 1)]
            row = dict(candidates=cand[0] + cand[1], candidates_plus=cand[0], candidates_minus=cand[1], runs={})
            for Q in QS:
                before = [s.stats() for s in searches]
                t = time.perf_counter()
                n_sites = 0
                for s in searches:
                    st, counts, n = s.run(queries[:Q], MAX_MM, 1 << 40)
                    nat.check(st, "crp_search_run")
                    n_sites += n
                wall = time.perf_counter() - t
                after = [s.stats() for s in searches]
                d = lambda k: sum(a[k] - b[k] for a, b in zip(after, before))
                if Q == QS[0]:  # the count kernels ran at create, the emit kernel in this first run; later runs reuse them
                    row["extract_ms"] = round(sum(a["extract_ms"] for a in after), 3)
                compare_ms = d("compare_ms")
                pairs = float(row["candidates"]) * Q
                floor_ms = pairs * VALU_PER_PAIR / ISSUE_RATE * 1e3
                row["runs"][str(Q)] = dict(
                    compare_ms=round(compare_ms, 3), compare_launches=int(d("compare_launches")),
                    pairs_per_s=pairs / (compare_ms * 1e-3), ms_per_query=round(compare_ms / Q, 5), sites=int(n_sites),
                    run_wall_s=round(wall, 3), issue_floor_ms=round(floor_ms, 3), fraction_of_issue_floor=round(floor_ms / compare_ms, 3),
                    gpu_ms_with_extraction=round(row["extract_ms"] + compare_ms, 3))
            row["candidate_bytes"] = int(sum(s.stats()["candidate_bytes"] for s in searches))
            for s in searches:
                s.close()
            out["patterns"][name] = row
        g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
