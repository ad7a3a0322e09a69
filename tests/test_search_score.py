"""The per-guide specificity score of the off-target search (search.py score=, crp_search_set_scheme / crp_search_run_scored;
DESIGN.md section 15, Specificity score): the definition stated twice, hand-made answers, refusals, host hit values, TSV
bytes, the ABI and the kernel's static ISA without a GPU; the device's sums against the reference, exactly, on the GPU."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

import search_reference as ref
import search_score_reference as sref
from cropsr_amd import _native as nat
from cropsr_amd import search as srch
from test_search import CAS12A, PAM_LEN, SACAS9, SPCAS9, SPCAS9_NAG, TSV_GENOME, _as_tuples, _planted_genome, _queries_for, _tsv_case

sys.path.insert(0, os.path.join(ROOT, "tools"))
import emit_isa_budget as isa  # noqa: E402

CAS12A_20 = "TTTV" + "N" * 20
ONE = 1 << 30


def _weights_for(pattern, seed=0):
    """The score argument of a pattern: hsu2013 where the guide region has 20 positions, else random weights with some
    exact 0 and 1 among them."""
    G = len(pattern) - PAM_LEN.get(pattern, 4)
    if G == 20:
        return "hsu2013", sref.W_HSU
    w = np.round(np.random.default_rng(100 + seed).random(G), 3)
    w[[1, G // 2]] = 0.0
    w[G - 2] = 1.0
    return w.tolist(), w.tolist()


# ------------------------------------------------------------------ the definition (CPU)
def test_two_statements_of_the_definition_agree():
    rng = np.random.default_rng(77)
    for G in (20, 17, 24):
        weights = sref.W_HSU if G == 20 else np.round(rng.random(G), 3).tolist()
        factor, shape = sref.tables(weights)
        masks = [0]
        for n in range(0, 9):
            for _ in range(60):
                masks.append(sum(1 << int(g) for g in rng.choice(G, n, replace=False)))
        masks += [(1 << n) - 1 for n in range(1, 9)] + [((1 << n) - 1) << (G - n) for n in range(1, 9)] + [1 | 1 << (G - 1)]
        v_np = sref.values(masks, factor, shape)
        for m, v in zip(masks, v_np.tolist()):
            v_loop, h_plain = sref.value_loop(m, weights, factor, shape)
            assert v_loop == v, (G, bin(m))
            n = bin(m).count("1")
            if n == 0:
                assert v == 0 and h_plain == 1.0  # (a site without mismatches is not summed)
            else:
                # the mean of the consecutive distances telescopes to d / (n - 1): the table form is the publication's form
                assert abs(h_plain * ONE - v) <= 0.5 + 1e-12 * h_plain * ONE, (G, bin(m))
                pos = [g for g in range(G) if (m >> g) & 1]
                h_tab = float(np.prod([factor[g] for g in pos])) * shape[n][pos[-1] - pos[0]]
                assert abs(h_tab - h_plain) <= 1e-12 * h_plain
        # the package's own statement and tables
        sc = srch.make_scheme("N" * G + "NGG", 3, "hsu2013" if G == 20 else weights)
        assert (sc.factor == factor).all() and (sc.shape == shape).all()
        assert (srch.mask_values(masks, sc) == v_np).all()


def test_known_answers_hsu2013():
    factor, shape = sref.tables(sref.W_HSU)
    v = sref.values([1 << 19, 1 | 1 << 19, 3 << 18, 0], factor, shape).tolist()
    f19, f18, f0 = 1.0 - 0.583, 1.0 - 0.685, 1.0
    assert abs(f19 - 0.417) < 1e-15 and abs(f18 - 0.315) < 1e-15
    assert v[0] == int(np.rint(f19 * ONE)) and abs(v[0] / ONE - 0.417) < 1e-9
    assert v[1] == int(np.rint(f0 * f19 * (1.0 / (((19.0 - 19 / 1.0) / 19.0) * 4.0 + 1.0) / 4.0) * ONE))
    assert abs(v[1] / ONE - 0.417 / 4) < 1e-9  # g = 0 and g = 19: as spread out as can be, no spread penalty
    assert abs(v[2] / ONE - 0.315 * 0.417 / (72 / 19 + 1) / 4) < 1e-9  # neighbours: mean distance 1
    assert v[3] == 0  # a guide's own site adds nothing
    sc = srch.make_scheme(SPCAS9, 3, "hsu2013")
    assert srch.mask_values([1 << 19, 1 | 1 << 19, 3 << 18, 0], sc).tolist() == v
    assert srch.specificity(np.array([0, ONE, 3 * ONE], dtype=np.uint64)).tolist() == [1.0, 0.5, 0.25]


def test_g_counts_from_the_pam_distal_end_on_either_side():
    sc3, sc5 = srch.make_scheme(SPCAS9, 3, "hsu2013"), srch.make_scheme(CAS12A_20, 4, "hsu2013")
    assert sc3.g_positions().tolist() == list(range(20)) == sref.guide_positions(SPCAS9, 3)
    assert sc5.g_positions().tolist() == list(range(23, 3, -1)) == sref.guide_positions(CAS12A_20, 4)
    assert (sc3.factor == sc5.factor).all() and sc5.factor[19] == 1.0 - 0.583
    # one mismatch next to the PAM, on either side, is the expensive one
    guide = "ACGTTGCAACGTTGCAACGT"
    q3, q5 = srch.check_query(SPCAS9, guide, 3), srch.check_query(CAS12A_20, guide, 4)
    c3 = (guide[:19] + "A" + "TGG").encode()  # the guide's last letter, next to NGG
    c5 = ("TTTA" + "C" + guide[1:]).encode()  # the guide's first letter, next to TTTV
    for pattern, P, q, contig, sc in ((SPCAS9, 3, q3, c3, sc3), (CAS12A_20, 4, q5, c5, sc5)):
        counts, s = ref.search([contig], pattern, [q], 1)
        sites = _sites_array(s)
        assert sites.size == 1 and int(sites["mismatches"][0]) == 1
        assert srch.site_masks(sites, [q], [contig], sc).tolist() == [1 << 19]
        assert srch.hit_values(sites, [q], [contig], sc).tolist() == [int(np.rint((1.0 - 0.583) * ONE))]


def _sites_array(s):
    sites = np.empty(s["query"].size, srch.SITE_DTYPE)
    for f in ref.SITE_FIELDS:
        sites[f] = s[f] if f != "strand" else np.where(s[f] == 0, b"+", b"-")
    return sites


# ------------------------------------------------------------------ refusals (CPU)
def test_refusals():
    q = srch.check_query(SPCAS9, "ACGTACGTACGTACGTACGT", 3)
    E = srch.SearchInputError
    with pytest.raises(E):
        srch.check_score(SPCAS9, None, "hsu2013", [q])  # no PAM length
    with pytest.raises(E):
        srch.check_score(SPCAS9, 3, "hsu2013", ["ACGTACGTACGTACGTACGTNGG"])  # a base in the PAM
    with pytest.raises(E):
        srch.check_score(CAS12A_20, 4, "hsu2013", ["TTTA" + "ACGTACGTACGTACGTACGT"])
    for bad in ([0.5] * 19, [0.5] * 21, [0.5] * 19 + [1.5], [0.5] * 19 + [-0.1], [0.5] * 19 + [float("nan")],
                [0.5] * 19 + [float("inf")], [0.5] * 19 + ["x"], "mit"):
        with pytest.raises(E):
            srch.check_score(SPCAS9, 3, bad, [q])
    for pattern, P in ((SACAS9, 6), (CAS12A, 4), ("N" * 18 + "NGG", 3)):  # G = 21, 23, 18
        with pytest.raises(E):
            srch.make_scheme(pattern, P, "hsu2013")
    with pytest.raises(E):
        srch.make_scheme("NNNGGNNN", 3, [0.5] * 5)  # letters outside the PAM
    # a guide shorter than the region is fine: its leading N never mismatch
    short = srch.check_query(SPCAS9, "GTACGTACGTACGTACGT", 3)
    assert short.startswith("NN") and srch.check_score(SPCAS9, 3, "hsu2013", [short]).factor.size == 20
    assert srch.check_score(SPCAS9, None, None, [q]) is None
    with pytest.raises(E):
        srch.parse_weights("0.1 0.2 zero")
    assert srch.parse_weights("# w\n0.1, 0.2\n0.3 # last\n") == [0.1, 0.2, 0.3]


def test_cli_refuses_bad_score_input_before_the_gpu(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">c1\nACGT\n")
    gd = tmp_path / "g.txt"
    gd.write_text("ACGTACGTACGTACGTACGT\n")
    full = tmp_path / "full.txt"
    full.write_text("ACGTACGTACGTACGTACGTNNN\n")
    pam = tmp_path / "pam.txt"
    pam.write_text("ACGTACGTACGTACGTACGTNGG\n")
    w19 = tmp_path / "w19.txt"
    w19.write_text(" ".join(["0.5"] * 19) + "\n")
    wbad = tmp_path / "wbad.txt"
    wbad.write_text(" ".join(["0.5"] * 19 + ["1.5"]) + "\n")
    w20 = tmp_path / "w20.txt"
    w20.write_text(" ".join(["0.5"] * 20) + "\n")
    out = tmp_path / "o.tsv"
    cnt = tmp_path / "c.tsv"
    base = ["--pattern", SPCAS9, "--guides", str(gd), "--pam-length", "3", "-o", str(out)]
    cases = [["--pattern", SPCAS9, "--guides", str(full), "-o", str(out), "--score", "hsu2013"],  # no --pam-length
             base + ["--score", "hsu2013", "--weights", str(w20)],  # mutually exclusive
             base + ["--score", "cfd"],
             base + ["--weights", str(w19)], base + ["--weights", str(wbad)], base + ["--weights", str(tmp_path / "none.txt")],
             ["--pattern", SPCAS9, "--guides", str(pam), "--pam-length", "3", "-o", str(out), "--score", "hsu2013"],
             ["--pattern", SACAS9, "--guides", str(gd), "--pam-length", "6", "-o", str(out), "--score", "hsu2013"],  # G = 21
             base + ["--no-sites", "--counts", str(cnt)],  # -o with --no-sites
             ["--pattern", SPCAS9, "--guides", str(gd), "--pam-length", "3", "--no-sites"],  # no --counts
             ["--pattern", SPCAS9, "--guides", str(gd), "--pam-length", "3"]]  # neither -o nor --no-sites
    for args in cases:
        cmd = [sys.executable, "-m", "cropsr_amd.search", "-f", str(fa)] + args
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 2 and "error:" in r.stderr, (args, r.stderr)
        assert not out.exists() and not cnt.exists()


# ------------------------------------------------------------------ host hit values (CPU)
def _rc(s):
    return s.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


def test_hit_values_on_a_planted_genome():
    guide = "GATTACAGATTACAGATTAC"
    for pattern, P, weights in ((SPCAS9, 3, "hsu2013"), (CAS12A_20, 4, "hsu2013"), (SACAS9, 6, _weights_for(SACAS9)[0])):
        T, pam3 = len(pattern), pattern.startswith("N")
        pam = {SPCAS9: "TGG", CAS12A_20: "TTTC", SACAS9: "CTGAAT"}[pattern]
        w_ref = sref.W_HSU if weights == "hsu2013" else weights
        G = T - P
        full = "A" * (G - 20) + guide  # a guide that fills the region
        queries = [srch.check_query(pattern, full, P), srch.check_query(pattern, guide[2:] if pam3 else guide[:-2], P)]

        def site(region):
            return (region + pam if pam3 else pam + region).encode()

        def sub(region, at, ch):
            return region[:at] + ch + region[at + 1:]

        exact = full
        one = sub(full, G - 1 if pam3 else 0, "a" if pam3 else "c")          # lower case, next to the PAM (g = G - 1)
        two = sub(sub(full, 3, "C" if full[3] != "C" else "G"), 9, "N")      # a non-base in the region mismatches at its g
        far = sub(full, 0 if pam3 else G - 1, "C" if pam3 else "A")         # PAM-distal (g = 0): outside the short guide
        contigs = [b"CC" + site(exact) + b"CCCCCC" + _rc(site(one)) + b"CC", b"TT" + _rc(site(two)) + b"TTTTTTTT" + site(far) + b"TT"]
        factor, shape = sref.tables(w_ref)
        counts, s, hit_sum = sref.search(contigs, pattern, queries, 3, P, factor, shape)
        sites = _sites_array(s)
        assert (counts[0][:3] == [1, 2, 1]).all(), pattern
        sc = srch.make_scheme(pattern, P, weights)
        assert srch.site_masks(sites, queries, contigs, sc).tolist() == s["mask"].tolist()
        v = srch.hit_values(sites, queries, contigs, sc)
        assert v.tolist() == s["value"].tolist()
        for q in range(2):
            assert sum(int(x) for x in v[sites["query"] == q].tolist()) == hit_sum[q]
        # worked by hand: g of each planted mismatch, the same for both PAM sides
        gpos = sref.guide_positions(pattern, P)
        g_two = sorted(gpos.index(p) for p in ((3, 9) if pam3 else (P + 3, P + 9)))
        want = {0: 0, 1 << (G - 1): None, (1 << g_two[0]) | (1 << g_two[1]): None, 1: None}
        assert sorted(set(s["mask"][s["query"] == 0].tolist())) == sorted(want)
        # the short guide does not see the PAM-distal mismatch: that site is a perfect copy for it
        short_far = [m for m, k, mm in zip(s["mask"].tolist(), s["contig"].tolist(), s["mismatches"].tolist())][-1]
        assert 0 in s["mask"][s["query"] == 1].tolist() and short_far in (0, 1)
        # BULGE_SITE_DTYPE rows: a bulge kind's site has the value 0
        b = np.zeros(sites.size, srch.BULGE_SITE_DTYPE)
        for f in srch.SITE_DTYPE.names:
            b[f] = sites[f]
        b["kind"][0::2] = 1
        vb = srch.hit_values(b, queries, contigs, sc)
        assert (vb[0::2] == 0).all() and (vb[1::2] == v[1::2]).all()


# ------------------------------------------------------------------ TSV bytes (CPU)
def test_scored_tsv_bytes():
    queries, counts, sites = _tsv_case()
    names, contig_names = ["g1"], ["c1", "c2"]
    plain_sites = srch.format_sites(names, queries, contig_names, TSV_GENOME, sites)
    plain_counts = srch.format_counts(names, queries, counts)
    # without the options: what test_search.py pins
    assert plain_sites == ("name\tquery\tcontig\tposition\tstrand\tmismatches\tsite\n"
                           "g1\tACGTACGTACGTACGTACGANNN\tc1\t2\t+\t0\tACGTACGTACGTACGTACGAAGG\n"
                           "g1\tACGTACGTACGTACGTACGANNN\tc2\t0\t-\t2\tACGTACGTACGnACGTACGtAGG\n")
    assert plain_counts == "name\tquery\tmm0\tmm1\tmm2\ng1\tACGTACGTACGTACGTACGANNN\t1\t0\t1\n"
    sc = srch.make_scheme(SPCAS9, 3, "hsu2013")
    v = srch.hit_values(sites, queries, TSV_GENOME, sc)
    # the second site mismatches at g = 11 and g = 19
    h = (1.0 - 0.508) * (1.0 - 0.583) * (1.0 / (((19.0 - 8.0) / 19.0) * 4.0 + 1.0) / 4.0)
    assert v.tolist() == [0, int(np.rint(h * ONE))]
    res = srch.SearchResult(counts, sites, (0, 0), np.array([int(v.sum())], dtype=np.uint64))
    text = srch.format_scored_sites(names, queries, contig_names, TSV_GENOME, res, sc)
    assert text == ("name\tquery\tcontig\tposition\tstrand\tmismatches\tsite\thit_score\n"
                    "g1\tACGTACGTACGTACGTACGANNN\tc1\t2\t+\t0\tACGTACGTACGTACGTACGAAGG\t\n"
                    "g1\tACGTACGTACGTACGTACGANNN\tc2\t0\t-\t2\tACGTACGTACGnACGTACGtAGG\t%.6f\n" % h)
    ctext = srch.format_scored_counts(names, queries, res)
    assert ctext == ("name\tquery\tmm0\tmm1\tmm2\thit_sum\tspecificity\n"
                     "g1\tACGTACGTACGTACGTACGANNN\t1\t0\t1\t%.6f\t%.6f\n" % (h, 1.0 / (1.0 + h)))
    # the reference formatter writes the same bytes
    rows = _as_tuples(sites)
    strings = [srch.site_string(TSV_GENOME[k], pos, "+-"[st], queries[q]) for q, k, pos, st, _ in rows]
    assert text == sref.format_sites(names, queries, contig_names, rows, strings, v.tolist())
    assert ctext == sref.format_counts(names, queries, counts, [int(v.sum())])
    # with bulges: the score columns on the kind-none line only, empty for a bulge kind's site
    kinds = srch.bulge_kinds(1, 0)
    b = np.zeros(2, srch.BULGE_SITE_DTYPE)
    for f in srch.SITE_DTYPE.names:
        b[f] = sites[f]
    b["kind"][1], b["bulge_size"][1], b["bulge_at"][1] = 1, 1, 3
    bres = srch.BulgeSearchResult(np.stack([counts, counts], axis=1), b, kinds, np.array([[0, 19]], np.uint8), None, res.hit_sum)
    lines = srch.format_scored_sites(names, queries, contig_names, TSV_GENOME, bres, sc).splitlines()
    assert lines[0].endswith("\tquery_aligned\thit_score") and lines[1].endswith("\t") and lines[2].endswith("\t")
    clines = srch.format_scored_counts(names, queries, bres).splitlines()
    assert clines[0] == "name\tquery\tbulge\tbulge_size\tmm0\tmm1\tmm2\thit_sum\tspecificity"
    assert clines[1].endswith("\t%.6f\t%.6f" % (h, 1.0 / (1.0 + h))) and clines[2].endswith("\tDNA\t1\t1\t0\t1\t\t")


# ------------------------------------------------------------------ ABI and ISA (CPU)
def test_library_declares_score_abi():
    L = nat.lib()
    with open(os.path.join(ROOT, "include", "cropsr_hip.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    assert ("int crp_search_set_scheme(crp_search *search, const double *factor, int n_factor, int pam_side, "
            "const double *shape);") in header
    assert ("int crp_search_run_scored(crp_search *search, const char *queries, uint64_t n_queries, int max_mm, "
            "uint64_t site_cap, uint32_t *counts, uint64_t *n_sites, uint64_t *hit_sum);") in header
    assert hasattr(L, "crp_search_set_scheme") and hasattr(L, "crp_search_run_scored")
    assert nat.SIGNATURES["crp_search_set_scheme"] == (ctypes.c_int, [ctypes.c_void_p, nat.f64p, ctypes.c_int, ctypes.c_int, nat.f64p])
    assert nat.SIGNATURES["crp_search_run_scored"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int,
                                                                      ctypes.c_uint64, nat.u32p, nat.u64p, nat.u64p])
    for name, v in (("CRP_SEARCH_PAM_3PRIME", nat.SEARCH_PAM_3PRIME), ("CRP_SEARCH_PAM_5PRIME", nat.SEARCH_PAM_5PRIME),
                    ("CRP_SEARCH_SHAPE_DOUBLES", nat.SEARCH_SHAPE_DOUBLES)):
        assert re.search(r"#define %s %d\b" % (name, v), header)
    assert nat.SEARCH_SHAPE_DOUBLES == srch.SHAPE_N * srch.SHAPE_D
    assert L.crp_abi_version() == 6 == nat.ABI_VERSION


@pytest.fixture(scope="module")
def search_isa():
    """(assembly, compiler remarks) of crp_search.hip for gfx950 with the library's flags."""
    try:
        hipcc = isa.hipcc()
    except SystemExit:
        pytest.skip("hipcc not found")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "crp_search.s")
        cmd = [hipcc] + isa.makefile_flags() + ["--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                                                "-Rpass-analysis=kernel-resource-usage", os.path.join(isa.CSRC, "crp_search.hip"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        with open(out) as f:
            return f.read(), r.stderr


def _kernel(asm, name):
    return next(m.group(1) for m in re.finditer(r"^(_ZN3crp\S*?\d+%s(?:E|I)\S*):" % name, asm, re.M))


def _figures(search_isa, name):
    """VGPRs, scratch, spills and VALU instructions of a kernel, and of its no-hit loop: the block that compares a lane's
    8 candidates with one query (the one with the 8 popcounts), which ends in the branch on "any hit"."""
    asm, remarks = search_isa
    mangled = _kernel(asm, name)
    res = isa.resources(remarks, mangled)
    blocks = isa.blocks_of(asm, mangled)
    loop = [b for b in blocks if sum(i.startswith("v_bcnt_u32_b32") for i in b[3]) == 8]
    assert len(loop) == 1, name
    assert loop[0][3][-1].startswith("s_cbranch"), name
    return dict(vgprs=int(res["VGPRs"]), scratch=int(res["ScratchSize [bytes/lane]"]), vgpr_spills=int(res["VGPRs Spill"]),
                valu=isa.counts([i for b in blocks for i in b[3]])["valu"], loop_valu=isa.counts(loop[0][3])["valu"],
                f64=isa.counts([i for b in blocks for i in b[3]])["f64"],
                atomics_x2=sum(i.startswith("global_atomic_add_x2") for b in blocks for i in b[3]))


def test_score_kernel_static_isa(search_isa):
    plain = _figures(search_isa, "search_compare_kernel")
    scored = _figures(search_isa, "search_score_compare_kernel")
    bulge = _figures(search_isa, "search_bulge_compare_kernel")
    print("search_compare_kernel", plain, "\nsearch_score_compare_kernel", scored, "\nsearch_bulge_compare_kernel", bulge)
    assert scored["scratch"] == 0 and scored["vgpr_spills"] == 0
    assert scored["loop_valu"] == plain["loop_valu"]  # (41 today: compared with the sibling kernel of the same build)
    assert scored["f64"] > 0 and scored["atomics_x2"] > plain["atomics_x2"]
    # the other two compare kernels are the parent's
    assert (plain["vgprs"], plain["valu"]) == (59, 342) and plain["scratch"] == 0
    assert (bulge["vgprs"], bulge["valu"]) == (92, 623) and bulge["scratch"] == 0


# ------------------------------------------------------------------ the library (GPU)
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def _case(pattern, seed, n_queries=20, chars=300_000, n_contigs=14, max_mm=8):
    rng = np.random.default_rng(1000 + seed)
    P = PAM_LEN.get(pattern, 4)
    G = len(pattern) - P
    if pattern in PAM_LEN:
        queries = _queries_for(rng, pattern, n_queries)
    else:
        queries = [srch.check_query(pattern, "".join(rng.choice(list("ACGT"), G)), P) for _ in range(n_queries)]
    queries[-1] = srch.check_query(pattern, "".join(rng.choice(list("ACGT"), G - 2)), P)  # a short guide next to the PAM
    contigs = _planted_genome(rng, pattern, chars, n_contigs, queries[:14] + queries[-1:], max_mm)
    return P, queries, contigs


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,seed", [(SPCAS9, 1), (SPCAS9_NAG, 2), (CAS12A, 3), (SACAS9, 4), (CAS12A_20, 5)])
def test_gpu_hit_sums_match_reference(engine, pattern, seed):
    P, queries, contigs = _case(pattern, seed)
    score, w_ref = _weights_for(pattern, seed)
    factor, shape = sref.tables(w_ref)
    scheme = srch.make_scheme(pattern, P, score)
    g = engine.genome(contigs)
    try:
        for M in (4, 8):
            want_counts, s, want_sum = sref.search(contigs, pattern, queries, M, P, factor, shape)
            res = g.search(pattern, queries, M, pam_len=P, score=score)
            assert res.hit_sum.dtype == np.uint64 and [int(x) for x in res.hit_sum] == want_sum, (pattern, M)
            assert sum(want_sum) > 0 and sum(1 for x in want_sum if x) >= 10
            assert res.specificity.tolist() == sref.specificity(want_sum)
            plain = g.search(pattern, queries, M, pam_len=P)
            assert plain.hit_sum is None and plain.specificity is None
            assert (res.counts == plain.counts).all() and (res.counts == want_counts).all()
            assert (res.sites == plain.sites).all() and res.sites.size == int(want_counts.sum())
            # the device's sums against the host's values of the fetched sites: a different route to the same integers
            v = srch.hit_values(res.sites, queries, contigs, scheme)
            assert v.tolist() == s["value"].tolist()
            for q in range(len(queries)):
                assert sum(int(x) for x in v[res.sites["query"] == q].tolist()) == int(res.hit_sum[q]), (pattern, M, q)
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_hit_sums_do_not_depend_on_the_cut(engine):
    """Several arenas, a budget that forces chunks, and many launches with a device site list that must grow (the compare
    runs twice: a hit must not be added twice) all give the uncut run's sums."""
    rng = np.random.default_rng(31)
    queries = _queries_for(rng, SPCAS9, 300)
    contigs = _planted_genome(rng, SPCAS9, 700_000, 20, queries[:40], 4)
    factor, shape = sref.tables(sref.W_HSU)
    want_counts, s, want_sum = sref.search(contigs, SPCAS9, queries, 4, 3, factor, shape)
    assert int(want_counts.sum()) > 16 * 4
    one = engine.genome(contigs)
    many = engine.genome(contigs, max_words=3000)
    try:
        assert len(many.arenas) > 3 and len(one.arenas) == 1
        uncut = one.search(SPCAS9, queries, 4, pam_len=3, score="hsu2013")
        assert [int(x) for x in uncut.hit_sum] == want_sum and (uncut.counts == want_counts).all()
        for g, budget in ((many, None), (one, 1), (many, 1)):
            res = g.search(SPCAS9, queries, 4, pam_len=3, score="hsu2013", budget=budget)
            assert (res.hit_sum == uncut.hit_sum).all() and (res.counts == uncut.counts).all(), budget
            assert (res.sites == uncut.sites).all()
        h = srch.ArenaSearch(one.arenas[0], SPCAS9)
        try:
            h.set_scheme(srch.make_scheme(SPCAS9, 3, "hsu2013"))
            h.set_limits(batch_queries=7, first_site_slots=16)
            st, counts, n, hit_sum = h.run_scored(queries, 4, 1 << 40)
            assert st == nat.CRP_OK and n == int(want_counts.sum()) and (counts == want_counts).all()
            assert h.stats()["compare_launches"] == 2 * 43  # ceil(300 / 7) launches, twice: the site list grew once
            assert [int(x) for x in hit_sum] == want_sum
            st, counts, n, hit_sum = h.run_scored(queries, 4, 1 << 40)  # the list is large enough now: one pass
            assert st == nat.CRP_OK and h.stats()["compare_launches"] == 3 * 43 and [int(x) for x in hit_sum] == want_sum
        finally:
            h.close()
        hb = srch.ArenaSearch(one.arenas[0], SPCAS9, budget=1)
        try:
            hb.set_scheme(srch.make_scheme(SPCAS9, 3, "hsu2013"))
            hb.set_limits(batch_queries=64, first_site_slots=16)
            st, counts, n, hit_sum = hb.run_scored(queries, 4, 1 << 40)
            assert st == nat.CRP_OK and hb.stats()["chunks"] >= 2 and [int(x) for x in hit_sum] == want_sum
        finally:
            hb.close()
    finally:
        one.close()
        many.close()


@pytest.mark.gpu
def test_gpu_score_only_and_abi_states(engine):
    P, queries, contigs = _case(SPCAS9, 9, n_queries=12, chars=200_000, n_contigs=6, max_mm=4)
    queries.append("N" * 23)  # every candidate hits with n = 0
    factor, shape = sref.tables(sref.W_HSU)
    want_counts, s, want_sum = sref.search(contigs, SPCAS9, queries, 4, 3, factor, shape)
    assert want_sum[-1] == 0 and int(want_counts[-1, 0]) > 1000 and sum(want_sum) > 0
    g = engine.genome(contigs)
    L = nat.lib()
    try:
        res = g.search(SPCAS9, queries, 4, pam_len=3, score="hsu2013", site_cap=0, sites=False)
        assert res.sites.size == 0 and (res.counts == want_counts).all() and [int(x) for x in res.hit_sum] == want_sum
        res = g.search(SPCAS9, queries, 4, pam_len=3, sites=False)  # counts only
        assert res.sites.size == 0 and (res.counts == want_counts).all() and res.hit_sum is None
        with pytest.raises(srch.SiteCapacityError):  # without sites=False the capacity behaviour is today's
            g.search(SPCAS9, queries, 4, pam_len=3, score="hsu2013", site_cap=0)
        h = srch.ArenaSearch(g.arenas[0], SPCAS9)
        try:
            blob = "".join(queries).encode()
            Q = len(queries)
            counts = np.zeros((Q, 5), dtype=np.uint32)
            hit_sum = np.zeros(Q, dtype=np.uint64)
            n = ctypes.c_uint64()
            args = (blob, Q, 4, 0, counts.ctypes.data_as(nat.u32p), ctypes.byref(n), hit_sum.ctypes.data_as(nat.u64p))
            assert L.crp_search_run_scored(h._h, *args) == nat.CRP_ERR_STATE  # no scheme
            sc = srch.make_scheme(SPCAS9, 3, "hsu2013")
            h.set_scheme(sc)
            assert L.crp_search_run_scored(h._h, *args) == nat.CRP_ERR_CAPACITY
            assert n.value == int(want_counts.sum()) and (counts == want_counts).all() and [int(x) for x in hit_sum] == want_sum
            assert L.crp_search_fetch(h._h, None, None, None, None, 1 << 40) == nat.CRP_ERR_STATE
            h.set_scheme(None)
            assert L.crp_search_run_scored(h._h, *args) == nat.CRP_ERR_STATE  # a cleared scheme
            # misuse
            f = sc.factor.ctypes.data_as(nat.f64p)
            sh = np.ascontiguousarray(sc.shape).reshape(-1)
            shp = sh.ctypes.data_as(nat.f64p)
            assert L.crp_search_set_scheme(h._h, f, 20, 0, None) == nat.CRP_ERR_INVALID
            assert L.crp_search_set_scheme(h._h, f, 0, 0, shp) == nat.CRP_ERR_INVALID
            assert L.crp_search_set_scheme(h._h, f, 24, 0, shp) == nat.CRP_ERR_INVALID
            assert L.crp_search_set_scheme(h._h, f, 20, 2, shp) == nat.CRP_ERR_INVALID
            assert L.crp_search_set_scheme(None, f, 20, 0, shp) == nat.CRP_ERR_INVALID
            for bad in (1.5, -0.5, float("nan"), float("inf")):
                fb = sc.factor.copy()
                fb[3] = bad
                assert L.crp_search_set_scheme(h._h, fb.ctypes.data_as(nat.f64p), 20, 0, shp) == nat.CRP_ERR_INVALID
                sb = sh.copy()
                sb[40] = bad
                assert L.crp_search_set_scheme(h._h, f, 20, 0, sb.ctypes.data_as(nat.f64p)) == nat.CRP_ERR_INVALID
            assert L.crp_search_run_scored(h._h, *args) == nat.CRP_ERR_STATE  # a refused scheme sets nothing
            assert L.crp_search_set_scheme(h._h, f, 20, 0, shp) == nat.CRP_OK
            pam = ("A" * 20 + "NGG").encode()
            assert L.crp_search_run_scored(h._h, pam, 1, 4, 0, None, ctypes.byref(n), hit_sum.ctypes.data_as(nat.u64p)) == nat.CRP_ERR_INVALID
            assert L.crp_search_run_scored(h._h, blob, Q, 4, 0, None, ctypes.byref(n), None) == nat.CRP_ERR_INVALID
            # an unscored run on the same handle is untouched by the scheme
            st, c, m = h.run(queries, 4, 1 << 40)
            assert st == nat.CRP_OK and (c == want_counts).all()
        finally:
            h.close()
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_scored_bulge_search(engine):
    P, queries, contigs = _case(SPCAS9, 12, n_queries=10, chars=150_000, n_contigs=6, max_mm=4)
    g = engine.genome(contigs)
    try:
        plain = g.search(SPCAS9, queries, 4, pam_len=3, score="hsu2013")
        unscored = g.search_bulges(SPCAS9, queries, 4, 3, 1, 1)
        res = g.search_bulges(SPCAS9, queries, 4, 3, 1, 1, score="hsu2013")
        assert (res.hit_sum == plain.hit_sum).all() and int(plain.hit_sum.sum()) > 0
        assert (res.specificity == plain.specificity).all()
        assert (res.counts == unscored.counts).all() and (res.sites == unscored.sites).all() and unscored.hit_sum is None
        assert (res.sites["kind"] != 0).any()
        only = g.search_bulges(SPCAS9, queries, 4, 3, 1, 1, score="hsu2013", sites=False)
        assert only.sites.size == 0 and (only.counts == res.counts).all() and (only.hit_sum == res.hit_sum).all()
        # the hit values of a bulge search's site list: kind none only
        v = srch.hit_values(res.sites, queries, contigs, srch.make_scheme(SPCAS9, 3, "hsu2013"))
        assert (v[res.sites["kind"] != 0] == 0).all()
        for q in range(len(queries)):
            assert sum(int(x) for x in v[res.sites["query"] == q].tolist()) == int(res.hit_sum[q])
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_scored_cli_end_to_end(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">c1 first\nTTACGTACGTACGT\nACGTACGAAGGTT\n>c2\nCCTACGTACGTNCGTACGTACGTAA\n")
    gd = tmp_path / "guides.txt"
    gd.write_text("ACGTACGTACGTACGTACGA g1\nCGTACGTACGTACGTACG g2\n")
    names = ["g1", "g2"]
    queries = [srch.check_query(SPCAS9, "ACGTACGTACGTACGTACGA", 3), srch.check_query(SPCAS9, "CGTACGTACGTACGTACG", 3)]
    wf = tmp_path / "w.txt"
    weights = [round(0.04 * k, 2) for k in range(20)]
    wf.write_text("# PAM-distal first\n" + " ".join(str(w) for w in weights[:10]) + "\n" + ", ".join(str(w) for w in weights[10:]) + "\n")
    base = [sys.executable, "-m", "cropsr_amd.search", "-f", str(fa), "--pattern", SPCAS9, "--guides", str(gd), "--pam-length", "3",
            "-m", "3"]
    for opt, w_ref in ((["--score", "hsu2013"], sref.W_HSU), (["--weights", str(wf)], weights)):
        factor, shape = sref.tables(w_ref)
        counts, s, hit_sum = sref.search(TSV_GENOME, SPCAS9, queries, 3, 3, factor, shape)
        rows = list(zip(*[s[f].tolist() for f in ref.SITE_FIELDS]))
        strings = [srch.site_string(TSV_GENOME[k], pos, "+-"[st], queries[q]) for q, k, pos, st, _ in rows]
        assert sum(hit_sum) > 0
        out, cnt = tmp_path / "sites.tsv", tmp_path / "counts.tsv"
        r = subprocess.run(base + opt + ["-o", str(out), "--counts", str(cnt)], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert out.read_text() == sref.format_sites(names, queries, ["c1", "c2"], rows, strings, s["value"].tolist())
        assert cnt.read_text() == sref.format_counts(names, queries, counts, hit_sum)
        only = tmp_path / "only.tsv"
        out.unlink()
        r = subprocess.run(base + opt + ["--no-sites", "--counts", str(only)], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert only.read_text() == cnt.read_text() and not out.exists()
    # without the options both files are today's
    r = subprocess.run(base + ["-o", str(out), "--counts", str(cnt)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    counts, s = ref.search(TSV_GENOME, SPCAS9, queries, 3)
    sites = _sites_array(s)
    assert out.read_text() == srch.format_sites(names, queries, ["c1", "c2"], TSV_GENOME, sites)
    assert cnt.read_text() == srch.format_counts(names, queries, counts)
