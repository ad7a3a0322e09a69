"""The self search (search.py search_self / --self, crp_search_self_*; DESIGN.md section 15, Self search): the definition
stated twice, hand-made answers, refusals, TSV bytes, the ABI and the compare kernel's static ISA without a GPU; the
device's rows against the reference and against the given-guides search, exactly, on the GPU."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

import search_score_reference as sref
import search_self_reference as selfref
from cropsr_amd import _native as nat
from cropsr_amd import search as srch
from test_search import CAS12A, PAM_LEN, SACAS9, SPCAS9, SPCAS9_NAG, _planted_genome, _queries_for
from test_search_score import CAS12A_20, _figures, _weights_for, search_isa  # noqa: F401  (search_isa: a fixture)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import emit_isa_budget as isa  # noqa: E402

ONE = 1 << 30
P_OF = dict(PAM_LEN)
P_OF[CAS12A_20] = 4


def _genome(rng, pattern, chars, n_contigs, families=30, plant_mm=2):
    """A planted genome (mixed case, N runs, IUPAC letters, U, short contigs) with families of near copies on both strands,
    overlapping '+' / '-' sites and exact copies."""
    P = P_OF[pattern]
    G = len(pattern) - P
    guides = [srch.check_query(pattern, "".join(rng.choice(list("ACGT"), G)), P) for _ in range(families)]
    contigs = _planted_genome(rng, pattern, chars, n_contigs, guides, plant_mm)
    if pattern.startswith("N"):  # a palindromic stretch: CCN ... NGG carries a '+' and a '-' site at one position
        pal = b"CCA" + b"ACGTTGCAACGTTGCAT"[:len(pattern) - 6] + b"TGG"
        contigs.append(bytearray(b"TT" + pal + b"TTTT" + pal + b"TT"))
    return [bytes(c) for c in contigs]


def _rows(res):
    return list(zip(res.sites["contig"].tolist(), res.sites["position"].tolist(), (res.sites["strand"] == b"-").astype(int).tolist()))


# ------------------------------------------------------------------ the definition (CPU)
def test_two_statements_of_the_definition_agree():
    for seed, (pattern, gp) in enumerate([(SPCAS9, None), (SPCAS9_NAG, SPCAS9), (CAS12A_20, None), (SACAS9, None)]):
        rng = np.random.default_rng(500 + seed)
        contigs = _genome(rng, pattern, 9000, 5, families=8)
        _, w = _weights_for(pattern, seed)
        for M in (0, 2, 4):
            a = selfref.search_self(contigs, pattern, M, P_OF[pattern], gp, w)
            b = selfref.search_self_pairs(contigs, pattern, M, P_OF[pattern], gp, w)
            assert a[0] == b[0] and a[1] == b[1] and len(a[0]) > 50
            assert (a[2] == b[2]).all() and a[3] == b[3]
            if M == 4:
                assert int(a[2].sum()) > 20 and sum(a[3]) > 0
    # NGG guides among NRG candidates: fewer guide sites than candidates, the rows count the NAG sites too
    rng = np.random.default_rng(9)
    contigs = _genome(rng, SPCAS9_NAG, 9000, 4, families=8)
    (k, pos, strand, O), g = selfref.guide_sites(contigs, SPCAS9_NAG, 3, SPCAS9)
    assert 0 < int(g.sum()) < g.size and (O[g][:, 21] == 2).all() and (O[~g][:, 21] == 0).any()


HAND = "ATATTATAATATTAATATAT"  # no G or C: the only sites are the three planted ones


def _hand_genome():
    a = HAND + "TGG"
    b = HAND[:19] + "A" + "TGG"            # one mismatch next to the PAM (g = 19)
    c = HAND[:5] + "N" + HAND[6:] + "TGG"  # a non-base at g = 5: a candidate, not a guide site
    return [("TTTT" + a + "TTTT" + b.lower() + "TTTT").encode(), ("TT" + c + "TT").encode()]


def test_known_answers():
    contigs = _hand_genome()
    for fn in (selfref.search_self, selfref.search_self_pairs):
        sites, guides, counts, hit_sum = fn(contigs, SPCAS9, 2, 3, None, sref.W_HSU)
        assert sites == [(0, 4, 0), (0, 31, 0)] and guides == [HAND, HAND[:19] + "A"]
        # the exact copy sees the g = 19 copy and the N copy at one mismatch each; the g = 19 copy sees the exact one at
        # one, the N copy at two (g = 5 and g = 19: d = 14)
        assert counts.tolist() == [[0, 2, 0], [0, 1, 1]]
        f5, f19 = 1.0 - 0.395, 1.0 - 0.583
        two = f5 * f19 * (1.0 / (((19.0 - 14.0) / 19.0) * 4.0 + 1.0) / 4.0)
        assert hit_sum == [int(np.rint(f19 * ONE)) + int(np.rint(f5 * ONE)), int(np.rint(f19 * ONE)) + int(np.rint(two * ONE))]
        assert abs(hit_sum[0] / ONE - (0.417 + 0.605)) < 1e-8
    sites, guides, counts, hit_sum = selfref.search_self(contigs, SPCAS9, 0, 3)
    assert counts.tolist() == [[0], [0]] and hit_sum is None


# ------------------------------------------------------------------ refusals (CPU)
def test_refusals():
    E = srch.SearchInputError
    ok = srch.check_self(SPCAS9_NAG, 4, 3, SPCAS9, "hsu2013")
    assert ok[:4] == (SPCAS9_NAG, SPCAS9, 4, 3) and ok[4].factor.size == 20
    assert srch.check_self(SPCAS9, 0, 3)[1] == SPCAS9 and srch.check_self(SPCAS9, 0, 3)[4] is None
    bad = [dict(pam_len=None), dict(max_mm=5), dict(max_mm=-1), dict(max_mm=1.5),
           dict(guide_pattern="N" * 19 + "ANGG"),           # a letter in the guide region
           dict(guide_pattern="N" * 21 + "RG"),             # wider than the pattern at a PAM position
           dict(guide_pattern="N" * 21 + "GGN"),            # another length
           dict(guide_pattern="N" * 21 + "GX"),
           dict(score="mit"), dict(score=[0.5] * 19), dict(score=[0.5] * 19 + [1.5])]
    for kw in bad:
        args = dict(pattern=SPCAS9, max_mm=3, pam_len=3)
        args.update(kw)
        with pytest.raises(E):
            srch.check_self(**args)
        with pytest.raises(E):  # search_self refuses before it touches the genome (None has no arenas)
            srch.search_self(None, args["pattern"], args["max_mm"], args["pam_len"], guide_pattern=args.get("guide_pattern"),
                             score=args.get("score"))
    with pytest.raises(E):
        srch.check_self(SACAS9, 3, 6, None, "hsu2013")  # G = 21
    with pytest.raises(E):
        srch.check_self("NNNGGNNN", 2, 3)  # letters outside the PAM
    with pytest.raises(E):
        srch.check_self("NNNGG", 3, 2)     # 3 guide positions cannot hold 4 segments


def test_cli_refuses_before_the_gpu(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">c1\nACGT\n")
    gd = tmp_path / "g.txt"
    gd.write_text("ACGTACGTACGTACGTACGT\n")
    out, cnt = tmp_path / "o.tsv", tmp_path / "c.tsv"
    base = ["--pattern", SPCAS9, "--pam-length", "3", "--self", "-o", str(out)]
    cases = [(["--pattern", SPCAS9, "--self", "-o", str(out)], "PAM"),  # no --pam-length
             (base + ["-m", "5"], "0..4"),
             (base + ["--guides", str(gd)], "--guides"),
             (base + ["--dna-bulge", "1"], "--dna-bulge"),
             (base + ["--rna-bulge", "1"], "--rna-bulge"),
             (base + ["--counts", str(cnt)], "--counts"),
             (["--pattern", SPCAS9, "--pam-length", "3", "--self", "--no-sites"], "--no-sites"),
             (["--pattern", SPCAS9, "--pam-length", "3", "--self"], "-o"),
             (base + ["--guide-pattern", "N" * 21 + "RG"], "accepts"),
             (base + ["--score", "cfd"], "cfd"),
             (["--pattern", SACAS9, "--pam-length", "6", "--self", "-o", str(out), "--score", "hsu2013"], "hsu2013"),
             (["--pattern", SPCAS9, "--pam-length", "3", "--guides", str(gd), "-o", str(out), "--guide-pattern", SPCAS9], "--self")]
    for args, word in cases:
        cmd = [sys.executable, "-m", "cropsr_amd.search", "-f", str(fa)] + args
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 2 and "error:" in r.stderr and word in r.stderr, (args, r.stderr)
        assert not out.exists() and not cnt.exists()


# ------------------------------------------------------------------ TSV bytes (CPU)
def test_tsv_bytes():
    sites = np.array([(0, 4, b"+"), (1, 31, b"-")], dtype=srch.SELF_SITE_DTYPE)
    guides = np.array([HAND.encode(), (HAND[:19] + "A").encode()])
    counts = np.array([[0, 2, 0], [3, 1, 1]], dtype=np.uint32)
    hs = np.array([ONE + ONE // 2, 3 * ONE], dtype=np.uint64)
    res = srch.SelfSearchResult(sites, guides, counts, hs, (3, 0), (5, 6))
    assert res.specificity.tolist() == [0.4, 0.25]
    text = "".join(srch.format_self(["c1", "c2"], res, block=1))
    assert text == ("contig\tposition\tstrand\tguide\tn0\tn1\tn2\thit_sum\tspecificity\n"
                    "c1\t4\t+\tATATTATAATATTAATATAT\t0\t2\t0\t1.500000\t0.400000\n"
                    "c2\t31\t-\tATATTATAATATTAATATAA\t3\t1\t1\t3.000000\t0.250000\n")
    assert text == "".join(srch.format_self(["c1", "c2"], res))  # (the block size does not show)
    assert text == selfref.format_rows(["c1", "c2"], [(0, 4, 0), (1, 31, 1)], [HAND, HAND[:19] + "A"], counts, hs.tolist())
    plain = srch.SelfSearchResult(sites, guides, counts, None, (3, 0), (5, 6))
    assert "".join(srch.format_self(["c1", "c2"], plain)).splitlines()[1] == "c1\t4\t+\tATATTATAATATTAATATAT\t0\t2\t0"
    empty = srch.SelfSearchResult(sites[:0], guides[:0], counts[:0], None, (0, 0), (0, 0))
    assert "".join(srch.format_self([], empty)) == "contig\tposition\tstrand\tguide\tn0\tn1\tn2\n"


# ------------------------------------------------------------------ ABI and ISA (CPU)
def test_library_declares_self_abi():
    L = nat.lib()
    with open(os.path.join(ROOT, "include", "cropsr_hip.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    c_types = {"crp_arena *": ctypes.c_void_p, "crp_search_self *": ctypes.c_void_p, "const crp_search_self *": ctypes.c_void_p,
               "const char *": ctypes.c_char_p, "int": ctypes.c_int, "uint64_t": ctypes.c_uint64, "uint64_t *": nat.u64p,
               "uint32_t *": nat.u32p, "uint8_t *": nat.u8p, "const double *": nat.f64p, "double *": nat.f64p,
               "crp_search_self **": nat.voidpp}
    names = ["create", "destroy", "set_limits", "set_scheme", "sizes", "order", "compare", "fetch", "stats"]
    for name in names:
        sym = "crp_search_self_" + name
        m = re.search(r"int %s\(([^)]*)\);" % sym, header)
        assert m, sym
        want = []
        for arg in m.group(1).split(","):
            t = re.match(r"\s*(.*?)(\w+)\s*$", arg).group(1).strip()
            want.append(c_types[t])
        assert nat.SIGNATURES[sym] == (ctypes.c_int, want), sym
        assert hasattr(L, sym)
    assert re.search(r"#define CRP_SEARCH_SELF_MAX_MM %d\b" % nat.SEARCH_SELF_MAX_MM, header) and nat.SEARCH_SELF_MAX_MM == srch.MAX_SELF_MM
    assert L.crp_abi_version() == 6 == nat.ABI_VERSION


@pytest.fixture(scope="module")
def self_isa():
    """(assembly, compiler remarks) of crp_search_self.hip for gfx950 with the library's flags."""
    try:
        hipcc = isa.hipcc()
    except SystemExit:
        pytest.skip("hipcc not found")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "crp_search_self.s")
        cmd = [hipcc] + isa.makefile_flags() + ["--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                                                "-Rpass-analysis=kernel-resource-usage", os.path.join(isa.CSRC, "crp_search_self.hip"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        with open(out) as f:
            return f.read(), r.stderr


def test_self_compare_kernel_static_isa(self_isa, search_isa):  # noqa: F811
    asm, remarks = self_isa
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    for scored in (0, 1):
        mangled = next(m.group(1) for m in re.finditer(r"^(_ZN3crp\S*search_self_compare_kernelILb%dE\S*):" % scored, asm, re.M))
        res = isa.resources(remarks, mangled)
        assert int(res["ScratchSize [bytes/lane]"]) == 0 and int(res["VGPRs Spill"]) == 0 and int(res["SGPRs Spill"]) == 0
        blocks = isa.blocks_of(asm, mangled)
        loop = [b for b in blocks if sum(i.startswith("v_bcnt_u32_b32") for i in b[3]) == 8]  # 8 pairs per trip
        assert len(loop) == 1 and loop[0][3][-1].startswith("s_cbranch")
        ins = loop[0][3]
        valu = isa.counts(ins)["valu"]
        print("search_self_compare_kernel<%d>" % scored, res["VGPRs"], "VGPRs, no-hit loop:", valu, "VALU per 8 pairs")
        # the candidates come through scalar loads (one of 8 words per field), nothing in the loop touches memory otherwise
        assert sum(i.startswith("s_load_dwordx8") for i in ins) == 3
        assert not any(i.startswith(("global_", "flat_", "buffer_", "ds_", "scratch_")) for i in ins)
        assert "%d VALU instructions per 8 pairs" % valu in design  # DESIGN section 15 quotes what the loop holds
        assert "%.3f per pair" % (valu / 8.0) in design
    # the three kernels of the given-guides search are the parent's
    plain = _figures(search_isa, "search_compare_kernel")
    scored = _figures(search_isa, "search_score_compare_kernel")
    bulge = _figures(search_isa, "search_bulge_compare_kernel")
    assert (plain["vgprs"], plain["valu"], plain["loop_valu"]) == (59, 342, 41)
    assert (bulge["vgprs"], bulge["valu"]) == (92, 623)
    assert (scored["vgprs"], scored["valu"], scored["loop_valu"]) == (SCORED_VGPRS, SCORED_VALU, 41)


SCORED_VGPRS, SCORED_VALU = 68, 550  # search_score_compare_kernel on the parent commit


# ------------------------------------------------------------------ the library (GPU)
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def _assert_equals_reference(res, want, scored):
    sites, guides, counts, hit_sum = want
    assert _rows(res) == sites
    assert [g.decode() for g in res.guides.tolist()] == guides
    assert res.counts.dtype == np.uint32 and (res.counts.astype(np.int64) == counts).all()
    if scored:
        assert res.hit_sum.dtype == np.uint64 and [int(x) for x in res.hit_sum] == hit_sum
        assert res.specificity.tolist() == sref.specificity(hit_sum)
    else:
        assert res.hit_sum is None and res.specificity is None


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,gp,seed", [(SPCAS9, None, 1), (SPCAS9_NAG, SPCAS9, 2), (SACAS9, None, 3), (CAS12A_20, None, 4),
                                             (CAS12A, None, 5)])
def test_gpu_matches_reference(engine, pattern, gp, seed):
    rng = np.random.default_rng(7000 + seed)
    contigs = _genome(rng, pattern, 60_000, 9, families=40)
    P = P_OF[pattern]
    score, w_ref = _weights_for(pattern, seed)
    g = engine.genome(contigs)
    try:
        for M in range(5):
            want = selfref.search_self(contigs, pattern, M, P, gp, w_ref)
            res = g.search_self(pattern, M, P, guide_pattern=gp, score=score)
            _assert_equals_reference(res, want, True)
            assert len(want[0]) > 200 and res.pairs[0] <= res.pairs[1] == len(want[0]) * sum(res.candidates)
            if M >= 2:
                assert int(want[2][:, 1:].sum()) > 100 and sum(want[3]) > 0
            plain = g.search_self(pattern, M, P, guide_pattern=gp)
            _assert_equals_reference(plain, (want[0], want[1], want[2], None), False)
    finally:
        g.close()


def _queries_of_rows(res, pattern, P):
    return [srch.check_query(pattern, gd.decode(), P) for gd in res.guides.tolist()]


def _mutated_copy(rng, seq, rate):
    a = np.frombuffer(seq, dtype=np.uint8).copy()
    at = np.nonzero(rng.random(a.size) < rate)[0]
    a[at] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), at.size)
    return a.tobytes()


@pytest.mark.gpu
def test_gpu_matches_given_guides_search_row_by_row(engine):
    """A few Mb with a second copy carrying 3 % substitutions (thousands of near copies), a poly-A run, and tandem
    repeats whose buckets are longer than one workgroup's tile of guide sites and one slice of candidates."""
    rng = np.random.default_rng(77)
    first = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 1_200_000).tobytes()
    contigs = [first, _mutated_copy(rng, first, 0.03), b"A" * 5000 + b"ACAGGTA" * 3000 + b"A" * 3000, (b"A" * 21 + b"GG") * 700]
    g = engine.genome(contigs)
    try:
        res = g.search_self(SPCAS9, 3, 3, score="hsu2013")
        queries = _queries_of_rows(res, SPCAS9, 3)
        assert len(queries) > 250_000
        ref_res = g.search(SPCAS9, queries, 3, pam_len=3, score="hsu2013", sites=False)
        want = ref_res.counts.astype(np.int64)
        want[:, 0] -= 1
        assert (res.counts.astype(np.int64) == want).all() and (res.hit_sum == ref_res.hit_sum).all()
        assert int((want[:, 1:].sum(axis=1) > 0).sum()) > 5000  # the near copies
        assert int(want[:, 0].max()) >= 2900                     # the tandem repeat: some 3 000 copies of one window
        assert res.pairs[0] < res.pairs[1] // 50
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_result_does_not_depend_on_the_cut(engine):
    rng = np.random.default_rng(31)
    contigs = _genome(rng, SPCAS9, 700_000, 20, families=60)
    one = engine.genome(contigs)
    many = engine.genome(contigs, max_words=3000)
    try:
        assert len(many.arenas) >= 3 and len(one.arenas) == 1
        uncut = one.search_self(SPCAS9, 4, 3, score="hsu2013")
        assert uncut.stats["compare_launches"] == 5 and int(uncut.counts[:, 1:].sum()) > 500
        cut = many.search_self(SPCAS9, 4, 3, score="hsu2013")
        low = one.search_self(SPCAS9, 4, 3, score="hsu2013", pairs_per_launch=1 << 18)
        both = many.search_self(SPCAS9, 4, 3, score="hsu2013", pairs_per_launch=1 << 18)
        assert low.stats["compare_launches"] >= 20
        for res in (cut, low, both):
            assert (res.sites == uncut.sites).all() and (res.guides == uncut.guides).all()
            assert (res.counts == uncut.counts).all() and (res.hit_sum == uncut.hit_sum).all()
            assert res.candidates == uncut.candidates and res.pairs[1] == uncut.pairs[1]
        assert low.pairs == uncut.pairs
    finally:
        one.close()
        many.close()


@pytest.mark.gpu
def test_gpu_pairs_agreeing_in_several_segments_count_once(engine):
    """Only exact and 1-mismatch copies: every pair agrees in at least M of the M + 1 segments."""
    rng = np.random.default_rng(5)
    base = "".join(rng.choice(list("ACGT"), 20))
    n_exact, variants = 40, []
    for p in (0, 4, 7, 12, 19):  # one substitution each, at different positions
        variants.append(base[:p] + {"A": "C", "C": "G", "G": "T", "T": "A"}[base[p]] + base[p + 1:])
    spacer = "TATATTTAATATAT"  # (no G or C: no site of its own, and none across a junction)
    seq = spacer.join([base + "TGG"] * n_exact + [v + "AGG" for v in variants])
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    contigs = [("TTTT" + seq + "TTTT").encode(), ("TTTT" + seq + "TTTT").encode().translate(comp)[::-1]]
    for M in (1, 2, 3, 4):
        want = selfref.search_self(contigs, SPCAS9, M, 3)
        n_sites = len(want[0])
        g = engine.genome(contigs)
        try:
            res = g.search_self(SPCAS9, M, 3)
        finally:
            g.close()
        assert (res.counts.astype(np.int64) == want[2]).all()
        # closed form for the rows of the exact copies (those whose guide is `base`): the other 2 * 40 - 1 exact copies, and
        # 2 * 5 variants at one mismatch; unrelated windows of the construction aside, every row's pairs are counted once
        rows = [i for i, gd in enumerate(res.guides.tolist()) if gd.decode() == base]
        assert len(rows) == 2 * n_exact and n_sites >= 2 * (n_exact + 5)
        for i in rows:
            assert res.counts[i, 0] == 2 * n_exact - 1 and res.counts[i, 1] == 2 * len(variants)


@pytest.mark.gpu
def test_gpu_capacity(engine):
    rng = np.random.default_rng(11)
    contigs = _genome(rng, SPCAS9, 200_000, 6)
    g = engine.genome(contigs)
    try:
        assert len(g.arenas) == 1
        with pytest.raises(srch.SelfCapacityError) as e:
            g.search_self(SPCAS9, 3, 3, budget=1000)
        need = e.value.needed
        assert "%d bytes" % need in str(e.value)
        with pytest.raises(srch.SelfCapacityError):
            g.search_self(SPCAS9, 3, 3, budget=need - 1)
        res = g.search_self(SPCAS9, 3, 3, budget=need)
        assert res.stats["device_bytes"] == need >= sum(res.candidates) * (45 + 4 * 4)
        want = selfref.search_self(contigs, SPCAS9, 3, 3)
        _assert_equals_reference(res, want, False)
        # the C ABI: the needed size comes back with the status, and no handle
        h, nb = ctypes.c_void_p(), ctypes.c_uint64()
        st = nat.lib().crp_search_self_create(g.arenas[0]._h, SPCAS9.encode(), None, 23, 3, 3, 1000, ctypes.byref(nb), ctypes.byref(h))
        assert st == nat.CRP_ERR_CAPACITY and nb.value == need and not h.value
        assert nat.lib().crp_search_self_create(g.arenas[0]._h, SPCAS9.encode(), None, 23, 3, 5, 0, None, ctypes.byref(h)) == nat.CRP_ERR_UNSUPPORTED
        assert nat.lib().crp_search_self_create(g.arenas[0]._h, SPCAS9.encode(), SPCAS9_NAG.encode(), 23, 3, 3, 0, None,
                                                ctypes.byref(h)) == nat.CRP_ERR_INVALID
    finally:
        g.close()


@pytest.mark.gpu
def test_gpu_cli_end_to_end(tmp_path):
    rng = np.random.default_rng(3)
    contigs = _genome(rng, SPCAS9_NAG, 20_000, 4, families=10)
    contigs = [c for c in contigs if len(c) > 0]
    names = ["c%d" % k for k in range(len(contigs))]
    fa = tmp_path / "g.fa"
    with open(fa, "wb") as f:
        for n, c in zip(names, contigs):
            f.write(b">" + n.encode() + b" x\n")
            for i in range(0, len(c), 61):
                f.write(c[i:i + 61] + b"\n")
    out = tmp_path / "guides.tsv"
    base = [sys.executable, "-m", "cropsr_amd.search", "-f", str(fa), "--pattern", SPCAS9_NAG, "--guide-pattern", SPCAS9, "--pam-length", "3",
            "--self", "-m", "3", "-o", str(out)]
    for opt, w in ((["--score", "hsu2013"], sref.W_HSU), ([], None)):
        r = subprocess.run(base + opt, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        sites, guides, counts, hit_sum = selfref.search_self(contigs, SPCAS9_NAG, 3, 3, SPCAS9, w)
        assert len(sites) > 100 and "guide sites" in r.stderr
        assert out.read_text() == selfref.format_rows(names, sites, guides, counts, hit_sum)


@pytest.mark.gpu
def test_gpu_medium_genome_sampled_rows(engine):
    """Tens of Mb, M = 3, scored: 2 048 seeded rows and the 64 rows with the largest counts against search(), exactly."""
    rng = np.random.default_rng(2025)
    first = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 10_000_000).tobytes()
    contigs = [first, _mutated_copy(rng, first[:4_000_000], 0.02), rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), 6_000_000).tobytes(),
               b"ACAGGTA" * 2000]
    g = engine.genome(contigs)
    try:
        res = g.search_self(SPCAS9, 3, 3, score="hsu2013")
        n = len(res.sites)
        assert n > 1_500_000
        pick = np.unique(np.concatenate([rng.choice(n, 2048, replace=False), np.argsort(res.counts.sum(axis=1), kind="stable")[-64:]]))
        queries = [srch.check_query(SPCAS9, res.guides[i].decode(), 3) for i in pick]
        want = g.search(SPCAS9, queries, 3, pam_len=3, score="hsu2013", sites=False)
        wc = want.counts.astype(np.int64)
        wc[:, 0] -= 1
        assert (res.counts[pick].astype(np.int64) == wc).all() and (res.hit_sum[pick] == want.hit_sum).all()
        assert int(wc.sum()) > 2000
    finally:
        g.close()
