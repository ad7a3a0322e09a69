"""--variants: cultivar variants under every target site (cropsr_amd/variants.py, csrc/crp_variants.cpp, csrc/crp_variants.hip).
The definition is restated twice in tests/variant_reference.py; the inputs come from tests/variant_cases.py, the genes of the
selection tests from tests/select_coding_cases.py, the selection's own definition from tests/select_reference.py,
tests/select_pairs_reference.py and tests/select_coding_reference.py (imported, not edited).

The variant limits under the plain, the pair and the coding kernel are checked here; under every kernel that includes
csrc/crp_select_predicate.inc -- the edit, splice, family and family step kernels and the spaced selection as well -- in
tests/test_select_predicate_matrix.py, whose docstring has the table of kernels and terms."""
import csv
import ctypes
import hashlib
import io
import json
import os
import re

import numpy as np
import pytest

from conftest import OracleBackend

import select_coding_cases
import select_coding_reference as cref
import select_pairs_reference as pref
import select_reference as sref
import variant_cases as cases
import variant_reference as ref
from cropsr_amd import _native as nat
from cropsr_amd import annotate, cli, coding, variants
from cropsr_amd import select as sel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


def _reference_columns(case):
    A = cases.arena(case)
    starts, ends1 = ref.track(A["intervals"])
    A["starts"], A["ends1"] = starts, ends1
    A["plus"] = ref.column_numpy(A["pos_plus"], False, case["l"], case["S"], starts, ends1)
    A["minus"] = ref.column_numpy(A["pos_minus"], True, case["l"], case["S"], starts, ends1)
    return A


def _raw_counts(pos, minus, l, S, intervals):
    s, e = np.array([iv[0] for iv in intervals], np.int64), np.array([iv[1] for iv in intervals], np.int64)
    return [int(((s <= b) & (e >= a)).sum()) for a, b in ref.windows(pos, minus, l, S)]


SMALL_CASES = [cases.sweep_cases()[1], cases.bucket_edges_case(), cases.bucket_fill_case()] + cases.extreme_cases()


@pytest.fixture(scope="module")
def small():
    return {c["name"]: (c, _reference_columns(c)) for c in SMALL_CASES}


@pytest.fixture(scope="module")
def random_case():
    c = cases.random_case()
    return c, _reference_columns(c)


# ---------------------------------------------------------------------------------------------- without a GPU: the definition
@pytest.mark.parametrize("name", [c["name"] for c in SMALL_CASES])
def test_rank_form_equals_the_touch_rule(small, name):
    case, A = small[name]
    for minus, key, col in ((False, "pos_plus", "plus"), (True, "pos_minus", "minus")):
        pos = A[key]
        pick = np.arange(pos.size)
        if len(A["intervals"]) > 1000:  # the filled bucket: the rows around it and every 9th of the others
            near = np.flatnonzero((pos.astype(np.int64) > 6144 + 200) & (pos.astype(np.int64) < 6144 + 1400))
            pick = np.unique(np.concatenate([near[::3], pick[::9]]))
        assert np.array_equal(ref.column_loop(pos[pick], minus, case["l"], case["S"], A["intervals"]), A[col][pick]), key


def _has_0_1_2(*runs):
    """every strand x window has rows with count 0, 1 and >= 2 (over the runs of one test)"""
    for strand in ("plus", "minus"):
        for k, v in enumerate(variants.unpack(np.concatenate([cols[strand] for cols in runs]))):
            for want, got in (("0", (v == 0).any()), ("1", (v == 1).any()), (">= 2", (v >= 2).any())):
                assert got, (strand, variants.HEADER[k], want)


def _kinds_matter(case, A):
    """insertions, deletions and SNPs each change at least one row"""
    for kind, test in (("snp", lambda s, e: e == s), ("insertion", lambda s, e: e == s - 1), ("deletion", lambda s, e: e > s)):
        rest = [(s, e) for s, e in A["intervals"] if not test(s, e)]
        assert len(rest) < len(A["intervals"]), kind
        st, en = ref.track(rest)
        changed = any(not np.array_equal(ref.column_numpy(A["pos_" + strand], strand == "minus", case["l"], case["S"], st, en), A[strand])
                      for strand in ("plus", "minus"))
        assert changed, kind


@pytest.mark.parametrize("name", ["sweep all"] + [c["name"] for c in SMALL_CASES if c["name"].startswith("ends")])
def test_the_small_cases_are_not_vacuous(small, name):
    case, A = small[name]
    # (the sweep's runs with one variant each give the rows with count 1, all its variants together the rows with more)
    _has_0_1_2(A, *([_reference_columns(c) for c in cases.sweep_cases()[0]] if name == "sweep all" else []))
    _kinds_matter(case, A)


def test_the_random_case_is_not_vacuous(random_case):
    case, A = random_case
    assert A["pos_plus"].size + A["pos_minus"].size > 200_000 and len(A["intervals"]) > 29_000
    _has_0_1_2(A)
    _kinds_matter(case, A)
    both = np.concatenate([A["plus"], A["minus"]])
    assert (both == 0).mean() <= 0.5
    spans = sum(1 for s, e in A["intervals"] if s >> 11 != (e + 1) >> 11)
    assert spans > 500  # intervals whose start and end lie in different buckets


def test_the_boundary_sweep_fires_rule_by_rule():
    singles, _ = cases.sweep_cases()
    i, j = cases.sweep_targets()
    assert abs(i - j) > 600 and len(singles) == 2 * (16 + 24 + 3)
    expect = {  # what -> (site, guide, seed, pam) of the target row
        "snp site a-1": (0, 0, 0, 0), "snp site a": {"+": (1, 1, 0, 0), "-": (1, 0, 0, 1)}, "snp site b": {"+": (1, 0, 0, 1), "-": (1, 1, 0, 0)},
        "snp site b+1": (0, 0, 0, 0), "snp guide a-1": {"+": (0, 0, 0, 0), "-": (1, 0, 0, 0)}, "snp guide b+1": {"+": (1, 0, 0, 0), "-": (0, 0, 0, 0)},
        "snp seed a": {"+": (1, 1, 1, 0), "-": (1, 1, 1, 0)}, "snp seed a-1": {"+": (1, 1, 0, 0), "-": (1, 0, 0, 0)},
        "snp seed b+1": {"+": (1, 0, 0, 0), "-": (1, 1, 0, 0)}, "snp pam a": (1, 0, 0, 1), "snp pam b": (1, 0, 0, 1),
        "snp pam a-1": {"+": (1, 0, 0, 0), "-": (0, 0, 0, 0)}, "snp pam b+1": {"+": (0, 0, 0, 0), "-": (1, 0, 0, 0)},
        "ins 0": (0, 0, 0, 0), "ins 23": (0, 0, 0, 0), "ins 1": {"+": (1, 1, 0, 0), "-": (1, 0, 0, 1)},
        # between the guide and the PAM's N ('+': junction i - 1 | i = a + 20; '-': junction j + 2 | j + 3 = a + 3): site only
        "ins 20": {"+": (1, 0, 0, 0), "-": (1, 1, 0, 0)}, "ins 3": {"+": (1, 1, 0, 0), "-": (1, 0, 0, 0)},
        "del N": (1, 0, 0, 0), "del over": (1, 1, 1, 1), "del into": {"+": (1, 1, 0, 0), "-": (1, 1, 1, 1)},
    }
    seen = set()
    for case in singles:
        A = cases.arena(case)
        minus = case["strand"] == "-"
        pos = (j if minus else i) + A["offsets"][0]
        got = tuple(_raw_counts(pos, minus, case["l"], case["S"], A["intervals"]))
        st, en = ref.track(A["intervals"])
        col = ref.column_numpy(np.array([pos]), minus, case["l"], case["S"], st, en)
        assert ref.pack(got) == int(col[0]), case["name"]
        want = expect.get(case["what"])
        if want is not None:
            want = want[case["strand"]] if isinstance(want, dict) else want
            assert got == want, (case["name"], got, want)
            seen.add(case["what"])
    assert seen == set(expect)


def test_saturation_rows_of_the_filled_bucket(small):
    case, A = small["bucket fill"]
    assert len(A["intervals"]) >= 5000
    b = np.array([s >> 11 for s, _ in A["intervals"]] + [(e + 1) >> 11 for _, e in A["intervals"]])
    assert (b == cases.FILL_BUCKET).all()  # one bucket holds all of it: both neighbours are empty
    for strand in ("plus", "minus"):
        bk = A["pos_" + strand] >> 11
        assert (bk == cases.FILL_BUCKET - 1).any() and (bk == cases.FILL_BUCKET + 1).any() and (bk == cases.FILL_BUCKET).any()
    h1, h2 = case["rows_255_256"]
    off = A["offsets"][0]
    assert _raw_counts(h1 + off, False, 20, 12, A["intervals"])[:3] == [255, 255, 255]
    assert _raw_counts(h2 + off, False, 20, 12, A["intervals"])[:3] == [256, 256, 256]
    r1, r2 = (int(np.flatnonzero(A["pos_plus"] == h + off)[0]) for h in (h1, h2))
    assert A["plus"][r1] & 0xFFFFFF == 0xFFFFFF and A["plus"][r2] & 0xFFFFFF == 0xFFFFFF
    raw = max(_raw_counts(int(p), False, 20, 12, A["intervals"])[0] for p in A["pos_plus"][(A["plus"] & 255) == 255][:40])
    assert raw > 400  # counts far above the saturation value


def test_bucket_edge_and_extreme_cases_hold_what_they_are_for(small):
    case, A = small["bucket edges"]
    assert {2047, 2048, 2049} <= set(A["pos_plus"].tolist()) and {4095, 4096, 4097} <= set(A["pos_minus"].tolist())
    assert any(s >> 11 != e >> 11 for s, e in A["intervals"]) and (2048, 2047) in A["intervals"]
    for p, strand in ((2047, "plus"), (2048, "plus"), (2049, "plus"), (4095, "minus"), (4096, "minus"), (4097, "minus")):
        assert A[strand][int(np.flatnonzero(A["pos_" + strand] == p)[0])] != 0
    for name in ("empty track", "all before the first hit", "all after the last hit"):
        c, X = small[name]
        assert not X["plus"].any() and not X["minus"].any() and X["pos_plus"].size and X["pos_minus"].size
        if name != "empty track":
            assert X["intervals"]
    c, X = small["all before the first hit"]
    assert max(e for _, e in X["intervals"]) < min(int(X["pos_plus"][0]) - 20, int(X["pos_minus"][0]))
    c, X = small["all after the last hit"]
    assert min(s for s, _ in X["intervals"]) > max(int(X["pos_plus"][-1]) + 2, int(X["pos_minus"][-1]) + 22)
    c, X = small["ends l=20 S=12"]
    n0, n1 = len(c["texts"][0]), len(c["texts"][1])
    j = X["offsets"][0] + n0 - 13  # the '-' row kept past the end of its contig: its guide runs 10 positions into the void
    r = int(np.flatnonzero(X["pos_minus"] == j)[0])
    assert j + 2 + 20 == X["offsets"][0] + n0 + 9 and variants.unpack(X["minus"][r:r + 1])[1][0] >= 2
    i = X["offsets"][1] + n1 - 3   # the '+' row on the last three letters of the last text: the arena's last text word
    assert int(X["pos_plus"][-1]) == i and (i + 2) >> 6 == (X["offsets"][1] + n1 - 1) >> 6 and X["plus"][-1] >> 24 >= 2


# ---------------------------------------------------------------------------------------------- without a GPU: the reader
VCF_HEAD = "##fileformat=VCFv4.2\n##contig=<ID=c1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\tS3\n"
VCF_BODY = [
    "c1\t100\t.\tA\tG\t50\tPASS\t.\tGT\t0/1\t0|0\t./.",
    "c1\t200\t.\tA\tC,T\t50\tPASS\t.\tGT:DP\t1/2:9\t0/0:3\t.",                 # multi-allelic SNP: one interval
    "c1\t300\t.\tAAAA\tAA,AAAAA,A\t50\tq10\t.\tGT\t0/1\t2|3\t0/0",               # a homopolymer: deletions of 2 and 3, an insertion
    "c1\t400\t.\tACGT\tAGGT,*,.\t50\t.\t.\tDP:GT\t4:0/1\t4:1|1\t4:.|2",           # an inner substitution; * and . skipped
    "c2\t10\t.\tN\t<DEL>,N[c1:5[,]c1:9]N,<INS:ME>\t50\tPASS\tSVTYPE=DEL\tGT\t1/2\t3/4\t0/0",
    "c2\t20\t.\tacgt\tAC\t50\tPASS\t.\tGT\t1/1\t0/0\t0/0",                        # lower case: compared without case
    "c2\t30\t.\tG\tG\t50\tPASS\t.\tGT\t1/1\t0/0\t0/0",                            # nothing left after stripping
    "c3\t5\t.\tTTGCA\tTTGCAGCA\t50\tLowQual\t.\tDP\t1\t2\t3",                     # no GT in FORMAT
    "c1\t999999999999\t.\tC\tCT\t50\tPASS\t.\tGT\t0/0\t0/0\t1",
]
READER_OPTIONS = [dict(), dict(pass_only=True), dict(samples=["S1"]), dict(samples=["S2", "S3"]), dict(samples=["S3"], pass_only=True)]


def _native_intervals(vs, chroms_want):
    """Per CHROM of the handle (starts, ends1) in coordinates: one text per CHROM at offset 0, dec = 1, first = 0."""
    assert list(vs.chrom_index) == list(chroms_want)
    out = {}
    for name in vs.chrom_index:
        s, e1 = vs.track([(name, 0, 0x7FFFFFF0, 0)], 1)
        out[name] = (s.tolist(), e1.tolist())
    return out


def _want_intervals(chroms):
    clip = lambda s, e: (s, min(e, 0x7FFFFFF0 - 1))
    out = {}
    for name, ivs in chroms.items():
        iv = sorted(set(clip(s, e) for s, e in ivs if s <= 0x7FFFFFF0))
        out[name] = (sorted(s for s, _ in iv), sorted(e + 1 for _, e in iv))
    return out


@pytest.mark.parametrize("options", READER_OPTIONS, ids=[repr(o) for o in READER_OPTIONS])
@pytest.mark.parametrize("ending", ["\n", "\r\n", "no-final-newline"])
def test_native_reader_equals_the_python_reader(options, ending):
    text = VCF_HEAD + "\n".join(VCF_BODY) + "\n"
    if ending == "\r\n":
        text = text.replace("\n", "\r\n")
    elif ending != "\n":
        text = text[:-1]
    data = text.encode()
    chroms, stats = ref.read_vcf(data, **options)
    vs = variants.VariantSet(source=data, **options)
    assert vs.stats == stats and _native_intervals(vs, chroms) == _want_intervals(chroms)
    if not options:
        assert chroms["c1"][:5] == [(100, 100), (200, 200), (301, 303), (302, 303), (304, 303)] and (401, 401) in chroms["c1"]
        assert chroms["c2"] == [(22, 23)] and stats["skipped_alt"] == 6 and stats["same_as_ref"] == 1 and chroms["c3"] == [(10, 9)]
    if options == dict(samples=["S1"]):
        assert chroms["c1"] == [(100, 100), (200, 200), (302, 303), (401, 401)] and "c3" not in chroms
    if options == dict(pass_only=True):
        assert (302, 303) not in chroms["c1"] and (401, 401) in chroms["c1"] and "c3" not in chroms and stats["filtered"] == 2


def test_native_reader_at_every_chunk_border():
    data = (VCF_HEAD + "\n".join(VCF_BODY)).replace("\n", "\r\n", 3).encode()
    chroms, stats = ref.read_vcf(data, samples=["S1", "S3"])
    want = _want_intervals(chroms)
    for cut in range(len(data) + 1):
        vs = variants.VariantSet(source=[data[:cut], data[cut:]], samples=["S1", "S3"])
        assert vs.stats == stats and _native_intervals(vs, chroms) == want, cut
        vs.close()
    vs = variants.VariantSet(source=[data[k:k + 1] for k in range(len(data))], samples=["S1", "S3"])
    assert vs.stats == stats and _native_intervals(vs, chroms) == want


def test_native_reader_reads_a_gz_file(tmp_path):
    import gzip
    data = (VCF_HEAD + "\n".join(VCF_BODY) + "\n").encode()
    with gzip.open(tmp_path / "v.vcf.gz", "wb") as f:
        f.write(data)
    (tmp_path / "v.vcf").write_bytes(data)
    a, b = variants.VariantSet(str(tmp_path / "v.vcf.gz")), variants.VariantSet(str(tmp_path / "v.vcf"), pass_only=False)
    assert a.stats == b.stats == ref.read_vcf(data)[1] and a.stats["alleles"] > 0


MALFORMED = [
    ("c1\t100\t.\tA", {}), ("c1\t1x0\t.\tA\tG", {}), ("c1\t0\t.\tA\tG", {}), ("c1\t\t.\tA\tG", {}), ("c1\t-5\t.\tA\tG", {}),
    ("c1\t1234567890123456\t.\tA\tG", {}), ("\t100\t.\tA\tG", {}), ("c1\t100\t.\tAX\tG", {}), ("c1\t100\t.\t\tG", {}), ("c1\t100\t.\tA\tG,", {}),
    ("c1\t100\t.\tA\tG,R", {}), ("c1\t100\t.\tA\tG*", {}), ("c1 100 . A G", {}), ("c1\t100\t.\tA\tG\t50", dict(pass_only=True)),
    ("c1\t100\t.\tA\tG\t50\tPASS\t.\tGT\t0/1", dict(samples=["S2"])), ("c1\t100\t.\tA\tG\t50\tPASS\t.\tGT\t0/x\t0\t0", dict(samples=["S1"])),
    ("c1\t100\t.\tA\tG\t50\tPASS\t.\tGT\t0/2\t0\t0", dict(samples=["S1"])), ("c1\t100\t.\tA\tG\t50\tPASS\t.\tGT\t0/\t0\t0", dict(samples=["S1"])),
    ("c1\t100\t.\tA\tG\t50\tPASS\t.", dict(samples=["S1"])),
]


@pytest.mark.parametrize("line,options", MALFORMED, ids=[repr(m[0])[:40] for m in MALFORMED])
def test_a_malformed_line_is_an_error_with_its_number(line, options):
    good = "c1\t50\t.\tA\tG\t50\tPASS\t.\tGT\t0/1\t0/1\t0/1"
    data = (VCF_HEAD + good + "\n" + line + "\n" + good + "\n").encode()
    with pytest.raises(ref.VcfError) as e:
        ref.read_vcf(data, **options)
    assert e.value.line_no == 5
    with pytest.raises(ValueError, match=r"line 5\b"):
        variants.VariantSet(source=data, **options)
    with pytest.raises(ValueError, match=r"line 5\b"):  # the same when the line is the last and lacks its line end
        variants.VariantSet(source=data[:data.index(line.encode()) + len(line.encode())], **options)


def test_unknown_samples_and_records_before_the_header_are_errors():
    data = (VCF_HEAD + VCF_BODY[0] + "\n").encode()
    with pytest.raises(ValueError, match="line 3.*S9"):
        variants.VariantSet(source=data, samples=["S1", "S9"])
    with pytest.raises(ref.VcfError):
        ref.read_vcf(data, samples=["S9"])
    with pytest.raises(ValueError, match="line 1"):
        variants.VariantSet(source=(VCF_BODY[0] + "\n").encode(), samples=["S1"])
    assert variants.VariantSet(source=(VCF_BODY[0] + "\n").encode()).stats["alleles"] == 1  # sites-only use needs no header
    assert variants.VariantSet(source=b"").stats["lines"] == 0


def test_layout_clips_dedups_and_shifts():
    rng = np.random.default_rng(4110)
    lines = []
    for name, n in (("a", 5000), ("b", 800)):
        for c in rng.integers(1, n + 40, 400).tolist():
            k = int(rng.integers(0, 4))
            ref_, alt = ("A", "C") if k == 0 else ("A", "AT") if k == 1 else ("A" * int(rng.integers(2, 60)), "A") if k == 2 else ("AC", "GT")
            lines.append("%s\t%d\t.\t%s\t%s" % (name, c, ref_, alt))
    lines += ["a\t1\t.\tAAAAA\tA", "a\t4990\t.\t" + "A" * 30 + "\tA", "zz\t7\t.\tA\tC"]
    data = ("\n".join(lines) + "\n").encode()
    chroms, _ = ref.read_vcf(data)
    vs = variants.VariantSet(source=data)
    # pieces of a cut contig (first != 0), a text without variants, the same contig twice in one arena (equal pairs count once
    # per arena only where they are equal IN ARENA POSITIONS), texts that end inside deletions
    layouts = [[("a", 0, 5000, 64), ("b", 0, 800, 5184)], [("a", 1000, 1500, 64), ("nobody", 0, 100, 1664), ("a", 2400, 2600, 1856)],
               [("b", 100, 1, 64), ("b", 0, 800, 192), ("b", 799, 1, 1088)], [("a", 4980, 20, 128)], []]
    for dec in (0, 1, 3):
        for entries in layouts:
            want = ref.layout(chroms, entries, dec)
            s, e1 = vs.track(entries, dec)
            ws, we = ref.track(want)
            assert np.array_equal(s, ws) and np.array_equal(e1, we), (dec, entries)
            assert all(e >= s_ - 1 for s_, e in want)
    full = ref.layout(chroms, layouts[0], 0)
    assert len(full) < sum(len(v) for k, v in chroms.items() if k != "zz") + 1 and len(full) > 700
    n = ctypes.c_uint64()
    e = np.array([[0, 0, 5000, 64]], np.uint64)
    L = nat.lib()
    assert L.crp_variants_track(vs._h, e.ctypes.data_as(nat.u64p), 1, 0, None, None, 0, ctypes.byref(n)) == nat.CRP_ERR_CAPACITY and n.value > 300
    small_s, small_e = np.zeros(5, np.uint32), np.zeros(5, np.uint32)
    assert L.crp_variants_track(vs._h, e.ctypes.data_as(nat.u64p), 1, 0, small_s.ctypes.data_as(nat.u32p), small_e.ctypes.data_as(nat.u32p), 5,
                                ctypes.byref(n)) == nat.CRP_ERR_CAPACITY and not small_s.any()
    bad = np.array([[0, 0, 5000, 64], [0, 0, 100, 64]], np.uint64)  # texts that overlap in the arena
    assert L.crp_variants_track(vs._h, bad.ctypes.data_as(nat.u64p), 2, 0, None, None, 0, ctypes.byref(n)) == nat.CRP_ERR_INVALID


def test_limits_and_packing():
    col = variants.pack([0, 3, 300, 7], [0, 2, 256, 7], [0, 1, 255, 0], [0, 0, 2, 7])
    assert col.tolist() == [0, 3 | 2 << 8 | 1 << 16, 0x02FFFFFF, 7 | 7 << 8 | 7 << 24] and col.dtype == np.uint32
    assert [v.tolist() for v in variants.unpack(col)] == [[0, 3, 255, 7], [0, 2, 255, 7], [0, 1, 255, 0], [0, 0, 2, 7]]
    assert variants.fields(col[1]) == (3, 2, 1, 0) and ref.pack((3, 2, 1, 0)) == int(col[1]) and ref.pack((300, 256, 255, 2)) == int(col[2])
    assert variants.Limits().passes(col).all() and variants.Limits(255, 255, 255, 255).astuple() == variants.Limits().astuple()
    assert variants.Limits(max_seed=0, max_pam=0).passes(col).tolist() == [True, False, False, False]
    assert variants.Limits(max_site=3).passes(col).tolist() == [True, True, False, False]
    assert variants.Limits(max_guide=2, max_pam=1).passes(col).tolist() == [True, True, False, False]
    assert variants.Limits(max_site=254).passes(col).tolist() == [True, True, False, True]
    with pytest.raises(ValueError):
        variants.Limits(max_seed=-1)
    assert variants.check_seed(None, 20) == 12 and variants.check_seed(None, 5) == 5 and variants.check_seed(20, 20) == 20
    for seed, l in ((0, 20), (21, 20), (1, 0), (1, 51)):
        with pytest.raises(ValueError):
            variants.check_seed(seed, l)
    with pytest.raises(ValueError, match="variants="):
        sel.Request(sel.Params(1), None, max_seed_variants=0)


def test_library_declares_the_abi():
    with open(os.path.join(ROOT, "include", "cropsr_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define CRP_ABI_VERSION 6\b", header) and nat.lib().crp_abi_version() == 6
    for name in ("crp_variants_create", "crp_variants_add_bytes", "crp_variants_finish", "crp_variants_destroy", "crp_variants_stats",
                 "crp_variants_track", "crp_variant_set_track", "crp_variant_counts", "crp_variant_counts_stats",
                 "crp_select_set_variant_limits"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in nat.SIGNATURES and getattr(nat.lib(), name)
    assert re.search(r"typedef struct crp_select_variant_limits \{\s*uint32_t max_site, max_guide, max_seed, max_pam;", header)
    assert ctypes.sizeof(nat.SelectVariantLimits) == 16


# ---------------------------------------------------------------------------------------------- the command line's refusals
@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    """tests/select_coding_cases.py's genome and genes as files, a seeded VCF over it, and the reference's columns per contig."""
    c = select_coding_cases.build(oracle)
    d = tmp_path_factory.mktemp("variants")
    c["gff_path"] = str(d / "genes.gff")
    with open(c["gff_path"], "w") as f:
        f.write(c["gff"])
    c["fasta_path"] = str(d / "genome.fa")
    with open(c["fasta_path"], "w") as f:  # one line per contig: read unformatted (dec = 0)
        f.write("".join(">%s\n%s\n" % (n, t.decode()) for n, t in zip(c["names"], c["contigs"]))[:-1])
    rng = np.random.default_rng(4111)
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tLINE1\tLINE2"]
    for name, t in zip(c["names"], c["contigs"]):
        for p in np.unique(rng.integers(1, len(t) - 30, len(t) // 45)).tolist():
            k = int(rng.integers(0, 5))
            r1 = chr(t[p - 1]).upper() if chr(t[p - 1]).upper() in "ACGT" else "N"
            ref_, alt = (r1, "ACGT"["ACGTN".index(r1) % 3 + 1 if r1 != "N" else 0]) if k < 3 else (r1, r1 + "GA") if k == 3 else \
                ("".join(ch if ch in "ACGTNacgtn" else "N" for ch in t[p - 1:p + int(rng.integers(1, 12))].decode()), r1)
            lines.append("%s\t%d\t.\t%s\t%s\t50\t%s\t.\tGT\t%s\t%s" % (name, p, ref_, alt, "PASS" if rng.random() < 0.8 else "q20",
                                                                    "0/1" if rng.random() < 0.7 else "0/0", "1|1" if rng.random() < 0.5 else "./."))
    c["vcf"] = ("\n".join(lines) + "\n").encode()
    c["vcf_path"] = str(d / "cultivar.vcf.gz")
    import gzip
    with gzip.open(c["vcf_path"], "wb") as f:
        f.write(c["vcf"])
    c["annotation"] = annotate.Annotation(c["gff_path"])
    c["genes"] = sref.gff_genes(c["gff"])
    c["models"] = cref.model_numpy(c["gff"])
    return c


REFUSALS = [
    (["--select-max-variants", "1"], "--select-max-variants", "belongs to --variants"),
    (["--select", "5", "--select-max-seed-variants", "0"], "--select-max-seed-variants", "belongs to --variants"),
    (["--select", "5", "--select-max-guide-variants", "0"], "--select-max-guide-variants", "belongs to --variants"),
    (["--select", "5", "--select-max-pam-variants", "0"], "--select-max-pam-variants", "belongs to --variants"),
    (["--variants-samples", "LINE1"], "--variants-samples", "belongs to --variants"),
    (["--variants-pass-only"], "--variants-pass-only", "belongs to --variants"),
    (["--variant-seed", "10"], "--variant-seed", "belongs to --variants"),
    (["--variants", "VCF"], "--variants", "belongs to --select"),
    (["--variants", "VCF", "-l", "0"], "--variants", "1..50"),
    (["--variants", "VCF", "-l", "51"], "--variants", "1..50"),
    (["--variants", "VCF", "--select", "5", "--variant-seed", "21"], "--variants", "1..20"),
    (["--variants", "VCF", "--select", "5", "--variant-seed", "0"], "--variants", "1..20"),
    (["--variants", "VCF", "-l", "10", "--variant-seed", "11"], "--variants", "1..10"),
    (["--variants", "VCF", "--select", "5", "--select-max-variants", "-1"], "--variants", "number of variants"),
    (["--variants", "VCF", "--select", "5", "--select-max-seed-variants", "x"], "--variants", "number of variants"),
    (["--variants", "VCF", "--select", "5", "--variants-samples", "A,,B"], "--variants", "sample names"),
    (["--variants", "VCF", "--select", "5", "--gpus", "2"], "--select", "one GPU"),  # (--variants belongs to --select, which refuses first)
    (["--variants", "VCF", "--select", "5", "--devices", "0,1"], "--select", "one GPU"),
    (["--variants", "no/such.vcf", "--select", "5"], "--variants", "no such file"),
]


class _NoScanBackend(OracleBackend):
    def scan(self, *a, **k):
        raise AssertionError("a refused command line reached the scan")


@pytest.mark.parametrize("extra,flag,text", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_cli_refusals_come_before_any_side_effect(case, oracle, tmp_path, monkeypatch, extra, flag, text):
    monkeypatch.chdir(tmp_path)
    extra = [case["vcf_path"] if x == "VCF" else x for x in extra]
    argv = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9", "-g", case["gff_path"]] + extra
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(argv), backend=_NoScanBackend(oracle), out=io.StringIO())
    assert flag in str(e.value.code) and text in str(e.value.code)
    assert os.listdir(tmp_path) == []


def test_cli_refuses_a_launchers_ranks_an_unknown_sample_and_a_malformed_vcf(case, oracle, tmp_path, monkeypatch):
    class Group:
        world, rank, local_rank = 2, 0, 0
    monkeypatch.chdir(tmp_path)
    base = ["-f", case["fasta_path"], "-o", str(tmp_path / "out.csv"), "--cas9", "-g", case["gff_path"], "--select", "5"]
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(base + ["--variants", case["vcf_path"]]), backend=_NoScanBackend(oracle), out=io.StringIO(), group=Group())
    assert "2 ranks" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(base + ["--variants", case["vcf_path"], "--variants-samples", "LINE9"]),
                backend=_NoScanBackend(oracle), out=io.StringIO())
    assert "--variants" in str(e.value.code) and "LINE9" in str(e.value.code)
    bad = tmp_path.parent / (tmp_path.name + "_bad.vcf")
    bad.write_bytes(case["vcf"] + b"c0\t12\t.\tA\tQ\n")
    with pytest.raises(SystemExit) as e:
        cli.run(cli.build_parser().parse_args(base + ["--variants", str(bad)]), backend=_NoScanBackend(oracle), out=io.StringIO())
    assert "--variants" in str(e.value.code) and "line %d" % (case["vcf"].count(b"\n") + 1) in str(e.value.code)
    assert os.listdir(tmp_path) == []


# ---------------------------------------------------------------------------------------------- on the GPU: the column
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def _device_column(arena, case, A):
    """Scan at the case's l, set the case's track, count: the device's tables must be the reference's rows."""
    n_plus, n_minus = arena.scan_score_device(case["l"])
    cols = arena.fetch(n_plus, n_minus)
    assert [int(o) for o in arena.offsets] == A["offsets"]
    assert np.array_equal(cols[0], A["pos_plus"]) and np.array_equal(cols[3], A["pos_minus"])
    arena.variant_set_track(A["starts"], A["ends1"])
    return arena.variant_counts(n_plus, n_minus, case["S"]), (n_plus, n_minus)


def _assert_columns(got, A, what):
    for g, strand in zip(got, ("plus", "minus")):
        bad = np.flatnonzero(g != A[strand])
        assert bad.size == 0, (what, strand, bad[:5], g[bad[:5]], A[strand][bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in SMALL_CASES])
def test_gpu_columns_equal_the_reference(engine, small, name):
    case, A = small[name]
    arena = engine.arena(case["texts"])
    try:
        got, (n_plus, n_minus) = _device_column(arena, case, A)
        _assert_columns(got, A, name)
        st = arena.variant_counts_stats()
        assert st == dict(kernel_ms=st["kernel_ms"], rows=n_plus + n_minus, guide_len=case["l"], seed=case["S"], variants=len(A["intervals"]))
        assert st["kernel_ms"] > 0
    finally:
        arena.close()


@pytest.mark.gpu
def test_gpu_boundary_sweep_one_variant_a_run(engine):
    singles, _ = cases.sweep_cases()
    arena = engine.arena(singles[0]["texts"])
    try:
        n_plus, n_minus = arena.scan_score_device(cases.SWEEP_L)
        cols = arena.fetch(n_plus, n_minus)
        touched = 0
        for case in singles:
            A = cases.arena(case)
            starts, ends1 = ref.track(A["intervals"])
            assert np.array_equal(cols[0], A["pos_plus"]) and np.array_equal(cols[3], A["pos_minus"])
            arena.variant_set_track(starts, ends1)
            gp, gm = arena.variant_counts(n_plus, n_minus, case["S"])
            assert np.array_equal(gp, ref.column_numpy(A["pos_plus"], False, case["l"], case["S"], starts, ends1)), case["name"]
            assert np.array_equal(gm, ref.column_numpy(A["pos_minus"], True, case["l"], case["S"], starts, ends1)), case["name"]
            touched += int(gp.any() or gm.any())
        assert touched >= len(singles) - 4
    finally:
        arena.close()


@pytest.mark.gpu
def test_gpu_random_case_every_row(engine, random_case):
    case, A = random_case
    g = engine.genome(case["texts"])
    try:
        assert len(g.arenas) == 1
        got, _ = _device_column(g.arenas[0], case, A)
        _assert_columns(got, A, "random")
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_arenas", [1, 3], ids=["one-arena", "three-arenas"])
@pytest.mark.parametrize("dec", [0, 1], ids=["plain", "decorated"])
def test_gpu_several_contigs_and_arenas_through_a_vcf(engine, dec, n_arenas):
    c = cases.vcf_case(dec)
    chroms, stats = ref.read_vcf(c["vcf"])
    for name, seq in zip(c["names"], c["seqs"]):  # the records speak of the genome's own letters: REF at POS is the text's
        for line in c["vcf"].decode().split("\n"):
            col = line.split("\t")
            if col[0] == name:
                p, r = int(col[1]), col[3]
                text = c["texts"][c["names"].index(name)]
                assert text[p + dec - 1:p + dec - 1 + len(r)].decode() == r[:max(0, len(seq) - p + 1)] + ("')," if dec else "")[:max(0, p + len(r) - 1 - len(seq))]
    vs = variants.VariantSet(source=c["vcf"])
    assert "nowhere" in vs.chrom_index and vs.stats == stats
    g = engine.genome(c["texts"], max_words=None if n_arenas == 1 else 130)
    try:
        assert len(g.arenas) == n_arenas
        hits = g.scan_score(c["l"])
        counts = [(h.n_plus, h.n_minus) for h in hits.per_arena]
        request = variants.Request(vs, c["names"], dec)
        got = g.variant_counts(request, counts)
        assert g.variant_stats["rows"] == hits.n_plus + hits.n_minus and g.variant_stats["seed"] == 12 and g.variant_stats["kernel_ms"] > 0
        total = 0
        for a, (arena, group) in enumerate(zip(g.arenas, g.groups)):
            entries = [(c["names"][k], 0, int(arena.lengths[j]), int(arena.offsets[j])) for j, k in enumerate(group)]
            starts, ends1 = ref.track(ref.layout(chroms, entries, dec))
            h = hits.per_arena[a]
            assert np.array_equal(got[a][0], ref.column_numpy(h.pos_plus, False, c["l"], c["S"], starts, ends1)), a
            assert np.array_equal(got[a][1], ref.column_numpy(h.pos_minus, True, c["l"], c["S"], starts, ends1)), a
            total += int(np.count_nonzero(got[a][0]) + np.count_nonzero(got[a][1]))
        assert total > 300 and g.variant_stats["variants"] > 200
        assert g.variant_counts(request, counts, seed=20, fetch=False) is None and g.variant_stats["seed"] == 20
    finally:
        g.close()
        vs.close()


@pytest.mark.gpu
def test_gpu_calls_out_of_order(engine):
    L = nat.lib()
    text = cases.sweep_text()
    arena = engine.arena([text])
    try:
        def status(fn):
            with pytest.raises(nat.CropsrHipError) as e:
                fn()
            return e.value.status, str(e.value)

        starts, ends1 = np.array([100, 200, 300], np.uint32), np.array([101, 250, 330], np.uint32)  # (100, 100), (200, 249), (300, 329)
        st, msg = status(lambda: arena.variant_counts(0, 0, 12))
        assert st == nat.CRP_ERR_STATE and "no hit tables" in msg
        assert status(arena.variant_counts_stats)[0] == nat.CRP_ERR_STATE
        n_plus, n_minus = arena.scan_score_device(0)
        st, msg = status(lambda: arena.variant_counts(n_plus, n_minus, 1))
        assert st == nat.CRP_ERR_INVALID and "guide length 0" in msg
        n_plus, n_minus = arena.scan_score_device(20)
        for S in (0, 21, -1):
            st, msg = status(lambda: arena.variant_counts(n_plus, n_minus, S))
            assert st == nat.CRP_ERR_INVALID and "1..20" in msg
        st, msg = status(lambda: arena.variant_counts(n_plus, n_minus, 12))
        assert st == nat.CRP_ERR_STATE and "crp_variant_set_track" in msg  # no track
        for bad_s, bad_e in (([5, 4], [6, 7]), ([4, 5], [7, 6]), ([4, 0x80000000], [5, 6]), ([4, 5], [5, 0x80000000])):
            st, msg = status(lambda: arena.variant_set_track(np.array(bad_s, np.uint32), np.array(bad_e, np.uint32)))
            assert st == nat.CRP_ERR_INVALID and "ascending" in msg
        assert L.crp_variant_set_track(None, None, None, 0) == nat.CRP_ERR_INVALID and L.crp_variant_counts(None, 12, None, None) == nat.CRP_ERR_INVALID
        with pytest.raises(ValueError):
            arena.variant_set_track(starts, ends1[:2])
        arena.variant_set_track(starts, ends1)
        h = sel.ArenaSelect(arena, [0, 1000], [900, 3900])
        try:
            limits = variants.Limits(max_seed=0, max_pam=0)
            h.set_variant_limits(limits)
            st, msg = status(lambda: h.run(sel.Params(5)))
            assert st == nat.CRP_ERR_STATE and "crp_variant_counts" in msg  # limits without a column
            assert arena.variant_counts(n_plus, n_minus, 12, fetch=False) is None  # NULL pointers: the column stays on the device
            vp, vm = arena.variant_counts(n_plus, n_minus, 12)
            cols = arena.fetch(n_plus, n_minus)
            assert np.array_equal(vp, ref.column_numpy(cols[0], False, 20, 12, starts, ends1)) and vp.any()
            assert np.array_equal(vm, ref.column_numpy(cols[3], True, 20, 12, starts, ends1)) and vm.any()
            h.run(sel.Params(5))
            assert h.stats()["bytes_per_row"] == 16
            arena.variant_set_track(np.empty(0, np.uint32), np.empty(0, np.uint32))  # n = 0: a valid track; a new track drops the column
            st, msg = status(lambda: h.run(sel.Params(5)))
            assert st == nat.CRP_ERR_STATE and "crp_variant_counts" in msg
            zp, zm = arena.variant_counts(n_plus, n_minus, 12)
            assert not zp.any() and not zm.any() and zp.size == n_plus and arena.variant_counts_stats()["variants"] == 0
            arena.scan_score_device(20)  # the next scan drops the column
            assert status(arena.variant_counts_stats)[0] == nat.CRP_ERR_STATE
            st, msg = status(lambda: h.run(sel.Params(5)))
            assert st == nat.CRP_ERR_STATE and "crp_variant_counts" in msg
            h.set_variant_limits(None)  # cleared: the plain selection again
            h.run(sel.Params(5))
            assert h.stats()["bytes_per_row"] == 12
        finally:  # (the handle goes before its arena and its context, whatever failed)
            h.close()
    finally:
        arena.close()


# ---------------------------------------------------------------------------------------------- on the GPU: the selection
def _arena_tables(hits, offsets):
    cat = lambda key, dt, add: np.concatenate([h[key].astype(dt) + (dt(o) if add else dt(0)) for h, o in zip(hits, offsets)])
    return dict(pos_plus=cat("pos_plus", np.uint32, True), score_plus=cat("score_plus", np.float64, False),
                pos_minus=cat("pos_minus", np.uint32, True), score_minus=cat("score_minus", np.float64, False))


@pytest.fixture(scope="module", params=[1, 3], ids=["one-arena", "three-arenas"])
def scanned(request, engine, case):
    """The case genome with tables and variant column resident, and per arena the reference's view of the same."""
    g = engine.genome(case["contigs"], max_words=None if request.param == 1 else 600)
    assert len(g.arenas) == request.param
    areq = annotate.Request(case["annotation"], case["names"], 0)
    vs = variants.VariantSet(case["vcf_path"], samples=["LINE1"])
    chroms, _ = ref.read_vcf(case["vcf"], samples=["LINE1"])
    try:
        hits = g.scan_score(20)
        dev = g.variant_counts(variants.Request(vs, case["names"], 0), [(h.n_plus, h.n_minus) for h in hits.per_arena])
        arenas = []
        for a, (arena, group) in enumerate(zip(g.arenas, g.groups)):
            tables = _arena_tables([case["hits"][k] for k in group], [int(o) for o in arena.offsets])
            for key in tables:
                assert np.array_equal(tables[key].view(np.uint8), getattr(hits.per_arena[a], key).view(np.uint8)), key
            entries = [(case["names"][k], 0, int(arena.lengths[j]), int(arena.offsets[j])) for j, k in enumerate(group)]
            starts, ends1 = ref.track(ref.layout(chroms, entries, 0))
            col = dict(plus=ref.column_numpy(tables["pos_plus"], False, 20, 12, starts, ends1),
                       minus=ref.column_numpy(tables["pos_minus"], True, 20, 12, starts, ends1))
            assert np.array_equal(dev[a][0], col["plus"]) and np.array_equal(dev[a][1], col["minus"])
            lo, hi, gene = sref.layout(case["genes"], entries, 0)
            arenas.append(dict(tables=tables, col=col, lo=lo, hi=hi, gene=gene, rows=cref.layout_rows(case["gff"], entries, 0),
                               model=areq.coding_layout(sel.arena_layout(g, a))))
    except BaseException:  # (nothing of this genome may outlive the engine)
        vs.close()
        g.close()
        raise
    yield dict(genome=g, request=areq, arenas=arenas, models=case["models"])
    vs.close()
    g.close()


LIMIT_SETS = [dict(max_site=0), dict(max_guide=0), dict(max_seed=0), dict(max_pam=0), dict(max_site=2, max_guide=1, max_seed=0, max_pam=0),
              dict(max_site=255, max_guide=255, max_seed=255, max_pam=255)]


def _also(A, limits):
    return {s: variants.Limits(**limits).passes(A["col"][s]) for s in ("plus", "minus")}


def _as_cds(also):
    """The numpy selection reference takes no extra mask: the rows that pass the limits, stated as its CDS filter -- id 1 where
    the row passes, 0 where not, and flags that keep id 1."""
    return dict(feat_plus=also["plus"].astype(np.uint32), feat_minus=also["minus"].astype(np.uint32), flags=np.array([0, 1], np.uint8))


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("n_in", "n_pass", "sel")):
        assert np.array_equal(np.asarray(g, np.uint32), np.asarray(w, np.uint32)), (what, name)


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])
@pytest.mark.parametrize("limits", LIMIT_SETS, ids=[",".join("%s=%d" % kv for kv in l.items()) for l in LIMIT_SETS])
def test_gpu_selection_honours_the_limits(scanned, limits, slice_rows):
    dropped = 0
    for a, A in enumerate(scanned["arenas"]):
        h = sel.ArenaSelect(scanned["genome"].arenas[a], A["lo"], A["hi"])
        try:
            if slice_rows:
                h.set_limits(slice_rows)
            h.set_variant_limits(variants.Limits(**limits))
            h.run(sel.Params(5, 0.1))
            got = h.fetch()
            assert h.stats()["bytes_per_row"] == 16
        finally:
            h.close()
        _same(got, sref.select_numpy(A["tables"], A["lo"], A["hi"], 5, 0.1, None, _as_cds(_also(A, limits))), "arena %d" % a)
        plain = sref.select_numpy(A["tables"], A["lo"], A["hi"], 5, 0.1)
        if min(limits.values()) == 255:  # limits of 255 select exactly what no limits select
            _same(got, plain, "limits of 255")
        dropped += int(plain[1].sum()) - int(np.asarray(got[1]).sum())
    assert dropped > 0 or min(limits.values()) == 255


@pytest.mark.gpu
def test_gpu_pairs_honour_the_limits(scanned):
    limits = dict(max_seed=0, max_pam=0)
    fewer = 0
    for a, A in enumerate(scanned["arenas"]):
        h = sel.ArenaSelect(scanned["genome"].arenas[a], A["lo"], A["hi"])
        try:
            h.set_variant_limits(variants.Limits(**limits))
            h.run_pairs(sel.Params(1, 0.1), sel.PairParams(5, 50, 500))
            got = h.fetch_pairs()
            h.set_variant_limits(variants.Limits(255, 255, 255, 255))
            h.run_pairs(sel.Params(1, 0.1), sel.PairParams(5, 50, 500))
            loose = h.fetch_pairs()
        finally:
            h.close()
        want = pref.pairs_numpy(A["tables"], A["lo"], A["hi"], 5, 50, 500, min_score=0.1, also=_also(A, limits))
        plain = pref.pairs_numpy(A["tables"], A["lo"], A["hi"], 5, 50, 500, min_score=0.1)
        for g, w, p, name in zip(got, want, loose, ("n_pass", "n_pairs", "pairs")):
            assert np.array_equal(np.asarray(g).reshape(-1), np.asarray(w).reshape(-1).astype(np.asarray(g).dtype)), (a, name)
            assert np.array_equal(np.asarray(p).reshape(-1), np.asarray(plain[("n_pass", "n_pairs", "pairs").index(name)]).reshape(-1)), (a, name)
        fewer += int(plain[1].sum()) - int(want[1].sum())
    assert fewer > 0


@pytest.mark.gpu
def test_gpu_coding_selection_honours_the_limits(scanned):
    limits, coding_limits = dict(max_guide=0, max_pam=0), (5, 80, 0)
    dropped = 0
    for a, A in enumerate(scanned["arenas"]):
        h = sel.ArenaSelect(scanned["genome"].arenas[a], A["lo"], A["hi"])
        try:
            h.set_variant_limits(variants.Limits(**limits))
            h.set_coding(A["model"])
            h.set_coding_limits(coding.Limits(*coding_limits))
            h.run(sel.Params(5, 0.1))
            got = h.fetch()
        finally:
            h.close()
        score = np.concatenate([A["tables"]["score_plus"], A["tables"]["score_minus"]])
        also = _also(A, limits)
        ok = (score >= np.float64(0.1)) & np.concatenate([also["plus"], also["minus"]])
        positions = cref.positions_numpy(A["tables"], scanned["models"], A["rows"])
        _same(got, cref.select_numpy(A["tables"], A["lo"], A["hi"], scanned["models"], A["rows"], 5, coding_limits, ok, positions=positions), a)
        plain = cref.select_numpy(A["tables"], A["lo"], A["hi"], scanned["models"], A["rows"], 5, coding_limits, score >= np.float64(0.1),
                                  positions=positions)
        dropped += int(plain[1].sum()) - int(np.asarray(got[1]).sum())
    assert dropped > 0


def _run(case, tmp_path, monkeypatch, extra, name):
    monkeypatch.chdir(tmp_path)
    out_csv = str(tmp_path / name)
    argv = ["-f", case["fasta_path"], "-g", case["gff_path"], "-o", out_csv, "--cas9", "--seed", "11", "--each-contig-once"] + list(extra)
    cli.run(cli.build_parser().parse_args(argv), backend=None, out=io.StringIO())
    return out_csv


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


@pytest.mark.gpu
def test_gpu_command_line_end_to_end(case, tmp_path, monkeypatch):
    flags = ["--select", "5", "--variants", case["vcf_path"], "--variants-samples", "LINE1"]
    plain = _run(case, tmp_path, monkeypatch, ["--select", "5"], "plain.csv")
    loose = _run(case, tmp_path, monkeypatch, flags + ["--select-max-variants", "255", "--select-max-guide-variants", "255",
                                                      "--select-max-seed-variants", "255", "--select-max-pam-variants", "255"], "loose.csv")
    clean = _run(case, tmp_path, monkeypatch, flags + ["--select-max-seed-variants", "0", "--select-max-pam-variants", "0", "--bench-json",
                                                      str(tmp_path / "bench.json")], "clean.csv")
    md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest()
    assert md5(plain) == md5(loose) == md5(clean)  # the main table has no column
    P, Lo, C = (_read(p + ".selected.csv") for p in (plain, loose, clean))
    assert Lo[0] == P[0] + variants.HEADER and C[0] == Lo[0] and [r[:-4] for r in Lo[1:]] == P[1:]  # limits of 255: the same selection
    chroms, _ = ref.read_vcf(case["vcf"], samples=["LINE1"])
    at = {n: P[0].index(n) for n in ("chromosome", "end_pos", "strand")}
    n_var = 0
    for rows_, must_be_clean in ((Lo[1:], False), (C[1:], True)):
        assert rows_
        for r in rows_:
            k = case["names"].index(r[at["chromosome"]])
            minus = r[at["strand"]] == "-"
            pos = int(r[at["end_pos"]]) - (3 if minus else 0)
            ivs = ref.layout(chroms, [(case["names"][k], 0, len(case["contigs"][k]), 0)], 0)
            want = _raw_counts(pos, minus, 20, 12, ivs) if ivs else [0, 0, 0, 0]
            assert [int(x) for x in r[-4:]] == [min(w, 255) for w in want], r
            n_var += want[0] > 0
            if must_be_clean:
                assert r[-2] == "0" and r[-1] == "0"
    assert n_var > 0 and len(C) <= len(Lo) and C[1:] != Lo[1:]
    with open(tmp_path / "bench.json") as f:
        stage = json.load(f)["variants"]
    assert stage["kernel_ms"] > 0 and stage["rows"] == sum(h["pos_plus"].size + h["pos_minus"].size for h in case["hits"])
    assert stage["parse_s"] > 0 and stage["variants"] > 0 and stage["alleles"] >= stage["variants"]
