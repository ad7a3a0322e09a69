"""On-target models for any nuclease (cropsr_amd/ontarget.py, csrc/crp_ontarget.hip, the model form of
csrc/crp_select_self.hip).

Without a GPU: the two statements of the reference against each other, the parser and every refusal, the key transform, the
built-in model against the golden weights and the golden 30-mer scores, the scan's rows against the model on the CPU oracle,
every command-line refusal, and the unchanged TSV without a model.  On the GPU: the device's sums against the numpy statement
bit for bit, the window edges, the scan as an independent check, the ranked selection against the extended statement of
section 28, and the command line end to end.  Every case first proves on the reference what it claims to exercise."""
import math

import numpy as np
import pytest

import ontarget_cases as oc
import ontarget_reference as oref
import select_self_cases as cases
import select_self_reference as ref
from cropsr_amd import ontarget
from cropsr_amd import search as srch
from cropsr_amd import select as sel_mod
from cropsr_amd import select_self as ss

NONE = ref.NONE
RS1_GEOMETRY = (23, 3, True)


def geometry_of(pid):
    pattern, _, P, pam3, _ = cases.PATTERNS[pid]
    return len(pattern), P, pam3


# ---------------------------------------------------------------- without a GPU

@pytest.mark.parametrize("mid", sorted(oc.MODEL_CASES))
def test_reference_statements_agree(mid):
    pid, W, left, gc = oc.MODEL_CASES[mid]
    geo = geometry_of(pid)
    T, P, _ = geo
    model = oref.as_dict(oc.random_model(1, W, left, T - P, gc), T - P)
    rng = np.random.default_rng([5, W, left])
    p = np.array([30.0] * 4 + [6.0] * 4 + [1.0] * 6)
    text = bytearray(rng.choice(np.frombuffer(b"ACGTacgtNnRU-\0", np.uint8), 3000, p=p / p.sum()).tobytes())
    text[1000:1400] = rng.choice(np.frombuffer(b"ACGT", np.uint8), 400).tobytes()  # a clean stretch: sums exist
    pos = np.concatenate([rng.integers(-80, 3080, 600), np.arange(990, 1410)])
    strand = rng.integers(0, 2, pos.size)
    a, b = oref.sums_loop(model, geo, bytes(text), pos, strand), oref.sums_numpy(model, geo, bytes(text), pos, strand)
    assert np.array_equal(oref.bits(a), oref.bits(b))
    assert np.isnan(a).sum() > 30 and (~np.isnan(a)).sum() > 100
    assert (oref.bits(a[np.isnan(a)]) == oref.NAN_BITS).all()
    # the package's own host statement, over letter codes
    ok = ~np.isnan(a)
    codes = np.array([[oref._letter_code(bytes(text), f, st) for f in oref.window_forward(model, geo, int(s), int(st))]
                      for s, st in zip(pos[ok], strand[ok])], np.uint8)
    glo, G = oref.region(geo)
    gcs = [sum((oref._letter_code(bytes(text), (s + T - 1 - p) if st else s + p, st) or 0) >= 2 for p in range(glo, glo + G))
           for s, st in zip(pos[ok], strand[ok])]
    m = oc.random_model(1, W, left, T - P, gc)
    assert np.array_equal(oref.bits(ontarget.sums_of_codes(m, codes, np.array(gcs))), oref.bits(a[ok]))


def test_reference_by_hand():
    """W = 3, left = 1 on a 4-letter pattern with a 2-letter PAM on the 3' side: text ACGTA, '+' site at 1 (CGTA), '-' site at 0."""
    single = np.zeros((3, 4))
    pair = np.zeros((2, 16))
    single[0, 0], single[1, 2], single[2, 3] = 1.0, 2.0, 4.0      # A at 0, C at 1, G at 2
    pair[0, 0 * 4 + 2], pair[1, 2 * 4 + 3] = 8.0, 16.0            # AC at 0, CG at 1
    model = dict(W=3, left=1, intercept=0.5, single=single, pair=pair, gc=np.array([0.0, 32.0, 64.0]))
    geo = (4, 2, True)
    # '+' at 1: window = forward 0, 1, 2 = A C G; guide region = pattern 0, 1 = C G: GC 2
    assert oref.sum_loop(model, geo, b"ACGTA", 1, 0) == 0.5 + 64.0 + 1 + 2 + 4 + 8 + 16
    # '-' at 0 (forward ACGT, oriented ACGT): window = forward 4, 3, 2 complemented = T A C; region = A C: GC 1
    single[0, 1], single[1, 0], single[2, 2] = 0.25, 0.125, 0.0625
    assert oref.sum_loop(model, geo, b"ACGTA", 0, 1) == 0.5 + 32.0 + 0.25 + 0.125 + 0.0625
    assert oref.sum_loop(model, geo, b"ACGTA", 2, 0) == 0.5 + 32.0  # (window C G T inside the text; no term of it is set)
    for s, st in ((0, 0), (4, 0), (1, 1)):  # a window position before the text / behind it
        assert math.isnan(oref.sum_loop(model, geo, b"ACGTA", s, st))
    assert math.isnan(oref.sum_loop(model, geo, b"ANGTA", 1, 0)) and oref.sum_loop(model, geo, b"acgta", 1, 0) == 95.5
    assert oref.sum_loop(model, geo, b"UCGTA", 1, 0) == 95.5  # U is A's code
    got = oref.sums_numpy(model, geo, b"ACGTA", [1, 0, 0], [0, 1, 0])
    assert got[0] == 95.5 and got[1] == 32.9375 and math.isnan(got[2])


MODEL_TEXT = """# a model
window 4
left 1   # one letter before the site
link logistic
intercept -0.25
single 0 A 0.5
single 3 g -1e-3
pair 2 CG 2
gc 0 1.5
gc 2 -3
"""


def test_parser():
    m = ontarget.parse_model(MODEL_TEXT, guide_letters=2)
    assert (m.window, m.left, m.link, m.intercept) == (4, 1, "logistic", -0.25)
    assert m.single[0, 0] == 0.5 and m.single[3, 3] == -1e-3 and m.pair[2, 2 * 4 + 3] == 2.0 and m.gc.tolist() == [1.5, 0.0, -3.0]
    assert np.count_nonzero(m.single) == 2 and np.count_nonzero(m.pair) == 1
    assert ontarget.parse_model(MODEL_TEXT.encode()).gc.tolist() == [1.5, 0.0, -3.0]
    # round trips: every term of a random model survives its text, bit for bit
    for W, left, gc in ((30, 5, True), (64, 20, False), (1, 0, True)):
        a = oc.random_model(3, W, left, 20, gc, "logistic")
        b = ontarget.parse_model(ontarget.format_model(a), 20)
        assert (b.window, b.left, b.link) == (W, left, "logistic") and b.intercept == a.intercept
        assert np.array_equal(a.single, b.single) and np.array_equal(a.pair, b.pair)
        assert (a.gc is None and b.gc is None) or np.array_equal(a.gc, b.gc)
    assert ontarget.parse_model("window 2\n").link == "identity"


BAD_MODELS = [
    ("window 4\nweight 0 A 1\n", "line 2: unknown statement"),
    ("window 4\nsingle 0 A\n", "line 2: unknown statement"),
    ("window 4\nsingle 4 A 1\n", "line 2: POS 4 is outside 0..3"),
    ("window 4\nsingle -1 A 1\n", "line 2: POS -1 is outside"),
    ("window 4\npair 3 AC 1\n", "line 2: POS 3 is outside 0..2"),
    ("single 9 A 1\nwindow 4\n", "line 1: POS 9 is outside 0..3"),
    ("window 4\nsingle 0 N 1\n", "line 2: 'N' is not 1 of the letters"),
    ("window 4\npair 0 AU 1\n", "line 2: 'AU' is not 2 of the letters"),
    ("window 4\npair 0 A 1\n", "line 2: 'A' is not 2 of the letters"),
    ("window 4\nsingle 0 A 1\n\nsingle 0 a 2\n", "line 4: single 0 A is given twice"),
    ("window 4\npair 1 AC 1\npair 1 AC 1\n", "line 3: pair 1 AC is given twice"),
    ("window 4\ngc 1 1\ngc 1 2\n", "line 3: gc 1 is given twice"),
    ("window 4\nintercept 1\nintercept 1\n", "line 3: `intercept` is given twice"),
    ("window 4\ngc 3 1\n", "line 2: COUNT 3 is outside 0..2"),
    ("window 4\nsingle 0 A nan\n", "line 2: 'nan' is not a finite number"),
    ("window 4\nintercept inf\n", "line 2: 'inf' is not a finite number"),
    ("window 4\nsingle 0 A x\n", "line 2: 'x' is not a number"),
    ("window 65\n", "line 1: the window is 1..64"),
    ("window 0\n", "line 1: the window is 1..64"),
    ("window 4\nleft 4\n", "line 2: left must be 0..3"),
    ("window 4\nlink probit\n", "line 2: the link is identity or logistic"),
    ("left 1\n", "no `window` statement"),
]


@pytest.mark.parametrize("text, want", BAD_MODELS, ids=[str(k) for k in range(len(BAD_MODELS))])
def test_parser_refusals(text, want):
    with pytest.raises(ValueError) as e:
        ontarget.parse_model(text, guide_letters=2)
    assert want in str(e.value) and "\n" not in str(e.value)


def test_model_refusals():
    for kw in (dict(window=0, left=0), dict(window=65, left=0), dict(window=4, left=4), dict(window=4, left=-1), dict(window=4, left=0, link="x"),
               dict(window=4, left=0, intercept=float("inf")), dict(window=2, left=0, single=[[0, 0, 0, float("nan")]] * 2)):
        with pytest.raises(ValueError):
            ontarget.Model(**kw)
    m = ontarget.Model(4, 0, gc=[0.0] * 22)
    m.check_geometry(24, 3, True)
    with pytest.raises(ValueError, match="above the guide region"):
        m.check_geometry(23, 3, True)
    rs1 = ontarget.rs1()
    rs1.check_geometry(23, 3, True)
    for geo in ((23, 3, False), (24, 3, True), (23, 2, True), (27, 4, False)):
        with pytest.raises(ValueError, match="rs1 is valid for"):
            rs1.check_geometry(*geo)


def test_value_and_threshold():
    s = np.array([0.0, -0.0, 1.5, -700.0, 800.0, -800.0, float("nan")])
    v = ontarget.value(s, "logistic")
    assert v[0] == 0.5 == v[1] and v[4] == 1.0 and v[5] == 0.0 and math.isnan(v[6]) and 0 < v[3] < 1e-300
    assert v[2] == 1.0 / (1.0 + math.exp(-1.5))
    ident = ontarget.value(s, "identity")
    assert np.array_equal(oref.bits(ident), oref.bits(s))
    assert ontarget.min_sum(0.25, "identity") == 0.25 and ontarget.min_sum(-3, "identity") == -3.0
    assert ontarget.min_sum(0.5, "logistic") == 0.0 and ontarget.min_sum(0.75, "logistic") == math.log(0.75 / 0.25)
    for x in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"lies in \(0, 1\)"):
            ontarget.min_sum(x, "logistic")
    with pytest.raises(ValueError):
        ontarget.min_sum(float("inf"), "identity")
    # Params: the conversion, and the refusals
    m_log, m_id = oc.zero_model(4, 0, "logistic"), oc.zero_model(4, 0)
    assert ss.Params(3, min_on_target=0.75).bind_model(m_log).min_sum == math.log(3.0)
    assert ss.Params(3, min_on_target=0.75).bind_model(m_id).min_sum == 0.75
    assert ss.Params(3).bind_model(None).min_sum is None and not ss.Params(3).uses_model
    for kw, text in ((dict(rank="on-target"), "rank on-target needs an on-target model"), (dict(min_on_target=0.5), "min_on_target needs an on-target model")):
        with pytest.raises(ValueError, match=text):
            ss.Params(3, **kw).bind_model(None)
    with pytest.raises(ValueError, match=r"lies in \(0, 1\)"):
        ss.Params(3, min_on_target=1.0).bind_model(m_log)
    with pytest.raises(ValueError, match="rank is specificity or on-target"):
        ss.Params(3, rank="best")


def test_key_transform():
    tiny = np.nextafter(0.0, 1.0)
    vals = np.array([-np.inf, -1.7976931348623157e308, -1e300, -2.5, -1.0, -2.2250738585072014e-308, -tiny * 3, -tiny, -0.0, 0.0, tiny, tiny * 3,
                     2.2250738585072014e-308, 1.0, np.nextafter(1.0, 2.0), 2.5, 1e300, 1.7976931348623157e308, np.inf])
    assert (np.diff(vals) >= 0).all() and (np.diff(vals) > 0).sum() == vals.size - 2
    key = ontarget.sort_key(vals)
    assert key.dtype == np.uint64
    assert key[8] == key[9] == np.uint64(1 << 63)            # -0.0 and +0.0 are one key
    k = [int(x) for x in key]
    assert all(a < b for a, b in zip(k[:8], k[1:9])) and all(a < b for a, b in zip(k[9:], k[10:]))  # strictly monotone elsewhere
    assert k == [oref.key_of(v) for v in vals]
    rng = np.random.default_rng(4)
    r = np.sort(np.concatenate([rng.normal(size=500) * 10.0 ** rng.integers(-300, 300, 500), [0.0, -0.0]]))
    kr = ontarget.sort_key(r).astype(object)
    assert all((a < b) == (x < y) for a, b, x, y in zip(kr[:-1], kr[1:], r[:-1], r[1:]))


def test_rs1_is_the_golden_weights(golden_dir):
    """Term for term: the reference scores the reverse complement of the oriented window (its guide-RNA conversion reverses
    and complements every slice), so window position w and letter b of the model are the golden tables' position 29 - w and
    letter complement(b); a pair (w, b1 b2) is the golden pair at 28 - w with letters complement(b2) complement(b1)."""
    import os
    z = np.load(os.path.join(str(golden_dir), "weights.npz"))
    m = ontarget.rs1()
    assert (m.window, m.left, m.link, m.gc, tuple(m.geometry)) == (30, 5, "logistic", None, RS1_GEOMETRY)
    first, second = z["first"].reshape(30, 4), z["second"].reshape(29, 4, 4)
    comp = [1, 0, 3, 2]  # A T C G -> T A G C
    n_terms = 0
    for w in range(30):
        for b in range(4):
            assert m.single[w, b] == first[29 - w, comp[b]]
            n_terms += first[29 - w, comp[b]] != 0
    for w in range(29):
        for b1 in range(4):
            for b2 in range(4):
                assert m.pair[w, b1 * 4 + b2] == second[28 - w, comp[b2], comp[b1]]
                n_terms += second[28 - w, comp[b2], comp[b1]] != 0
    assert n_terms == np.count_nonzero(z["first"]) + np.count_nonzero(z["second"]) > 60
    assert m.intercept == float(z["consts"][0]) + float(z["consts"][1])
    assert m.terms() == 60


def rs1_bound():
    """The derived bound on |s - s'| for two orders of adding rs1's terms: 2 n 2^-53 A (n terms, A the sum of |weights|)."""
    m = ontarget.rs1()
    return 2.0 * m.terms() * 2.0 ** -53 * m.abs_weight()


def test_rs1_scores_the_golden_vectors(golden_dir):
    import os
    z = np.load(os.path.join(str(golden_dir), "rs1_vectors.npz"))
    seqs, want = z["seqs"], z["libm"]
    m = oref.as_dict(ontarget.rs1(), 20)
    base = np.isin(seqs, np.frombuffer(b"ACGT", np.uint8)).all(axis=1)
    uracil = np.isin(seqs, np.frombuffer(b"ACGTacgtUu", np.uint8)).all(axis=1) & ~base
    # the recorded 30-mer is the string the reference scores: the reverse complement of the oriented window.  As the whole
    # text it is the window of the '-' site that starts at 2: forward 29 down to 0, complemented
    sums = np.array([oref.sum_loop(m, RS1_GEOMETRY, bytes(s), 2, 1) for s in seqs])
    # The fixture's strings are what the reference scores AFTER its upper(): a byte outside upper-case ACGT is scored by it with
    # that letter's terms left out.  Such a vector is skipped: with N, IUPAC or decoration it has no sum here; a lower-case
    # letter or a U does have one (case is ignored, U is A's code), which is not what the fixture recorded for the raw byte
    assert np.array_equal(np.isnan(sums), ~(base | uracil))
    skipped = ~base
    assert int(skipped.sum()) == 2402 == seqs.shape[0] - int(base.sum()) and int(base.sum()) == 1694  # (of 4 096)
    assert int(np.isnan(sums).sum()) == 1848
    v = ontarget.value(sums[base], "logistic")
    bound = rs1_bound() / 4 + 4 * np.spacing(want[base])
    err = np.abs(v - want[base])
    print("largest |value - recorded| %.3g, bound %.3g" % (err.max(), bound.min()))
    assert (err <= bound).all()


def scan_join(texts, rows_of, sums_of):
    """The join of section 3: per contig k, rows_of(k) = the scan's dict (pos_*, pre_*, score_*), sums_of(k, starts, strand) =
    the model's sums of sites with local starts.  Returns (n rows with a score, n clipped rows, largest |s + pre|, largest
    |value - score| - 4 ulp as a fraction of its bound); asserts the set condition on both sides."""
    n_real = n_clipped = 0
    worst_s = 0.0
    bound = rs1_bound()
    for k, t in enumerate(texts):
        h = rows_of(k)
        for strand, tag in ((0, "plus"), (1, "minus")):
            pos, pre, score = np.asarray(h["pos_" + tag], np.int64), np.asarray(h["pre_" + tag]), np.asarray(h["score_" + tag])
            start = pos - 20 if strand == 0 else pos
            real = score != -1.0
            # every guide site of the contig, stated on the letters: N20 NGG on '+', CCN N20 on '-'
            u = np.frombuffer(t, np.uint8)
            n = max(len(t) - 22, 0)
            if strand == 0:
                site = np.nonzero((u[21:21 + n] == 71) & (u[22:22 + n] == 71))[0]
            else:
                site = np.nonzero((u[0:n] == 67) & (u[1:1 + n] == 67))[0]
            s = sums_of(k, site, np.full(site.size, strand))
            has = ~np.isnan(s)
            # the set: rows with a score <-> guide sites with a sum, nothing left out on either side
            assert np.array_equal(np.sort(start[real]), site[has]), (k, tag)
            # clipped rows carry neither a score nor a sum (some are no guide site at all: the guide leaves the contig)
            clipped = start[~real]
            assert not np.isin(clipped, site[has]).any()
            n_real += int(real.sum())
            n_clipped += int((~real).sum())
            # values: the scan's pre = -(s1 + s2 + intersect + low_gc) (the reference negates the sum before exp; crp_score.h
            # keeps that sign), so s = -pre up to the order of the additions
            order = np.argsort(start[real], kind="stable")
            ds = np.abs(s[has] + pre[real][order])
            assert (ds <= bound).all(), (k, tag, ds.max(), bound)
            worst_s = max(worst_s, float(ds.max()) if ds.size else 0.0)
            sc = score[real][order]
            dv = np.abs(ontarget.value(s[has], "logistic") - sc)
            assert (dv <= bound / 4 + 4 * np.spacing(sc)).all(), (k, tag, dv.max())
    return n_real, n_clipped, worst_s


def test_scan_condition_on_the_oracle(oracle):
    """The CPU oracle's scan of the scan genome against the reference statement of rs1: the genome meets section 3's
    condition (no row left out on either side, clipped rows exist), and the values agree within the derived bound."""
    texts = oc.scan_genome()
    m = oref.as_dict(ontarget.rs1(), 20)
    hits = [oracle.scan_score(t, 20) for t in texts]
    n_real, n_clipped, worst = scan_join(texts, lambda k: hits[k], lambda k, st, sd: oref.sums_numpy(m, RS1_GEOMETRY, texts[k], st, sd))
    print("rows with a score %d, clipped %d, largest |s + pre| %.3g of bound %.3g" % (n_real, n_clipped, worst, rs1_bound()))
    assert n_real > 500 and n_clipped >= 8


BASE = ["-f", "genome.fa", "--pattern", "TTTV" + "N" * 23, "--pam-length", "4", "-m", "3"]
NGG = ["-f", "genome.fa", "--pattern", "N" * 20 + "NGG", "--pam-length", "3", "-m", "3"]
SEL = ["--self", "-o", "o", "-g", "x.gff", "--select", "5"]


def refusals(tmp_path):
    good, logi = tmp_path / "good.model", tmp_path / "logistic.model"
    good.write_text("window 34\nleft 4\nsingle 0 A 1\ngc 23 1\n")
    logi.write_text("window 34\nleft 4\nlink logistic\n")
    bad, deep = tmp_path / "bad.model", tmp_path / "deep.model"
    bad.write_text("window 34\nsingle 40 A 1\n")
    deep.write_text("window 34\ngc 24 1\n")
    return [
        (BASE + ["--guides", "g.txt", "-o", "o", "--on-target", str(good)], "--on-target belongs to --self"),
        (BASE + SEL + ["--select-rank", "on-target"], "--select-rank on-target needs --on-target"),
        (BASE + SEL + ["--select-min-on-target", "0.5"], "--select-min-on-target needs --on-target"),
        (BASE + ["--self", "-o", "o", "--select-rank", "on-target", "--on-target", str(good)], "--select-rank belongs to --select"),
        (BASE + ["--self", "-o", "o", "--select-min-on-target", "1", "--on-target", str(good)], "--select-min-on-target belongs to --select"),
        (BASE + ["--self", "-o", "o", "--on-target", "rs1"], "rs1 is valid for a pattern of 23 letters"),
        (NGG[:3] + ["N" * 21 + "NGG"] + NGG[4:] + ["--self", "-o", "o", "--on-target", "rs1"], "rs1 is valid for"),
        (BASE + SEL + ["--on-target", str(logi), "--select-min-on-target", "1.0"], "lies in (0, 1)"),
        (BASE + SEL + ["--on-target", str(logi), "--select-min-on-target", "0"], "lies in (0, 1)"),
        (NGG + SEL + ["--on-target", "rs1", "--select-min-on-target", "-0.5"], "lies in (0, 1)"),
        (BASE + ["--self", "-o", "o", "--on-target", str(bad)], "line 2: POS 40 is outside 0..33"),
        (BASE + ["--self", "-o", "o", "--on-target", str(deep)], "line 2: COUNT 24 is outside 0..23"),
        (BASE + ["--self", "-o", "o", "--on-target", str(tmp_path / "none.model")], "none.model"),
        (BASE + SEL + ["--on-target", str(good), "--select-rank", "best"], "invalid choice"),
    ]


@pytest.mark.parametrize("k", range(14))
def test_command_line_refusals(k, tmp_path, capsys, monkeypatch):
    """Refused through ap.error before the genome is read or the GPU is opened: neither genome.fa nor x.gff exists."""
    import cropsr_amd.engine as engine
    monkeypatch.setattr(engine, "Engine", lambda *a, **kw: pytest.fail("the GPU was opened"))
    table = refusals(tmp_path)
    assert len(table) == 14
    argv, text = table[k]
    with pytest.raises(SystemExit) as e:
        srch.main(argv)
    assert e.value.code == 2
    assert text in capsys.readouterr().err


def test_tsv_without_a_model_is_unchanged():
    """format_self and format_selection of results without a model have no on_target column; with one, the same rows end with
    repr of the value, empty where a site has no sum."""
    sites = np.zeros(3, srch.SELF_SITE_DTYPE)
    sites["contig"], sites["position"], sites["strand"] = [0, 0, 1], [5, 9, 0], [b"+", b"-", b"+"]
    res = srch.SelfSearchResult(sites, np.array([b"ACGT", b"TTTT", b"GGCA"]), np.array([[0, 1], [2, 0], [0, 0]], np.uint32), None, (3, 1), (4, 12))
    plain = "".join(srch.format_self(["chrA", "chrB"], res))
    assert plain == "contig\tposition\tstrand\tguide\tn0\tn1\nchrA\t5\t+\tACGT\t0\t1\nchrA\t9\t-\tTTTT\t2\t0\nchrB\t0\t+\tGGCA\t0\t0\n"
    res.on_target_sum = np.array([0.0, float("nan"), 1.5])
    res.on_target = ontarget.value(res.on_target_sum, "logistic")
    with_model = "".join(srch.format_self(["chrA", "chrB"], res)).split("\n")
    assert [ln.rsplit("\t", 1)[0] for ln in with_model[:-1]] == plain.split("\n")[:-1]
    assert [ln.rsplit("\t", 1)[1] for ln in with_model[:-1]] == ["on_target", "0.5", "", repr(1.0 / (1.0 + math.exp(-1.5)))]
    rows = np.zeros(2, ss.ROW_DTYPE)
    rows["gene"], rows["rank"], rows["contig"], rows["position"], rows["strand"], rows["cut"] = [1, 1], [1, 2], [0, 1], [5, 7], [b"+", b"-"], [22, 13]
    args = (["gene:a", "gene:b"], np.array([0, 9]), np.array([0, 4]), rows, np.array([b"ACGT", b"TTGA"]), np.array([[0, 2], [1, 0]], np.uint32),
            None, np.array([1, 2], np.uint64))
    plain = ss.format_selection(["c0", "c1"], ss.Selection(*args))
    assert plain == "gene\trank\tpassing\tcontig\tposition\tstrand\tguide\tcut\tn0\tn1\ngene:b\t1\t4\tc0\t5\t+\tACGT\t22\t0\t2\ngene:b\t2\t4\tc1\t7\t-\tTTGA\t13\t1\t0\n"
    with_model = ss.format_selection(["c0", "c1"], ss.Selection(*args, on_target_sum=np.array([-2.0, 0.25]), link="identity")).split("\n")
    assert [ln.rsplit("\t", 1)[0] for ln in with_model[:-1]] == plain.split("\n")[:-1]
    assert [ln.rsplit("\t", 1)[1] for ln in with_model[:-1]] == ["on_target", "-2.0", "0.25"]


def test_nothing_else_imports_ontarget():
    """The model is opt-in: the package's other modules import ontarget inside the functions that use a model only."""
    import cropsr_amd
    import sys
    assert "cropsr_amd.ontarget" in sys.modules  # (this file's import)
    import ast
    import pathlib
    for path in pathlib.Path(cropsr_amd.__file__).parent.glob("*.py"):
        if path.name == "ontarget.py":
            continue
        tree = ast.parse(path.read_text())
        for node in tree.body:  # module level only
            if isinstance(node, ast.ImportFrom):
                assert all(a.name != "ontarget" for a in node.names), path.name


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


class Session:
    """The self-search handles of one genome under one pattern, and per arena the fetched rows of its guide sites and the
    arena's letters.  M < 0: no order and no compare are run (the model needs none)."""

    def __init__(self, engine, pid, three, contigs=None, M=-1, scored=False, pattern=None):
        pat, gp, P, pam3, c = cases.PATTERNS[pid]
        if pattern is not None:
            pat, gp = pattern, None
        self.T, self.P, self.pam3, self.G = len(pat), P, pam3, len(pat) - P
        self.geo = (self.T, P, pam3)
        self.c = ref.default_cut(self.T, P, pam3) if c is None else c
        self.region = ref.region_mask(self.T, P, pam3)
        self.contigs = cases.genome() if contigs is None else contigs
        self.genome = engine.genome(self.contigs, max_words=480) if three else engine.genome(self.contigs)
        self.handles, self.rows, self.texts = [], [], []
        self.M = max(M, 0)
        try:
            assert len(self.genome.arenas) == (3 if three else 1)
            score = None if not scored else ("hsu2013" if self.G == 20 else [0.5] * self.G)
            pat, gpat, _, _, scheme = srch.check_self(pat, self.M, P, gp, score)
            self.pattern = pat
            srch._self_handles(self.genome, pat, gpat, P, self.M, scheme, None, None, self.handles)
            if M >= 0:
                srch._self_compare_all(self.handles, M)
            for a, h in enumerate(self.handles):
                pos, strand, hi, lo, counts, hs = h.fetch(scored)
                arena = self.genome.arenas[a]
                group = [self.contigs[t] for t in self.genome.groups[a]]
                cpos, cstrand = cases.candidates(group, arena.offsets, pat)
                where = {(int(p), int(st)): i for i, (p, st) in enumerate(zip(cpos, cstrand))}
                cand = np.array([where[(int(p), int(st))] for p, st in zip(pos, strand)], np.uint32)
                self.rows.append(dict(pos=pos, strand=strand, hi=hi, lo=lo, counts=counts, hit_sum=hs, cand=cand, n_cand=cpos.size))
                self.texts.append(oref.arena_text(group, arena.offsets))
        except BaseException:
            self.close()
            raise

    def close(self):
        for h in self.handles:
            h.close()
        self.genome.close()

    def run_model(self, model):
        """The device's sums of every arena, and the numpy statement's over the fetched rows and the host text."""
        got, want = [], []
        d = oref.as_dict(model, self.G)
        for h, rows, text in zip(self.handles, self.rows, self.texts):
            h.set_model(model, self.G)
            h.run_model()
            got.append(h.fetch_model())
            want.append(oref.sums_numpy(d, self.geo, text, rows["pos"], rows["strand"]))
        return got, want

    def spec(self, k, **kw):
        return ref.spec(self.T, self.c, self.region, k, **kw)


@pytest.fixture(scope="module")
def sessions(engine):
    made = {}

    def get(pid, three=False, M=-1, scored=False):
        key = (pid, three, M, scored)
        if key not in made:
            made[key] = Session(engine, pid, three, M=M, scored=scored)
        return made[key]

    yield get
    for s in made.values():
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("three", [False, True], ids=["1arena", "3arenas"])
@pytest.mark.parametrize("mid", sorted(oc.MODEL_CASES))
def test_sums_are_exact(sessions, mid, three):
    """fetch_model against the numpy statement, bit for bit, NaN pattern included, on every guide site of the four-text genome."""
    pid, W, left, gc = oc.MODEL_CASES[mid]
    s = sessions(pid, three)
    for with_gc in (gc, not gc):
        model = oc.random_model(2, W, left, s.G, with_gc)
        got, want = s.run_model(model)
        n_nan = n_sum = 0
        for a, (g, w) in enumerate(zip(got, want)):
            # the loop statement agrees on a sample (the statements' agreement is proven in full without a GPU)
            pick = np.arange(0, w.size, max(1, w.size // 200))
            loop = oref.sums_loop(oref.as_dict(model, s.G), s.geo, s.texts[a], s.rows[a]["pos"][pick], s.rows[a]["strand"][pick])
            assert np.array_equal(oref.bits(loop), oref.bits(w[pick]))
            assert g.shape == w.shape and np.array_equal(oref.bits(g), oref.bits(w)), (mid, a, with_gc)
            n_nan += int(np.isnan(w).sum())
            n_sum += int((~np.isnan(w)).sum())
        assert n_sum > 20
        if W >= 30:
            assert n_nan > 0  # windows over an N run or a contig's end
        st = s.handles[0].model_stats()
        assert st["model_rows"] == s.rows[0]["n_cand"] and st["model_ms"] >= 0.0
    # a candidate that is no guide site is not in the fetched rows (...NRG candidates against ...NGG guides)
    if pid == "ngg":
        assert s.rows[0]["n_cand"] > s.rows[0]["pos"].size


@pytest.mark.gpu
@pytest.mark.parametrize("W, left", [(30, 5), (64, 20), (64, 63), (64, 0)])
def test_window_edges(engine, W, left):
    """Sites whose windows reach a contig's first and last letter exactly and go one letter past, windows into the leading
    separator word and past the last text, N and lower-case letters in the flanks and the PAM's N -- the NaN and non-NaN sets
    from the host text."""
    texts, planted = oc.edge_genome(W, left)
    s = Session(engine, "ngg", False, contigs=texts)
    try:
        rows, text = s.rows[0], s.texts[0]
        arena = s.genome.arenas[0]
        offs = [int(o) for o in arena.offsets]
        model = oc.random_model(4, W, left, s.G, True)
        d = oref.as_dict(model, s.G)
        (got,), (want,) = s.run_model(model)
        # the claims, on the reference
        assert offs[0] >= 64 and offs[0] - max(left, W - 23 - left) >= 0  # (no window of a site starts before arena position 0 ...)
        for strand in (0, 1):
            assert set((rows["pos"][rows["strand"] == strand] % 64).tolist()) == set(range(64))  # every offset modulo 64
        at = {(int(p), int(st)): i for i, (p, st) in enumerate(zip(rows["pos"], rows["strand"]))}
        kinds = set()
        for name, (k, start, strand, has) in planted.items():
            i = at[(offs[k] + start, strand)]
            assert math.isnan(want[i]) == (not has), name
            assert math.isnan(oref.sum_loop(d, s.geo, text, offs[k] + start, strand)) == (not has), name
            kinds.add(name.rsplit("-", 1)[0] if name[-1] in "01pm" else name)
        assert "plus-at-end" in kinds and (left == 0 or {"plus-first-past", "minus-last-past"} <= kinds)  # (left = 0: no left flank)
        if W == 30:
            assert {"plus-first-exact", "plus-last-exact", "plus-last-past", "minus-first-exact", "minus-first-past", "minus-last-exact",
                    "left-n", "left-lower", "right-n", "right-lower", "pam-n-n", "pam-n-lower"} <= kinds
        # ... but the first text's first windows lie in the leading separator word (void: no sum), and the last site's right
        # flank lies behind the last text, in the arena's last words and beyond them
        if left:
            k, start, strand, _ = planted["plus-first-past-0"]
            assert min(oref.window_forward(d, s.geo, offs[k] + start, strand)) == offs[0] - 1
        k, start, _, has = planted["plus-at-end"]
        assert offs[k] + start + 22 == offs[-1] + len(texts[-1]) - 1
        # a candidate that is no guide site: an NAG site is a candidate, and not in the fetched rows
        cpos, cstrand = cases.candidates(texts, arena.offsets, s.pattern)
        assert set(at) < set(zip(cpos.tolist(), cstrand.tolist()))
        assert np.array_equal(oref.bits(got), oref.bits(want))
        assert np.isnan(want).sum() >= 8 and (~np.isnan(want)).sum() > 100
    finally:
        s.close()


@pytest.mark.gpu
def test_against_the_scan(engine):
    """The independent check: the scan's own score of every NGG row against rs1 on the N20NGG guide sites of the same genome.
    The set condition (no row left out on either side; clipped rows carry neither) and the values, within the bound derived
    from the order of the additions alone.  The sign: the scan's pre is -(sum) (the reference negates before exp), so
    s = -pre."""
    texts = oc.scan_genome()
    g = engine.genome(texts)
    handles = []
    try:
        assert len(g.arenas) == 1
        arena = g.arenas[0]
        hits = arena.scan_score(20, want_pre=True)
        pattern = "N" * 20 + "NGG"
        srch._self_handles(g, pattern, pattern, 3, 0, None, None, None, handles)
        h = handles[0]
        h.set_model(ontarget.rs1(), 20)
        h.run_model()
        pos, strand, _, _, _, _ = h.fetch(False)
        sums = h.fetch_model()
        offs = np.asarray(arena.offsets, np.int64)
        table = {(int(p), int(st)): float(v) for p, st, v in zip(pos, strand, sums)}

        def sums_of(k, starts, sd):
            # every guide site the letters state is one the device found, once
            out = np.array([table.pop((int(offs[k] + s0), int(st))) for s0, st in zip(starts, sd)], np.float64)
            return out

        n_real, n_clipped, worst = scan_join(texts, hits.contig, sums_of)
        assert not table  # and the device found no other
        print("rows with a score %d, clipped %d, largest |s + pre| %.3g of bound %.3g" % (n_real, n_clipped, worst, rs1_bound()))
        assert n_real > 500 and n_clipped >= 8
    finally:
        for h in handles:
            h.close()
        g.close()


# ---- the ranked selection ------------------------------------------------------------------------------------------------

def run_select(s, a, lo, hi, params, slice_rows=0, items_per_launch=0, sel=None):
    """fetch_self()'s dict with on_target_sum of one run on arena a (sel: an open ArenaSelect to reuse)."""
    own = sel is None
    if own:
        sel = sel_mod.ArenaSelect(s.genome.arenas[a], lo, hi)
    try:
        sel.set_limits(slice_rows)
        sel.set_self_limits(items_per_launch)
        sel.set_self_model(params.rank == "on-target", params.min_sum)
        sel.run_self(params.resolve(s.T, s.P, s.pam3), s.handles[a])
        got = sel.fetch_self()
        got["on_target_sum"] = sel.fetch_self_model()
        return got, sel.self_stats()
    finally:
        if own:
            sel.close()


def spec_of(s, p):
    return ref.spec(s.T, p.cut_offset if p.cut_offset is not None else s.c, s.region, p.k, max_mm0=p.max_mm0, max_hit_sum=p.max_hit_sum,
                    gc_min=p.gc_min, gc_max=p.gc_max, max_t_run=p.max_t_run)


def check_select(s, a, lo, hi, params, sums, **kw):
    """One run against the extended statement: sel, n_in, n_pass and the gathered sums, exactly."""
    params.cut_offset = s.c
    got, stats = run_select(s, a, lo, hi, params, **kw)
    rows = s.rows[a]
    want = oref.select_ranked(rows, lo, hi, spec_of(s, params), sums, params.rank == "on-target", params.min_sum, ref)
    assert np.array_equal(got["n_in"], want[0]) and np.array_equal(got["n_pass"], want[1]), (got["n_pass"], want[1])
    assert np.array_equal(got["sel"], want[2])
    row_of = np.full(rows["n_cand"] + 1, -1, np.int64)
    row_of[rows["cand"]] = np.arange(rows["cand"].size)
    have = want[2] != NONE
    r = row_of[want[2][have]]
    assert (r >= 0).all()
    assert np.array_equal(oref.bits(got["on_target_sum"][have]), oref.bits(sums[r]))
    assert (oref.bits(got["on_target_sum"][~have]) == oref.NAN_BITS).all()
    assert np.array_equal(got["arena_pos"][have], rows["pos"][r]) and np.array_equal(got["counts"][have], rows["counts"][r])
    return got, want, stats


def model_params(model, k, **kw):
    return ss.Params(k, **kw).bind_model(model)


@pytest.mark.gpu
@pytest.mark.parametrize("slices", ["default", "sliced"])
@pytest.mark.parametrize("K", [1, 5, 64])
@pytest.mark.parametrize("key", [("ngg", False), ("cas12a", True)], ids=["ngg-1arena", "cas12a-3arenas"])
def test_ranked_gene_sizes(sessions, key, K, slices):
    """Genes of 0, 1, K - 1, K, K + 1, 64, 65 and 129 passing sites (chosen on the fetched rows with a sum; sites without a sum
    lie inside them: in n_in, never in n_pass), whole-arena genes, default slices and slices of 64 rows with two items a launch."""
    pid, three = key
    s = sessions(pid, three, M=1, scored=True)
    W, left = (30, 5) if pid == "ngg" else (34, 4)
    model = oc.random_model(6, W, left, s.G, True)
    got, want = s.run_model(model)
    sizes = sorted({0, 1, max(K - 1, 0), K, K + 1, 64, 65, 129})
    n_without = 0
    for a, rows in enumerate(s.rows):
        assert np.array_equal(oref.bits(got[a]), oref.bits(want[a]))
        sums = got[a]
        has = ~np.isnan(sums)
        few = has.sum() < 400
        use = [n for n in sizes if not few or n <= 5]
        with_sum = {key_: (v[has] if isinstance(v, np.ndarray) else v) for key_, v in rows.items() if key_ != "n_cand"}
        lo, hi = cases.size_genes(with_sum, s.T, s.c, use)
        end = int(s.genome.arenas[a].offsets[-1] + s.genome.arenas[a].lengths[-1])
        lo, hi = np.concatenate([lo, [0]]).astype(np.uint32), np.concatenate([hi, [end]]).astype(np.uint32)
        kw = dict(slice_rows=64, items_per_launch=2) if slices == "sliced" else {}
        p = model_params(model, K, rank="on-target")
        _, w, stats = check_select(s, a, lo, hi, p, sums, **kw)
        assert w[1][:len(use)].tolist() == use and w[0][-1] == rows["pos"].size and w[1][-1] == has.sum()
        n_without += int((w[0] > w[1]).sum())
        if slices == "sliced" and not few:
            assert stats["self_items"] > len(lo) and stats["self_launches"] > 1  # genes were cut, and merged
    assert n_without > 0  # sites without a sum inside a gene


@pytest.mark.gpu
def test_ranked_ties_zero_and_straddle(sessions):
    """Equal sums: the tandem repeats of 70 copies per strand (one window each: one sum), whose ties fill more than one wave's
    list and are broken by the cut letter, then the strand; a model with every weight 0.0 (every sum +0.0: the tie order
    alone); a model whose sums are GC - G / 2 (equal sums on both sides of zero, -0.0 none, 0.0 many)."""
    s = sessions("ngg", False, M=1, scored=True)
    rows = s.rows[0]
    arena = s.genome.arenas[0]
    offs = [int(o) for o in arena.offsets]
    unit = len(cases.UNIT)
    rep = [(offs[0] + 9000 + 2 * unit, offs[0] + 9000 + unit * (cases.REPEATS - 1)), (offs[2] + 10000 + unit, offs[2] + 10000 + unit * (cases.REPEATS - 2))]
    end = offs[-1] + int(arena.lengths[-1])
    lo = np.array([rep[0][0], rep[1][0], 0, rep[0][0]], np.uint32)
    hi = np.array([rep[0][1], rep[1][1], end, rep[1][1]], np.uint32)
    for model, name in ((oc.random_model(8, 30, 5, s.G, False), "random"), (oc.zero_model(30, 5), "zero"), (oc.gc_only_model(30, 5, s.G), "gc")):
        (sums,), (want,) = s.run_model(model)
        assert np.array_equal(oref.bits(sums), oref.bits(want))
        cut = ref.cut_letters(rows["pos"], rows["strand"], s.T, s.c)
        if name == "random":  # the claim: inside each repeat gene at least 65 sites of one strand share the largest sum
            for g, strand in ((0, 0), (1, 1)):
                inside = (cut >= lo[g]) & (cut <= hi[g]) & ~np.isnan(sums) & (rows["strand"] == strand)
                vals, n = np.unique(sums[inside], return_counts=True)
                assert n.max() >= 65, (g, n.max())
            assert (sums[~np.isnan(sums)] > 0).any() and (sums[~np.isnan(sums)] < 0).any()
        if name == "zero":
            assert (oref.bits(sums[~np.isnan(sums)]) == 0).all()
        if name == "gc":
            v = sums[~np.isnan(sums)]
            assert (v == 0.0).sum() > 50 and (v < 0).sum() > 50 and (v > 0).sum() > 50 and np.unique(v).size <= 21
        for K in (5, 64):
            for kw in (dict(), dict(slice_rows=64, items_per_launch=2)):
                got, w, _ = check_select(s, 0, lo, hi, model_params(model, K, rank="on-target"), sums, **kw)
                if name == "zero":  # pure tie order: the cut letters ascend, '+' before '-' on one letter
                    r = np.searchsorted(rows["cand"], w[2][2][w[2][2] != NONE])
                    t = cut[r] * 2 + rows["strand"][r]
                    assert (np.diff(t) > 0).all() and t[0] == (cut * 2 + rows["strand"])[~np.isnan(sums)].min()


@pytest.mark.gpu
@pytest.mark.parametrize("link", ["identity", "logistic"])
def test_threshold_and_filters(sessions, link):
    """min_on_target exactly at a site's value, one ulp below and one ulp above, through the Params path; the specificity
    filters stay filters (max_perfect = 0, min_specificity on the scored handle), alone and with the model's rank."""
    s = sessions("ngg", False, M=1, scored=True)
    rows = s.rows[0]
    model = oc.random_model(9, 30, 5, s.G, True, link)
    (sums,), _ = s.run_model(model)
    end = int(s.genome.arenas[0].offsets[-1] + s.genome.arenas[0].lengths[-1])
    lo, hi = np.array([0, 5000], np.uint32), np.array([end, 9000], np.uint32)
    have = np.sort(sums[~np.isnan(sums)])
    v = float(have[have.size // 2])
    if link == "identity":
        for x, n in ((v, (have >= v).sum()), (np.nextafter(v, -np.inf), (have >= v).sum()), (np.nextafter(v, np.inf), (have > v).sum())):
            p = model_params(model, 5, rank="on-target", min_on_target=float(x))
            assert p.min_sum == float(x)
            _, w, _ = check_select(s, 0, lo, hi, p, sums)
            assert w[1][0] == n
        assert (have >= v).sum() > (have > v).sum()
    else:
        x = 0.6
        p = model_params(model, 5, rank="on-target", min_on_target=x)
        assert p.min_sum == math.log(x / (1 - x))
        _, w, _ = check_select(s, 0, lo, hi, p, sums)
        assert 0 < w[1][0] == (have >= p.min_sum).sum() < have.size
        # exactly at a site's sum and an ulp on either side: Params objects whose min_sum the conversion gave, then moved
        for ms, n in ((v, (have >= v).sum()), (np.nextafter(v, np.inf), (have > v).sum())):
            p = model_params(model, 5, rank="on-target", min_on_target=0.5)
            p.min_sum = float(ms)
            _, w, _ = check_select(s, 0, lo, hi, p, sums)
            assert w[1][0] == n
    # a bound without the rank: the order stays the specificity order, the sum only filters
    p = model_params(model, 5, min_on_target=0.55 if link == "logistic" else v)
    _, w_spec, _ = check_select(s, 0, lo, hi, p, sums)
    _, w_rank, _ = check_select(s, 0, lo, hi, model_params(model, 5, rank="on-target", min_on_target=0.55 if link == "logistic" else v), sums)
    assert np.array_equal(w_spec[1], w_rank[1]) and not np.array_equal(w_spec[2], w_rank[2])
    # the specificity filters
    all_pass = check_select(s, 0, lo, hi, model_params(model, 64, rank="on-target"), sums)[1][1]
    for kw in (dict(max_perfect=0), dict(min_specificity=0.5), dict(max_perfect=0, min_specificity=0.2, gc_min=8, gc_max=14, max_t_run=3)):
        _, w, _ = check_select(s, 0, lo, hi, model_params(model, 64, rank="on-target", **kw), sums)
        assert (w[1] <= all_pass).all() and ("max_perfect" not in kw or w[1][0] < all_pass[0]), kw  # (the repeats' sites have perfect copies)


@pytest.mark.gpu
def test_specificity_rank_and_handle_reuse(sessions):
    """rank = specificity with a model set and run reproduces the selection without a model, bit for bit; one select handle run
    by model, by specificity and by model again gives the first result again; a handle whose model has not run is refused."""
    from cropsr_amd import _native as nat
    s = sessions("cas12a", False, M=1, scored=True)
    rows = s.rows[0]
    end = int(s.genome.arenas[0].offsets[-1] + s.genome.arenas[0].lengths[-1])
    lo, hi = np.array([0, 3000, 700], np.uint32), np.array([end, 20000, 800], np.uint32)
    model = oc.random_model(10, 34, 4, s.G, True)
    sel = sel_mod.ArenaSelect(s.genome.arenas[0], lo, hi)
    try:
        # before any model: the plain selection, and the refusal of the model's rank
        s.handles[0].set_model(model, s.G)  # (set, not run: the sums of an earlier test's run are dropped)
        plain_p = ss.Params(7).resolve(s.T, s.P, s.pam3)
        sel.run_self(plain_p, s.handles[0])
        plain = sel.fetch_self()
        assert np.isnan(sel.fetch_self_model()).all()
        sel.set_self_model(True, None)
        with pytest.raises(nat.CropsrHipError, match="model run first"):
            sel.run_self(plain_p, s.handles[0])
        sel.set_self_model(False, None)
        (sums,), _ = s.run_model(model)
        want_plain = ref.select_numpy(rows, lo, hi, s.spec(7))
        assert np.array_equal(plain["sel"], want_plain[2])
        by_model_p = model_params(model, 7, rank="on-target")
        first, _ = run_select(s, 0, lo, hi, by_model_p, sel=sel)
        spec, _ = run_select(s, 0, lo, hi, model_params(model, 7), sel=sel)
        again, _ = run_select(s, 0, lo, hi, by_model_p, sel=sel)
        for key in plain:
            assert np.array_equal(spec[key], plain[key]), key  # with a model on the handle, every bit of section 28
            assert np.array_equal(first[key], again[key]), key
        assert np.array_equal(oref.bits(first["on_target_sum"]), oref.bits(again["on_target_sum"]))
        assert not np.array_equal(first["sel"], spec["sel"])
        want = oref.select_ranked(rows, lo, hi, s.spec(7), sums, True, None, ref)
        assert np.array_equal(first["sel"], want[2]) and np.array_equal(first["n_pass"], want[1])
    finally:
        sel.close()


@pytest.mark.gpu
def test_set_model_refusals(sessions):
    """Each refusal of crp_search_self_set_model leaves a text and no side effect: the model that was run stays fetchable."""
    from cropsr_amd import _native as nat
    import ctypes
    s = sessions("ngg", False)
    h = s.handles[0]
    model = oc.random_model(11, 30, 5, s.G, True)
    (before,), _ = s.run_model(model)
    L = nat.lib()
    one = (ctypes.c_double * 256)(*([0.0] * 256))
    bad = (ctypes.c_double * 256)(*([0.0] * 7 + [float("nan")] + [0.0] * 248))
    inf = (ctypes.c_double * 1008)(*([0.0] * 20 + [float("inf")] + [0.0] * 987))
    for args, text in (((0, 0, 0.0, one, None, None, 0), "window of 1..64"), ((65, 0, 0.0, one, None, None, 0), "window of 1..64"),
                       ((30, 30, 0.0, one, None, None, 0), "left must be 0..29"), ((30, -1, 0.0, one, None, None, 0), "left must be 0..29"),
                       ((30, 5, 0.0, one, None, one, 20), "gc table has 20 weights"), ((30, 5, 0.0, one, None, one, 22), "gc table has 22 weights"),
                       ((30, 5, float("nan"), one, None, None, 0), "intercept is not a finite"), ((30, 5, 0.0, bad, None, None, 0), "single-letter weight"),
                       ((30, 5, 0.0, one, inf, None, 0), "pair weight"), ((30, 5, 0.0, one, None, bad, 21), "gc weight")):
        st = L.crp_search_self_set_model(h._h, *args)
        assert st == nat.CRP_ERR_INVALID, args
        with pytest.raises(nat.CropsrHipError, match=text):
            h._check(st, "crp_search_self_set_model")
        assert np.array_equal(oref.bits(h.fetch_model()), oref.bits(before))


GFF_TWO_TEXTS = """##gff-version 3
c0\ttest\tgene\t10031\t10570\t.\t+\t.\tID=rep
c0\ttest\tgene\t2001\t9000\t.\t+\t.\tID=g1
c1\ttest\tgene\t100\t4000\t.\t-\t.\tID=g2
c3\ttest\tgene\t1\t5003\t.\t+\t.\tID=g5
"""


@pytest.mark.gpu
def test_equal_sums_over_three_arenas(engine, tmp_path):
    """search_self(on_target=, select=) and the host's assemble: texts 0 and 2 carry one FASTA name and lie in different arenas;
    the gene `rep` covers the '+' repeat of the one and the '-' repeat of the other.  Under the GC model every repeat site has
    one sum, so the gene's equal-sum rows lie in two arenas and must come out as in one arena: the first text's, then the
    second's.  The per-site columns of the result are the handles' sums in the result's order."""
    from cropsr_amd import annotate
    contigs, names = cases.genome(), ["c0", "c1", "c0", "c3"]
    gff = tmp_path / "two.gff3"
    gff.write_text(GFF_TWO_TEXTS)
    pattern, K = "N" * 20 + "NGG", 30
    model = oc.gc_only_model(30, 5, 20)
    ann = annotate.Annotation(str(gff))
    out = {}
    try:
        for three in (False, True):
            g = engine.genome(contigs, max_words=480) if three else engine.genome(contigs)
            try:
                assert len(g.arenas) == (3 if three else 1)
                req = ss.Request(ss.Params(K, 17, rank="on-target", min_on_target=-20.0), annotate.Request(ann, names, 0), slice_rows=64 if three else None)
                res = srch.search_self(g, pattern, 1, 3, select=req, on_target=model)
                out[three] = (ss.format_selection(names, res.selection), res)
            finally:
                g.close()
    finally:
        ann.close()
    assert out[False][0].split("\n") == out[True][0].split("\n")
    one, three = out[False][1], out[True][1]
    assert np.array_equal(one.sites, three.sites) and np.array_equal(oref.bits(one.on_target_sum), oref.bits(three.on_target_sum))
    assert np.array_equal(oref.bits(one.on_target), oref.bits(one.on_target_sum))  # identity link
    sel = one.selection
    rep = sel.rows["gene"] == 0
    assert rep.sum() == K and np.unique(sel.on_target_sum[rep]).size == 1
    strands = sel.rows["strand"][rep].tolist()
    n_plus = strands.count(b"+")
    assert 15 <= n_plus < K and strands == [b"+"] * n_plus + [b"-"] * (K - n_plus)  # the first text's rows, then the second's
    for gi in range(len(sel.labels)):  # every gene's list descends in the sum; rows of equal sums ascend in (text, cut)
        v = sel.on_target_sum[sel.rows["gene"] == gi]
        assert (np.diff(v) <= 0).all() and not np.isnan(v).any()
    # the result's per-site sums against the statement, through the result's own site rows
    text = oref.arena_text(contigs, [0, 40000, 80000, 120000], tail=0)
    pos = np.array([0, 40000, 80000, 120000])[one.sites["contig"]] + one.sites["position"]
    # (contig indices of the result are FASTA records: texts 0 and 2 are separate records here)
    want = oref.sums_numpy(oref.as_dict(model, 20), RS1_GEOMETRY, text, pos, one.sites["strand"] == b"-")
    assert np.array_equal(oref.bits(one.on_target_sum), oref.bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("nuclease", ["ngg-rs1", "cas12a-file"])
def test_command_line_end_to_end(engine, tmp_path, nuclease):
    """One genome through python -m cropsr_amd.search --self --on-target: the appended on_target fields of both TSVs re-derived
    from search_self's result, the leading fields equal to those of the same command without --on-target."""
    from cropsr_amd import annotate
    contigs, names = cases.genome(), ["c0", "c1", "c2", "c3"]
    fa, gff = tmp_path / "g.fa", tmp_path / "g.gff3"
    fa.write_bytes(b"".join(b">" + n.encode() + b" x\n" + c + b"\n" for n, c in zip(names, contigs)))
    gff.write_text(GFF_TWO_TEXTS.replace("10031\t10570", "9001\t10570"))
    if nuclease == "ngg-rs1":
        pattern, P, spec, model, extra = "N" * 20 + "NGG", 3, "rs1", ontarget.rs1(), ["--select-min-on-target", "0.2"]
    else:
        pattern, P = "TTTV" + "N" * 23, 4
        model = oc.random_model(12, 34, 4, 23, True, "identity")
        spec = str(tmp_path / "cas12a.model")
        (tmp_path / "cas12a.model").write_text(ontarget.format_model(model))
        extra = []
    base = ["-f", str(fa), "--pattern", pattern, "--pam-length", str(P), "--self", "-m", "1", "-g", str(gff), "--select", "6"]
    plain, with_model = tmp_path / "plain.tsv", tmp_path / "model.tsv"
    assert srch.main(base + ["-o", str(plain)]) == 0
    assert srch.main(base + ["-o", str(with_model), "--on-target", spec, "--select-rank", "specificity"]) == 0
    ann = annotate.Annotation(str(gff))
    g = engine.genome(contigs)
    try:
        req = ss.Request(ss.Params(6), annotate.Request(ann, names, 0))
        res = srch.search_self(g, pattern, 1, P, select=req, on_target=model)
    finally:
        g.close()
        ann.close()
    for path, plain_path, values in ((with_model, plain, res.on_target), (str(with_model) + ".selected.tsv", str(plain) + ".selected.tsv", res.selection.on_target)):
        lines, plain_lines = open(path).read().split("\n"), open(plain_path).read().split("\n")
        assert lines[-1] == "" and len(lines) == len(plain_lines) == len(values) + 2
        assert [ln.rsplit("\t", 1)[0] for ln in lines[:-1]] == plain_lines[:-1]  # the leading fields: the same command without a model
        assert [ln.rsplit("\t", 1)[1] for ln in lines[:-1]] == ["on_target"] + ["" if v != v else repr(float(v)) for v in values]
        assert any(v != v for v in res.on_target) and sum(v == v for v in values) > 10
    if nuclease == "ngg-rs1":
        assert ((res.on_target[~np.isnan(res.on_target)] > 0) & (res.on_target[~np.isnan(res.on_target)] < 1)).all()
    # ranked by the model, with a bound: the selection file's values descend inside every gene and respect the bound
    ranked = tmp_path / "ranked.tsv"
    assert srch.main(base + ["-o", str(ranked), "--on-target", spec, "--select-rank", "on-target"] + extra) == 0
    rows = [ln.split("\t") for ln in open(str(ranked) + ".selected.tsv").read().split("\n")[1:-1]]
    assert len(rows) > 6
    by_gene = {}
    for r in rows:
        by_gene.setdefault(r[0], []).append(float(r[-1]))
    for v in by_gene.values():
        assert v == sorted(v, reverse=True) and (not extra or min(v) >= 0.2)
