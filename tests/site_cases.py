"""Inputs of tests/test_sites.py, shared by its CPU and GPU tests: small genomes with planted recognition sites, so that every
rule and edge of the restriction-site masks (cropsr_amd/sites.py) is met -- check(case) asserts on the reference's columns,
on the CPU, that a case holds what it is for, before the GPU tests look at the device.

A case is dict(name, texts, l, flanks, enzymes [(name, motif)]).  arena(case) lays the texts out as an arena does (64-aligned,
one separator word between texts, the first at 64: variant_cases.offsets) and gives the arena as one byte string (void = 0),
the texts' bounds and the kept positions."""
import numpy as np

import site_reference as ref
from variant_cases import kept, offsets

BUILTIN = [("BsaI", "GGTCTC"), ("BbsI", "GAAGAC"), ("BsmBI", "CGTCTC"), ("SapI", "GCTCTTC"), ("AarI", "CACCTGC"),
           ("EcoRI", "GAATTC"), ("BamHI", "GGATCC"), ("HindIII", "AAGCTT"), ("XbaI", "TCTAGA"), ("PstI", "CTGCAG"), ("SacI", "GAGCTC"),
           ("KpnI", "GGTACC"), ("SalI", "GTCGAC"), ("XhoI", "CTCGAG"), ("NcoI", "CCATGG"), ("NdeI", "CATATG"), ("EcoRV", "GATATC"),
           ("SmaI", "CCCGGG"), ("SpeI", "ACTAGT"), ("NheI", "GCTAGC"), ("BglII", "AGATCT"), ("ClaI", "ATCGAT"), ("SphI", "GCATGC"),
           ("ApaI", "GGGCCC"), ("NotI", "GCGGCCGC"), ("MspI", "CCGG"), ("HaeIII", "GGCC"), ("AluI", "AGCT"), ("TaqI", "TCGA"),
           ("RsaI", "GTAC"), ("HinfI", "GANTC"), ("BstNI", "CCWGG")]
SOFT = np.frombuffer(b"ACGTACGTACGTACGTacgtN", dtype=np.uint8)  # the smoke test's alphabet: soft-masked letters and N runs
AT = np.frombuffer(b"AT", dtype=np.uint8)
FLANKS = [8, 64, 300, 100000]  # the built-in set's m_max, a plane word, the default, larger than every text


def arena(case):
    """dict(offsets, bytes (the arena as a string, void = 0), bounds [(t0, t1)], pos_plus, pos_minus (uint32))."""
    offs = offsets(case["texts"])
    size = offs[-1] + ((len(case["texts"][-1]) + 63) // 64 + 1) * 64
    buf = bytearray(size)
    for t, o in zip(case["texts"], offs):
        buf[o:o + len(t)] = t
    per = [kept(t, case["l"]) for t in case["texts"]]
    cat = lambda k: np.concatenate([p[k].astype(np.int64) + o for p, o in zip(per, offs)]).astype(np.uint32)
    return dict(offsets=offs, bytes=bytes(buf), bounds=[(o, o + len(t)) for t, o in zip(case["texts"], offs)], pos_plus=cat(0),
                pos_minus=cat(1))


def motifs(case):
    return [m for _, m in case["enzymes"]]


def reference(case, A, flank):
    """{plus, minus: site_reference.columns_numpy} of the case's rows at one flank."""
    return {s: ref.columns_numpy(A["bytes"], A["bounds"], A["pos_" + s], s == "minus", case["l"], flank, motifs(case)) for s in ("plus", "minus")}


# ------------------------------------------------------------------------------------------------ the usual genome
def random_texts():
    rng = np.random.default_rng(2701)
    return [rng.choice(SOFT, n).tobytes() for n in (50000, 3001, 70, 27000)]


def random_case():
    """~80 kb in four texts, soft-masked letters and N among them, the built-in 32 enzymes: every alignment of a window to the
    plane words, every mask bit, and a text of 70 letters between neighbours."""
    return dict(name="random", texts=random_texts(), l=20, flanks=FLANKS, enzymes=BUILTIN)


def check_random(case, A):
    """Every strand has rows with in_guide set and clear, assay set, span >= 1 with amp == 2, span == 0 with amp == 1; the
    amplicon's ends meet bits 0 and 63 of a plane word on rows that have a site across the cut; every enzyme occurs."""
    for flank in case["flanks"]:
        cols = reference(case, A, flank)
        for s in ("plus", "minus"):
            c = cols[s]
            assert (c["in_guide"] != 0).any() and (c["in_guide"] == 0).any(), (s, flank)
            assert (c["assay"] != 0).any(), (s, flank)
            assert ((c["span"] == 0) & (c["amp"] == 1)).any(), (s, flank)
            if flank in (64, 300):  # (an amplicon of 16 letters rarely holds two sites of one enzyme, a whole text rarely only two: the planted case has these rows)
                assert ((c["span"] >= 1) & (c["amp"] == 2)).any(), (s, flank)
            if flank > 8:
                assert ((c["span"] >= 1) & (c["amp"] > 2)).any(), (s, flank)
    cols = reference(case, A, 64)
    for s, minus in (("plus", False), ("minus", True)):
        p = A["pos_" + s].astype(np.int64)
        c = p + 6 if minus else p - 3
        spanning = (cols[s]["span"] >= 1).any(axis=1)
        for m in (4, 6):
            for bit in (0, 63):
                assert (((c + 64 - m + 1) & 63) == bit)[spanning].any() and (((c - 64) & 63) == bit)[spanning].any(), (s, m, bit)
    seen = np.zeros(len(case["enzymes"]), bool)
    for e, m in enumerate(motifs(case)):
        seen[e] = ref.occurrences_numpy(A["bytes"], m).any()
    assert seen.sum() >= 30  # (NotI's eight letters may not occur in 80 kb)


def short_text_case():
    """A text of 70 letters with one row of each strand and a site across each cut, between neighbours whose sites lie fewer
    than 300 positions away -- in the last letters of the text before and the first of the text behind.  They must not count."""
    rng = np.random.default_rng(2708)
    before = bytearray(rng.choice(AT, 500).tobytes())
    before[-6:] = b"GAATTC"
    before[-30:-26] = b"ACGT"
    behind = bytearray(rng.choice(AT, 400).tobytes())
    behind[:6] = b"GAATTC"
    behind[10:14] = b"ACGT"
    short = bytearray(rng.choice(AT, 70).tobytes())
    short[6:9] = b"CCA"           # j = 6, c = 12
    short[9:15] = b"GAATTC"       # q = c - 3
    short[43:46] = b"TGG"         # i = 43, c = 40
    short[37:41] = b"ACGT"        # q = c - 3
    short[50:54] = b"ACGT"        # a second one in the same text: no assay
    return dict(name="short text", texts=[bytes(before), bytes(short), bytes(behind)], l=20, flanks=[16, 64, 300, 100000],
                enzymes=[("six", "GAATTC"), ("four", "ACGT")])


def check_short_text(case, A):
    t0, t1 = A["bounds"][1]
    assert t1 - t0 == 70 and A["bounds"][0][1] > t0 - 300 and A["bounds"][2][0] < t1 + 300
    for flank in (64, 300, 100000):
        cols = reference(case, A, flank)
        for s, at, e, amp in (("minus", t0 + 6, 0, 1), ("plus", t0 + 43, 1, 2)):
            r = np.flatnonzero(A["pos_" + s] == at)
            assert r.size == 1
            assert cols[s]["span"][r[0], e] == 1 and cols[s]["amp"][r[0], e] == amp and (cols[s]["assay"][r[0]] >> e & 1) == (amp == 1), (flank, s)
        # without the clipping at the text's ends the neighbours' sites would have counted
        loose = ref.columns_numpy(A["bytes"], [(0, len(A["bytes"]))], A["pos_minus"], True, 20, flank, motifs(case))
        r = np.flatnonzero(A["pos_minus"] == t0 + 6)[0]
        assert loose["amp"][r, 0] == (1 if flank == 64 else 3), flank


# ------------------------------------------------------------------------------------------------ planted windows
LONG16 = "GATTACAGATTACAGA"   # 16 letters, not a palindrome
PLANT_SET = [("four", "ACGT"), ("six", "GAATTC"), ("seven", "GCTCTTC"), ("eight", "GCGGCCGC"), ("sixteen", LONG16), ("hinf", "GANTC"),
             ("bstn", "CCWGG"), ("oneway", "GGTCTC"), ("acaca", "ACACA")]
# motifs over every IUPAC letter: GA?TC with each of the 15 letters against the four bases the random text puts there
IUPAC_SET = [("x" + ch, "GAT" + ch + "ATC") for ch in "ACGTRYSWKMBDHVN"]


class Planter:
    """A text of A and T (no hit, no site of PLANT_SET) into which windows are planted 200 letters apart.  want collects what
    the reference must say about them: (what, key, enzyme name, value) at flank 64."""

    def __init__(self, seed, n):
        self.rng = np.random.default_rng(seed)
        self.text = bytearray(self.rng.choice(AT, n).tobytes())
        self.at = 100
        self.rows = {}  # what -> (strand, string index of the match)
        self.want = []

    def put(self, p, s):
        self.text[p:p + len(s)] = s.encode() if isinstance(s, str) else s

    def plus(self, what, site, q_rel, **want):
        """A '+' hit (TGG, match index i) and `site` at string index c + q_rel, c = i - 3; the site may cover the PAM's first
        letter.  Returns i."""
        i = self.at + 70
        assert q_rel + len(site) <= 4
        self.put(i, "TGG")
        self.put(i - 3 + q_rel, site)
        self.rows["+ " + what] = ("plus", i)
        self.want += [("+ " + what,) + tuple(k.split("_", 1)) + (v,) for k, v in want.items()]
        self.at += 200
        return i

    def minus(self, what, site, q_rel, **want):
        """A '-' hit (CCA, match index j) and `site` at string index c + q_rel, c = j + 6; the site may cover the PAM's last
        letter.  Returns j."""
        j = self.at + 70
        assert q_rel >= -4
        self.put(j, "CCA")
        self.put(j + 6 + q_rel, site)
        self.rows["- " + what] = ("minus", j)
        self.want += [("- " + what,) + tuple(k.split("_", 1)) + (v,) for k, v in want.items()]
        self.at += 200
        return j


def planted_case():
    """One text of A and T with planted windows, named for what can go wrong; PLANT_SET's lengths are 4, 5, 6, 7, 8 and 16.
    l = 20.  A keyword of plus() / minus() is <column>_<enzyme> = the value the reference must give at flank 64."""
    P = Planter(2702, 16010)
    eight, six, four = "GCGGCCGC", "GAATTC", "ACGT"
    # span: q = c - m + 1 and c - 1 count, c - m and c do not; both strands
    P.plus("span eight q=c-m", eight, -8, span_eight=0, assay_eight=0)
    P.plus("span eight q=c-m+1", eight, -7, span_eight=1, assay_eight=1)
    for strand in (P.plus, P.minus):
        strand("span four q=c-m", four, -4, span_four=0, assay_four=0)
        strand("span four q=c-m+1", four, -3, span_four=1, assay_four=1)
        strand("span four q=c-1", four, -1, span_four=1, assay_four=1)
        strand("span four q=c", four, 0, span_four=0, assay_four=0)
    P.minus("span six q=c-1", six, -1, span_six=1, assay_six=1)
    P.minus("span six q=c", six, 0, span_six=0, assay_six=0, guide_six=1)
    # in-guide: a footprint flush with either end counts, one letter into the PAM or one past the 5' end does not
    P.plus("guide 5' flush", six, -17, guide_six=1)
    P.plus("guide 3' flush", six, -3, guide_six=1)
    P.plus("guide past 5'", six, -18, guide_six=0)
    P.plus("guide into PAM", six, -2, guide_six=0)
    P.minus("guide 3' flush", six, -3, guide_six=1)
    P.minus("guide 5' flush", six, 11, guide_six=1)
    P.minus("guide past 5'", six, 12, guide_six=0)
    P.minus("guide into PAM", six, -4, guide_six=0)
    # the sixteen-letter motif inside a guide, its footprint starting at plane bits 0, 48, 49 and 63 (the text lies at arena
    # offset 64: a string index and its arena position share the bit)
    for bit in (0, 48, 49, 63):
        base = ((P.at + 63) // 64) * 64 + 64 + bit
        P.put(base, LONG16)
        P.put(base + 20, "TGG")
        P.rows["+ sixteen at bit %d" % bit] = ("plus", base + 20)
        P.want.append(("+ sixteen at bit %d" % bit, "guide", "sixteen", 1))
        P.at = base + 220
    # the reverse strand alone
    P.plus("sixteen reverse", ref.rc_loop(LONG16), -17, guide_sixteen=1)
    P.minus("oneway reverse", "GAGACC", 0, guide_oneway=1, span_oneway=0)
    P.minus("oneway forward", "GGTCTC", -1, guide_oneway=1, span_oneway=1, assay_oneway=1)
    P.minus("seven reverse", "GAAGAGC", -2, span_seven=1, assay_seven=1)
    # motif N over a genome N: no occurrence; over a base: one.  U is A as packed; soft-masked letters match; an IUPAC letter of
    # the genome is no base
    P.plus("hinf N", "GANTC", -12, guide_hinf=0)
    P.plus("hinf base", "GAATC", -12, guide_hinf=1)
    P.plus("six U", "GAUTTC", -12, guide_six=1)
    P.plus("six soft", "gaATtc", -12, guide_six=1)
    P.plus("six IUPAC letter", "GARTTC", -12, guide_six=0)
    P.minus("bstn A", "CCAGG", 2, guide_bstn=1)
    P.minus("bstn T", "CCTGG", 2, guide_bstn=1)
    P.minus("bstn C", "CCCGG", 2, guide_bstn=0)
    # the amplicon's edge (flank 64): a second site whose footprint ends at c + 64 is inside, one letter further is outside;
    # one that starts at c - 64 is inside, one letter earlier is outside
    for what, q2, n in (("amp last inside hi", 64 - 6, 2), ("amp first outside hi", 64 - 5, 1), ("amp first inside lo", -64, 2),
                        ("amp last outside lo", -65, 1)):
        i = P.plus(what, six, -3, span_six=1, amp_six=n, assay_six=int(n == 1))
        P.put(i - 3 + q2, six)
        j = P.minus(what, six, -3, span_six=1, amp_six=n, assay_six=int(n == 1))
        P.put(j + 6 + q2, six)
    # two overlapping sites across the cut: ACACACA holds ACACA at 0 and at 2
    P.minus("overlapping", "ACACACA", -4, span_acaca=2, amp_acaca=2, assay_acaca=0)
    # the first letters of the text and its last m letters
    P.put(0, six)
    end = len(P.text)
    P.put(end - 40, "CCA")
    P.rows["- last letters"] = ("minus", end - 40)
    P.put(end - 6, six)
    assert P.at < end - 700
    return dict(name="planted", texts=[bytes(P.text)], l=20, flanks=[16, 64, 300, 100000], enzymes=PLANT_SET, rows=P.rows, want=P.want)


def _row(A, rows, what):
    strand, idx = rows[what]
    pos = A["pos_" + strand].astype(np.int64)
    at = np.flatnonzero(pos == idx + A["offsets"][0])
    assert at.size == 1, what
    return strand, int(at[0])


def check_planted(case, A):
    E = {n: e for e, (n, _) in enumerate(case["enzymes"])}
    assert sorted(set(len(m) for m in motifs(case))) == [4, 5, 6, 7, 8, 16]
    c64, c300 = reference(case, A, 64), reference(case, A, 300)
    for what, key, name, value in case["want"]:
        strand, r = _row(A, case["rows"], what)
        if key in ("span", "amp"):
            got = int(c64[strand][key][r, E[name]])
        else:
            got = int(c64[strand]["in_guide" if key == "guide" else "assay"][r]) >> E[name] & 1
        assert got == value, (what, key, name, got, value)
    assert len(case["want"]) > 70
    for b in (0, 48, 49, 63):
        strand, r = _row(A, case["rows"], "+ sixteen at bit %d" % b)
        assert (int(A["pos_plus"][r]) - 20) & 63 == b
    # the text's first and last letters hold a site; the last one is the only one in the amplicon of the last row
    occ = ref.occurrences_numpy(A["bytes"], "GAATTC")
    t0, t1 = A["bounds"][0]
    # (the text ends inside a plane word; the arena keeps a separator word behind its last text, so the successor word the
    # kernel reads for the halo always exists there and is void: the "no successor" branch is met by that void word alone)
    assert occ[t0] and occ[t1 - 6] and not occ[t1 - 5:].any() and (t1 & 63) != 0
    strand, r = _row(A, case["rows"], "- last letters")
    assert c300[strand]["amp"][r, E["six"]] == 1 and c300[strand]["span"][r, E["six"]] == 0
    for s in ("plus", "minus"):  # and the guard against empty masks, on both strands
        c = c64[s]
        assert (c["in_guide"] != 0).any() and (c["in_guide"] == 0).any() and (c["assay"] != 0).any(), s
        assert ((c["span"] >= 1) & (c["amp"] == 2)).any() and ((c["span"] == 0) & (c["amp"] == 1)).any(), s


# ------------------------------------------------------------------------------------------------ further cases
def iupac_case():
    """Each IUPAC motif letter against each base: GAT?ATC, fifteen enzymes, over a text that holds GAT + base + ATC for all four
    bases inside guides, and plain random text."""
    P = Planter(2703, 3000)
    for b in "ACGT":
        P.plus("base " + b, "GAT" + b + "ATC", -12)
        P.minus("base " + b, "GAT" + b + "ATC", 2)
    rng = np.random.default_rng(2704)
    return dict(name="iupac", texts=[bytes(P.text), rng.choice(SOFT, 6000).tobytes()], l=20, flanks=[16, 300], enzymes=IUPAC_SET, rows=P.rows)


def check_iupac(case, A):
    cols = reference(case, A, 300)
    for b in "ACGT":
        for sign in "+-":
            strand, r = _row(A, case["rows"], "%s base %s" % (sign, b))
            got = int(cols[strand]["in_guide"][r])
            want = sum(1 << e for e, (_, m) in enumerate(case["enzymes"]) if b in ref.IUPAC[m[3]] or ref.COMPLEMENT[b] in ref.IUPAC[m[3]])
            # (GAT?ATC read on the other strand is GAT comp(?) ATC: the letter matches b or its complement)
            assert got == want, (sign, b)
            assert 0 < bin(got).count("1") < 15


def length_cases():
    """l = 1 and l = 50 (and m > l at l = 1 .. 15) over the planted text and a random one."""
    rng = np.random.default_rng(2705)
    texts = [planted_case()["texts"][0][:6000], rng.choice(SOFT, 5000).tobytes()]
    return [dict(name="l=%d" % l, texts=texts, l=l, flanks=[16, 300], enzymes=PLANT_SET) for l in (1, 5, 50)]


def check_lengths(case, A):
    cols = reference(case, A, 300)
    both = np.concatenate([cols["plus"]["in_guide"], cols["minus"]["in_guide"]])
    longer = sum(1 << e for e, m in enumerate(motifs(case)) if len(m) > case["l"])
    assert not (both & np.uint32(longer)).any()
    if case["l"] == 50:
        assert (both != 0).any() and (both == 0).any()
    assert (np.concatenate([cols["plus"]["assay"], cols["minus"]["assay"]]) != 0).any()


TABLE_SET = [("aatt", "AATT"), ("ttaa", "TTAA"), ("atgga", "ATGGA"), ("tatat", "TATAT")]


def table_case(n):
    """Exactly n '+' rows beside an empty '-' table: A and T with n planted TGGA."""
    rng = np.random.default_rng(2706 + n)
    text = bytearray(rng.choice(AT, 40 + 12 * n + 40).tobytes())
    for k in range(n):
        text[40 + 12 * k:44 + 12 * k] = b"TGGA"
    return dict(name="%d rows" % n, texts=[bytes(text)], l=20, flanks=[16, 300], enzymes=TABLE_SET)


def check_table(case, A, n):
    assert A["pos_plus"].size == n and A["pos_minus"].size == 0
    c = reference(case, A, 16)["plus"]
    assert (c["in_guide"] != 0).any() and (c["assay"] != 0).any() and (c["assay"] == 0).any()


def one_enzyme_case():
    """E = 1, and a flank of the motif's own length: the planted text with ACGT alone."""
    return dict(name="one enzyme", texts=planted_case()["texts"], l=20, flanks=[4, 300], enzymes=[("four", "ACGT")])


def check_one(case, A):
    for flank in case["flanks"]:
        cols = reference(case, A, flank)
        for s in ("plus", "minus"):
            assert set(np.unique(cols[s]["in_guide"])) == {0, 1} and set(np.unique(cols[s]["assay"])) == ({0, 1} if flank == 4 else {0}), (s, flank)


def small_cases():
    """[(case, check)] of every case but the random one."""
    out = [(planted_case(), check_planted), (short_text_case(), check_short_text), (iupac_case(), check_iupac), (one_enzyme_case(), check_one)]
    out += [(c, check_lengths) for c in length_cases()]
    out += [(table_case(n), (lambda n: lambda case, A: check_table(case, A, n))(n)) for n in (64, 65, 256, 257)]
    return out
