"""Every term of the row predicate under every kernel that reads it.

cropsr_amd/csrc/crp_select_predicate.inc states once, for the device, whether a table row PASSES ("in the gene" apart).  Seven
kernels paste that text into their own row loop -- each with its own row, in, score and scored -- and the spaced selection reads
the key the pair pass kernel writes with it; each host entry point fills the predicate's tables and bounds with its own call of
fill_predicate.  Sharing the text does not make a kernel right, so here every kernel meets every term: tests/
select_predicate_reference.py states the predicate for the tests (twice), and each kernel's own reference takes the mask of
passing rows through the argument it already has.

Case genome: tests/high_position_cases.py without its filler (five contigs, 8.1 kb, six genes; test_high_positions.Case and
Placed produce every kernel's reference over it at the placement NO_FILLER).  The columns come from the references:
guide_properties_reference, repair_reference (flank 30), variant_reference.column_numpy over a seeded track in arena positions
(an interval per 50 letters, plus PLANTED), specificity_join_cases.join (M = 3, hsu2013) and annotate_oracle.host_join with
select_reference.cds_flags.

The cells -- kernel x term -- and the test that holds each.  M: test_gpu_cell here (K = 5, whole genes and slices of 64; K = 64
as well in the plain and spaced `all` cells), exact in n_in, n_pass and sel (pairs: n_pass, n_pairs, pairs; spaced: n_pass,
n_spaced, sel; step: gain, key, cover, gene, strand and row of every family's proposal, against nothing covered and against
what one greedy step covers).  Beside M, where another module held the cell before:

  kernel (file that includes the text)        min_score  specificity  require_cds  properties  repair  variants  all
  plain   (crp_select.hip)                    M s        M s h        M s          M p         M r     M v       M
  pairs   (crp_select_pairs.hip)              M q        M q          M q          M q         M q     M v       M q
  coding  (crp_select_coding.hip)             M c        M c          M c          M c         M       M v       M
  edit    (crp_select_edit.hip)               M e        M            M e          M e         M e     M         M
  splice  (crp_select_splice.hip)             M x        M            M x          M x         M x     M         M
  family  (crp_select_family.hip)             M f        M f          M f          M f         M f     M         M
  step    (crp_select_family_set.hip)         M          M            M            M           M       M         M
  spaced  (reads the pair pass key)           M d        M d          M d          M           M       M         M

  s test_select.py, h test_high_positions.py, p test_guide_properties.py, r test_repair_outcome.py, v test_variants.py,
  q test_select_pairs.py, c test_select_coding.py, e test_base_edit.py, x test_splice_edit.py, f test_families.py
  (test_gpu_family_limits_combined_with_the_other_limits), d test_select_spacing.py.  test_family_sets.py runs the step kernel
  under the family limit max_perfect_outside alone.

Each kernel has its own limit in force: coding CODING_LIMITS, edit window 4..8 and EDIT_LIMITS, splice the editor cbe and
SPLICE_LIMITS, family min_members = 2 and max_perfect_outside = 0, spaced D = 20, pairs the window 50..500.  The family and the
step kernel always read the joined columns, so an unjoined row fails in every one of their cells.  No cell is skipped: what
the library refuses -- pairs or the spaced selection with coding, edit, splice or family limits -- are kernels' own limits
against each other, not a kernel against a term.

No cell is vacuous (test_no_cell_is_vacuous, on the references alone): the term lowers n_pass in some gene, some gene keeps
passing rows, and -- min_score apart, which may only shorten a list from below -- the term changes some gene's picks.  The
thresholds are THRESHOLDS; CELL holds the cells that need another one on this genome, IN_ALL what `all` loosens so that a row
is left, each with what the common threshold gave.  Two kinds of cell need more than a threshold:
  require_cds under coding, edit, splice and step.  The term reads flags[feat[row]], and the flags are whatever bytes the host
    sets.  With the product's flags (a CDS label in the label set) these kernels' own limits already imply the term here, so the
    four cells set other bytes over the same label sets (CDS_BUT_TIE, ONE_CDS): the device reads the same column and the same
    array, and rows fail.  Every other cell with require_cds uses select_reference.cds_flags, `all` of these kernels too.
  splice x specificity.  The ten splice rows of this genome share one count and one hit sum.  The cell runs on the first two
    contigs of the splice kernel's own case genome (tests/splice_edit_cases.py; OWN_GENOME), with its own Matrix and Device.
The step's second covered word -- what one greedy step over the same candidates covers -- completes both families here, so
the expected proposals against it are "none": the kernel must find no gain.

test_gpu_genome_level_family_sets goes through scan_score(select=Request(...)) with family sets, a variant set read from a
VCF the test writes, max_seed_variants = 0, the property limits and require_cds: family_sets.py's own call of _set_row_limits.

test_every_including_kernel_has_its_row: a kernel that pastes the predicate must be named in INCLUDES, and so in the matrix."""
import os

import numpy as np
import pytest

import family_set_reference as fsr
import select_pairs_reference as pairs_ref
import select_predicate_reference as pred
import select_reference as selref
import select_spacing_reference as spaced_ref
import test_high_positions as thp
import variant_reference as vref
from cropsr_amd import annotate, baseedit, coding, properties, repair, variants
from cropsr_amd import families as fam
from cropsr_amd import search as srch
from cropsr_amd import select as sel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
L, SEED_LEN, FLANK = 20, 12, 30
K, K_ALL, SPACING = 5, 64, 20
EVERY = 10 ** 9
PAIR_WINDOW = thp.PAIR_WINDOW
CODING_LIMITS, EDIT_LIMITS, SPLICE_LIMITS, FAMILY_LIMITS = (5, 65, 0), (0, 100, 20), (0, 100, 20, "any"), thp.FAMILY_LIMITS
SETS = 3  # the genome-level run's S: the family of three

# the file that pastes crp_select_predicate.inc -> the matrix's name of its kernel; the spaced selection includes nothing
INCLUDES = {"crp_select.hip": "plain", "crp_select_pairs.hip": "pairs", "crp_select_coding.hip": "coding", "crp_select_edit.hip": "edit",
            "crp_select_splice.hip": "splice", "crp_select_family.hip": "family", "crp_select_family_set.hip": "step"}
KERNELS = ("plain", "pairs", "coding", "edit", "splice", "family", "step", "spaced")
TERMS = ("min_score", "specificity", "cds", "properties", "repair", "variants", "all")
READS_THE_JOIN = ("family", "step")  # their host calls refuse a run without the joined columns

THRESHOLDS = dict(min_score=dict(min_score=0.2),
                  specificity=dict(joined=True, max_mm0=thp.BOUNDS[0], max_hit_sum=thp.BOUNDS[1]),  # max_perfect 0, min_specificity 0.5
                  cds=dict(require_cds=True), properties=dict(props=(7, 14, 4, 3, 5)), repair=dict(repair=(300, 55)),
                  variants=dict(variants=(255, 255, 0, 0)))
# Flag bytes per label-set id of the case GFF (Matrix checks them against the strings) for the cells in which the product's
# flags -- a CDS label in the set -- cannot fail a row: a cut inside a gene's coding sequence, a stop codon or a splice site
# under the window all lie under a CDS label here, because the one-exon CDS of `tie` covers hp_tie's introns as well.
CDS_BUT_TIE = (1, 0, 0, 1, 0, 0, 1, 0)  # a CDS label other than CDS:tie: the introns of tie_introns are flagged 0
ONE_CDS = (0, 1, 0, 1, 0, 0, 1, 0)      # exactly one CDS label: the exons of tie_introns are flagged 0
# where the common threshold leaves a cell vacuous on this genome (what it left, beside each)
CELL = {
    ("coding", "cds"): dict(require_cds=CDS_BUT_TIE),  # n_pass unchanged in every gene
    ("edit", "cds"): dict(require_cds=ONE_CDS),        # likewise, and under CDS_BUT_TIE too: the planted stop lies in an exon
    ("splice", "cds"): dict(require_cds=CDS_BUT_TIE),  # likewise
    ("step", "cds"): dict(require_cds=ONE_CDS),        # both families' proposals unchanged: their best rows lie under a CDS
    ("edit", "repair"): dict(repair=(300, 65)),        # (300, 55) takes one row of sj_g0 and none of its five picks
    ("family", "repair"): dict(repair=(300, 60)),      # (300, 55) takes none of the eleven rows the family limits pass
    ("step", "repair"): dict(repair=(300, 73)),        # the proposals' rows have 72.0 % and 74.0 % out of frame
    ("step", "properties"): dict(props=(7, 12, 3, 2, 3)),  # (7, 14, 4, 3, 5) passes both proposals' rows
    # max_perfect 0 passes no row that hits a second family member with a perfect copy
    ("family", "specificity"): dict(joined=True, max_mm0=1, max_hit_sum=thp.BOUNDS[1]),
}
# The ten rows that pass the splice limits here all have one perfect copy and a hit sum of 0: no threshold tells them apart.
# The cell runs on the splice kernel's own case genome (tests/splice_edit_cases.py) with the common thresholds; in `all`, on
# this genome, the splice kernel gets a bound they meet.
OWN_GENOME = {("splice", "specificity"): "splice"}
# `all` ANDs the terms as the single cells have them, but for these: with them no row is left
IN_ALL = {("splice", "specificity"): dict(joined=True, max_mm0=1, max_hit_sum=thp.BOUNDS[1]),
          ("splice", "properties"): dict(props=(5, 15, 5, 4, 6)),   # three of the ten rows are left
          ("family", "specificity"): dict(joined=True, max_mm0=5, max_hit_sum=thp.BOUNDS[1])}  # one row of sj_g0 is left
# (contig, first index, last index) of intervals beside the seeded background
PLANTED = [(1, 199, 199)]  # under the PAM of tie_introns' best splice row ('-', j = 198): the background leaves its five picks clean


def limits_of(kernel, term):
    """The predicate's terms of a cell, as select_predicate_reference takes them; term None: the kernel without a term."""
    out = dict(joined=True) if kernel in READS_THE_JOIN else {}
    if term == "all":
        for t in TERMS[:-1]:
            out.update(IN_ALL.get((kernel, t)) or CELL.get((kernel, t)) or THRESHOLDS[t])
    elif term is not None:
        out.update(THRESHOLDS[term] if (kernel, term) in OWN_GENOME else CELL.get((kernel, term), THRESHOLDS[term]))
    return out


def variant_intervals(case, planted=()):
    """[(contig, s, e)] in string indices: per contig a seeded interval every 50 letters -- SNPs, some deletions of 2..12
    letters, some insertions (s, s - 1) -- and the planted ones; distinct."""
    rng = np.random.default_rng(2501)
    out = set(planted)
    for k, n in enumerate(case.lengths):
        for s in rng.integers(1, n - 13, n // 50).tolist():
            kind = rng.random()
            out.add((k, s, s) if kind < 0.8 else (k, s, s + int(rng.integers(1, 12))) if kind < 0.9 else (k, s, s - 1))
    return sorted(out)


def vcf_of(case, intervals):
    """The intervals as VCF records, anchored on the letter before where the alleles differ in length."""
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    letter = lambda k, i: chr(case.contigs[k][i]).upper() if chr(case.contigs[k][i]).upper() in "ACGT" else "N"
    for k, s, e in intervals:
        if e == s:
            ref_, alt = letter(k, s), "ACGT"[("ACGTN".index(letter(k, s)) + 1) % 4]
            pos = s + 1
        elif e < s:
            ref_, alt, pos = letter(k, s - 1), letter(k, s - 1) + "GA", s
        else:
            ref_, alt, pos = "".join(letter(k, i) for i in range(s - 1, e + 1)), letter(k, s - 1), s
        lines.append("%s\t%d\t.\t%s\t%s\t50\tPASS\t." % (case.names[k], pos, ref_, alt))
    return ("\n".join(lines) + "\n").encode()


def _as_cds(mask, n_plus):
    """select_numpy and spaced_numpy take no extra mask: the passing rows stated as their CDS filter (test_variants.py's trick)."""
    return dict(feat_plus=mask[:n_plus].astype(np.uint32), feat_minus=mask[n_plus:].astype(np.uint32), flags=np.array([0, 1], np.uint8))


class Matrix:
    """The case genome without a filler, its columns from the references, and every cell's expected result: computed once."""

    def __init__(self, case, planted=()):
        self.case, self.p = case, case.placed(thp.NO_FILLER)
        p = self.p
        self.intervals = variant_intervals(case, planted)
        self.track = vref.track([(s + p.offsets[k], e + p.offsets[k]) for k, s, e in self.intervals])
        t = p.tables
        var = (vref.column_numpy(t["pos_plus"], False, L, SEED_LEN, *self.track), vref.column_numpy(t["pos_minus"], True, L, SEED_LEN, *self.track))
        strings = case.annotation.strings
        self.flags = selref.cds_flags([strings[i] for i in range(len(strings))])
        self.cols = pred.columns(t, p.spec(), (p.cat(case.features(), 0), p.cat(case.features(), 1)), self.flags,
                                 (p.cat(case.props(), 0), p.cat(case.props(), 1)), (p.cat(case.repair(FLANK), 0), p.cat(case.repair(FLANK), 1)), var)
        self.n_plus = p.n_plus
        self._cache = {}

    def mask(self, limits):
        return pred.mask_numpy(self.cols, limits)

    def candidates(self, limits):
        """(candidates of family_set_reference, n_pass per gene of the GFF) over the rows that pass `limits`."""
        import test_families as tf
        c, p, mask = self.case, self.p, self.mask(limits)
        fam_ref = c.family_rows(3)
        row_of = {s: r for r, s in enumerate(fam_ref["sites"])}
        also = lambda kc, strand, i: mask[int(p.rows_before["minus" if strand else "plus"][kc]) + i + (self.n_plus if strand else 0)]
        want = tf._reference_selection(c, c.hits, c.join(3, "hsu2013"), fam_ref, row_of, EVERY, also=also)
        passing = [[(kc, pos, st, r, i) for (kc, pos, st, _, r), i in zip(w[2], w[3])] for w in want]
        key_of = lambda kc, st, i: int(np.float64(c.hits[kc]["score_minus" if st else "score_plus"][i]).view(np.uint64))
        cands = fsr.candidates(c.genes, c.gene_family, c.gene_member, passing, fam_ref, {k: 0 for k in range(len(c.contigs))}, key_of)
        return cands, [w[1] for w in want]

    def step(self, limits):
        """(n_pass per gene, [(covered words, per family None or (gain, key, cover, gene, strand, row as sel packs it))]) against
        nothing covered and against what one greedy step over these candidates covers."""
        c, p = self.case, self.p
        cands, n_pass = self.candidates(limits)
        after = {pick["family"]: pick["covered"] for pick in fsr.greedy_loop(cands, c.sizes, 1)[0]}
        out = []
        for covered in ([0] * len(c.sizes), [after.get(f, 0) for f in range(len(c.sizes))]):
            best = fsr.arena_best(cands, c.sizes, covered, 0)
            out.append((covered, [None if b is None else (b["gain"], b["key"], b["cover"], b["gene"], b["strand"],
                                                           int(p.rows_before["minus" if b["strand"] else "plus"][b["contig"]]) + b["index"] | b["strand"] << 31)
                                  for b in best]))
        return n_pass, out

    def want(self, kernel, term, k=K):
        """The cell's expected result (term None: the kernel with its own limit alone)."""
        return self.expected(kernel, limits_of(kernel, term), k)

    def expected(self, kernel, limits, k):
        key = (kernel, tuple(sorted(limits.items())), k)
        if key not in self._cache:
            self._cache[key] = self._expected(kernel, limits, k, key)
        return self._cache[key]

    def _expected(self, kernel, limits, k, key):
        c, p, mask = self.case, self.p, self.mask(limits)
        t = p.tables
        if kernel == "plain":
            return selref.select_numpy(t, p.lo, p.hi, k, 0.0, None, _as_cds(mask, self.n_plus))
        if kernel == "pairs":
            return pairs_ref.pairs_numpy(t, p.lo, p.hi, k, *PAIR_WINDOW, also=dict(plus=mask[:self.n_plus], minus=mask[self.n_plus:]))
        if kernel == "coding":
            return thp.cref.select_numpy(t, p.lo, p.hi, c.models, p.rows, k, CODING_LIMITS, ok=mask, positions=p.positions())
        if kernel == "edit":
            return thp.eref.select_numpy(p.local_tables, p.member, c.models, p.local_rows, k, p.edits(), EDIT_LIMITS, ok=mask)
        if kernel == "splice":
            return thp.spref.select_numpy(p.local_tables, p.member, c.models, p.local_rows, k, p.splices(), SPLICE_LIMITS, ok=mask)
        if kernel == "family":
            return p.select_family(k, FAMILY_LIMITS, also=mask, key=key)[:3]
        if kernel == "step":
            return self.step(limits)
        assert kernel == "spaced"
        return spaced_ref.spaced_numpy(t, p.lo, p.hi, k, SPACING, 0.0, None, _as_cds(mask, self.n_plus))


def n_pass_of(kernel, result):
    return np.asarray(result[0 if kernel in ("pairs", "spaced", "step") else 1], np.int64)


def picks_of(kernel, result):
    return repr(result[1]) if kernel == "step" else np.asarray(result[2]).tobytes()


@pytest.fixture(scope="module")
def matrix(oracle, tmp_path_factory):
    return Matrix(thp.Case(oracle, tmp_path_factory.mktemp("predicate_matrix")), PLANTED)


def _splice_case(orc):
    """The first two contigs of tests/splice_edit_cases.py (36 kb, 61 genes) as a dict of high_position_cases.build's keys."""
    import splice_edit_cases
    b = splice_edit_cases.build(orc)
    names = b["names"][:2]
    gff = "\n".join(line for line in b["gff"].split("\n") if line.startswith("#") or line.split("\t")[0] in names) + "\n"
    genes = [(label[len("gene:"):], names.index(seqid), max(start - 1, 0), min(end - 1, len(b["contigs"][names.index(seqid)]) - 1))
             for seqid, start, end, label in selref.gff_genes(gff)]
    return dict(contigs=b["contigs"][:2], names=names, hits=b["hits"][:2], gff=gff, genes=genes, families="", guides=[])


@pytest.fixture(scope="module")
def own(oracle, tmp_path_factory):
    """name -> the Matrix over a kernel's own case genome, for the cells of OWN_GENOME."""
    assert set(OWN_GENOME.values()) == {"splice"}
    return dict(splice=Matrix(thp.Case(oracle, tmp_path_factory.mktemp("predicate_matrix_splice"), built=_splice_case(oracle))))


def _genome_level_limits():
    """require_cds, the property limits and max_seed_variants = 0, behind the joined columns the family sets read."""
    return dict(joined=True, require_cds=True, props=THRESHOLDS["properties"]["props"], variants=(255, 255, 0, 255))


def _limit_sets():
    sets = [limits_of(kernel, term) for kernel in KERNELS for term in (None,) + TERMS]
    sets.append(_genome_level_limits())
    return [dict(s) for s in {tuple(sorted(s.items())) for s in sets}]


# ---------------------------------------------------------------------------------------------- without a GPU
def test_numpy_and_loop_agree(matrix, own):
    """The two statements of the predicate on the case genome's columns for every set of limits a test here uses, and on the
    hand-made rows that hold the packing's edges, where the expected mask is written out."""
    for limits in _limit_sets():
        a, b = pred.mask_numpy(matrix.cols, limits), pred.mask_loop(matrix.cols, limits)
        assert np.array_equal(a, b), limits
        assert a.any() and not a.all(), limits  # (rows without a score pass nothing)
    for (kernel, term), name in OWN_GENOME.items():
        limits = limits_of(kernel, term)
        assert np.array_equal(pred.mask_numpy(own[name].cols, limits), pred.mask_loop(own[name].cols, limits)), (kernel, term)
    cols, cases = pred.edge_rows()
    for limits, want in cases:
        assert pred.mask_numpy(cols, limits).tolist() == want, limits
        assert pred.mask_loop(cols, limits).tolist() == want, limits


def test_the_columns_hold_every_terms_both_outcomes(matrix):
    """Every single term passes rows and fails rows among the scored rows of the case genome; the columns hold unjoined rows
    and rows without a label set (mh = 0 is among select_predicate_reference.edge_rows: no window of this genome is without
    a microhomology); the cells' own flag bytes are what their comments say; and the VCF that the genome-level run reads lays
    out to the very track the cells use."""
    c, p, cols = matrix.case, matrix.p, matrix.cols
    scored = cols["score"] != -1.0
    assert scored.sum() > 800 and len(c.contigs) == 5 and sum(c.lengths) > 8000 and len(c.genes) == 6
    for term in TERMS[:-1]:
        m = matrix.mask(THRESHOLDS[term])
        assert 20 < m.sum() < scored.sum() - 20, term
    assert ((cols["counts0"] == NONE) & scored).sum() >= 5 and ((cols["feat"] == NONE) & scored).sum() >= 5
    strings = [c.annotation.strings[i].split(";") for i in range(len(c.annotation.strings))]
    assert CDS_BUT_TIE == tuple(int(any(lab.startswith("CDS:") and lab != "CDS:tie" for lab in labs)) for labs in strings)
    assert ONE_CDS == tuple(int(sum(lab.startswith("CDS:") for lab in labs) == 1) for labs in strings)
    kinds = [(e == s, e > s, e < s) for _, s, e in matrix.intervals]
    assert all(sum(k[i] for k in kinds) >= 5 for i in range(3)) and abs(len(kinds) - sum(c.lengths) // 50) <= 5 + len(PLANTED)
    chroms, stats = vref.read_vcf(vcf_of(c, matrix.intervals))
    assert stats["alleles"] == len(matrix.intervals)
    starts, ends1 = vref.track(vref.layout(chroms, p.entries, 0))
    assert np.array_equal(starts, matrix.track[0]) and np.array_equal(ends1, matrix.track[1])


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_cell_is_vacuous(matrix, own, kernel):
    """On the references alone, for every term: it lowers n_pass in some gene, some gene keeps passing rows, and -- every term
    but min_score -- some gene's picks (the step's proposals) are not those of the same kernel without the term."""
    for term in TERMS:
        m = own[OWN_GENOME[(kernel, term)]] if (kernel, term) in OWN_GENOME else matrix
        base, got = m.want(kernel, None), m.want(kernel, term)
        a, b = n_pass_of(kernel, got), n_pass_of(kernel, base)
        assert (a <= b).all() and (a < b).any(), (kernel, term, "lowers n_pass nowhere")
        assert (a > 0).any(), (kernel, term, "passes nothing")
        if term != "min_score":
            assert picks_of(kernel, got) != picks_of(kernel, base), (kernel, term, "changes no pick")
    if kernel in ("plain", "spaced"):  # K = 64 in the `all` cells
        assert picks_of(kernel, matrix.want(kernel, "all", K_ALL)) != picks_of(kernel, matrix.want(kernel, None, K_ALL))
        assert (np.asarray(matrix.want(kernel, "all", K_ALL)[2]) != NONE).sum(axis=1).max() > K


def test_the_genome_level_limits_change_the_sets(matrix):
    """test_gpu_genome_level_family_sets is not vacuous: its limits change the greedy sets, and each of require_cds, the
    property limits and max_seed_variants = 0 takes candidates away on its own."""
    c = matrix.case
    limits = _genome_level_limits()
    cands, n_pass = matrix.candidates(limits)
    free, n_free = matrix.candidates(dict(joined=True))
    picks, complete = fsr.greedy_loop(cands, c.sizes, SETS)
    assert picks and picks != fsr.greedy_loop(free, c.sizes, SETS)[0] and sum(n_pass) < sum(n_free)
    for single in (dict(joined=True, require_cds=True), dict(joined=True, props=limits["props"]), dict(joined=True, variants=limits["variants"])):
        assert sum(matrix.candidates(single)[1]) < sum(n_free), single


def test_every_including_kernel_has_its_row():
    """The files under cropsr_amd/csrc that paste the predicate are exactly the ones the matrix names: a new kernel that
    includes the text fails here until it has a row (INCLUDES, KERNELS, limits_of, the cell test)."""
    csrc = os.path.join(ROOT, "cropsr_amd", "csrc")
    have = set()
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".cpp", ".h", ".inc")):
            with open(os.path.join(csrc, name)) as f:
                if any(line.lstrip().startswith("#include") and "crp_select_predicate.inc" in line for line in f):
                    have.add(name)
    assert have == set(INCLUDES)
    assert set(INCLUDES.values()) | {"spaced"} == set(KERNELS) and len(set(INCLUDES.values())) == len(INCLUDES)


# ---------------------------------------------------------------------------------------------- on the GPU
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


class Device:
    """The case genome resident with every column the predicate reads -- each checked against the reference's once -- and
    the arena's self-search handle with the plain and the family join."""

    def __init__(self, engine, m):
        c, p = m.case, m.p
        self.genome = engine.genome(c.contigs)
        self.handles = []
        try:
            assert len(self.genome.arenas) == 1
            self.arena = self.genome.arenas[0]
            assert [int(o) for o in self.arena.offsets] == p.offsets
            self.request = annotate.Request(c.annotation, c.names, 0)
            hits = self.genome.scan_score(L)
            h = hits.per_arena[0]
            for key in ("pos_plus", "pos_minus", "score_plus", "score_minus"):
                assert np.array_equal(getattr(h, key).view(np.uint8), p.tables[key].view(np.uint8)), key
            counts = [(h.n_plus, h.n_minus)]
            n = m.n_plus
            same = lambda got, name: np.array_equal(got[0], m.cols[name][:n]) and np.array_equal(got[1], m.cols[name][n:])
            assert same(self.genome.annotate(self.request, counts)[0], "feat")
            self.flags = c.annotation.cds_flags()
            assert np.array_equal(np.asarray(self.flags, np.uint8), m.flags)
            assert same(self.genome.guide_properties(counts)[0], "props")
            assert same(self.genome.repair_scores(counts, FLANK)[0], "repair")
            self.arena.variant_set_track(*m.track)
            assert same(self.arena.variant_counts(h.n_plus, h.n_minus, SEED_LEN), "variants")
            self.table = thp._family_table(c) if c.families else None
            pattern, gp, M, scheme = srch.check_specificity(L, 3)
            srch._self_handles(self.genome, pattern, gp, srch.SPECIFICITY_PAM_LEN, M, scheme, None, None, self.handles)
            srch._self_compare_all(self.handles, M)
            if self.table is not None:
                srch._family_compare_all(self.handles, fam.genome_rows(self.table, self.genome, self.request), 0)
            self.handles[0].join_hits(L)
            if self.table is not None:
                self.handles[0].family_join_hits(L)
            lo, hi, gene = self.request.gene_layout(sel.arena_layout(self.genome, 0))
            assert np.array_equal(lo, p.lo) and np.array_equal(hi, p.hi) and np.array_equal(gene, p.gene)
        except BaseException:
            self.close()
            raise

    def close(self):
        for x in self.handles:
            x.close()
        self.genome.close()


@pytest.fixture(scope="module")
def dev(engine, matrix):
    d = Device(engine, matrix)
    yield d
    d.close()


@pytest.fixture(scope="module")
def own_dev(engine, own):
    devices = {}
    try:
        for name, m in own.items():
            devices[name] = Device(engine, m)
        yield devices
    finally:
        for d in devices.values():
            d.close()


def _params(k, limits):
    params = sel.Params(k, limits.get("min_score", 0.0), require_cds=bool(limits.get("require_cds")))
    params.max_mm0, params.max_hit_sum = limits.get("max_mm0", sel.NO_BOUND_MM0), limits.get("max_hit_sum", sel.NO_BOUND_SUM)
    return params


def _set_limits(h, dev, limits):
    if limits.get("require_cds"):
        h.set_flags(dev.flags if limits["require_cds"] is True else np.array(limits["require_cds"], np.uint8))
    h.set_property_limits(properties.Limits(*limits["props"]) if "props" in limits else None)
    h.set_repair_limits(repair.Limits(*limits["repair"]) if "repair" in limits else None)
    h.set_variant_limits(variants.Limits(*limits["variants"]) if "variants" in limits else None)


RESULT = dict(pairs=("n_pass", "n_pairs", "pairs"), spaced=("n_pass", "n_spaced", "sel"))  # every other kernel: n_in, n_pass, sel


def _same(kernel, got, want, what):
    assert len(got) == len(want) == 3
    for g, w, name in zip(got, want, RESULT.get(kernel, ("n_in", "n_pass", "sel"))):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and np.array_equal(g.astype(np.uint64), w.astype(np.uint64)), (what, name)


@pytest.mark.gpu
@thp.SLICES
@pytest.mark.parametrize("term", TERMS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_gpu_cell(request, dev, matrix, kernel, term, slice_rows):
    """One cell: the kernel with its own limit and the term's limits on an ArenaSelect of the resident case genome, whole genes
    and slices of 64, every number against the kernel's reference over the rows select_predicate_reference passes."""
    if (kernel, term) in OWN_GENOME:  # the cell's own case genome, device and all
        name = OWN_GENOME[(kernel, term)]
        dev, matrix = request.getfixturevalue("own_dev")[name], request.getfixturevalue("own")[name]
    p = matrix.p
    limits = limits_of(kernel, term)
    joined = dev.handles[0] if limits.get("joined") else None
    h = sel.ArenaSelect(dev.arena, p.lo, p.hi)
    try:
        if slice_rows:
            h.set_limits(slice_rows)
            h.set_pair_limits(slice_rows)
        _set_limits(h, dev, limits)
        ks = (K, K_ALL) if term == "all" and kernel in ("plain", "spaced") else (K,)
        if kernel in ("coding", "edit", "splice"):
            h.set_coding(dev.request.coding_layout(sel.arena_layout(dev.genome, 0)))
        if kernel == "coding":
            h.set_coding_limits(coding.Limits(*CODING_LIMITS))
        elif kernel == "edit":
            h.set_edit_limits(baseedit.Window(*thp.WINDOW), baseedit.Limits(*EDIT_LIMITS))
        elif kernel == "splice":
            h.set_splice_limits(baseedit.Window(*thp.WINDOW), "cbe", baseedit.SpliceLimits(*SPLICE_LIMITS))
        elif kernel in ("family", "step"):
            g = np.asarray(p.gene, np.int64)
            h.set_family(dev.table.gene_family[g], np.array([dev.table.family_size(int(x)) for x in g], np.uint32))
            if kernel == "family":
                h.set_family_limits(sel.FamilyLimits(**FAMILY_LIMITS))
            else:
                h.set_family_members(dev.table.gene_member[g])
        for k in ks:
            what = "%s x %s, K = %d" % (kernel, term, k)
            want = matrix.want(kernel, term, k)
            if kernel == "pairs":
                h.run_pairs(_params(1, limits), sel.PairParams(k, *PAIR_WINDOW), joined)
                _same(kernel, h.fetch_pairs(), want, what)
            elif kernel == "spaced":
                h.run_spaced(_params(k, limits), SPACING, joined)
                _same(kernel, h.fetch_spaced(), want, what)
            elif kernel == "step":
                n_pass, steps = want
                for covered, best_want in steps:
                    best = h.family_step(_params(1, limits), joined, np.array(covered, np.uint64))
                    for f, w in enumerate(best_want):
                        if w is None:
                            assert best["gain"][f] == 0, (what, covered, f)
                            continue
                        got = (int(best["gain"][f]), int(best["key"][f]), int(best["cover"][f]), int(p.gene[int(best["gene"][f])]),
                               int(best["row"][f]) >> 31, int(best["row"][f]))
                        assert got == w and int(best["tie"][f]) & 1 == w[4], (what, covered, f)
                # the candidates are the rows behind n_pass: the plain run of the same handle counts them
                h.run(_params(1, limits), joined)
                assert np.array_equal(h.fetch()[1], np.asarray(n_pass, np.uint32)[np.asarray(p.gene, np.int64)]), what
            else:
                h.run(_params(k, limits), joined)
                _same(kernel, h.fetch(), want, what)
                if slice_rows and kernel == "plain":
                    assert h.stats()["merged_genes"] == thp._merged_genes(p, slice_rows) >= 4
    finally:
        h.close()


@pytest.mark.gpu
def test_gpu_genome_level_family_sets(engine, matrix, tmp_path):
    """scan_score(select=Request(...)) with family sets, a VariantSet read from a VCF, max_seed_variants = 0, the property
    limits and require_cds against greedy_loop over the candidates that pass the same terms: family_sets.py's own
    _set_row_limits, and the variant column by way of the reader and the genome's layout."""
    c, p = matrix.case, matrix.p
    limits = _genome_level_limits()
    cands, n_pass = matrix.candidates(limits)
    want, complete = fsr.greedy_loop(cands, c.sizes, SETS)
    path = tmp_path / "cultivar.vcf"
    path.write_bytes(vcf_of(c, matrix.intervals))
    vs = variants.VariantSet(str(path))
    g = engine.genome(c.contigs)
    try:
        areq = annotate.Request(c.annotation, c.names, 0)
        gc_min, gc_max, max_run, max_t_run, max_stem = limits["props"]
        req = sel.Request(sel.Params(K, require_cds=True), areq, families=thp._family_table(c), family_sets=SETS,
                          variants=variants.Request(vs, c.names, 0), max_seed_variants=0, gc_min=gc_min, gc_max=gc_max, max_run=max_run,
                          max_t_run=max_t_run, max_stem=max_stem)
        hits = g.scan_score(L, specificity={}, select=req)
        S = hits.selection
        n = matrix.n_plus
        assert np.array_equal(hits.variants[0][0], matrix.cols["variants"][:n]) and np.array_equal(hits.variants[0][1], matrix.cols["variants"][n:])
        assert S.n_pass.tolist() == n_pass
        have = [(int(x["family"]), int(x["step"]), int(x["gene"]), int(x["contig"]), int(x["position"]), x["strand"], int(x["index"]), int(x["gain"]),
                 int(x["cover"]), int(x["covered"]), int(np.float64(x["score"]).view(np.uint64))) for x in S.family_sets]
        assert have == [(x["family"], x["step"], x["gene"], x["contig"], x["position"], b"+-"[x["strand"]:x["strand"] + 1], x["index"], x["gain"],
                         x["cover"], x["covered"], x["key"]) for x in want]
        assert S.family_complete.tolist() == list(complete) and len(have) > 0
    finally:
        g.close()
        vs.close()
