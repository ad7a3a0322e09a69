"""Arena positions with bit 30 set: the post-scan kernels behind a filler contig (tests/high_position_cases.py), at two
placements -- "straddle", where arena position 2^30 falls between the two copies of the tie contig's block, and "top", where the
arena is as long as the library accepts and every case position lies within 2^20 of 2^31.  Expected values come from the suite's
references run on the case contigs alone (results are contig-relative); every comparison is exact.  The tests without a GPU
prove on the references' own rows that the GPU tests are not vacuous: the ties, the keys on both sides of 2^30, the windows
that reach past the last text word.

Covered on the GPU, each at both placements on one upload and one scan: the hit tables; guide properties and repair scores;
the annotation look-up; the off-target seeds and counts; the given-guide searches (plain, scored, pair table, bulges); the self
search and the specificity join; the family rows, join and selection; the plain, pair, coding, edit and splice selections and
their evaluation kernels; the selection behind the join; the variant counts; the family step; the restriction-site planes,
ranks and columns (crp_sites.hip: eight enzymes of tests/high_position_site_cases.py, every flank, the index over every word of
the arena, and the plain selection over the resident column); the spaced selection (crp_select_spaced.hip); the distinct
pairs (crp_select_pairs_distinct.hip); and the self selection (crp_select_self.hip), at the handle and through
search.search_self(select=...)."""
import numpy as np
import pytest

import base_edit_reference as eref
import family_reference as fref
import family_set_reference as fsr
import guide_properties_reference as gref
import high_position_cases as hp
import high_position_site_cases as hs
import repair_reference as rref
import search_bulge_reference as bref
import search_pair_reference as pref
import search_reference as ref
import search_score_reference as sref
import search_self_reference as selfref
import select_coding_reference as cref
import select_pairs_distinct_reference as dref
import select_pairs_reference as pairs_ref
import select_reference as selref
import select_self_cases as self_cases
import select_self_reference as ssref
import select_spacing_reference as spacing_ref
import site_reference as site_ref
import specificity_join_cases as join_cases
import splice_edit_reference as spref
import variant_reference as vref
from cropsr_amd import _native as nat
from cropsr_amd import annotate, baseedit, coding
from cropsr_amd import families as fam
from cropsr_amd import search as srch
from cropsr_amd import select as sel
from cropsr_amd import select_self as ss
from cropsr_amd import sites

NONE = 0xFFFFFFFF
L = 20
KS = (1, 5, 33, 64)             # 5 and 33 are odd and below the tie gene's 52 pairs: the K-th pick and the first row left out tie
TIE_KS = (1, 5, 33)
KP = (1, 5)
PAIR_WINDOW = (50, 500)
FLANKS = (30, 32)
PATTERN, GUIDE_PATTERN, SPCAS9 = "N" * L + "NRG", "N" * L + "NGG", "N" * 21 + "GG"
WINDOW = (4, 8)
CODING_LIMITS = (None, (0, 100, 0), (5, 65, 0))
EDIT_LIMITS = (None, (0, 100, 20))
SPLICE_LIMITS = (None, (0, 100, 20, "any"))
FAMILY_LIMITS = dict(min_members=2, max_perfect_outside=0)
FAMILY_TIE_LIMITS = dict(min_members=1)  # every joined row passes: the tie gene's pairs decide in the family item kernel
BOUNDS = (0, sel.max_hit_sum_for(0.5))  # max_perfect 0, min_specificity 0.5
VARIANT_SEED = 12
ALL_ONES = (1 << 64) - 1
NO_FILLER = "no-filler"  # Case.layout's third placement: the case contigs alone (tests/test_select_predicate_matrix.py); not in hp.PLACEMENTS
TWIN = hp.COPY[1] - hp.COPY[0]  # a row of the tie block and its twin in the other copy lie exactly this far apart
SPACINGS = (0, 1, 30, TWIN, TWIN + 1)
KP_DISTINCT = (1, 5, 33)
SELF_T, SELF_P, SELF_CUT = L + 3, 3, 17  # PATTERN's geometry: the cut letter is i - 3 of a '+' site and j + 6 of a '-' site
SELF_REGION = ssref.region_mask(SELF_T, SELF_P, True)
SELF_HANDLES = [(0, True), (0, False), (3, True), (3, False)]  # (M, scored)
# the limit runs of the self selection, and n_pass of every layout row under each (None: no limit; without mismatches every
# hit sum is 0 and the bound drops nothing) -- test_self_selection_holds_its_cases
SELF_LIMITS = dict(perfect=dict(max_mm0=0), hit_sum=dict(max_hit_sum=BOUNDS[1]), sequence=dict(gc_min=9, gc_max=12, max_t_run=2), cds=dict(cds=True))
SELF_N_PASS = {None: [362, 107, 107, 110, 149, 21], "perfect": [357, 0, 0, 104, 146, 21], "hit_sum": [358, 107, 107, 108, 147, 21],
               "sequence": [144, 28, 28, 64, 62, 12], "cds": [227, 107, 107, 0, 122, 0]}
# of the tie gene's 107 guide sites, this many of the first copy and one fewer of the second share the best e: at this K the
# K-th site and the first one left out lie on either side of 2^30, below it both lie in the first copy
SELF_TIE_K = {0: 54, 3: 53}


class Case:
    """The case contigs, their GFF and what the references say about them: computed once, never changed."""

    def __init__(self, orc, tmp, built=None):
        """built: None for hp.build(orc), or another case genome as a dict of hp.build's keys."""
        self.__dict__.update(hp.build(orc) if built is None else built)
        self.orc = orc
        self.lengths = [len(t) for t in self.contigs]
        self.gff_path = str(tmp / "cases.gff")
        with open(self.gff_path, "w") as f:
            f.write(self.gff)
        self.annotation = annotate.Annotation(self.gff_path)
        self.gff_genes = selref.gff_genes(self.gff)
        self.models = cref.model_numpy(self.gff)
        self.idents = [g[0] for g in self.genes]
        self.fam_names, self.gene_family, self.gene_member, self.sizes, _ = fref.table(fref.parse(self.families), self.idents)
        self.max_words = int(nat.lib().crp_arena_max_words())
        self.pair = join_cases.pair_table(L)
        self._cache = {}

    def once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    # ---- the layout
    def layout(self, placement):
        """(filler length, offsets of the case contigs, words of the arena) by the restated rule."""
        if placement == NO_FILLER:
            return (0,) + hp.offsets_of(self.lengths)
        n = hp.filler_length(placement, self.lengths, self.max_words)
        offsets, words = hp.offsets_of([n] + self.lengths)
        return n, offsets[1:], words

    def placed(self, placement):
        return self.once(("placed", placement), lambda: Placed(self, placement))

    # ---- per contig
    def props(self):
        return self.once("props", lambda: [(gref.column_numpy(t, h["pos_plus"], False, L), gref.column_numpy(t, h["pos_minus"], True, L))
                                           for t, h in zip(self.contigs, self.hits)])

    def repair(self, F):
        return self.once(("repair", F), lambda: [(rref.column_numpy(t, h["pos_plus"], False, F), rref.column_numpy(t, h["pos_minus"], True, F))
                                                 for t, h in zip(self.contigs, self.hits)])

    def features(self):
        from oracle import annotate_oracle
        return self.once("features", lambda: [annotate_oracle.host_join(self.annotation, n, 0, 0, h, L, len(t))
                                              for n, t, h in zip(self.names, self.contigs, self.hits)])

    def offtarget(self):
        return self.once("offtarget", lambda: self.orc.offtarget_genome(self.contigs, L))

    # ---- the searches
    def queries(self):
        """The three planted guides of the join genome, and the guide of a '+' row in the middle of the tie block."""
        h = self.hits[hp.TIE]
        i = int(h["pos_plus"][len(hp.tie_pairs(self.hits, "plus")) // 2])
        guides = [g.decode() for g in self.guides] + [self.contigs[hp.TIE][i - L:i].decode()]
        return [srch.check_query(SPCAS9, g, 3) for g in guides]

    def search(self, kind, M):
        def make():
            q = self.queries()
            if kind == "plain":
                counts, s = ref.search(self.contigs, SPCAS9, q, M)
                return counts, s, None
            assert kind == "hsu2013"
            return sref.search(self.contigs, SPCAS9, q, M, 3, *sref.tables(sref.W_HSU))
        return self.once(("search", kind, M), make)

    def search_pair(self, M):
        def make():
            pair, pam = pref.random_table(np.random.default_rng(77), SPCAS9, 3, (1, 2))
            return (pair, pam), pref.search(self.contigs, SPCAS9, self.queries(), M, 3, pair, (1, 2), pam)
        return self.once(("search_pair", M), make)

    def bulges(self, M):
        return self.once(("bulges", M), lambda: bref.search(self.contigs, SPCAS9, self.queries(), M, 3, 1, 1))

    def self_search(self, M, scored):
        return self.once(("self", M, scored), lambda: selfref.search_self(self.contigs, PATTERN, M, 3, GUIDE_PATTERN, sref.W_HSU if scored else None))

    def self_columns(self, M, scored):
        """The rows of self_search(M, scored) as select_self_reference takes them, but for the arena positions: contig, forward
        start in the contig, strand, hi, lo (the guide's letters, A = 00 T = 01 C = 10 G = 11, letter k at bit k), counts, hit_sum."""
        def make():
            sites, guides, counts, hit_sum = self.self_search(M, scored)
            code = {"A": 0, "T": 1, "C": 2, "G": 3}
            hi = np.array([sum((code[ch] >> 1) << k for k, ch in enumerate(g)) for g in guides], np.uint32)
            lo = np.array([sum((code[ch] & 1) << k for k, ch in enumerate(g)) for g in guides], np.uint32)
            contig, start, strand = (np.array(x, np.int64) for x in zip(*sites))
            return dict(contig=contig, start=start, strand=strand.astype(np.uint8), hi=hi, lo=lo, counts=np.asarray(counts, np.uint32),
                        hit_sum=None if hit_sum is None else np.array([int(x) for x in hit_sum], np.uint64))
        return self.once(("self_columns", M, scored), make)

    def enzymes(self):
        return self.once("enzymes", lambda: hs.enzymes(self.contigs, self.hits))

    def join(self, M, kind):
        score = {"none": None, "hsu2013": "hsu2013", "pair": self.pair}[kind]
        return self.once(("join", M, kind), lambda: join_cases.join(self.hits, join_cases.rows(self.contigs, L, M, "NRG", score), L, M))

    def family_rows(self, M, C=0):
        return self.once(("family", M, C), lambda: fref.family_rows(self.contigs, PATTERN, M, GUIDE_PATTERN, self.genes, self.gene_family,
                                                                     self.gene_member, C, ("weights", sref.W_HSU)))

    def step_candidates(self):
        """The candidates of the family sets (family_set_reference.FIELDS; contig-relative, every contig in arena 0): every
        joined, scored row of every family gene, from the family tests' plain loop (M = 3, hsu2013, no limits)."""
        import test_families as tf

        def make():
            fam_ref = self.family_rows(3)
            row_of = {s: r for r, s in enumerate(fam_ref["sites"])}
            want = tf._reference_selection(self, self.hits, self.join(3, "hsu2013"), fam_ref, row_of, 10 ** 9)
            passing = [[(kc, pos, st, r, i) for (kc, pos, st, _, r), i in zip(w[2], w[3])] for w in want]
            key_of = lambda kc, st, i: int(np.float64(self.hits[kc]["score_minus" if st else "score_plus"][i]).view(np.uint64))
            return fsr.candidates(self.genes, self.gene_family, self.gene_member, passing, fam_ref, {k: 0 for k in range(len(self.contigs))}, key_of)
        return self.once("step_candidates", make)


class Placed:
    """One placement as the references see it: the case contigs' tables at their arena positions, the genes' ranges and
    coding rows there, and for the string references of the edits the same letters moved down by `base` (a multiple of 64:
    their outcomes do not depend on where the arena begins)."""

    def __init__(self, case, placement):
        self.case, self.placement = case, placement
        self.filler, self.offsets, self.words = case.layout(placement)
        self.tables = hp.arena_tables(case.hits, self.offsets)
        self.entries = [(n, 0, ln, o) for n, ln, o in zip(case.names, case.lengths, self.offsets)]
        self.lo, self.hi, self.gene = selref.layout(case.gff_genes, self.entries, 0)
        self.ids = [case.idents[int(g)] for g in self.gene]
        self.rows = cref.layout_rows(case.gff, self.entries, 0)
        self.member = cref.membership(self.tables, self.lo, self.hi)
        self.n_plus = len(self.tables["pos_plus"])
        self.rows_before = dict(plus=np.cumsum([0] + [len(h["pos_plus"]) for h in case.hits]),
                                minus=np.cumsum([0] + [len(h["pos_minus"]) for h in case.hits]))
        self.base = self.offsets[0] - 64
        self.local_tables = dict(self.tables, pos_plus=self.tables["pos_plus"] - np.uint32(self.base),
                                 pos_minus=self.tables["pos_minus"] - np.uint32(self.base))
        self.local_rows = [(g, shift - self.base, a - self.base, b - self.base) for g, shift, a, b in self.rows]
        self.local_arena = eref.make_arena(case.contigs, [o - self.base for o in self.offsets])
        self._cache = {}

    def once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def cat(self, per_contig, strand):
        """A column of the arena's table of one strand from per-contig (plus, minus) pairs."""
        return np.concatenate([c[strand] for c in per_contig])

    def spec(self, M=3, kind="hsu2013"):
        cols = self.case.join(M, kind)
        cat = lambda key: np.concatenate([c[key] for c in cols])
        return dict(counts_plus=cat("self_counts_plus"), sum_plus=cat("self_sum_plus"), counts_minus=cat("self_counts_minus"),
                    sum_minus=cat("self_sum_minus"))

    def packed_members(self):
        """(layout row, table row as sel packs it, index into the concatenated tables) of every (gene, row in the gene)."""
        g, t = np.nonzero(self.member)
        return g.astype(np.uint32), np.where(t < self.n_plus, t, (t - self.n_plus) | (1 << 31)).astype(np.uint32), t

    def select(self, K, min_score=0.0, bounds=None):
        """select_numpy; bounds: None, or (max_mm0, max_hit_sum) over the references' joined columns (M = 3, hsu2013)."""
        spec = None if bounds is None else dict(self.spec(), max_mm0=bounds[0], max_hit_sum=bounds[1])
        return self.once(("select", K, min_score, bounds), lambda: selref.select_numpy(self.tables, self.lo, self.hi, K, min_score, spec))

    def pairs(self, K):
        return self.once(("pairs", K), lambda: pairs_ref.pairs_numpy(self.tables, self.lo, self.hi, K, *PAIR_WINDOW))

    def joined_spec(self, bounds):
        return None if bounds is None else dict(self.spec(), max_mm0=bounds[0], max_hit_sum=bounds[1])

    def spaced(self, K, D, min_score=0.0, bounds=None):
        """spaced_numpy; bounds as select()."""
        return self.once(("spaced", K, D, min_score, bounds),
                         lambda: spacing_ref.spaced_numpy(self.tables, self.lo, self.hi, K, D, min_score, self.joined_spec(bounds)))

    def distinct(self, K):
        return self.once(("distinct", K), lambda: dref.distinct_numpy(self.tables, self.lo, self.hi, K, *PAIR_WINDOW))

    def site_columns(self, flank):
        """Per strand site_reference.columns_numpy of Case.enzymes() over the letters moved down by `base`."""
        return self.once(("sites", flank), lambda: hs.columns(self, [m for _, m in self.case.enzymes()], flank))

    def select_sites(self, K, flank, forbid, need):
        """select_numpy over the rows whose reference masks at `flank` pass (forbid, need)."""
        def make():
            col = self.site_columns(flank)
            also = {s: site_ref.passes_numpy(col[s]["value"], forbid, need) for s in ("plus", "minus")}
            cds = dict(feat_plus=also["plus"].astype(np.uint32), feat_minus=also["minus"].astype(np.uint32), flags=np.array([0, 1], np.uint8))
            return selref.select_numpy(self.tables, self.lo, self.hi, K, 0.0, None, cds)
        return self.once(("select_sites", K, flank, forbid, need), make)

    def candidates(self):
        """(arena start, strand) of every candidate of PATTERN in extraction order: the case contigs' (the filler has none)."""
        return self.once("candidates", lambda: self_cases.candidates(self.case.contigs, self.offsets, PATTERN))

    def self_rows(self, M, scored):
        """The reference's guide sites at their arena positions, as select_self_reference's rows: in the device's extraction
        order, with each site's index among the candidates of PATTERN on the case contigs (the filler has none)."""
        def make():
            c = self.case.self_columns(M, scored)
            pos = c["start"] + np.array(self.offsets, np.int64)[c["contig"]]
            key = ((pos >> 6) << 7) | (c["strand"].astype(np.int64) << 6) | (pos & 63)  # by (64-position word, strand, position)
            order = np.argsort(key, kind="stable")
            assert np.unique(key).size == key.size
            cpos, cstrand = self.candidates()
            where = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(cpos, cstrand))}
            cand = np.array([where[(int(a), int(b))] for a, b in zip(pos[order], c["strand"][order])], np.uint32)
            assert (np.diff(cand.astype(np.int64)) > 0).all()
            return dict(pos=pos[order].astype(np.uint32), strand=c["strand"][order], hi=c["hi"][order], lo=c["lo"][order], counts=c["counts"][order],
                        hit_sum=None if c["hit_sum"] is None else c["hit_sum"][order], cand=cand)
        return self.once(("self_rows", M, scored), make)

    def cds_track(self):
        """(points, ids, flags): the module's annotation over the device's layout -- the filler, then the case contigs at
        their arena positions -- and its CDS flags."""
        def make():
            c = self.case
            request = annotate.Request(c.annotation, [hp.FILLER_NAME] + c.names, 0)
            layout = [(0, 64, self.filler)] + [(k + 1, o, n) for k, (o, n) in enumerate(zip(self.offsets, c.lengths))]
            return tuple(request.track(layout)) + (c.annotation.cds_flags(),)
        return self.once("cds_track", make)

    def self_spec(self, K, cds=False, **limits):
        return ssref.spec(SELF_T, SELF_CUT, SELF_REGION, K, track=self.cds_track() if cds else None, **limits)

    def self_select(self, M, scored, K, **limits):
        key = ("self_select", M, scored, K, tuple(sorted(limits.items())))
        return self.once(key, lambda: ssref.select_numpy(self.self_rows(M, scored), self.lo, self.hi, self.self_spec(K, **limits)))

    def positions(self):
        return self.once("positions", lambda: cref.positions_numpy(self.tables, self.case.models, self.rows))

    def select_coding(self, K, limits):
        return self.once(("coding", K, limits), lambda: cref.select_numpy(self.tables, self.lo, self.hi, self.case.models, self.rows, K, limits,
                                                                           positions=self.positions()))

    def edits(self):
        return self.once("edits", lambda: eref.outcomes(self.local_tables, self.member, self.case.models, self.local_rows, self.local_arena, WINDOW))

    def select_edit(self, K, limits):
        return self.once(("edit", K, limits), lambda: eref.select_numpy(self.local_tables, self.member, self.case.models, self.local_rows, K,
                                                                         self.edits(), limits))

    def splices(self):
        return self.once("splices", lambda: spref.outcomes(self.local_tables, self.member, self.case.models, self.local_rows, self.local_arena,
                                                           WINDOW, "cbe"))

    def select_splice(self, K, limits):
        return self.once(("splice", K, limits), lambda: spref.select_numpy(self.local_tables, self.member, self.case.models, self.local_rows, K,
                                                                            self.splices(), limits))

    def variants(self):
        """The variant track of test_gpu_variant_counts in arena positions -- dict(intervals, starts, ends1) -- with the
        expected columns plus and minus (variant_reference.column_numpy over the tables, seed 12) and `filled`: the arena
        position of the '+' row of the tie block whose site window holds more than 255 intervals.
          background  under every case contig an interval every 40 letters: SNPs, deletions, insertions -- at `straddle` on
                      both sides of 2^30
          spanning    one deletion from the last rows of the tie block's first copy to the first rows of its second: at
                      `straddle` it spans 2^30 (at `top` 2^30 lies in the filler, and so does this interval)
          filled      every interval [s, e] inside the site window of one '+' row in the middle of the first copy: 276 distinct
                      ones in one bucket of 2 048 positions, so its site and guide counts saturate
          tail        two deletions from hp_tail's first letters to 2^31 - 2 and 2^31 - 3, the largest ends a track takes
                      (ends1 = 2^31 - 1), and an insertion before hp_tail's last letter"""
        def make():
            c, t = self.case, self.tables
            rng = np.random.default_rng(25)
            iv = set()
            for off, n in zip(self.offsets, c.lengths):
                for s in (rng.integers(1, n - 13, n // 40) + off).tolist():
                    kind = rng.random()
                    iv.add((s, s) if kind < 0.7 else (s, s + int(rng.integers(1, 12))) if kind < 0.85 else (s, s - 1))
            tie = self.offsets[hp.TIE]
            iv.add((tie + hp.COPY[0] + hp.BLOCK - 20, tie + hp.COPY[1] + 20))
            pairs = hp.tie_pairs(c.hits, "plus")
            filled = int(c.hits[hp.TIE]["pos_plus"][pairs[len(pairs) // 2][0]]) + tie
            iv.update((s, e) for s in range(filled - L, filled + 3) for e in range(s, filled + 3))
            tail = self.offsets[-1]
            iv.update([(tail + 1, hp.TWO31 - 2), (tail + 2, hp.TWO31 - 3), (tail + hp.TAIL_LEN - 1, tail + hp.TAIL_LEN - 2)])
            starts, ends1 = vref.track(sorted(iv))
            return dict(intervals=sorted(iv), starts=starts, ends1=ends1, filled=filled,
                        plus=vref.column_numpy(t["pos_plus"], False, L, VARIANT_SEED, starts, ends1),
                        minus=vref.column_numpy(t["pos_minus"], True, L, VARIANT_SEED, starts, ends1))
        return self.once("variants", make)

    def select_family(self, K, limits, also=None, key=None):
        """Per layout row (n_in, n_pass, sel as the device packs it, the reference's values of the selected rows), from the
        family tests' plain loop over genes and rows; the joined columns are the references', not a device's.  also: None, or
        a boolean per row of the concatenated tables -- the predicate's other terms --, cached under `key`."""
        import test_families as tf

        def make():
            c = self.case
            fam_ref = c.family_rows(3)
            row_of = {s: r for r, s in enumerate(fam_ref["sites"])}
            bound = None if limits.get("min_specificity_outside") is None else sel.max_hit_sum_for(limits["min_specificity_outside"])
            more = None if also is None else (lambda kc, strand, i: also[int(self.rows_before["minus" if strand else "plus"][kc]) + i +
                                                                         (self.n_plus if strand else 0)])
            want = tf._reference_selection(c, c.hits, c.join(3, "hsu2013"), fam_ref, row_of, K, None, None,
                                           (limits.get("min_members"), limits.get("max_perfect_outside"), bound), also=more)
            n_in, n_pass, picked, values = [], [], np.full((len(self.gene), K), NONE, np.uint32), []
            for r, g in enumerate(self.gene):
                w = want[int(g)]
                n_in.append(w[0])
                n_pass.append(w[1])
                vals = []
                for j, ((kc, _, strand, v, site), i) in enumerate(zip(w[2], w[3])):
                    picked[r, j] = (int(self.rows_before["minus" if strand else "plus"][kc]) + i) | (strand << 31)
                    vals.append(v + (fam_ref["fam_cover"][site] if c.gene_family[int(g)] != fref.NONE and
                                     int(fam_ref["site_family"][site]) == c.gene_family[int(g)] else 0,))
                values.append(vals)
            return np.array(n_in, np.uint32), np.array(n_pass, np.uint32), picked, values
        assert (also is None) == (key is None)
        return self.once(("family", K, tuple(sorted(limits.items())), key), make)


@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    return Case(oracle, tmp_path_factory.mktemp("high_positions"))


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("n_in", "n_pass", "sel")):
        assert np.array_equal(np.asarray(g, np.uint32), np.asarray(w, np.uint32)), (what, name)


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _cut(tables, packed):
    """Arena cut site of a row as sel packs it."""
    minus, r = int(packed) >> 31, int(packed) & 0x7FFFFFFF
    return int(tables["pos_minus"][r]) if minus else int(tables["pos_plus"][r]) - 3


def _score_bits(tables, packed):
    minus, r = int(packed) >> 31, int(packed) & 0x7FFFFFFF
    return int(_bits(tables["score_minus" if minus else "score_plus"])[r])


# ---------------------------------------------------------------------------------------------- without a GPU
def test_the_filler_yields_nothing(oracle):
    """A contig of A: no row, no candidate of any pattern used here on either strand, no guide site."""
    stretch = bytes(hp.filler(5000))
    h = oracle.scan_score(stretch, L)
    assert h["pos_plus"].size == 0 and h["pos_minus"].size == 0
    patterns = [PATTERN, GUIDE_PATTERN, SPCAS9] + [bref.kind_pattern(SPCAS9, 3, b, 1) for b in ("DNA", "RNA")]
    for p in patterns:
        assert "G" in p.rstrip("N")[-3:]  # every pattern's PAM holds a G: an all-N pattern would make every filler position a candidate
        assert ref.candidates([stretch], p)[0].size == 0, p
    (k, _, _, _), g = selfref.guide_sites([stretch], PATTERN, 3, GUIDE_PATTERN)
    assert k.size == 0 and g.size == 0
    assert all(o["seed_plus"].size == 0 and o["seed_minus"].size == 0 for o in oracle.offtarget_genome([stretch], L))


def test_layout_of_both_placements(case):
    s, t = case.placed("straddle"), case.placed("top")
    for p in (s, t):
        assert p.filler % 64 == 0 and p.filler > 2**30 - 2**20 and all(o % 64 == 0 for o in p.offsets)
        assert p.offsets[-1] + case.lengths[-1] <= hp.TWO31 - 1
    # straddle: 2^30 between the copies of the tie block; the join genome's first contig below it, everything else above
    tie = s.offsets[hp.TIE]
    assert tie + hp.TIE_AT == hp.TWO30 and tie + hp.COPY[0] + hp.BLOCK < hp.TWO30 <= tie + hp.COPY[1]
    assert s.offsets[0] + case.lengths[0] < hp.TWO30 and all(o >= hp.TWO30 for o in s.offsets[hp.TIE + 1:])
    k = s.ids.index("tie")
    assert int(s.lo[k]) < hp.TWO30 <= int(s.hi[k]) and s.ids.index("tie_introns") == k + 1 and int(s.lo[k + 1]) < hp.TWO30 <= int(s.hi[k + 1])
    # top: the arena has the most words the library takes, the last text word is the tail's last, all within 2^20 of 2^31
    assert t.words == case.max_words
    assert (t.offsets[-1] + hp.TAIL_LEN) // 64 == t.words - 1 and hp.TAIL_LEN % 64 == 0
    for key in ("pos_plus", "pos_minus"):
        assert (hp.TWO31 - t.tables[key].astype(np.int64) < 2**20).all() and (t.tables[key] >> 30 == 1).all()
    assert hp.TWO31 - int(t.lo.min()) < 2**20
    # ... and some row's farthest reach (a flank-32 repair window behind a '-' cut boundary) lies past the last text word
    text_end = 64 * (t.words - 1)
    reach = max(int(t.tables["pos_plus"].max()) - 3 + 32, int(t.tables["pos_minus"].max()) + 3 + L + 32)
    assert reach >= text_end and int(t.tables["pos_plus"].max()) + 3 == text_end  # the tail's last '+' row: its PAM ends the text


def test_straddle_ties_decide_the_selection(case):
    """Every scored row of copy 1 has a bit-equal partner in copy 2 on the other side of 2^30; at K = 1 and the odd Ks the
    reference's K-th pick and the first row it leaves out are such a pair -- a signed compare of cut << 1 | strand swaps them."""
    s = case.placed("straddle")
    k = s.ids.index("tie")
    h = case.hits[hp.TIE]
    n_pairs = 0
    for strand in ("plus", "minus"):
        pairs = hp.tie_pairs(case.hits, strand)
        pos, score = h["pos_" + strand].astype(np.int64) + s.offsets[hp.TIE], h["score_" + strand]
        assert 2 * len(pairs) == pos.size  # every row of the contig is in a pair: the filler letters around the copies hold none
        for a, b in pairs:
            assert _bits(score)[a] == _bits(score)[b] and score[a] != -1.0
            assert pos[a] + 32 < hp.TWO30 <= pos[b] - 32
        n_pairs += len(pairs)
    assert n_pairs > max(TIE_KS) and s.member[k].sum() == 2 * n_pairs > 64  # (more than 64 rows: cut and merged at slices of 64)
    for name, select in (("plain", lambda K: s.select(K)), ("coding", lambda K: s.select_coding(K, (0, 100, 0))),
                         ("edit", lambda K: s.select_edit(K, (0, 100, 20))), ("family", lambda K: s.select_family(K, FAMILY_TIE_LIMITS)[:3])):
        ks = [K for K in TIE_KS if select(K)[1][k] > K]  # (few rows write a stop codon: K = 1 at the least)
        assert ks and (name == "edit" or ks == list(TIE_KS))
        for K in ks:
            n_in, n_pass, picked = select(K)
            kth, left_out = picked[k][K - 1], select(K + 1)[2][k][K]
            assert _score_bits(s.tables, kth) == _score_bits(s.tables, left_out), (name, K)
            assert _cut(s.tables, kth) < hp.TWO30 <= _cut(s.tables, left_out), (name, K)
    # the gene with an intron in either copy: a splice site that an edit destroys, in both copies
    k = s.ids.index("tie_introns")
    n_in, n_pass, picked = s.select_splice(1, (0, 100, 20, "any"))
    assert n_pass[k] >= 2 and n_pass[k] % 2 == 0
    kth, left_out = picked[k][0], s.select_splice(2, (0, 100, 20, "any"))[2][k][1]
    assert _score_bits(s.tables, kth) == _score_bits(s.tables, left_out) and _cut(s.tables, kth) < hp.TWO30 <= _cut(s.tables, left_out)
    # the pair selection: equal keys, one pair on either side; at odd KP the last pick and the first pair left out
    k = s.ids.index("tie")
    for K in KP:
        n_pass, n_pairs, pairs = s.pairs(K)
        assert n_pairs[k] > K
        (a1, b1), (a2, b2) = pairs[k][K - 1], s.pairs(K + 1)[2][k][K]
        assert sorted((_score_bits(s.tables, a1), _score_bits(s.tables, b1))) == sorted((_score_bits(s.tables, a2), _score_bits(s.tables, b2)))
        assert _cut(s.tables, b1) < hp.TWO30 <= _cut(s.tables, a2)


def test_straddle_keys_on_both_sides(case):
    """The rows the specificity join and the family join must match, and the candidates their binary searches run over,
    lie on both sides of the position where join_key and family_key gain bit 31."""
    s = case.placed("straddle")
    fam_ref = case.family_rows(3)
    for M in (0, 3):
        below = above = 0
        for k, cols in enumerate(case.join(M, "hsu2013")):
            for strand in ("plus", "minus"):
                joined = cols["self_counts_" + strand][:, 0] != join_cases.NO_COUNT
                pos = case.hits[k]["pos_" + strand].astype(np.int64)[joined] + s.offsets[k]
                below, above = below + int((pos < hp.TWO30).sum()), above + int((pos >= hp.TWO30).sum())
        assert below >= 64 and above >= 64, M
    k, pos, strand = fam_ref["cand"]
    arena_pos = pos + np.array(s.offsets)[k]
    assert (arena_pos < hp.TWO30).sum() >= 64 and (arena_pos >= hp.TWO30).sum() >= 64
    in_family = fam_ref["site_family"] != NONE
    site_pos = np.array([p + s.offsets[kc] for kc, p, _ in fam_ref["sites"]])
    assert (in_family & (site_pos < hp.TWO30)).sum() >= 64 and (in_family & (site_pos >= hp.TWO30)).sum() >= 64


def test_expected_arrays_are_not_trivial(case):
    """Every step's expectation holds something a wrong kernel would miss."""
    for F in FLANKS:
        assert all(np.unique(np.concatenate(r)).size > 5 for r in case.repair(F)[:4])
    assert all(np.unique(np.concatenate(p)).size > 5 for p in case.props())
    feats = case.features()
    ids = np.concatenate([np.concatenate(f) for f in feats])
    assert np.unique(ids).size >= 8 and (ids == NONE).any()
    ot = case.offtarget()
    assert sum(int((o["ot_plus"][:, 0] != NONE).sum()) for o in ot) > 300 and any((o["ot_plus"][:, 0] > 0).any() for o in ot)
    for M in (0, 3):
        counts, sites, _ = case.search("plain", M)
        assert (counts.sum(axis=1) >= 1).all() and counts[-1].sum() >= 2  # (the tie block's guide: a site on either side of 2^30)
        assert set(sites["contig"].tolist()) >= {0, 1, 2, 3} and set(sites["strand"].tolist()) == {0, 1}
        _, (pc, _, hit_sum) = case.search_pair(M)
        assert (pc == counts).all() and (M == 0 or sum(hit_sum) > 0)
        bc, bs = case.bulges(M)
        assert bc[:, 0].sum() == counts.sum() and (M == 0 or (bc[:, 1:].sum() > 0 and set(bs["kind"].tolist()) == {0, 1, 2}))
        sites, _, counts, hit_sum = case.self_search(M, True)
        assert len(sites) > 800 and counts[:, 0].sum() >= 100 and (M == 0 or (counts[:, 1:].sum() > 10 and sum(hit_sum) > 0))
    f = case.family_rows(3)
    assert f["fam_counts"][:, 0].sum() >= 100 and set(f["fam_cover"]) >= {0, 1, 7} and sum(f["fam_sum"]) > 0
    for name in hp.PLACEMENTS:
        p = case.placed(name)
        off, cover = p.positions()
        assert (off[p.member] != cref.NOT_INSIDE).sum() > 200 and (off[p.member] == cref.NOT_INSIDE).sum() > 20
        assert sum(int((o[3] != eref.NO_STOP).sum()) for o in p.edits()) >= 4
        assert sum(int((o[4] != spref.NO_SITE).sum() + (o[5] != spref.NO_SITE).sum()) for o in p.splices()) >= 4
        for K in KS:
            n_in, n_pass, picked = p.select(K)
            assert (n_pass > 64).sum() >= 3 and (picked[:, 0] != NONE).all() and np.unique(picked[:, 0] >> 31).size == 2
            assert (p.select(K, 0.0, BOUNDS)[1] < n_pass).any()
        n_in, n_pass, picked, values = p.select_family(5, FAMILY_LIMITS)
        assert 0 < n_pass.sum() < p.select(5)[1].sum() and any(v[2] >= 2 for vals in values for v in vals)
        assert (p.pairs(5)[1] > 5).sum() >= 3


def test_variant_track_holds_its_cases(case):
    """On the reference's column: rows with a count on both sides of 2^30 at `straddle`, the spanning deletion among what
    they count; a saturated field over a bucket of more than 255 entries; hp_tail's rows counted, under ends1 = 2^31 - 1."""
    for name in hp.PLACEMENTS:
        p = case.placed(name)
        v, t = p.variants(), p.tables
        col = np.concatenate([v["plus"], v["minus"]])
        pos = np.concatenate([t["pos_plus"], t["pos_minus"]]).astype(np.int64)
        assert (np.concatenate([vref.column_loop(t["pos_plus"][::7], False, L, VARIANT_SEED, v["intervals"]),
                                vref.column_loop(t["pos_minus"][::7], True, L, VARIANT_SEED, v["intervals"])]) ==
                np.concatenate([v["plus"][::7], v["minus"][::7]])).all()  # (the touch rule, variant by variant, on every 7th row)
        assert v["starts"].size == len(v["intervals"]) > 400 and int(v["ends1"].max()) == hp.TWO31 - 1
        kinds = [(e == s, e > s, e < s) for s, e in v["intervals"]]
        assert all(sum(k[i] for k in kinds) >= 10 for i in range(3))
        spanning = (p.offsets[hp.TIE] + hp.COPY[0] + hp.BLOCK - 20, p.offsets[hp.TIE] + hp.COPY[1] + 20)
        assert spanning in v["intervals"]
        if name == "straddle":
            assert ((col != 0) & (pos < hp.TWO30)).sum() >= 64 and ((col != 0) & (pos >= hp.TWO30)).sum() >= 64
            assert spanning[0] < hp.TWO30 - 500 and hp.TWO30 + 400 < spanning[1]
            st, en = vref.track([x for x in v["intervals"] if x != spanning])
            without = np.concatenate([vref.column_numpy(t["pos_plus"], False, L, VARIANT_SEED, st, en),
                                      vref.column_numpy(t["pos_minus"], True, L, VARIANT_SEED, st, en)])
            assert ((without != col) & (pos < hp.TWO30)).any() and ((without != col) & (pos >= hp.TWO30)).any()
        else:
            assert (pos >= hp.TWO30).all() and (col != 0).sum() >= 128
        # the filled bucket: one bucket of the starts' index holds the 276 intervals, and the row's site and guide fields saturate
        filled = v["filled"]
        assert (filled - L) >> 11 == (filled + 2) >> 11 and int((v["starts"] >> 11 == filled >> 11).sum()) > 255
        r = int(np.flatnonzero(t["pos_plus"] == filled)[0])
        assert v["plus"][r] & 0xFFFF == 0xFFFF and sum(1 for s, e in v["intervals"] if s <= filled + 2 and e >= filled - L) >= 276
        assert p.offsets[hp.TIE] + hp.COPY[0] < filled - L and filled + 2 < p.offsets[hp.TIE] + hp.COPY[0] + hp.BLOCK
        # hp_tail: every row counts the deletions that run to the top
        for strand in ("plus", "minus"):
            mine = v[strand][p.rows_before[strand][-2]:]
            assert mine.size >= 2 and ((mine & 255) >= 2).all() and mine[-1] >> 24 >= 1


def test_family_step_ties_lie_across_two30(case):
    """twins has one member, tie: every candidate gains 1, the best score occurs once in either copy of the block, and
    cut << 1 | strand decides between the two.  At `straddle` the winner's word has bit 31 clear and the loser's has it set -- a
    signed compare takes the loser --; at `top` every word has bit 31 set.  homeo's candidates lie on both sides of 2^30."""
    cands = case.step_candidates()
    twins, homeo = case.fam_names.index("twins"), case.fam_names.index("homeo")
    assert case.sizes[twins] == 1 and case.sizes[homeo] == 3
    mine = [c for c in cands if c[0] == twins]
    best = mine[fsr.best_loop(mine, 0)]
    tied = [c for c in mine if c[6] == best[6]]
    assert len(tied) == 2 and best[6] == max(c[6] for c in mine)
    loser = [c for c in tied if c != best][0]
    for name in hp.PLACEMENTS:
        p = case.placed(name)
        word = lambda c: ((c[3] + p.offsets[c[2]]) << 1 | c[4]) & 0xFFFFFFFF
        assert word(best) < word(loser)
        if name == "straddle":
            assert best[3] + p.offsets[best[2]] < hp.TWO30 <= loser[3] + p.offsets[loser[2]]
            assert word(best) >> 31 == 0 and word(loser) >> 31 == 1
            cuts = np.array([c[3] + p.offsets[c[2]] for c in cands if c[0] == homeo])
            assert (cuts < hp.TWO30).sum() >= 64 and (cuts >= hp.TWO30).sum() >= 64
        else:
            assert word(best) >> 31 == 1 and word(loser) >> 31 == 1
    # against all ones but one member's bit only the rows that cover that member gain: other proposals than against nothing
    for bit in range(3):
        covered = [ALL_ONES ^ 1 << bit] * len(case.sizes)
        want = fsr.arena_best(cands, case.sizes, covered, 0)
        assert want[homeo] is not None and want[homeo]["gain"] == 1 and (want[twins] is None) == (bit != 0)
    assert fsr.arena_best(cands, case.sizes, [0, 0], 0)[homeo]["gain"] == 3


def _bit(mask, e):
    return (np.asarray(mask, np.uint32) >> np.uint32(e)) & np.uint32(1)


def test_site_columns_hold_their_cases(case):
    """On site_reference's own columns.  The two cut-out motifs occur once in either copy of the tie block and nowhere else;
    every other enzyme has rows with its in_guide bit set and clear on both strands.  At `straddle` and flank 1000 four rows per
    strand have a cut-out site across their cut and an amplicon that crosses 2^30 -- a_lo < 2^30 <= the last start a_hi - m -- with
    exactly one occurrence in it, so their assay bit stands on rank(q_hi) - rank(a_lo) across the chunk whose scanned sum
    begins another trip of the rank scan (2^30 is a multiple of 256 chunks of 1 024 words); no other enzyme has such a row.  At
    flank 100000 the same rows count 2 and lose the bit, at 300 they count 1 without crossing."""
    enzymes = case.enzymes()
    names, motifs = [n for n, _ in enzymes], [m for _, m in enzymes]
    assert names == [n for n, _ in hs.FIXED] + list(hs.CUT_OUT) and len(enzymes) == 8 and len(set(motifs)) == 8
    for m in motifs[-2:]:
        assert len(m) == 8 and set(m) <= set("ACGT") and [hs.count_in(t, m) for t in case.contigs] == [0, 2, 0, 0, 0], m
    stretch = bytes(hp.filler(5000))
    assert [hs.count_in(stretch, m) for m in motifs] == [4997, 4985, 0, 0, 0, 0, 0, 0]  # poly_a and span16 at every filler position
    assert sites.is_palindrome("AGCT") and not sites.is_palindrome("CCTC") and not sites.is_palindrome("AAAA") and sites.is_palindrome("CCWGG")
    rows_of = hs.cut_out_rows(case.hits)
    for name in hp.PLACEMENTS:
        p = case.placed(name)
        for flank in hs.FLANKS:
            col = p.site_columns(flank)
            assert col["plus"]["value"].size == 414 and col["minus"]["value"].size == 462
            # in_guide does not depend on the flank or on the placement
            assert [int(_bit(col["plus"]["in_guide"], e).sum()) for e in range(8)] == [63, 193, 26, 61, 19, 16, 4, 0], (name, flank)
            assert [int(_bit(col["minus"]["in_guide"], e).sum()) for e in range(8)] == [83, 213, 50, 54, 13, 20, 4, 0], (name, flank)
        assert [int(_bit(p.site_columns(16)[s]["assay"], 1).sum()) for s in ("plus", "minus")] == [105, 119]  # span16 at the smallest flank
        # the plain loop over strings on every third row, at the flank of the crossing rows
        occ = site_ref.occurrences_loop(p.local_arena, motifs)
        for s in ("plus", "minus"):
            pos = p.local_tables["pos_" + s][::3]
            assert np.array_equal(site_ref.column_loop(p.local_arena, hs.local_bounds(p), pos, s == "minus", L, hs.CROSSING_FLANK, motifs, occ),
                                  p.site_columns(hs.CROSSING_FLANK)[s]["value"][::3]), (name, s)
        for s, e in (("plus", 6), ("minus", 7)):
            first = int(p.rows_before[s][hp.TIE])
            for flank, crossing, amp in ((300, False, 1), (hs.CROSSING_FLANK, name == "straddle", 1), (100000, name == "straddle", 2)):
                col = p.site_columns(flank)[s]
                a_lo, last_start, cut = hs.amplicon(p, s, flank, 8)
                cross = (a_lo < hp.TWO30) & (hp.TWO30 <= last_start)
                spanning = np.flatnonzero(col["span"][:, e] >= 1)
                assert spanning.size == 4 and first + rows_of[s] in spanning.tolist(), (name, s, flank)  # two rows at either copy
                assert (col["amp"][spanning, e] == amp).all() and (_bit(col["assay"], e)[spanning] == (amp == 1)).all(), (name, s, flank)
                assert int(_bit(col["assay"], e).sum()) == (4 if amp == 1 else 0)
                assert (cross[spanning] == crossing).all(), (name, s, flank)
                if flank == hs.CROSSING_FLANK:  # the six other enzymes: rows cross, none with a spanning site and a count of 1
                    for other in range(6):
                        a_lo, last_start, _ = hs.amplicon(p, s, flank, len(motifs[other]))
                        cross = (a_lo < hp.TWO30) & (hp.TWO30 <= last_start)
                        assert int(cross.sum()) == ((44 if s == "plus" else 64) if name == "straddle" else 0)
                        assert not (cross & (col["span"][:, other] >= 1) & (col["amp"][:, other] == 1)).any()
        # the selection of test_gpu_site_columns: eight rows of either tie gene have a cut-out assay at flank 1000, four of them a
        # four-cutter in their guide; the four left are '-' rows, two in either copy
        forbid, need = hs.mask(names, hs.FOUR_CUTTERS), hs.mask(names, hs.CUT_OUT)
        assert (forbid, need) == (0b1100, 0b11000000)
        assert p.select_sites(5, hs.CROSSING_FLANK, 0, need)[1].tolist() == [0, 8, 8, 0, 0, 0]
        assert p.select_sites(5, hs.CROSSING_FLANK, forbid, 0)[1].tolist() == [279, 84, 84, 84, 127, 14] and p.select(5)[1].tolist() == [360, 108, 108, 118, 149, 20]
        n_in, n_pass, picked = p.select_sites(5, hs.CROSSING_FLANK, forbid, need)
        assert n_pass.tolist() == [0, 4, 4, 0, 0, 0] and (picked[1][:4] >> 31 == 1).all() and picked[1][4] == NONE
        assert sorted(_cut(p.tables, x) < hp.TWO30 for x in picked[1][:4]) == ([False, False, True, True] if name == "straddle" else [False] * 4)
    # top: the last '+' row of hp_tail has its window of the occurrence planes in the last word that holds text, and its
    # amplicon ends at the text's end at every flank
    t = case.placed("top")
    pos = int(t.tables["pos_plus"][-1])
    cut, end = pos - 3, t.offsets[-1] + hp.TAIL_LEN
    assert min(pos - L, cut - 15) >> 6 == t.words - 2 == (end - 1) >> 6 and all(cut + flank >= end for flank in hs.FLANKS)
    assert hs.amplicon(t, "plus", 16, 4)[1][-1] == end - 4


def test_site_columns_need_the_texts_bounds(case):
    """Clipping the amplicon at the text's start decides masks.  Stated on the moved-down letters with a run of A and a separator
    word in front of sj_c0, as the filler lies on the device: with the bounds replaced by one text over everything, at flank 300
    one row per strand gets another mask.  It is a row of hp_tail, whose amplicon then reaches over the separator word into
    sj_c2; no row of sj_c0 within 300 letters of its start has a site across its cut and a count of 1, so none of them changes
    (the issue expected them there; the reference says otherwise)."""
    p = case.placed("straddle")
    motifs = [m for _, m in case.enzymes()]
    lead = 1024
    arena = b"\0" * 64 + b"A" * (lead - 128) + b"\0" * 64 + p.local_arena[64:]
    bounds = [(a + lead - 64, b + lead - 64) for a, b in hs.local_bounds(p)]
    assert arena[bounds[0][0]:bounds[0][1]] == case.contigs[0] and arena[bounds[-1][0]:bounds[-1][1]] == case.contigs[-1]
    real = hs.columns(p, motifs, 300, bounds, arena, lead - 64)
    for s in ("plus", "minus"):
        assert np.array_equal(real[s]["value"], p.site_columns(300)[s]["value"])  # what lies in front of the first text changes nothing
    one = hs.columns(p, motifs, 300, [(0, len(arena))], arena, lead - 64)
    for s, row, was, now in (("plus", 405, 0x80000000B, 0xB), ("minus", 455, 0x10000000B, 0xB)):
        changed = np.flatnonzero(real[s]["value"] != one[s]["value"])
        assert changed.tolist() == [row] and row >= p.rows_before[s][-2], s
        assert (int(real[s]["value"][row]), int(one[s]["value"][row])) == (was, now)
        a_lo, _, cut = hs.amplicon(p, s, 300, 4)
        assert a_lo[row] == p.offsets[-1] > cut[row] - 300  # clipped at the start of its text


def test_spaced_selection_holds_its_cases(case):
    """spaced_numpy equals spaced_loop; D = 0 is the plain selection; at `straddle` the tie gene's picks lie on both sides of
    2^30 for every D; a row's twin is exactly TWIN away, so D = TWIN takes it second and D = TWIN + 1 cannot; at D = 0 the K-th
    pick and the first row left out have bit-equal scores and cut sites on either side of 2^30."""
    for name in hp.PLACEMENTS:
        p = case.placed(name)
        k = p.ids.index("tie")
        for K in KS:
            for D in SPACINGS:
                want = p.spaced(K, D)
                loop = spacing_ref.spaced_loop(p.tables, p.lo, p.hi, K, D)
                assert all(np.array_equal(a, b) for a, b in zip(want, loop)), (name, K, D)
                picks = want[2][k][want[2][k] != NONE]
                below = sum(_cut(p.tables, x) < hp.TWO30 for x in picks)
                if name == "straddle":
                    expected = {0: {1: (1, 0), 5: (3, 2), 33: (17, 16), 64: (32, 32)}[K], 1: {1: (1, 0), 5: (3, 2), 33: (17, 16), 64: (32, 32)}[K],
                                30: {1: (1, 0), 5: (3, 2), 33: (9, 9), 64: (9, 9)}[K]}.get(D, (1, 0) if K == 1 else (1, 1))
                    assert (below, len(picks) - below) == expected, (K, D)
                else:
                    assert below == 0 and len(picks) == int(want[1][k]) > 0
            n_in, n_pass, picked = p.select(K)
            assert np.array_equal(p.spaced(K, 0)[0], n_pass) and np.array_equal(p.spaced(K, 0)[2], picked)
            assert np.array_equal(p.spaced(K, 0)[1], np.minimum(n_pass, K))
            bounded = p.spaced(K, 30, 0.2, BOUNDS)
            assert (bounded[0] < p.spaced(K, 30)[0]).any() and bounded[1].sum() > 0
        # the twin
        at, beyond = p.spaced(5, TWIN)[2][k], p.spaced(5, TWIN + 1)[2][k]
        assert at[0] == beyond[0] and at[1] != beyond[1] and at[2] == beyond[2] == NONE
        assert _cut(p.tables, at[1]) - _cut(p.tables, at[0]) == TWIN and _score_bits(p.tables, at[0]) == _score_bits(p.tables, at[1])
        assert abs(_cut(p.tables, beyond[1]) - _cut(p.tables, beyond[0])) > TWIN
        if name == "straddle":
            for K in TIE_KS:
                kth, left_out = p.spaced(K, 0)[2][k][K - 1], p.spaced(K + 1, 0)[2][k][K]
                assert _score_bits(p.tables, kth) == _score_bits(p.tables, left_out) and _cut(p.tables, kth) < hp.TWO30 <= _cut(p.tables, left_out)


def test_distinct_pairs_hold_their_cases(case):
    """distinct_numpy equals distinct_walk; KP = 1 is the plain pair selection; at KP = 5 and 33 the distinct pairs are other
    pairs than the plain ones; at `straddle` the tie gene's distinct pairs lie on both sides of 2^30, none across it; hp_tail's
    gene runs out of pairs before KP = 33."""
    for name in hp.PLACEMENTS:
        p = case.placed(name)
        k, tail = p.ids.index("tie"), p.ids.index("tail_gene")
        for K in KP_DISTINCT:
            want = p.distinct(K)
            walk = dref.distinct_walk(p.tables, p.lo, p.hi, K, *PAIR_WINDOW)
            assert all(np.array_equal(np.asarray(a, np.uint64), np.asarray(b, np.uint64)) for a, b in zip(want, walk)), (name, K)
            plain = pairs_ref.pairs_numpy(p.tables, p.lo, p.hi, K, *PAIR_WINDOW)
            assert np.array_equal(want[0], plain[0]) and np.array_equal(want[1], plain[1])
            assert np.array_equal(want[3], plain[2]) == (K == 1), (name, K)
            assert want[1].tolist() == [17532, 2182, 2182, 4528, 7437, 49] and want[2].tolist() == [min(K, 33)] * 5 + [min(K, 6)]
            mine = want[3][k][:int(want[2][k])]
            sides = [(_cut(p.tables, a) < hp.TWO30, _cut(p.tables, b) < hp.TWO30) for a, b in mine]
            assert all(a == b for a, b in sides)
            below = sum(a for a, _ in sides)
            assert (below, len(sides) - below) == ({1: (1, 0), 5: (3, 2), 33: (17, 16)}[K] if name == "straddle" else (0, K))
        assert int(p.distinct(33)[2][tail]) == 6 < 33 and (p.distinct(33)[3][tail][6:] == NONE).all()


def _self_cut(rows, i):
    return int(ssref.cut_letters(rows["pos"][i], rows["strand"][i], SELF_T, SELF_CUT))


def test_self_selection_holds_its_cases(case):
    """select_numpy equals select_loop.  Every site of the tie block has its twin as its one perfect copy, so some 53 sites of
    either copy share the gene's best e and the word cut << 1 | strand alone orders them: at `straddle` the first copy's words
    have bit 31 clear and the second copy's have it set -- a signed compare takes the second copy first.  For K in TIE_KS the
    K-th site and the first one left out tie in the first copy; at K = SELF_TIE_K they tie across 2^30.  tail_gene holds '+' and
    '-' sites; at `top` the word of every selected site has bit 31 set; the CDS, perfect-copy and sequence limits each change
    some gene's sel, the hit-sum bound lowers n_pass."""
    for name in hp.PLACEMENTS:
        p = case.placed(name)
        k, tail = p.ids.index("tie"), p.ids.index("tail_gene")
        for M, scored in SELF_HANDLES:
            rows = p.self_rows(M, scored)
            assert rows["pos"].size == 867 and (rows["hit_sum"] is not None) == scored and rows["counts"].shape == (867, M + 1)
            row_of = {int(c): i for i, c in enumerate(rows["cand"])}
            e = ssref.row_keys(rows)
            for K in KS:
                want = p.self_select(M, scored, K)
                if K in (1, 33):
                    loop = ssref.select_loop(rows, p.lo, p.hi, p.self_spec(K))
                    assert all(np.array_equal(a, b) for a, b in zip(want, loop)), (name, M, scored, K)
                assert (want[2][:, 0] != NONE).all() and (want[0] == want[1]).all()
                if name == "top":
                    for c in want[2][want[2] != NONE]:
                        i = row_of[int(c)]
                        assert (_self_cut(rows, i) << 1 | int(rows["strand"][i])) >> 31 == 1
            inside = [i for i in range(867) if int(p.lo[tail]) <= _self_cut(rows, i) <= int(p.hi[tail])]
            assert int(p.self_select(M, scored, 1)[0][tail]) == len(inside) == 21 and sum(int(rows["strand"][i]) for i in inside) == 10  # 11 '+' sites and 10 '-'
            if name == "straddle":
                cut = ssref.cut_letters(rows["pos"], rows["strand"], SELF_T, SELF_CUT)
                mine = (cut >= int(p.lo[k])) & (cut <= int(p.hi[k]))
                best = mine & (e == min(e[mine]))
                below, above = int((best & (cut < hp.TWO30)).sum()), int((best & (cut >= hp.TWO30)).sum())
                assert (int(mine.sum()), below, above) == (107, SELF_TIE_K[M], SELF_TIE_K[M] - 1)
                for K in TIE_KS + (SELF_TIE_K[M],):
                    kth, left_out = row_of[int(p.self_select(M, scored, K)[2][k][K - 1])], row_of[int(p.self_select(M, scored, K + 1)[2][k][K])]
                    assert best[kth] and best[left_out] and _self_cut(rows, kth) < hp.TWO30, (M, scored, K)
                    assert (_self_cut(rows, left_out) >= hp.TWO30) == (K == SELF_TIE_K[M]), (M, scored, K)
            plain = p.self_select(M, scored, 5)
            for what, limits in SELF_LIMITS.items():
                if what == "hit_sum" and not scored:
                    continue
                got = p.self_select(M, scored, 5, **limits)
                loop = ssref.select_loop(rows, p.lo, p.hi, p.self_spec(5, **limits))
                assert all(np.array_equal(a, b) for a, b in zip(got, loop)), (name, M, scored, what)
                assert got[1].tolist() == SELF_N_PASS[what if what != "hit_sum" or M else None], (name, M, scored, what)
                # (a hit-sum bound drops a gene's least specific sites: it lowers n_pass and, while K sites pass, leaves sel)
                assert np.array_equal(got[2], plain[2]) == (what == "hit_sum"), (name, M, scored, what)
            assert plain[1].tolist() == SELF_N_PASS[None]
        points, ids, flags = p.cds_track()
        assert int(points.max()) >> 30 == 1 and flags.any() and not flags.all()


# ---------------------------------------------------------------------------------------------- on the GPU
@pytest.fixture(scope="module")
def engine():
    from cropsr_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


class Device:
    def __init__(self, engine, case, placement):
        import time
        self.case, self.ref = case, case.placed(placement)
        t0 = time.perf_counter()
        text = hp.filler(self.ref.filler)
        self.genome = engine.genome([text] + case.contigs)
        del text  # (a gigabyte or two of host memory: gone before the references need theirs)
        self.upload_s = time.perf_counter() - t0
        assert len(self.genome.arenas) == 1
        self.arena = self.genome.arenas[0]
        self.request = annotate.Request(case.annotation, [hp.FILLER_NAME] + case.names, 0)
        self.scan()
        print("high positions, %s: upload %.2f s, first scan %.2f s" % (placement, self.upload_s, time.perf_counter() - t0 - self.upload_s))

    def scan(self):
        self.hits = self.genome.scan_score(L)
        self.counts = [(h.n_plus, h.n_minus) for h in self.hits.per_arena]
        return self.hits

    def select(self):
        return sel.ArenaSelect(self.arena, self.ref.lo, self.ref.hi)

    def model(self):
        return self.request.coding_layout(sel.arena_layout(self.genome, 0))


@pytest.fixture(scope="module", params=hp.PLACEMENTS)
def dev(request, engine, case):
    d = Device(engine, case, request.param)
    yield d
    d.genome.close()


@pytest.mark.gpu
def test_gpu_ground(dev, case):
    """The layout is the restated one, the filler holds no row, the case contigs' rows are the oracle's, and the positions
    are as high as claimed."""
    p = dev.ref
    assert [int(o) for o in dev.arena.offsets] == [64] + p.offsets and dev.arena.stats()["n_words"] == p.words
    assert dev.arena.stats()["n_chars"] == p.filler + sum(case.lengths)
    if p.placement == "top":
        assert p.words == int(nat.lib().crp_arena_max_words())
    filler = dev.hits.contig(0)
    assert all(filler[key].size == 0 for key in ("pos_plus", "score_plus", "pos_minus", "score_minus"))
    for k, want in enumerate(case.hits):
        got = dev.hits.contig(k + 1)
        for key in ("pos_plus", "pos_minus"):
            assert np.array_equal(got[key], want[key]), (k, key)
        for key in ("score_plus", "score_minus"):
            assert np.array_equal(_bits(got[key]), _bits(want[key])), (k, key)
    h = dev.hits.per_arena[0]
    for key in ("pos_plus", "pos_minus"):
        assert np.array_equal(getattr(h, key), p.tables[key]) and int(getattr(h, key).max()) <= hp.TWO31 - 1
        high = getattr(h, key) >> 30 == 1
        assert high.all() if p.placement == "top" else (high.sum() >= 64 and (~high).sum() >= 64)
    lo, hi, gene = dev.request.gene_layout(sel.arena_layout(dev.genome, 0))
    assert np.array_equal(lo, p.lo) and np.array_equal(hi, p.hi) and np.array_equal(gene, p.gene)


@pytest.mark.gpu
def test_gpu_properties_and_repair(dev, case):
    p = dev.ref
    (pp, pm), = dev.genome.guide_properties(dev.counts)
    assert np.array_equal(pp, p.cat(case.props(), 0)) and np.array_equal(pm, p.cat(case.props(), 1))
    for F in FLANKS:
        (rp, rm), = dev.genome.repair_scores(dev.counts, F)
        assert np.array_equal(rp, p.cat(case.repair(F), 0)) and np.array_equal(rm, p.cat(case.repair(F), 1)), F


@pytest.mark.gpu
def test_gpu_annotation_lookup(dev, case):
    """Label-set ids per row: the numpy statement over the product's interval table, and every id's string against the
    brute-force statement (all features of the GFF that contain the cut site, in file order)."""
    from oracle import annotate_oracle
    p = dev.ref
    (fp, fm), = dev.genome.annotate(dev.request, dev.counts)
    want = case.features()
    assert np.array_equal(fp, p.cat(want, 0)) and np.array_equal(fm, p.cat(want, 1))
    feats = list(annotate_oracle.gff_rows(case.gff_path))
    strings = case.annotation.strings
    n_labelled = 0
    for got, key, before in ((fp, "plus", p.rows_before["plus"]), (fm, "minus", p.rows_before["minus"])):
        for k, (name, h) in enumerate(zip(case.names, case.hits)):
            pos = h["pos_" + key].astype(np.int64)
            cut = pos - 3 if key == "plus" else pos
            for r in np.flatnonzero(h["score_" + key] != -1.0):
                labels = []
                for seqid, ftype, start, end, attrs in feats:
                    lab = annotate_oracle.label(ftype, attrs)
                    if seqid == name and start <= cut[r] + 1 <= end and lab not in labels:
                        labels.append(lab)
                i = int(got[before[k] + r])
                assert ("" if i == NONE else strings[i]) == ";".join(labels), (key, k, r)
                n_labelled += bool(labels)
    assert n_labelled > 500


@pytest.mark.gpu
@pytest.mark.parametrize("seeds_from_scan", [True, False], ids=["seeds-from-scan", "seeds-from-planes"])
def test_gpu_offtarget_seeds_and_counts(dev, case, seeds_from_scan):
    want = case.offtarget()
    try:
        hits = dev.genome.scan_score(L, offtarget=True, seeds_from_scan=seeds_from_scan)
        sp, sm = dev.arena.offtarget_seeds(hits.n_plus, hits.n_minus)
        assert np.array_equal(sp, np.concatenate([w["seed_plus"] for w in want])) and np.array_equal(sm, np.concatenate([w["seed_minus"] for w in want]))
        for k, w in enumerate(want):
            got = hits.contig(k + 1)
            assert np.array_equal(got["ot_plus"], w["ot_plus"]) and np.array_equal(got["ot_minus"], w["ot_minus"]), k
    finally:
        dev.scan()


def _site_tuples(sites, fields):
    cols = [(sites[f] == b"-").astype(int).tolist() if f == "strand" else sites[f].tolist() for f in fields]
    return list(zip(*cols))


def _want_tuples(s, fields):
    """The reference's sites with the case contigs renumbered as the device's genome has them (the filler is contig 0)."""
    cols = [(s[f] + 1).tolist() if f == "contig" else s[f].tolist() for f in fields]
    return sorted(zip(*cols))


@pytest.mark.gpu
@pytest.mark.parametrize("M", [0, 3])
def test_gpu_given_guide_search(dev, case, M):
    """Counts, hit sums and every site -- decoded on the host from start | strand << 31 -- of the plain, the hsu2013-scored
    and the pair-table search, and of the search with one DNA and one RNA bulge."""
    q = case.queries()
    counts, s, _ = case.search("plain", M)
    res = dev.genome.search(SPCAS9, q, M)
    assert np.array_equal(res.counts, counts) and _site_tuples(res.sites, ref.SITE_FIELDS) == _want_tuples(s, ref.SITE_FIELDS)
    assert res.sites.size == counts.sum() and sum(res.candidates) == ref.candidates(case.contigs, SPCAS9)[0].size
    counts, s, hit_sum = case.search("hsu2013", M)
    res = dev.genome.search(SPCAS9, q, M, pam_len=3, score="hsu2013")
    assert np.array_equal(res.counts, counts) and [int(x) for x in res.hit_sum] == hit_sum
    assert _site_tuples(res.sites, ref.SITE_FIELDS) == _want_tuples(s, ref.SITE_FIELDS)
    (pair, pam), (counts, s, hit_sum) = case.search_pair(M)
    res = dev.genome.search(SPCAS9, q, M, pam_len=3, score=srch.PairTable(pair, (1, 2), pam))
    assert np.array_equal(res.counts, counts) and [int(x) for x in res.hit_sum] == hit_sum
    assert _site_tuples(res.sites, ref.SITE_FIELDS) == _want_tuples(s, ref.SITE_FIELDS)
    counts, s = case.bulges(M)
    res = dev.genome.search_bulges(SPCAS9, q, M, 3, 1, 1)
    assert np.array_equal(res.counts, counts) and _site_tuples(res.sites, bref.FIELDS) == _want_tuples(s, bref.FIELDS)
    assert np.array_equal(res.sites["bulge_size"], np.array([size for _, size in res.kinds], np.uint8)[res.sites["kind"]])


def _assert_joined(case, p, got, M, kind):
    """The joined columns of the case contigs (got: per contig of the device's genome, the filler first)."""
    want = case.join(M, kind)
    assert all(v.shape[0] == 0 for v in got[0].values())
    unjoined = 0
    for k, w in enumerate(want):
        for key in ("self_counts_plus", "self_counts_minus", "self_sum_plus", "self_sum_minus"):
            g = got[k + 1][key]
            assert g.dtype == w[key].dtype and g.shape == w[key].shape, (k, key)
            if key.startswith("self_counts"):  # the failure of a misordered key search: a joined row with the sentinel
                unjoined += int(((g[:, 0] == join_cases.NO_COUNT) & (w[key][:, 0] != join_cases.NO_COUNT)).sum())
    assert unjoined == 0, "%d rows the join should have matched carry the unjoined sentinel" % unjoined
    for k, w in enumerate(want):
        for key in ("self_counts_plus", "self_counts_minus", "self_sum_plus", "self_sum_minus"):
            assert np.array_equal(got[k + 1][key], w[key]), (k, key)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [0, 3])
def test_gpu_self_search_and_specificity_join(dev, case, M):
    sites, guides, counts, hit_sum = case.self_search(M, True)
    res = dev.genome.search_self(PATTERN, M, 3, guide_pattern=GUIDE_PATTERN, score="hsu2013")
    got = list(zip((res.sites["contig"].astype(np.int64) - 1).tolist(), res.sites["position"].tolist(), (res.sites["strand"] == b"-").astype(int).tolist()))
    assert got == sites
    assert [g.decode() for g in res.guides] == guides and np.array_equal(res.counts.astype(np.int64), counts)
    assert [int(x) for x in res.hit_sum] == hit_sum
    plain = dev.genome.search_self(PATTERN, M, 3, guide_pattern=GUIDE_PATTERN)
    assert np.array_equal(plain.counts.astype(np.int64), case.self_search(M, False)[2]) and plain.hit_sum is None
    for kind in ("hsu2013", "none", "pair"):
        score = {"none": None, "hsu2013": "hsu2013", "pair": srch.PairTable(case.pair[0], case.pair[1], case.pair[2])}[kind]
        _assert_joined(case, dev.ref, dev.genome.specificity_columns(L, max_mm=M, score=score), M, kind)


def _family_table(case):
    return fam.FamilyTable(fam.parse_families(case.families), case.annotation.genes()[0])


@pytest.mark.gpu
def test_gpu_families(dev, case):
    """The family rows of the self search, the joined family columns, and the family selection through
    scan_score(select=...) at K = 1 and 5."""
    p = dev.ref
    table = _family_table(case)
    assert table.gene_family.tolist() == case.gene_family and table.size.tolist() == case.sizes
    rows = fam.genome_rows(table, dev.genome, dev.request)
    want = case.family_rows(3)
    res = dev.genome.search_self(PATTERN, 3, 3, guide_pattern=GUIDE_PATTERN, score="hsu2013", families=rows)
    got = list(zip((res.sites["contig"].astype(np.int64) - 1).tolist(), res.sites["position"].tolist(), (res.sites["strand"] == b"-").astype(int).tolist()))
    assert got == want["sites"]
    assert np.array_equal(res.site_family, want["site_family"]) and np.array_equal(res.site_gene, want["site_gene"])
    assert np.array_equal(res.fam_counts.astype(np.int64), want["fam_counts"])
    assert [int(x) for x in res.fam_sum] == want["fam_sum"] and [int(x) for x in res.fam_cover] == want["fam_cover"]
    # the joined family columns, per row of the case contigs' tables
    row_of = {s: r for r, s in enumerate(want["sites"])}
    cols = dev.genome.specificity_columns(L, families=rows)
    _assert_joined(case, p, cols, 3, "hsu2013")
    missing = 0
    for k, h in enumerate(case.hits):
        for strand, name in ((0, "plus"), (1, "minus")):
            pos = h["pos_" + name].astype(np.int64)
            r = np.array([row_of.get((k, int(x), strand), -1) for x in (pos - L if strand == 0 else pos).tolist()], dtype=np.int64)
            c = cols[k + 1]
            joined = r >= 0
            missing += int((c["fam_counts_" + name][joined][:, 0] == nat.SELF_UNJOINED_COUNT).sum())
            assert np.array_equal(c["fam_counts_" + name][joined].astype(np.int64), want["fam_counts"][r[joined]]), (k, name)
            assert [int(x) for x in c["fam_sum_" + name][joined]] == [want["fam_sum"][i] for i in r[joined].tolist()]
            assert [int(x) for x in c["fam_cover_" + name][joined]] == [want["fam_cover"][i] for i in r[joined].tolist()]
            assert np.array_equal(c["site_family_" + name][joined], want["site_family"][r[joined]])
            assert (c["fam_counts_" + name][~joined] == nat.SELF_UNJOINED_COUNT).all() and (c["site_family_" + name][~joined] == NONE).all()
    assert missing == 0
    # the selection with family limits, through the genome-level call
    try:
        for K in (1, 5):
            n_in, n_pass, picked, values = p.select_family(K, FAMILY_LIMITS)
            req = sel.Request(sel.Params(K), dev.request, families=table, **FAMILY_LIMITS)
            S = dev.genome.scan_score(L, specificity={}, select=req).selection
            order = np.argsort(p.gene, kind="stable")  # the Selection lists genes in GFF order
            assert np.array_equal(S.n_in, n_in[order]) and np.array_equal(S.n_pass, n_pass[order])
            at = 0
            for r in order:
                for j, v in enumerate(values[r]):
                    row = S.rows[at]
                    packed = int(picked[r, j])
                    minus, t = packed >> 31, packed & 0x7FFFFFFF
                    kc = int(np.searchsorted(p.rows_before["minus" if minus else "plus"], t, "right")) - 1
                    pos = int(p.tables["pos_minus" if minus else "pos_plus"][t]) - p.offsets[kc]
                    assert (int(row["gene"]), int(row["rank"]), int(row["contig"]), int(row["position"]), row["strand"]) == \
                        (int(p.gene[r]), j + 1, kc + 1, pos, b"-" if minus else b"+")
                    assert (int(S.outside_mm0[at]), int(S.outside_hit_sum[at]), int(S.members_hit[at]), int(S.family_size[at]),
                            int(S.fam_cover[at])) == v
                    at += 1
            assert at == len(S.rows) > 0
    finally:
        dev.scan()


def _merged_genes(p, slice_rows):
    t = p.tables
    cp, cm = t["pos_plus"].astype(np.int64) - 3, t["pos_minus"].astype(np.int64)
    n = sum(np.searchsorted(c, p.hi.astype(np.int64), "right") - np.searchsorted(c, p.lo.astype(np.int64), "left") for c in (cp, cm))
    return int((n > (slice_rows or 65536)).sum())


SLICES = pytest.mark.parametrize("slice_rows", [None, 64], ids=["default-slices", "slices-of-64"])


KERNELS = ("plain", "pairs", "coding", "edit", "splice")


@pytest.mark.gpu
@SLICES
@pytest.mark.parametrize("kernel", KERNELS)
def test_gpu_selection(dev, case, kernel, slice_rows):
    """n_in, n_pass and sel of every gene from the plain, the coding, the edit and the splice item kernels and the pair
    selection, at the default slices and with the genes cut into slices of 64 rows and merged."""
    p = dev.ref
    h = dev.select()
    try:
        if slice_rows:
            h.set_limits(slice_rows)
            h.set_pair_limits(slice_rows)
        if kernel == "plain":
            for K in KS:
                h.run(sel.Params(K))
                _same(h.fetch(), p.select(K), "plain K=%d" % K)
                assert h.stats()["merged_genes"] == _merged_genes(p, slice_rows) and (not slice_rows or _merged_genes(p, slice_rows) >= 4)
            return
        if kernel == "pairs":
            for K in KP:
                h.run_pairs(sel.Params(1), sel.PairParams(K, *PAIR_WINDOW))
                n_pass, n_pairs, pairs = h.fetch_pairs()
                want = p.pairs(K)
                assert np.array_equal(n_pass, want[0]) and np.array_equal(n_pairs, want[1]) and np.array_equal(pairs, want[2]), K
            return
        h.set_coding(dev.model())
        for K in KS:
            if kernel == "coding":
                for limits in CODING_LIMITS:
                    h.set_coding_limits(None if limits is None else coding.Limits(*limits))
                    h.run(sel.Params(K))
                    _same(h.fetch(), p.select_coding(K, limits), "coding K=%d %s" % (K, limits))
            elif kernel == "edit":
                for limits in EDIT_LIMITS:
                    h.set_edit_limits(baseedit.Window(*WINDOW), None if limits is None else baseedit.Limits(*limits))
                    h.run(sel.Params(K))
                    _same(h.fetch(), p.select_edit(K, limits), "edit K=%d %s" % (K, limits))
            else:
                for limits in SPLICE_LIMITS:
                    h.set_splice_limits(baseedit.Window(*WINDOW), "cbe", None if limits is None else baseedit.SpliceLimits(*limits))
                    h.run(sel.Params(K))
                    _same(h.fetch(), p.select_splice(K, limits), "splice K=%d %s" % (K, limits))
    finally:
        h.close()


@pytest.mark.gpu
def test_gpu_eval_kernels(dev, case):
    """coding_eval, edit_eval and splice_eval for every (gene, row in the gene): they read pos_minus[row] + 6 and
    pos_plus[row] - 3 and the step tables at these positions."""
    p = dev.ref
    g, packed, t = p.packed_members()
    h = dev.select()
    try:
        model = dev.model()
        assert int(model["at"].max()) >> 30 == 1
        h.set_coding(model)
        off, cover = h.coding_eval(g, packed)
        want = p.positions()
        assert np.array_equal(off, want[0][g, t]) and np.array_equal(cover, want[1][g, t]) and g.size == int(p.member.sum()) > 500
        targets, stops, stop_off = h.edit_eval(baseedit.Window(*WINDOW), g, packed)
        five = h.splice_eval(baseedit.Window(*WINDOW), "cbe", g, packed)
        at = 0
        for r, (edit, splice) in enumerate(zip(p.edits(), p.splices())):
            n = edit[0].size
            assert np.array_equal(t[at:at + n], edit[0]) and np.array_equal(t[at:at + n], splice[0])
            for got, want_col in zip((targets, stops, stop_off), edit[1:]):
                assert np.array_equal(got[at:at + n], want_col), ("edit", r)
            for got, want_col in zip(five, splice[1:]):
                assert np.array_equal(got[at:at + n], want_col), ("splice", r)
            at += n
        assert at == g.size
    finally:
        h.close()


@pytest.mark.gpu
@SLICES
def test_gpu_selection_behind_the_join(dev, case, slice_rows):
    """The selection over the joined specificity columns, and the family item kernel with its evaluation, on one arena's
    handles: the predicate reads the columns the join wrote at these rows."""
    p = dev.ref
    table = _family_table(case)
    pattern, gp, M, scheme = srch.check_specificity(L, 3)
    handles = []
    h = None
    try:
        srch._self_handles(dev.genome, pattern, gp, srch.SPECIFICITY_PAM_LEN, M, scheme, None, None, handles)
        srch._self_compare_all(handles, M)
        srch._family_compare_all(handles, fam.genome_rows(table, dev.genome, dev.request), 0)
        handles[0].join_hits(L)
        handles[0].family_join_hits(L)
        h = dev.select()
        if slice_rows:
            h.set_limits(slice_rows)
        for K in KS:
            params = sel.Params(K, 0.2)
            params.max_mm0, params.max_hit_sum = BOUNDS
            h.run(params, handles[0])
            _same(h.fetch(), p.select(K, 0.2, BOUNDS), "joined K=%d" % K)
        g = np.asarray(p.gene, np.int64)
        h.set_family(table.gene_family[g], np.array([table.family_size(int(x)) for x in g], np.uint32))
        for K, limits in [(K, FAMILY_LIMITS) for K in (1, 5, 64)] + [(K, FAMILY_TIE_LIMITS) for K in KS]:
            h.set_family_limits(sel.FamilyLimits(**limits))
            h.run(sel.Params(K), handles[0])
            n_in, n_pass, picked, values = p.select_family(K, limits)
            got = h.fetch()
            _same(got, (n_in, n_pass, picked), "family K=%d" % K)
            r, c = np.nonzero(picked != NONE)
            ev = h.family_eval(handles[0], r.astype(np.uint32), picked[r, c])
            assert [tuple(int(x[i]) for x in ev) for i in range(r.size)] == [values[a][b] for a, b in zip(r.tolist(), c.tolist())]
    finally:
        if h is not None:
            h.close()
        for x in handles:
            x.close()


@pytest.mark.gpu
def test_gpu_genome_level_selection(dev, case):
    """Genome.scan_score(select=...) with the specificity join, the CDS flag and the pairs: the Selection's rows are the
    reference's picks, contig-relative."""
    p = dev.ref
    try:
        params = sel.Params(5, 0.2, max_perfect=0, min_specificity=0.5)
        hits = dev.genome.scan_score(L, specificity=dict(max_mm=3), select=sel.Request(params, dev.request, pairs=sel.PairParams(5, *PAIR_WINDOW)))
        S = hits.selection
        spec = dict(p.spec(), max_mm0=BOUNDS[0], max_hit_sum=BOUNDS[1])
        n_in, n_pass, picked = p.select(5, 0.2, BOUNDS)
        order = np.argsort(p.gene, kind="stable")
        assert np.array_equal(S.n_in, n_in[order]) and np.array_equal(S.n_pass, n_pass[order]) and S.n_pass.sum() > 20
        want = []
        for r in order:
            for j, packed in enumerate(picked[r]):
                if packed == NONE:
                    break
                minus, t = int(packed) >> 31, int(packed) & 0x7FFFFFFF
                kc = int(np.searchsorted(p.rows_before["minus" if minus else "plus"], t, "right")) - 1
                want.append((int(p.gene[r]), j + 1, kc + 1, int(p.tables["pos_minus" if minus else "pos_plus"][t]) - p.offsets[kc],
                             b"-" if minus else b"+", int(_bits(p.tables["score_minus" if minus else "score_plus"])[t])))
        got = [(int(r["gene"]), int(r["rank"]), int(r["contig"]), int(r["position"]), r["strand"], int(_bits(r["score"]))) for r in S.rows]
        assert got == want
        pw = pairs_ref.pairs_numpy(p.tables, p.lo, p.hi, 5, *PAIR_WINDOW, min_score=0.2, spec=spec)
        assert np.array_equal(S.n_pairs, pw[1][order]) and S.n_pairs.sum() > 0 and len(S.pairs) == int(np.minimum(pw[1], 5).sum())
        _assert_joined(case, p, hits.columns, 3, "hsu2013")
    finally:
        dev.scan()


@pytest.mark.gpu
def test_gpu_variant_counts(dev, case):
    """crp_variant_counts behind the filler: the bucket index of a position with bit 30 set, the last bucket, the windows'
    far ends j + 2 + l and ends1 up to 2^31 - 1 -- every row against variant_reference.column_numpy -- and an empty track."""
    v = dev.ref.variants()
    n_plus, n_minus = dev.counts[0]
    dev.arena.variant_set_track(np.empty(0, np.uint32), np.empty(0, np.uint32))
    zp, zm = dev.arena.variant_counts(n_plus, n_minus, VARIANT_SEED)
    assert zp.size == n_plus and zm.size == n_minus and not zp.any() and not zm.any()
    dev.arena.variant_set_track(v["starts"], v["ends1"])
    for got, strand in zip(dev.arena.variant_counts(n_plus, n_minus, VARIANT_SEED), ("plus", "minus")):
        bad = np.flatnonzero(got != v[strand])
        assert bad.size == 0, (strand, bad[:5], got[bad[:5]], v[strand][bad[:5]], dev.ref.tables["pos_" + strand][bad[:5]])
    assert dev.arena.variant_counts_stats()["variants"] == len(v["intervals"])


@pytest.mark.gpu
def test_gpu_family_step(dev, case):
    """crp_select_family_step behind the filler, whole genes and slices of 64: the proposals of homeo and twins against
    nothing covered and against all ones but one member's bit, from family_set_reference.arena_best.  The tie gene's bit-equal
    scores on either side of 2^30 leave the choice to the word cut << 1 | strand, in the step kernel and in the pick kernel."""
    p = dev.ref
    cands = case.step_candidates()
    table = _family_table(case)
    F = len(case.sizes)
    words = [[0] * F] + [[ALL_ONES ^ 1 << bit] * F for bit in range(3)]
    pattern, gp, M, scheme = srch.check_specificity(L, 3)
    handles = []
    h = None
    try:
        srch._self_handles(dev.genome, pattern, gp, srch.SPECIFICITY_PAM_LEN, M, scheme, None, None, handles)
        srch._self_compare_all(handles, M)
        srch._family_compare_all(handles, fam.genome_rows(table, dev.genome, dev.request), 0)
        handles[0].join_hits(L)
        handles[0].family_join_hits(L)
        h = dev.select()
        g = np.asarray(p.gene, np.int64)
        h.set_family(table.gene_family[g], np.array([table.family_size(int(x)) for x in g], np.uint32))
        h.set_family_members(table.gene_member[g])
        for slice_rows in (0, 64):
            h.set_limits(slice_rows)
            for covered in words:
                best = h.family_step(sel.Params(1), handles[0], np.array(covered, np.uint64))
                want = fsr.arena_best(cands, case.sizes, covered, 0)
                for f, w in enumerate(want):
                    what = (slice_rows, covered[f], case.fam_names[f])
                    if w is None:
                        assert best["gain"][f] == 0, what
                        continue
                    row = int(p.rows_before["minus" if w["strand"] else "plus"][w["contig"]]) + w["index"] | w["strand"] << 31
                    tie = ((w["cut"] + p.offsets[w["contig"]]) << 1 | w["strand"]) & 0xFFFFFFFF
                    got = (int(best["gain"][f]), int(best["key"][f]), int(best["cover"][f]), int(g[int(best["gene"][f])]), int(best["row"][f]),
                           int(best["tie"][f]))
                    assert got == (w["gain"], w["key"], w["cover"], w["gene"], row, tie), what
            if slice_rows:
                assert h.family_step_stats()["items"] > len(g)  # the genes of more than 64 rows are cut
    finally:
        if h is not None:
            h.close()
        for x in handles:
            x.close()


def _same_named(got, want, names, what=""):
    for g, w, name in zip(got, want, names):
        assert np.array_equal(np.asarray(g, np.uint64), np.asarray(w, np.uint64)), (what, name)


@pytest.mark.gpu
def test_gpu_site_columns(dev, case):
    """crp_sites.hip behind the filler: the planes and the three rank kernels over every word of the arena -- 64 trips of the
    scan over the chunk sums at `straddle`, 128 at `top`, each from a non-zero carry (poly_a, span16) --, and the column kernel
    at every flank against site_reference over the moved-down letters.  The index's size is the stated formula; planes and
    ranks survive a re-scan; the plain selection reads this column."""
    p = dev.ref
    es = sites.EnzymeSet(case.enzymes())
    assert es.names == [n for n, _ in case.enzymes()] and es.m_max == 16
    try:
        first = {}
        for flank in hs.FLANKS:
            (gp, gm), = dev.genome.site_columns(es, dev.counts, flank)
            want = p.site_columns(flank)
            for got, s in ((gp, "plus"), (gm, "minus")):
                bad = np.flatnonzero(got != want[s]["value"])
                assert bad.size == 0, (flank, s, bad[:5], [hex(int(x)) for x in got[bad[:5]]], [hex(int(x)) for x in want[s]["value"][bad[:5]]])
            first[flank] = (gp, gm)
            st = dev.arena.site_stats()
            assert (st["rows"], st["enzymes"], st["flank"]) == (p.n_plus + len(p.tables["pos_minus"]), 8, flank)
            assert st["bytes"] == hs.index_bytes(8, p.words) == dev.genome.site_stats["bytes"]
        print("high positions, %s: site index of 8 enzymes %d bytes, planes %.2f ms, ranks %.2f ms" %
              (p.placement, st["bytes"], st["planes_ms"], st["rank_ms"]))
        built = (st["planes_ms"], st["rank_ms"])
        dev.scan()
        assert dev.arena.site_stats()["rows"] == 0  # the column is gone with the tables it belonged to
        for flank in (hs.CROSSING_FLANK, 16):
            (gp, gm), = dev.genome.site_columns(es, dev.counts, flank)
            assert np.array_equal(gp, first[flank][0]) and np.array_equal(gm, first[flank][1]), flank
        st = dev.arena.site_stats()
        assert (st["planes_ms"], st["rank_ms"]) == built  # nothing was built again
        # the plain selection over the resident column: no four-cutter in the guide, an assay with a cut-out motif at flank 1000
        dev.genome.site_columns(es, dev.counts, hs.CROSSING_FLANK, fetch=False)
        forbid, need = es.mask(list(hs.FOUR_CUTTERS)), es.mask(list(hs.CUT_OUT))
        h = dev.select()
        try:
            h.set_site_limits((forbid, need))
            for slice_rows in (0, 64):
                h.set_limits(slice_rows)
                for K in (1, 5):
                    h.run(sel.Params(K))
                    _same(h.fetch(), p.select_sites(K, hs.CROSSING_FLANK, forbid, need), "sites K=%d, slices of %d" % (K, slice_rows))
        finally:
            h.close()
    finally:
        dev.scan()


@pytest.mark.gpu
@SLICES
def test_gpu_spaced_selection(dev, case, slice_rows):
    """crp_select_spaced.hip behind the filler, whole genes and the piece path (slices of 64: one round per launch and the
    pick kernel): the tie words cut << 1 | strand on either side of bit 31 and the unsigned distances |cut - cut(p)| up to the
    twin's TWIN and one more."""
    p = dev.ref
    h = dev.select()
    try:
        if slice_rows:
            h.set_limits(slice_rows)
        for K in KS:
            for D in SPACINGS:
                h.run_spaced(sel.Params(K), D)
                _same_named(h.fetch_spaced(), p.spaced(K, D), ("n_pass", "n_spaced", "sel"), "spaced K=%d D=%d" % (K, D))
                assert h.spaced_stats()["spaced_cut_genes"] == (_merged_genes(p, slice_rows) if slice_rows else 0)
        assert not slice_rows or _merged_genes(p, slice_rows) >= 4
    finally:
        h.close()


@pytest.mark.gpu
@SLICES
def test_gpu_spaced_selection_behind_the_join(dev, case, slice_rows):
    """The spaced selection with the specificity bounds over the joined columns (test_gpu_selection_behind_the_join's set-up)."""
    p = dev.ref
    pattern, gp, M, scheme = srch.check_specificity(L, 3)
    handles = []
    h = None
    try:
        srch._self_handles(dev.genome, pattern, gp, srch.SPECIFICITY_PAM_LEN, M, scheme, None, None, handles)
        srch._self_compare_all(handles, M)
        handles[0].join_hits(L)
        h = dev.select()
        if slice_rows:
            h.set_limits(slice_rows)
        for K in KS:
            params = sel.Params(K, 0.2)
            params.max_mm0, params.max_hit_sum = BOUNDS
            h.run_spaced(params, 30, handles[0])
            _same_named(h.fetch_spaced(), p.spaced(K, 30, 0.2, BOUNDS), ("n_pass", "n_spaced", "sel"), "joined spaced K=%d" % K)
    finally:
        if h is not None:
            h.close()
        for x in handles:
            x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair_slice_rows, per_launch", [(0, 0), (64, 0), (64, 1)], ids=["default-slices", "slices-of-64", "slices-of-64-one-item-a-launch"])
def test_gpu_distinct_pairs(dev, case, pair_slice_rows, per_launch):
    """crp_select_pairs_distinct.hip behind the filler: partner runs streamed by position and the later rounds' skip over keys
    whose ties the cut sites decide, whole genes, cut genes, and one item a launch (the step and pick launches of every round).
    KP = 1 is the plain pair run bit for bit."""
    p = dev.ref
    h = dev.select()
    try:
        h.set_pair_limits(pair_slice_rows)
        h.set_pair_distinct_limits(per_launch)
        for K in KP_DISTINCT:
            h.run_pairs_distinct(sel.Params(1), sel.PairParams(K, *PAIR_WINDOW, distinct=True))
            got = h.fetch_pairs_distinct()
            _same_named(got, p.distinct(K), ("n_pass", "n_pairs", "n_distinct", "pairs"), "distinct KP=%d" % K)
            stats = h.pairs_distinct_stats()
            assert not pair_slice_rows or stats["cut_genes"] >= 4
            if K == 1:
                h.run_pairs(sel.Params(1), sel.PairParams(1, *PAIR_WINDOW))
                plain = h.fetch_pairs()
                assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and np.array_equal(got[3], plain[2])
    finally:
        h.close()


class SelfSession:
    """The self search of the device's genome under PATTERN, as tests/test_select_self.py's Session: the open handle and the
    fetched rows of its guide sites -- which must be the reference's at their arena positions."""

    def __init__(self, dev, M, scored):
        self.genome, self.handles = dev.genome, []
        try:
            pattern, gp, M, P, scheme = srch.check_self(PATTERN, M, SELF_P, GUIDE_PATTERN, "hsu2013" if scored else None)
            srch._self_handles(dev.genome, pattern, gp, P, M, scheme, None, None, self.handles)
            srch._self_compare_all(self.handles, M)
            pos, strand, hi, lo, counts, hit_sum = self.handles[0].fetch(scored)
            want = dev.ref.self_rows(M, scored)
            cpos, cstrand = dev.ref.candidates()
            assert tuple(self.handles[0].sizes()) == (int((cstrand == 0).sum()), int((cstrand == 1).sum()), want["pos"].size)
            assert np.array_equal(pos, want["pos"]) and np.array_equal(strand, want["strand"])
            assert np.array_equal(counts, want["counts"]) and (not scored or np.array_equal(hit_sum, want["hit_sum"]))
            assert np.array_equal(hi & np.uint32(SELF_REGION), want["hi"]) and np.array_equal(lo & np.uint32(SELF_REGION), want["lo"])
            self.rows = [dict(pos=pos, strand=strand, hi=hi, lo=lo, counts=counts, hit_sum=hit_sum if scored else None, cand=want["cand"])]
        except BaseException:
            self.close()
            raise

    def close(self):
        for h in self.handles:
            h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("M, scored", SELF_HANDLES, ids=["M%d-%s" % (m, "scored" if s else "counts") for m, s in SELF_HANDLES])
def test_gpu_self_selection(dev, case, M, scored):
    """crp_select_self.hip behind the filler: the keys position << 1, the bounds kernel's one word past the last, the item
    kernel's cut << 1 | strand and the CDS look-up's bucket cut >> 11 (at `top` the last one), whole genes, slices of 64 and one
    item a launch, against select_self_reference over the reference's rows."""
    import test_select_self as tss
    p = dev.ref
    s = SelfSession(dev, M, scored)
    try:
        for K in KS + (SELF_TIE_K[M],):
            sp = p.self_spec(K)
            for slice_rows in (0, 64):
                got, stats = tss.run_gpu(s, 0, p.lo, p.hi, sp, slice_rows)
                tss.assert_equal(s, 0, got, p.self_select(M, scored, K), sp)
                assert not slice_rows or stats["self_items"] > len(p.lo)
        got, stats = tss.run_gpu(s, 0, p.lo, p.hi, p.self_spec(5), 64, 1)
        tss.assert_equal(s, 0, got, p.self_select(M, scored, 5), p.self_spec(5))
        assert stats["self_launches"] == stats["self_items"] > len(p.lo)
        for what, limits in SELF_LIMITS.items():
            if what == "hit_sum" and not scored:
                continue
            sp = p.self_spec(5, **limits)
            for slice_rows in (0, 64):
                got, _ = tss.run_gpu(s, 0, p.lo, p.hi, sp, slice_rows)
                tss.assert_equal(s, 0, got, p.self_select(M, scored, 5, **limits), sp)
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_genome_level_self_selection(dev, case):
    """search.search_self(genome, select=...) -- Genome.search_self does not take select= --: the Selection's rows are the
    handle-level picks, contig-relative -- gene, rank, contig, position, strand and cut -- without and with require_cds."""
    import test_select_self as tss
    p = dev.ref
    offsets = np.array(p.offsets, np.int64)
    for cds in (False, True):
        s = SelfSession(dev, 3, True)
        try:
            sp = p.self_spec(5, cds=cds)
            got, _ = tss.run_gpu(s, 0, p.lo, p.hi, sp)
            tss.assert_equal(s, 0, got, p.self_select(3, True, 5, **(dict(cds=True) if cds else {})), sp)
        finally:
            s.close()
        request = ss.Request(ss.Params(5, require_cds=cds), dev.request, slice_rows=64 if cds else None)
        S = srch.search_self(dev.genome, PATTERN, 3, SELF_P, guide_pattern=GUIDE_PATTERN, score="hsu2013", select=request).selection
        order = np.argsort(p.gene, kind="stable")  # the Selection lists genes in GFF order
        assert np.array_equal(S.n_in, got["n_in"][order]) and np.array_equal(S.n_pass, got["n_pass"][order])
        want = []
        for r in order:
            for j in np.flatnonzero(got["sel"][r] != NONE):
                pos, minus = int(got["arena_pos"][r, j]), int(got["strand"][r, j])
                kc = int(np.searchsorted(offsets, pos, "right")) - 1
                cut = pos + (SELF_T - SELF_CUT if minus else SELF_CUT)
                want.append((int(p.gene[r]), int(j) + 1, kc + 1, pos - p.offsets[kc], b"-" if minus else b"+", cut - p.offsets[kc]))
        rows = [(int(r["gene"]), int(r["rank"]), int(r["contig"]), int(r["position"]), r["strand"], int(r["cut"])) for r in S.rows]
        assert rows == want and len(rows) == (20 if cds else 30)
