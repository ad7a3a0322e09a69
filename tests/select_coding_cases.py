"""The inputs of tests/test_select_coding.py.

ZOO: small GFF texts, one per thing the model builder can get wrong, over contigs of a few hundred letters -- small enough
that the tests compare every cut boundary of every text with the restated definition.

build(orc): the 80 kb genome of select_cases with a GFF of its own, whose genes, transcripts and exons are cut from the
oracle's rows: exon edges lie on the rows' own cut boundaries, so that a cut at the first letter of an exon, one letter in,
at its last letter and one past it all occur -- the tests check that on the reference's rows before they look at the device.
"""
import numpy as np

import select_cases

# Steps per gene row.  The issue's list names 1 where this says 0: the layout cannot make a row of one step -- a step that
# leaves "nothing holds" is followed by the one that returns to it, and a one-letter exon gives 2 -- so 0 is its smallest
# row; test_gpu_a_row_of_one_step sends a hand-made one-step model through both kernels instead.
STEP_COUNTS = (0, 2, 63, 64, 65, 129, 257)


def _row(seq, typ, start, end, strand, attrs):
    return "%s\ttest\t%s\t%d\t%d\t.\t%s\t.\t%s" % (seq, typ, start, end, strand, attrs)


def _zoo():
    z = {}
    z["plain"] = [_row("s", "gene", 10, 200, "+", "ID=g"), _row("s", "mRNA", 10, 200, "+", "ID=t;Parent=g"),
                  _row("s", "CDS", 20, 40, "+", "ID=c1;Parent=t"), _row("s", "CDS", 60, 90, "+", "ID=c2;Parent=t"),
                  _row("s", "CDS", 150, 180, "+", "ID=c3;Parent=t")]
    z["minus"] = [r.replace("\t+\t", "\t-\t") for r in z["plain"]]
    z["comma_parent"] = [_row("s", "gene", 10, 200, "+", "ID=g"), _row("s", "gene", 100, 300, "-", "ID=h"),
                         _row("s", "mRNA", 10, 300, "+", "ID=t;Parent=x,g,,h"), _row("s", "mRNA", 10, 200, "+", "ID=u;Parent=g,g"),
                         _row("s", "CDS", 20, 40, "+", "Parent=t,u"), _row("s", "CDS", 120, 140, "+", "Parent=u,u"),
                         _row("s", "CDS", 150, 260, "+", "Parent=t")]
    z["child_before_parent"] = [_row("s", "CDS", 20, 40, "+", "Parent=t"), _row("s", "mRNA", 10, 200, "+", "ID=t;Parent=g"),
                                _row("s", "CDS", 60, 90, "+", "Parent=t"), _row("s", "gene", 10, 200, "-", "ID=g")]
    z["cds_off_the_gene"] = [_row("s", "gene", 10, 200, "+", "ID=g"), _row("s", "CDS", 20, 40, "+", "Parent=g"),
                             _row("s", "CDS", 60, 90, "+", "Parent=g")]
    z["implicit_and_explicit"] = [_row("s", "mRNA", 10, 200, "+", "ID=t;Parent=g"), _row("s", "gene", 10, 200, "+", "ID=g"),
                                  _row("s", "CDS", 20, 40, "+", "Parent=g"), _row("s", "CDS", 60, 80, "+", "Parent=t"),
                                  _row("s", "mRNA", 10, 200, "+", "ID=u;Parent=g"), _row("s", "CDS", 100, 120, "+", "Parent=u")]
    z["duplicate_ids"] = [_row("s", "gene", 10, 200, "+", "ID=g"), _row("s", "gene", 50, 250, "-", "ID=g"),
                          _row("s", "mRNA", 10, 200, "+", "ID=t;Parent=g"), _row("s", "mRNA", 10, 200, "+", "ID=t;Parent=g"),
                          _row("s", "CDS", 20, 40, "+", "Parent=t"), _row("s", "CDS", 60, 90, "+", "Parent=g")]
    z["mrna_on_another_seqid"] = [_row("s", "gene", 10, 200, "+", "ID=g"), _row("other", "mRNA", 10, 200, "+", "ID=t;Parent=g"),
                                  _row("other", "CDS", 20, 40, "+", "Parent=t"), _row("s", "mRNA", 10, 200, "+", "ID=u;Parent=g"),
                                  _row("other", "CDS", 60, 80, "+", "Parent=u"), _row("s", "CDS", 100, 130, "+", "Parent=u")]
    z["transcript_type"] = [_row("s", "gene", 10, 200, "-", "ID=g"), _row("s", "transcript", 10, 200, "-", "ID=t;Parent=g"),
                            _row("s", "CDS", 20, 40, "-", "Parent=t"), _row("s", "exon", 20, 60, "-", "Parent=t")]
    z["strand_dot"] = [_row("s", "gene", 10, 200, ".", "ID=g"), _row("s", "CDS", 20, 40, "+", "Parent=g"),
                       _row("s", "gene", 10, 200, "?", "ID=h"), _row("s", "CDS", 20, 40, "+", "Parent=h"),
                       _row("s", "gene", 10, 200, "+-", "ID=i"), _row("s", "CDS", 20, 40, "+", "Parent=i")]
    z["transcript_without_cds"] = [_row("s", "gene", 10, 200, "+", "ID=g"), _row("s", "mRNA", 10, 200, "+", "ID=t;Parent=g"),
                                   _row("s", "mRNA", 10, 200, "+", "ID=u;Parent=g"), _row("s", "CDS", 20, 40, "+", "Parent=u"),
                                   _row("s", "gene", 210, 260, "+", "ID=empty"), _row("s", "mRNA", 210, 260, "+", "ID=v;Parent=empty")]
    z["overlapping_and_duplicate_cds"] = [_row("s", "gene", 10, 200, "+", "ID=g"), _row("s", "mRNA", 10, 200, "+", "ID=t;Parent=g"),
                                          _row("s", "CDS", 20, 40, "+", "Parent=t"), _row("s", "CDS", 30, 50, "+", "Parent=t"),
                                          _row("s", "CDS", 20, 40, "+", "Parent=t"), _row("s", "CDS", 51, 60, "+", "Parent=t"),
                                          _row("s", "CDS", 25, 28, "+", "Parent=t"), _row("s", "CDS", 62, 70, "+", "Parent=t")]
    z["short_cds"] = [_row("s", "gene", 10, 200, "+", "ID=g"), _row("s", "mRNA", 10, 200, "+", "ID=t;Parent=g"),
                      _row("s", "CDS", 20, 20, "+", "Parent=t"), _row("s", "CDS", 30, 31, "+", "Parent=t"),
                      _row("s", "gene", 10, 200, "-", "ID=h"), _row("s", "CDS", 50, 50, "-", "Parent=h")]
    z["start_after_end"] = [_row("s", "gene", 10, 200, "+", "ID=g"), _row("s", "CDS", 40, 20, "+", "Parent=g"),
                            _row("s", "CDS", 60, 90, "+", "Parent=g"), _row("s", "gene", 10, 200, "+", "ID=h"),
                            _row("s", "CDS", 40, 20, "+", "Parent=h"), _row("s", "gene", 200, 10, "+", "ID=backwards"),
                            _row("s", "CDS", 20, 40, "+", "Parent=backwards")]
    z["tie"] = [_row("s", "gene", 10, 200, "-", "ID=g"), _row("s", "mRNA", 10, 200, "-", "ID=t;Parent=g"),
                _row("s", "mRNA", 10, 200, "-", "ID=u;Parent=g"), _row("s", "CDS", 100, 129, "-", "Parent=u"),
                _row("s", "CDS", 20, 34, "-", "Parent=t"), _row("s", "CDS", 60, 74, "-", "Parent=t"),
                _row("s", "gene", 210, 300, "+", "ID=h"), _row("s", "mRNA", 210, 300, "+", "ID=v;Parent=h"),
                _row("s", "CDS", 220, 229, "+", "Parent=h"), _row("s", "CDS", 240, 249, "+", "Parent=v")]
    z["outside_gene_and_contig"] = [_row("s", "gene", 100, 200, "+", "ID=g"), _row("s", "CDS", 0, 120, "+", "Parent=g"),
                                    _row("s", "CDS", 180, 700, "+", "Parent=g"), _row("s", "gene", 300, 900, "-", "ID=h"),
                                    _row("s", "CDS", 330, 800, "-", "Parent=h"), _row("s", "gene", 350, 360, "-", "ID=far"),
                                    _row("s", "CDS", 600, 650, "-", "Parent=far")]
    z["empty_values"] = [_row("s", "gene", 10, 200, "+", "ID="), _row("s", "CDS", 20, 40, "+", "Parent="),
                         _row("s", "gene", 10, 200, "+", "Name=n"), _row("s", "mRNA", 10, 200, "+", "Parent=g"),
                         _row("s", "gene", 10, 200, "+", "ID=g;ID=other"), _row("s", "CDS", 50, 70, "+", "Parent=g;Parent=other"),
                         _row("s", "CDS", 80, 90, "+", " Parent=g ; Note=x")]
    z["nested_and_antisense"] = [_row("s", "gene", 10, 300, "+", "ID=outer"), _row("s", "CDS", 20, 60, "+", "Parent=outer"),
                                 _row("s", "CDS", 200, 260, "+", "Parent=outer"), _row("s", "gene", 100, 150, "+", "ID=nested"),
                                 _row("s", "CDS", 110, 140, "+", "Parent=nested"), _row("s", "gene", 30, 250, "-", "ID=anti"),
                                 _row("s", "CDS", 40, 220, "-", "Parent=anti")]
    z["odd_lines"] = ["##gff-version 3", "", "s\ttest\tmRNA\t10\t200", _row("s", "gene", 10, 200, "+", "ID=g"),
                      "s\ttest\tmRNA\t1x\t200\t.\t+\t.\tID=t;Parent=g", "s\ttest\tCDS\t\t40\t.\t+\t.\tParent=g",
                      "s\ttest\tCDS\t20\t40\t.\t+\t.\tParent=g\textra\tfields", "# s\ttest\tCDS\t60\t90\t.\t+\t.\tParent=g",
                      "s\ttest\tCDS\t1234567890123456789\t40\t.\t+\t.\tParent=g", "\t\t\t\t\t\t\t\t", "s\ttest\tCDS\t100\t110\t.\t+\t.\t"]
    return {name: "\n".join(rows) + "\n" for name, rows in z.items()}


ZOO = _zoo()
ZOO_CONTIGS = {"s": 400, "other": 300}  # lengths of the contig strings the zoo's seqids name


class _Gff:
    """GFF lines from string indices (dec = 0: coordinate = index + 1)."""

    def __init__(self):
        self.lines, self.ids = ["##gff-version 3"], []

    def gene(self, seq, lo, hi, ident, strand):
        self.lines.append(_row(seq, "gene", lo + 1, hi + 1, strand, "ID=" + ident))
        self.ids.append(ident)

    def mrna(self, seq, lo, hi, ident, parent, strand):
        self.lines.append(_row(seq, "mRNA", lo + 1, hi + 1, strand, "ID=%s;Parent=%s;longest=1" % (ident, parent)))

    def cds(self, seq, exons, parent, strand):
        for a, b in exons:
            self.lines.append(_row(seq, "CDS", a + 1, b + 1, strand, "Parent=" + parent))


def boundaries(hit):
    """Ascending cut boundaries of a contig's scored rows: i - 3 on the '+' table, j + 6 on the '-' table."""
    cp = hit["pos_plus"].astype(np.int64)[hit["score_plus"] != -1.0] - 3
    cm = hit["pos_minus"].astype(np.int64)[hit["score_minus"] != -1.0] + 6
    return np.unique(np.concatenate([cp, cm]))


def build(orc):
    """dict(contigs, names, gff, hits, ids, exact: {gene id: (first letter, last letter) of its one exon})."""
    texts, names = select_cases.contigs(), list(select_cases.NAMES)
    hits = [orc.scan_score(t, 20) for t in texts]
    B = [boundaries(h) for h in hits]
    gff = _Gff()
    exact = {}

    def near(k, x):
        return int(B[k][np.searchsorted(B[k], x)])

    def edge_exons(k, x):
        """Four exons from x on whose edges lie on rows' boundaries: a cut at the first letter (c = a), one letter in
        (c = a + 1), at the last letter (c = b) and one past it (c = b + 1)."""
        x1, x2, x3, x4 = near(k, x), near(k, x + 150), near(k, x + 300), near(k, x + 450)
        return [(x1, x1 + 60), (x2 - 1, x2 + 58), (x3 - 50, x3), (x4 - 51, x4 - 1)]

    # '+' and '-' genes with edge-aligned exons, rows in the introns
    for seq, k, strand, ident in (("c0", 0, "+", "edges_plus"), ("c1", 2, "-", "edges_minus")):
        ex = edge_exons(k, 1100)
        gff.gene(seq, 1000, 1900, ident, strand)
        gff.mrna(seq, 1000, 1900, ident + ".1", ident, strand)
        gff.cds(seq, ex, ident + ".1", strand)
    # one exon, hanging off the gene; three exons
    gff.gene("c0", 2000, 2400, "one_exon", "-")
    gff.cds("c0", [(2050, 2350)], "one_exon", "-")
    gff.gene("c0", 2500, 3200, "three_exons", "+")
    gff.mrna("c0", 2500, 3200, "three_exons.1", "three_exons", "+")
    gff.cds("c0", [(2550, 2650), (2800, 2900), (3000, 3150)], "three_exons.1", "+")
    # two transcripts that share only their first exon; the second one is the longer: primary
    gff.gene("c0", 3300, 4300, "shared_first", "+")
    gff.mrna("c0", 3300, 4300, "shared_first.1", "shared_first", "+")
    gff.mrna("c0", 3300, 4300, "shared_first.2", "shared_first", "+")
    gff.cds("c0", [(3350, 3500), (3700, 3800)], "shared_first.1", "+")
    gff.cds("c0", [(3350, 3500), (3900, 4200)], "shared_first.2", "+")
    # the primary tie: equal lengths, the earlier row wins
    gff.gene("c0", 4400, 5000, "tie", "-")
    gff.mrna("c0", 4400, 5000, "tie.1", "tie", "-")
    gff.mrna("c0", 4400, 5000, "tie.2", "tie", "-")
    gff.cds("c0", [(4700, 4899)], "tie.2", "-")
    gff.cds("c0", [(4450, 4549), (4600, 4699)], "tie.1", "-")
    # a gene nested in another's intron, and an antisense gene over the outer one's second exon: shared rows, other answers
    gff.gene("c0", 13000, 17000, "outer", "+")
    gff.cds("c0", [(13100, 13600), (15500, 16500)], "outer", "+")
    gff.gene("c0", 14000, 14800, "nested", "+")
    gff.cds("c0", [(14100, 14700)], "nested", "+")
    gff.gene("c0", 15000, 16800, "antisense", "-")
    gff.cds("c0", [(15200, 16000), (16200, 16700)], "antisense", "-")
    # no model: no CDS; a strand that is none
    gff.gene("c0", 17500, 18000, "no_cds", "+")
    gff.gene("c0", 18100, 18600, "no_strand", ".")
    gff.cds("c0", [(18150, 18550)], "no_strand", "+")
    # clipped by the start of the text (coordinate 0 is index -1) and running past the contig's end, '-': its offsets
    # count the letters beyond the end
    gff.lines.append(_row("c0", "gene", 0, 600, "+", "ID=clipped_left"))
    gff.ids.append("clipped_left")
    gff.lines.append(_row("c0", "CDS", 0, 400, "+", "Parent=clipped_left"))
    n2 = len(texts[3])
    gff.gene("c2", n2 - 600, n2 + 500, "past_end", "-")
    gff.cds("c2", [(n2 - 500, n2 - 300), (n2 - 150, n2 + 300)], "past_end", "-")
    # limits hit with equality: one exon of 200 letters whose letter 10 (min 5 %) resp. 130 (max 65 %) begins at a row's boundary
    for ident, at, strand, want in (("exact_min", 19000, "+", 10), ("exact_max", 19500, "+", 130), ("exact_min_minus", 22000, "-", 190),
                                    ("exact_max_minus", 22500, "-", 70)):
        x = near(0, at + want)
        a = x - want  # off = c - a on a '+' gene, 200 - (c - a) on a '-' gene
        gff.gene("c0", a - 30, a + 230, ident, strand)
        gff.cds("c0", [(a, a + 199)], ident, strand)
        exact[ident] = (a, a + 199)
    # step counts per gene row: an exon of 2+ letters gives three change points, a one-letter exon two
    at = 1000
    for steps, full, single in ((2, 0, 1), (63, 21, 0), (64, 20, 2), (65, 21, 1), (129, 43, 0), (257, 85, 1)):
        assert 3 * full + 2 * single == steps
        exons, x = [], at + 10
        for j in range(full + single):
            n = 12 if j < full else 1
            exons.append((x, x + n - 1))
            x += n + 8
        ident = "steps%d" % steps
        strand = "+" if steps % 2 else "-"
        gff.gene("c2", at, x + 10, ident, strand)
        gff.mrna("c2", at, x + 10, ident + ".1", ident, strand)
        gff.cds("c2", exons, ident + ".1", strand)
        at = x + 100
    assert at < n2 - 700
    return dict(contigs=texts, names=names, gff="\n".join(gff.lines) + "\n", hits=hits, ids=gff.ids, exact=exact)
