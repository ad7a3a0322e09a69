"""The small genome and GFF of tests/test_select.py: a few contigs of 6-30 kb and genes cut from the oracle's own rows,
so that every run length, edge and tie the selection kernels can get wrong is present -- the tests check that on the
reference's rows before they look at the device."""
import numpy as np

RUN_SIZES = (0, 1, 2, 4, 5, 6, 63, 64, 65, 129)  # K - 1, K, K + 1 for K = 1, 5, 64; a wave's trip +- 1; two trips + 1
NAMES = ["c0", "orphan", "c1", "c2"]
REPEAT_AT, REPEAT_UNIT, REPEAT_COPIES = 5000, b"ATCAGTACGATCAGGTACATGCATCCATGATCAGTACATA", 70
PAL_AT = 12000


def _revcomp(b):
    return bytes(b).translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def contigs():
    rng = np.random.default_rng(2016)
    rand = lambda n: rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()
    c0 = bytearray(rand(30000))
    c0[REPEAT_AT:REPEAT_AT + len(REPEAT_UNIT) * REPEAT_COPIES] = REPEAT_UNIT * REPEAT_COPIES
    # a reverse palindrome centred at i = PAL_AT + 28: the '+' hit at i and the '-' hit at i - 3 share their cut site
    # and their 30-mer, so their scores tie and only "'+' before '-'" orders them
    left = rand(25) + b"CCA"
    c0[PAL_AT:PAL_AT + 56] = left + _revcomp(left)
    c0[20000:20012] = b"N" * 12
    c0[21000:21060] = bytes(c0[21000:21060]).lower()
    c1 = bytearray(rand(20000))
    c1[7000:7003] = b"NNN"
    c2 = bytearray(rand(24000))
    c2[100:130] = b"N" * 30
    return [bytes(c0), rand(6000), bytes(c1), bytes(c2)]


def build(orc):
    """dict(contigs, names, gff (text), hits (the oracle's per contig), pal_cut, genes_by_id {id: row of the GFF's genes})."""
    texts = contigs()
    hits = [orc.scan_score(t, 20) for t in texts]
    lines = ["##gff-version 3", "# a comment", ""]
    ids = []

    def gene(seq, lo, hi, ident, attrs=None):
        """string indices lo..hi (dec = 0) -> 1-based coordinates"""
        lines.append("%s\ttest\tgene\t%d\t%d\t.\t+\t.\t%s" % (seq, lo + 1, hi + 1, attrs if attrs is not None else "ID=" + ident))
        ids.append(ident)

    def cds(seq, lo, hi, ident):
        lines.append("%s\ttest\tCDS\t%d\t%d\t.\t+\t0\tID=%s" % (seq, lo + 1, hi + 1, ident))

    def runs(contig, strand, tag):
        h = hits[contig]
        cut = h["pos_" + strand].astype(np.int64) - (3 if strand == "plus" else 0)
        scored = h["score_" + strand] != -1.0
        k = 200
        for n in RUN_SIZES:
            k += 37
            assert scored[k - 1:k + n + 1].all()
            if n == 0:
                while cut[k + 1] - cut[k] < 2:
                    k += 1
                gene(NAMES[contig], cut[k] + 1, cut[k + 1] - 1, "%s_run0" % tag)
            else:
                gene(NAMES[contig], cut[k], cut[k + n - 1], "%s_run%d" % (tag, n))

    runs(2, "plus", "p")
    runs(3, "minus", "m")
    # one strand only: a '+' cut site that no '-' row shares
    cp, cm = hits[2]["pos_plus"].astype(np.int64) - 3, hits[2]["pos_minus"].astype(np.int64)
    only = [int(c) for c, s in zip(cp[50:400], hits[2]["score_plus"][50:400]) if s != -1.0 and c not in set(cm.tolist())][0]
    gene("c1", only, only, "plus_only")
    n0, n3 = len(texts[0]), len(texts[3])
    gene("c0", 0, 400, "first_rows")                    # from the first character: the tables' first rows
    lines.append("c0\ttest\tgene\t0\t250\t.\t-\t.\tID=clipped_left")  # coordinate 0: index -1, clipped
    ids.append("clipped_left")
    gene("c2", n3 - 300, n3 + 500, "last_rows")         # past the end: clipped, holds the tables' last rows, unscored ones among them
    gene("c1", 0, len(texts[2]) - 1, "whole_c1")
    gene("c0", 1000, 9000, "outer")
    gene("c0", 2000, 3000, "nested")
    gene("c0", 8000, 11000, "overlapping")
    gene("c0", 2000, 3000, "duplicate")
    gene("c0", 2000, 3000, "nested")                    # the same label twice
    gene("c0", REPEAT_AT - 100, REPEAT_AT + len(REPEAT_UNIT) * REPEAT_COPIES + 100, "repeat")
    pal_cut = PAL_AT + 28 - 3
    gene("c0", pal_cut, pal_cut, "palindrome")
    gene("c0", 19990, 20030, "n_run")                   # rows whose guide holds an N: no guide site, unjoined
    gene("c0", 25000, 29000, "no_cds")
    lines.append("c0\ttest\tgene\t500\t400\t.\t+\t.\tID=backwards")       # start > end: no range
    ids.append("backwards")
    lines.append("nowhere\ttest\tgene\t10\t900\t.\t+\t.\tID=unknown_seqid")
    ids.append("unknown_seqid")
    gene("c0", n0 + 10, n0 + 90, "beyond_end")          # clipping leaves nothing
    # labels by Name / Parent / nothing, blanks around the attributes
    gene("c1", 3000, 3500, "by_name", " Name=by_name ; Note=x")
    gene("c1", 3600, 3900, "by_parent", "Parent=by_parent")
    gene("c1", 4000, 4100, ".", "Note=none")
    # odd lines the parser must pass over
    lines += ["c1\ttest\tgene\t12x\t40\t.\t+\t.\tID=bad_start", "c1\ttest\tgene\t10\t40", "c1\ttest\tmRNA\t10\t4000\t.\t+\t.\tID=an_mrna",
              "c1\ttest\tgene\t\t40\t.\t+\t.\tID=empty_start", "###"]
    # CDS rows: inside some genes, across the repeat, none in no_cds
    cds("c0", 1500, 1900, "outer.cds1")
    cds("c0", 2400, 2700, "nested.cds1")
    cds("c0", REPEAT_AT + 400, REPEAT_AT + 2000, "repeat.cds1")
    cds("c1", 100, 9000, "whole.cds1")
    cds("c2", n3 - 200, n3 - 1, "last.cds1")
    cds("c2", 3000, 16000, "m.cds")
    return dict(contigs=texts, names=list(NAMES), gff="\n".join(lines) + "\n", hits=hits, pal_cut=pal_cut, ids=ids)
