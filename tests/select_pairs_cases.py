"""The genome of tests/test_select_pairs.py: tests/select_cases.py's contigs and genes, plus the genes only the pair
selection needs.  The tests check on the reference's rows that each holds what its name claims."""
import numpy as np

import select_cases as cases


def build(orc):
    """select_cases.build(orc) with further gene rows appended to the GFF (the contigs are unchanged):
    one_strand     a stretch of c1 with at least three '+' cut sites and no '-' row's cut site in it
    repeat_core    the tandem repeat of c0 without its first and last copy: every row is one of a few 30-mers, each about
                   70 times, so hundreds of pairs tie on both scores
    short_pair     two neighbouring '+' cut sites of c2 and whatever lies between: a gene of very few rows
    """
    c = cases.build(orc)
    lines = c["gff"].rstrip("\n").split("\n")

    def gene(seq, lo, hi, ident):
        lines.append("%s\ttest\tgene\t%d\t%d\t.\t+\t.\tID=%s" % (seq, lo + 1, hi + 1, ident))
        c["ids"].append(ident)

    h = c["hits"][2]
    cp = (h["pos_plus"].astype(np.int64) - 3)[h["score_plus"] != -1.0]
    cm = h["pos_minus"].astype(np.int64)
    # the longest run of consecutive '+' cut sites without a '-' row between them
    before, upto = np.searchsorted(cm, cp, "left"), np.searchsorted(cm, cp, "right")
    best, start = (0, 0), 0
    for k in range(1, cp.size + 1):
        if k == cp.size or upto[k] != before[start]:
            best = max(best, (k - start, start))
            start = k
    n, k0 = best
    assert n >= 3
    gene("c1", int(cp[k0]), int(cp[k0 + n - 1]), "one_strand")
    h = c["hits"][3]
    cp = (h["pos_plus"].astype(np.int64) - 3)[h["score_plus"] != -1.0]
    gene("c2", int(cp[700]), int(cp[701]), "short_pair")
    unit = len(cases.REPEAT_UNIT)
    gene("c0", cases.REPEAT_AT + unit, cases.REPEAT_AT + unit * (cases.REPEAT_COPIES - 1) - 1, "repeat_core")
    c["gff"] = "\n".join(lines) + "\n"
    return c
