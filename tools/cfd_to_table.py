#!/usr/bin/env python3
"""Converts the two dictionaries the CFD publication's code distributes (Doench et al. 2016: mismatch scores and PAM
scores, as pickle or JSON files) into a pair-table file for `python -m cropsr_amd.search --score-table` on a 20 + NGG
pattern (NNNNNNNNNNNNNNNNNNNNNGG or ...NRG and the like, --pam-length 3).  DESIGN.md section 15, Pair tables, states the
key mapping:

  mismatch key  `rU:dG,20`: r = the guide's letter as RNA (U is the query letter T), d = the complement of the
                protospacer-sense site letter (dG: the site holds C), the number = the position counted from the
                PAM-distal end, 1-based (g = position - 1)
  PAM key       the last two letters of the site's PAM, such as `AG` (pam-offsets 1 2 of a 3-letter PAM)

The published numbers themselves are not part of this project: bring the files.

    python tools/cfd_to_table.py mismatch_score.pkl pam_scores.pkl -o cfd.txt
"""
import argparse
import json
import pickle
import re
import sys

G = 20
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def load(path):
    """A dictionary from a pickle or a JSON file (tried in that order)."""
    with open(path, "rb") as f:
        data = f.read()
    try:
        d = pickle.loads(data)
    except Exception:  # noqa: BLE001  (not a pickle: JSON)
        d = json.loads(data.decode())
    if not isinstance(d, dict):
        raise ValueError("%s does not hold a dictionary" % path)
    return {(k.decode() if isinstance(k, bytes) else str(k)): float(v) for k, v in d.items()}


def convert(mismatch, pam):
    """The table file's text from the two dictionaries; ValueError for a key outside the format or a missing entry."""
    pair = {}
    for key, v in mismatch.items():
        m = re.fullmatch(r"r([ACGU]):d([ACGT]),(\d+)", key)
        if not m or not 1 <= int(m.group(3)) <= G:
            raise ValueError("mismatch key %r is not of the form rU:dG,20 with a position 1..%d" % (key, G))
        a = "T" if m.group(1) == "U" else m.group(1)
        b = COMPLEMENT[m.group(2)]
        if a == b:
            continue  # (a match: not a mismatch entry)
        pair[(int(m.group(3)) - 1, a, b)] = v
    lines = ["# pair table of the CFD form for a 20-position guide region and a 3-letter PAM (cfd_to_table.py)",
             "pam-offsets 1 2"]
    for key in sorted(pam):
        if not re.fullmatch(r"[ACGT]{2}", key):
            raise ValueError("PAM key %r is not two letters of ACGT" % key)
        lines.append("pam %s %r" % (key, pam[key]))
    for g in range(G):
        for a in "ACGT":
            for b in "ACGT":
                if a == b:
                    continue
                if (g, a, b) not in pair:
                    raise ValueError("no mismatch entry for position %d, guide letter %s, site letter %s (key r%s:d%s,%d)" % (
                        g + 1, a, b, "U" if a == "T" else a, COMPLEMENT[b], g + 1))
                lines.append("pair %d %s %s %r" % (g, a, b, pair[(g, a, b)]))
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mismatch", help="the mismatch-score dictionary (pickle or JSON)")
    ap.add_argument("pam", help="the PAM-score dictionary (pickle or JSON)")
    ap.add_argument("-o", "--output", required=True, help="the pair-table file to write")
    args = ap.parse_args(argv)
    try:
        text = convert(load(args.mismatch), load(args.pam))
    except (OSError, ValueError) as e:
        ap.error(str(e))
    with open(args.output, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
