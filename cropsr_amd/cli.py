"""`python -m cropsr_amd` -- the CROPSR command line on top of the MI355X engine.

Same flags, defaults, stdout lines, time.txt and CSV bytes as the reference's
CROPSR.py (v1.11b); the PAM scan and the scoring run in libcropsr_hip.so
instead of re/str.replace/numpy.  Reference anchors are given per step.

Differences that are NOT observable in the outputs:
  * all contigs are uploaded and scanned in ONE arena pass before the per-contig
    output loop starts (the reference scans inside the loop, CROPSR.py:413-434);
  * the 5 s sleep per contig (CROPSR.py:478) is kept only with --reference-sleep.
"""
import argparse
import sys
import time
from multiprocessing import cpu_count

import numpy as np

from . import fasta, hitcols, rows

__version__ = "1.11b"  # the CROPSR version whose behaviour is reproduced

BANNER = r"""
################################################################################
##                                                                            ##
##                                                                            ##
##          .o88b.   d8888b.    .d88b.    d8888b.   .d8888.   d8888b.         ##
##         d8P  Y8   88  `8D   .8P  Y8.   88  `8D   88'  YP   88  `8D         ##
##         8P        88oobY'   88    88   88oodD'   `8bo.     88oobY'         ##
##         8b        88`8b     88    88   88ººº       `Y8b.   88`8b           ##
##         Y8b  d8   88 `88.   `8b  d8'   88        db   8D   88 `88.         ##
##          `Y88P'   88   YD    `Y88P'    88        `8888Y'   88   YD         ##
##                                                                            ##
##                                                                            ##
################################################################################
U.S. Dept. of Energy's Center for Advanced Bioenergy and Bioproducts Innovation
University of Illinois at Urbana-Champaign
"""


def build_parser():
    """The reference's flags (CROPSR.py:24-49) plus engine options that default
    to reference behaviour."""
    p = argparse.ArgumentParser(prog="CROPSR.py")
    p.add_argument("-f", "--fasta", metavar="", required=True, dest="f",
                   help="[required] path to input file in FASTA format")
    p.add_argument("-g", "--gff", metavar="", dest="g", help="path to input file in GFF format")
    p.add_argument("-p", "--phytozome", metavar="", dest="p", default=None,
                   help="path to input annotation info file in TXT format, default = None")
    p.add_argument("-o", "--output", metavar="", dest="o", default="data.csv",
                   help="path to output file, default = data.csv")
    p.add_argument("-l", "--length", metavar="", dest="l", type=int, default=20,
                   help="length of the gRNA se3quence, default = 20")
    p.add_argument("-L", "--flanking", metavar="", dest="L", type=int, default=200,
                   help="length of flanking region for verification, default = 200")
    p.add_argument("--cas9", action="store_true",
                   help="specifies that design will be made for the Cas9 CRISPR system")
    p.add_argument("-v", "--verbose", action="store_true",
                   help="prints visual indicators for each iteration")
    eng = p.add_argument_group("MI355X engine")
    eng.add_argument("--device", type=int, default=None,
                     help="HIP device index, default = 0 (LOCAL_RANK under torch.distributed.run)")
    eng.add_argument("--gpus", type=int, default=1,
                     help="run on this many GPUs of the node, one process per GPU: contigs (cut where longer than a "
                          "GPU's share) are scanned in parallel and the hit tables gathered to the first one over RCCL; "
                          "the ranks are started here unless a launcher (torch.distributed.run) already did")
    eng.add_argument("--devices", default=None, metavar="LIST",
                     help="run on these HIP devices from THIS one process, e.g. 0,1,2,3: the genome is cut into equal "
                          "contiguous shares, every device scans its own and the hit tables are gathered to the first one "
                          "(RCCL) -- all inside the library (its node handle); no launcher, no ranks.  Same CSV bytes")
    eng.add_argument("--seed", type=int, default=None,
                     help="seed numpy's global RNG so crispr_id is reproducible (reference: unseeded)")
    eng.add_argument("--csv-writer", choices=["native", "python"], default="native",
                     help="native: multi-threaded C++ row formatter (same bytes); python: csv module like the reference")
    eng.add_argument("--each-contig-once", action="store_true",
                     help="NOT reference behaviour: write every contig's rows once instead of re-writing all "
                          "earlier contigs on every pass (the reference never clears Complete_dataset, "
                          "CROPSR.py:407, which makes multi-contig genomes quadratic)")
    eng.add_argument("--reference-sleep", action="store_true",
                     help="also reproduce the reference's 5 s pause per contig")
    eng.add_argument("--score-finalize", choices=["gpu", "host"], default="gpu",
                     help="gpu (default): on_site_score comes from the GPU, whose exp is glibc's -- the bytes the "
                          "reference prints on a host without AVX-512; host: the GPU delivers the pre-sigmoid sum "
                          "(CROPSR.py:312) and THIS host's numpy applies 1/(1+np.exp(.)) (CROPSR.py:313), so the CSV "
                          "equals what the reference prints on this very host (numpy's exp differs in the last bit "
                          "between CPU families)")
    eng.add_argument("--offtarget", action="store_true",
                     help="NOT in the reference: genome-wide off-target seed scan; appends four columns "
                          "offtarget_seed_mm0..3 (other PAM-adjacent sites whose 12-nt PAM-proximal seed differs in "
                          "0..3 places; -1 where the guide has no 12-base seed)")
    eng.add_argument("--specificity", action="store_true",
                     help="NOT in the reference: genome-wide specificity of every guide, full length: every row's guide against "
                          "every candidate site of the genome (the self search of cropsr_amd.search, joined onto the rows on the "
                          "GPU); appends the columns self_mm0..self_mmM (other candidate sites with exactly that many mismatches), "
                          "self_hit_sum and specificity = 1 / (1 + self_hit_sum / 2^30); -1 where the row's guide is no guide site "
                          "(a character that is no base, a window the contig end cuts); one GPU")
    eng.add_argument("--specificity-mismatches", type=int, default=None, metavar="M",
                     help="with --specificity: most mismatches counted (0..4, default 3)")
    eng.add_argument("--specificity-pam", default=None, metavar="PAM",
                     help="with --specificity: the PAM of the candidate sites, 3 letters over ACGTRYSWKMBDHVN that accept what NGG "
                          "accepts (default NRG: NAG sites count as off-targets)")
    # (the two exclude each other: specificity_request refuses the pair with the other refusals, in one voice)
    eng.add_argument("--specificity-weights", metavar="FILE", default=None,
                     help="with --specificity: mismatch weights, one number in [0, 1] per guide position, PAM-distal first, in "
                          "place of the Hsu 2013 weights (which exist for -l 20 only); not with --specificity-table")
    eng.add_argument("--specificity-table", metavar="FILE", default=None,
                     help="with --specificity: a hit score of the CFD form, the pair table of FILE (cropsr_amd.search "
                          "parse_pair_table, tools/cfd_to_table.py); not with --specificity-weights")
    eng.add_argument("--annotate", action="store_true",
                     help="NOT in the reference (which parses the GFF and drops it, CROPSR.py:375): fill the "
                          "`features` column with the gene/CDS rows of the GFF (-g) that contain the cut site, "
                          "named through the Phytozome annotation_info file (-p) when given")
    eng.add_argument("--select", type=int, default=None, metavar="K",
                     help="NOT in the reference: for every `gene` row of the GFF (-g), the K (1..64) best-scoring guides whose cut "
                          "site lies in the gene and that pass the --select-* thresholds, chosen on the GPU and written to their own "
                          "small CSV (gene, rank, passing, then the main table's fields without crispr_id); -l 20, one GPU")
    eng.add_argument("--select-output", metavar="FILE", default=None,
                     help="with --select: the selection file, default = the -o path + .selected.csv")
    eng.add_argument("--select-min-score", type=float, default=None, metavar="X",
                     help="with --select: only guides with on_site_score >= X (default 0)")
    eng.add_argument("--select-max-perfect", type=int, default=None, metavar="N",
                     help="with --select and --specificity: only guides with at most N other perfect copies (self_mm0 <= N)")
    eng.add_argument("--select-min-specificity", type=float, default=None, metavar="S",
                     help="with --select and --specificity: only guides whose specificity is at least S (S <= 0: no bound)")
    eng.add_argument("--select-cds", action="store_true",
                     help="with --select: only guides whose cut site lies in a CDS row of the GFF (positional, like --annotate)")
    eng.add_argument("--select-only", action="store_true",
                     help="with --select: write the selection file only, not the main table (no ids are drawn)")
    eng.add_argument("--select-min-spacing", type=int, default=None, metavar="D",
                     help="with --select: the K guides of a gene cut at least D letters of the assembly apart -- the guides are taken "
                          "best first, and one whose cut site lies within D - 1 letters of a guide already taken is passed over -- "
                          "chosen on the GPU (1..2147483647; 1 only forbids two guides with one cut site); the selection file keeps its "
                          "columns, `rank` is the pick order and `passing` counts all passing guides; not together with the coding-"
                          "position, stop-codon, splice-site or family filters")
    eng.add_argument("--properties", action="store_true",
                     help="NOT in the reference: the guide's own sequence quality, computed on the GPU from the l letters of every "
                          "row's guide; appends the columns guide_gc (letters that are C or G), guide_run (longest run of one base), "
                          "guide_t_run (longest run of T in the spacer: TTTT ends Pol III transcription) and guide_stem (longest "
                          "hairpin stem with a loop of at least 3); -l 1..50, one GPU")
    eng.add_argument("--select-pairs", type=int, default=None, metavar="KP",
                     help="with --select: also the best KP (1..64) PAIRS of passing guides of every gene -- two guides in one array that "
                          "cut out the piece between them, ranked by the weaker guide's on_site_score -- chosen on the GPU and written "
                          "to their own file; the deletion length is the distance between the two cut boundaries (for a PAM-out "
                          "nickase pair the published offset is that length - 34)")
    eng.add_argument("--pairs-min-distance", type=int, default=None, metavar="D",
                     help="with --select-pairs: the shortest deletion, in letters (default 50; at least 1)")
    eng.add_argument("--pairs-max-distance", type=int, default=None, metavar="D",
                     help="with --select-pairs: the longest deletion, in letters (default 500; at most 65535)")
    eng.add_argument("--pairs-frameshift", action="store_true",
                     help="with --select-pairs: only deletions whose length is no multiple of 3")
    eng.add_argument("--pairs-distinct", action="store_true",
                     help="with --select-pairs: the KP pairs of a gene share no guide -- the pairs are taken greedily in rank order, and "
                          "a pair is taken only if neither of its guides belongs to a pair taken before it; `rank` is the pick order")
    eng.add_argument("--pairs-orientation", default=None, metavar="WHICH",
                     help="with --select-pairs: any (default), pam-out ('-' guide left, '+' guide right: the nickase layout) or pam-in")
    eng.add_argument("--pairs-output", metavar="FILE", default=None,
                     help="with --select-pairs: the pairs file, default = the -o path + .pairs.csv")
    eng.add_argument("--select-gc-min", type=int, default=None, metavar="PCT",
                     help="with --select: only guides with at least PCT %% GC (an integer 0..100; as a count: ceil(PCT * l / 100))")
    eng.add_argument("--select-gc-max", type=int, default=None, metavar="PCT",
                     help="with --select: only guides with at most PCT %% GC (an integer 0..100; as a count: floor(PCT * l / 100))")
    eng.add_argument("--select-max-run", type=int, default=None, metavar="N",
                     help="with --select: only guides whose longest run of one base has at most N letters")
    eng.add_argument("--select-max-t-run", type=int, default=None, metavar="N",
                     help="with --select: only guides whose longest run of T has at most N letters (3 keeps TTTT out)")
    eng.add_argument("--select-max-stem", type=int, default=None, metavar="N",
                     help="with --select: only guides whose longest hairpin stem has at most N pairs")
    eng.add_argument("--repair-scores", action="store_true",
                     help="with --select: what the cut does to the gene, predicted from the letters around it (microhomology-"
                          "mediated end joining, Bae et al. 2014) on the GPU; every row of the selection file gets two more fields, "
                          "mh_score (microhomology score) and oof_score (the share, in percent, of the predicted deletions "
                          "that shift the frame; -1 where there is no microhomology); one GPU")
    eng.add_argument("--coding", action="store_true",
                     help="with --select: where in the gene's coding sequence every selected guide cuts, from the mRNA / CDS rows "
                          "and Parent links of the GFF; every row of the selection file gets five more fields, cds_offset, cds_length, "
                          "cds_percent (of the gene's longest coding transcript; empty when the cut is not inside it), transcripts_cut "
                          "and transcripts; like its three filters, not together with --select-pairs")
    eng.add_argument("--select-coding-min", default=None, metavar="PCT",
                     help="with --select: only guides that cut inside the coding sequence of the gene's longest coding transcript, at "
                          "least PCT %% of its length from its start (an integer 0..100); implies --coding")
    eng.add_argument("--select-coding-max", default=None, metavar="PCT",
                     help="with --select: ... and at most PCT %% of its length from its start (an integer 0..100; 65 keeps the last "
                          "third out, where a frameshift leaves a nearly whole protein); implies --coding")
    eng.add_argument("--select-transcripts", default=None, metavar="PCT",
                     help="with --select: only guides that cut inside the coding sequence of at least PCT %% of the gene's coding "
                          "transcripts (an integer 0..100; 100: every isoform); implies --coding")
    eng.add_argument("--families", default=None, metavar="FILE",
                     help="with --select and --specificity: gene families for polyploid genomes, a text file of gene<TAB>family "
                          "lines (the gene as the selection file prints it after 'gene:'; homeolog or orthogroup tables).  Near copies "
                          "inside the guide's own family are told from those outside it on the GPU; every row of the selection file "
                          "gets seven more fields, family, family_size, members_hit, members, outside_mm0, outside_hit_sum and "
                          "outside_specificity; a family has at most 64 members in the annotation; one GPU")
    eng.add_argument("--family-cover-mismatches", default=None, metavar="C",
                     help="with --families: a family member counts as hit when the guide has a site with NGG in it within C mismatches "
                          "(0 .. --specificity-mismatches; default 0: exact copies)")
    eng.add_argument("--select-min-members", default=None, metavar="N|all",
                     help="with --families: only guides that hit at least N members of the gene's family (all: every member)")
    eng.add_argument("--select-max-perfect-outside", default=None, metavar="N",
                     help="with --families: only guides with at most N perfect copies outside the gene's family "
                          "(--select-max-perfect counts the homeologs too)")
    eng.add_argument("--select-min-specificity-outside", default=None, metavar="S",
                     help="with --families: only guides whose specificity, with the hits inside the gene's family left out, is at least S")
    eng.add_argument("--family-sets", default=None, metavar="S",
                     help="with --families: per gene family, at most S guides (1..64) that together cut as many of its members as "
                          "possible, chosen greedily on the GPU from the guides that pass the selection's filters: each step takes "
                          "the guide that cuts the most members not cut yet (the multiplex set for a family whose copies have "
                          "diverged); one row per chosen guide goes to --family-sets-output")
    eng.add_argument("--family-sets-output", default=None, metavar="FILE",
                     help="with --family-sets: where the family sets go (default: the -o path + .family_sets.csv)")
    eng.add_argument("--base-edit", action="store_true",
                     help="with --select: what a cytosine base editor does under every selected guide: the C's of a window of the "
                          "protospacer become T's, which can turn CAA, CAG, CGA or (from the other strand) TGG of the gene's longest "
                          "coding transcript into a stop codon without a cut; every row of the selection file gets four more fields, "
                          "edit_targets, stop_codons, stop_codon (the first one's number in the coding sequence) and stop_percent (the "
                          "last two empty when no stop is written)")
    eng.add_argument("--base-edit-window", default=None, metavar="LO-HI",
                     help="with --select: the editing window in protospacer positions counted from the PAM-distal end (1..20, "
                          "default 4-8); implies --base-edit")
    eng.add_argument("--select-stop", action="store_true",
                     help="with --select: only guides with which the base editor writes a stop codon into the gene's longest coding "
                          "transcript; implies --base-edit; not together with the --select-coding filters or --select-pairs")
    eng.add_argument("--select-stop-min", default=None, metavar="PCT",
                     help="with --select: ... whose first stop codon lies at least PCT %% of the coding length from its start (an "
                          "integer 0..100); implies --select-stop")
    eng.add_argument("--select-stop-max", default=None, metavar="PCT",
                     help="with --select: ... and at most PCT %% of the coding length from its start (an integer 0..100); implies "
                          "--select-stop")
    eng.add_argument("--select-max-edit-targets", default=None, metavar="N",
                     help="with --select: ... and whose window holds at most N letters the editor converts (0..20: bystander "
                          "edits); implies --select-stop")
    eng.add_argument("--base-editor", default=None, metavar="cbe|abe",
                     help="with --select: the base editor of the splice-site test: cbe (cytosine, C -> T; the default) or abe "
                          "(adenine, A -> G); abe writes no stop codon, so not together with --base-edit or the --select-stop options")
    eng.add_argument("--splice-edit", action="store_true",
                     help="with --select: what the base editor does to the splice sites of the gene's longest coding transcript under "
                          "every selected guide: a converted letter in the GT that opens an intron or the AG that closes it destroys the "
                          "site without a cut; every row of the selection file gets four more fields, splice_targets, splice_sites, "
                          "donor_percent and acceptor_percent (the coding letters 5' of the intron in percent of the coding length; "
                          "empty without a destroyed site of that kind); window: --base-edit-window")
    eng.add_argument("--select-splice", nargs="?", const="any", default=None, metavar="donor|acceptor|any",
                     help="with --select: only guides with which the base editor destroys a canonical splice site of that kind "
                          "(default any) of the gene's longest coding transcript; implies --splice-edit; with the --select-stop "
                          "options as well a guide passes by either test; not together with the --select-coding filters or --select-pairs")
    eng.add_argument("--select-splice-min", default=None, metavar="PCT",
                     help="with --select: ... whose intron lies behind at least PCT %% of the coding length (an integer 0..100); "
                          "implies --select-splice")
    eng.add_argument("--select-splice-max", default=None, metavar="PCT",
                     help="with --select: ... and behind at most PCT %% of the coding length (an integer 0..100); implies --select-splice; "
                          "--select-max-edit-targets bounds the window's converted letters of this test too")
    eng.add_argument("--repair-flank", default=None, metavar="F",
                     help="with --repair-scores or a repair filter: letters looked at on either side of the cut (2..32, default 30)")
    eng.add_argument("--select-min-oof", default=None, metavar="PCT",
                     help="with --select: only guides whose out-of-frame score is at least PCT (an integer 0..100; above 0 a guide "
                          "without any microhomology fails)")
    eng.add_argument("--select-min-mh", default=None, metavar="X",
                     help="with --select: only guides whose microhomology score is at least X (a decimal with at most one "
                          "fractional digit)")
    eng.add_argument("--variants", default=None, metavar="FILE",
                     help="with --select: a VCF (text or .gz) of the cultivar against this assembly; every selection-file row ends "
                          "with var_site, var_guide, var_seed and var_pam, the variants that touch its target site, guide, seed and PAM")
    eng.add_argument("--variants-samples", default=None, metavar="A,B",
                     help="with --variants: only the ALT alleles that the GT of at least one of these samples holds")
    eng.add_argument("--variants-pass-only", action="store_true", help="with --variants: only records whose FILTER is PASS or .")
    eng.add_argument("--variant-seed", default=None, metavar="S",
                     help="with --variants: the PAM-proximal letters of the guide that make the seed (1..-l, default 12)")
    eng.add_argument("--select-max-variants", default=None, metavar="N",
                     help="with --variants: only guides with at most N variants under guide + PAM")
    eng.add_argument("--select-max-guide-variants", default=None, metavar="N",
                     help="with --variants: only guides with at most N variants under the guide")
    eng.add_argument("--select-max-seed-variants", default=None, metavar="N",
                     help="with --variants: only guides with at most N variants under the seed")
    eng.add_argument("--select-max-pam-variants", default=None, metavar="N",
                     help="with --variants: only guides with at most N variants under the two fixed letters of the PAM")
    eng.add_argument("--sites", action="store_true",
                     help="with --select: every row of the selection file ends with guide_sites and assay_enzymes, the restriction enzymes "
                          "whose recognition site lies inside the guide and those that give a cut-site assay (names joined by ;)")
    eng.add_argument("--enzymes", default=None, metavar="FILE",
                     help="with --select: an enzyme set of your own (name<TAB>motif lines, # comments) in place of the built-in 32")
    eng.add_argument("--select-no-site", default=None, metavar="NAMES",
                     help="with --select: only guides without a recognition site of these enzymes (comma list; `cloning`: BsaI, BbsI, "
                          "BsmBI, SapI and AarI of the built-in set)")
    eng.add_argument("--select-assay", default=None, metavar="NAMES|any",
                     help="with --select: only guides whose edit can be read by a cut-site assay with one of these enzymes")
    eng.add_argument("--assay-flank", default=None, metavar="A",
                     help="with --sites / --select-assay: the amplicon reaches A letters to either side of the cut (default 300)")
    eng.add_argument("--bench-json", metavar="PATH", default=None,
                     help="write stage timings of this run (read, upload+scan, fetch, format+write) as one JSON object")
    return p


def import_gff_file(gff, verbose, out=sys.stdout):
    """Side effects of CROPSR.py:77-95.  The table is parsed exactly as the
    reference parses it and, exactly as there, never used."""
    import pandas as pd
    start_index = 0
    with open(gff, "r") as raw:
        if verbose:
            print(f"Annotation file {gff} successfully imported", file=out)
        lines = raw.readlines()
        for index, line in enumerate(lines):
            if "##" not in line:
                start_index = index
                break
    cols = ["chromosome", "source", "feature", "start", "end", "score", "strand", "phase", "attributes"]
    table = pd.read_csv(gff, sep="\t", skiprows=start_index, header=None, names=cols)
    if verbose:
        print("Annotation database successfully generated", file=out)
    return table


class EngineResident:
    """Hit tables of this rank's texts, still in HBM (parallel.sharded_scan's Resident)."""

    def __init__(self, backend, genome, counts, guide_len, want_pre):
        self.backend, self.genome, self.counts = backend, genome, counts
        self.guide_len, self.want_pre = guide_len, want_pre
        self.layout = []
        for k in range(genome.n_contigs):
            a, j = genome._where[k]
            self.layout.append((a, int(genome.arenas[a].offsets[j]), int(genome.arenas[a].lengths[j])))
        self._ot = False
        self._annotated = False

    def annotate(self, request):
        """The annotation join over this rank's resident tables (annotate.Request for ITS texts); the ids stay in HBM
        and travel with the tables in gather()."""
        self.genome.annotate(request, self.counts, fetch=False)
        self.backend.last_annotate_s = self.genome.annotate_s
        self._annotated = True

    def offtarget(self, group, own_by_arena):
        eng = self.backend.engine
        eng.offtarget_reset()
        for a, arena in enumerate(self.genome.arenas):
            own = own_by_arena[a] if a < len(own_by_arena) else []
            arena.offtarget_add(self.guide_len, np.asarray(own, dtype=np.uint64).reshape(-1, 2))
        if self.backend.transport == "rccl":
            eng.offtarget_reduce()  # the histogram is summed over the ranks on xGMI
        else:  # ranks sharing a GPU: sum the (sparse) histograms over the control sockets
            h = eng.offtarget_hist()
            idx = np.flatnonzero(h)
            total = np.zeros_like(h)
            for i, v in group.all_gather((idx, h[idx])):
                np.add.at(total, i, v)
            eng.offtarget_hist(total)
        eng.offtarget_solve()
        for arena, (n_plus, n_minus) in zip(self.genome.arenas, self.counts):
            arena.offtarget_counts(n_plus, n_minus, fetch=False)
        self._ot = True

    def _host_cols(self, arena, n_plus, n_minus, offtarget, features):
        c = arena.fetch(n_plus, n_minus, self.want_pre)
        cols = {"pos_plus": c[0], "score_plus": c[1] if self.want_pre else c[2],
                "pos_minus": c[3], "score_minus": c[4] if self.want_pre else c[5]}
        if offtarget:
            cols["ot_plus"], cols["ot_minus"] = arena.offtarget_counts(n_plus, n_minus)
        if features:
            cols["feat_plus"], cols["feat_minus"] = arena.annotate_lookup(n_plus, n_minus)
        return cols

    def gather(self, group, dst, offtarget, features=False):
        """[rank][arena] -> column dict on dst.  With want_pre the f64 column carries the pre-sigmoid
        sum (the root finalises the score on its host)."""
        from . import _native as nat
        from . import parallel
        eng = self.backend.engine
        if self.backend.transport != "rccl":
            mine = [self._host_cols(a, n[0], n[1], offtarget, features) for a, n in zip(self.genome.arenas, self.counts)]
            return parallel.gather_host(group, mine, dst, offtarget, features)
        n_arenas = group.all_gather(len(self.genome.arenas))
        out = [[] for _ in range(group.world)]
        for rnd in range(max(n_arenas)):
            arena = self.genome.arenas[rnd] if rnd < len(self.genome.arenas) else None
            err, counts = None, None
            try:
                counts = eng.gather_hits(arena, dst, offtarget, pre=self.want_pre, features=features)
            except nat.CropsrHipError as e:
                # crp_gather_hits agrees on what can fail on one rank BEFORE the tables move (a rank without tables, a
                # root that cannot size its receive buffers): every rank is back from the same call, so all of them
                # reach check() below and raise the same RankError.  Anything else (an RCCL or HIP error inside the
                # exchange) is this rank's alone, its peers may be blocked in ncclSend/Recv: take the run down NOW
                # (abort channel; exits with status 3) instead of waiting for them in check().
                if e.status not in nat.AGREED_GATHER_ERRORS:
                    group.abort("%s: %s" % (type(e).__name__, e))
                err = "%s: %s" % (type(e).__name__, e)
            group.check(err)
            if group.rank == dst:
                for r in range(group.world):
                    if rnd < n_arenas[r]:
                        out[r].append(eng.gathered_fetch(r, counts, offtarget, features))
        return out if group.rank == dst else None

    def release(self):
        self.genome.close()


class EngineBackend:
    """The product's hit provider: libcropsr_hip.so on one MI355X."""

    def __init__(self, device=0, group=None, finalize="gpu"):
        import os
        from .engine import Engine
        self.engine = Engine(device)
        self.finalize = finalize
        self.group = group
        # rccl: the tables cross xGMI inside the library; host: every rank copies its tables over its
        # own PCIe link and the control sockets carry them (ranks sharing one GPU, where RCCL cannot run)
        self.transport = os.environ.get("CROPSR_GATHER", "rccl")
        self.last_annotate_s = None  # --bench-json: seconds the last annotation join took on this rank
        self.last_stream = None      # --bench-json: crp_scan_stream's own numbers for the last plain scan
        self.last_specificity = None  # --bench-json: the self-search handles' times of the last --specificity scan
        self.last_properties = None   # --bench-json: the property kernel's time and rows of the last scan that ran it
        self.last_repair = None       # --bench-json: the repair kernel's time, rows and flank of the last scan that ran it
        self.last_sites = None        # --bench-json: the site kernels' times, rows, enzymes, flank and bytes of the last scan that ran them
        self.last_variants = None     # --bench-json: the variant kernel's time, rows, seed and track size of the last scan that ran it

    def connect(self):
        """Collective over the group: create the RCCL communicator (transport "rccl")."""
        if self.group is not None and self.transport == "rccl":
            from .rendezvous import RankError
            try:
                self.engine.comm_init(self.group)
            except RankError as e:
                # every rank has this error (comm_init agrees on it): the job of the run is the CSV, and the tables can
                # travel over the control sockets instead
                import sys
                if self.group.rank == 0:
                    sys.stderr.write("cropsr_amd: no RCCL communicator (%s); the final exchange uses the host transport\n" % e)
                self.transport = "host"

    def _finalize(self, hits):
        """--score-finalize=host: CROPSR.py:313 on this host's numpy, from the GPU's pre-sigmoid sum."""
        for strand in ("plus", "minus"):
            pre = hits.pop("pre_" + strand, None)
            if pre is not None and self.finalize == "host":
                hits["score_" + strand] = host_sigmoid(pre)
        return hits

    def warm_up(self):
        """On the start-up helper thread, while the FASTA is still being read: the lanes of the pipelined scan (two further
        streams, four slice arenas with their tables, the landing buffers)."""
        import os
        if self.group is None and os.environ.get("CROPSR_STREAM", "1") != "0":
            self.engine.stream_prepare()
            # and one scan of a few hundred characters through them: a process's first launch of the scan kernels loads their
            # code object (17-25 ms, otherwise paid by the genome's first slice)
            self.engine.scan_stream([np.frombuffer(b"ACGTTGCAAGGCCTTA" * 40, dtype=np.uint8)], 20)

    def scan(self, contig_strings, guide_len, offtarget=False, annotation=None, specificity=None, select=None, properties=False):
        """One pass on the GPU for all contig strings (seam 1 + 2).  The plain scan goes through crp_scan_stream -- upload,
        scan and table fetch as a pipeline over slices of the genome, the host link busy in both directions (the reference's
        loop is produce-and-consume per contig too, CROPSR.py:409-474); CROPSR_STREAM=0, or the opt-in steps that work on
        resident tables (offtarget, annotation), take the arena calls: upload, one scan, fetch.  annotation
        (annotate.Request): the hit dicts also carry feat_plus / feat_minus, the label-set id of every row, joined on the GPU
        while the tables are resident.  specificity (the arguments of search.specificity_columns): the hit dicts also carry
        self_counts_* / self_sum_*, the self search's rows joined onto the resident tables.  select (select.Request): the returned list is a
        select.HitList whose .selection holds the best K guides of every gene, chosen on the GPU while the tables (and the
        joined specificity columns) are resident.  properties: the hit dicts also carry props_plus / props_minus, the packed
        guide properties of every row (properties.py), computed on the GPU while the tables are resident."""
        import os
        if not offtarget and annotation is None and specificity is None and select is None and not properties and os.environ.get("CROPSR_STREAM", "1") != "0":
            want_pre = self.finalize == "host"
            hits = self.engine.scan_stream(contig_strings, guide_len, want_pre=want_pre)
            self.last_stream = hits.stream_stats  # (--bench-json)
            out = []
            for k in range(len(contig_strings)):
                h = hits.contig(k)
                if want_pre:  # the f64 column is the pre-sigmoid sum: CROPSR.py:313 on this host's numpy
                    h["score_plus"], h["score_minus"] = host_sigmoid(h["score_plus"]), host_sigmoid(h["score_minus"])
                out.append(h)
            self.last_annotate_s = None
            return out
        genome = self.engine.genome(contig_strings)  # as many arenas as the genome needs
        try:
            more = {} if select is None else dict(select=select)
            if properties:
                more["properties"] = True
            hits = genome.scan_score(guide_len, want_pre=self.finalize == "host", offtarget=offtarget, annotation=annotation,
                                     specificity=specificity, **more)
            out = [self._finalize(hits.contig(k)) for k in range(len(contig_strings))]
            if select is not None:
                from . import select as sel
                out = sel.HitList(out)
                out.selection = hits.selection
            self.last_annotate_s = genome.annotate_s
            self.last_specificity = getattr(hits.columns, "stats", None)  # (--bench-json)
            self.last_properties = genome.properties_stats
            self.last_repair = genome.repair_stats
            self.last_variants = genome.variant_stats
            self.last_sites = genome.site_stats
        finally:
            genome.close()
        return out

    def scan_resident(self, texts, guide_len, offtarget=False):
        """The same scan with the tables left in HBM, for parallel.sharded_scan.  offtarget: the off-target step
        follows, so the scan also writes the seed words it works on."""
        want_pre = self.finalize == "host"
        genome = self.engine.genome(texts)
        counts = [a.scan_score_device(guide_len, want_pre, want_seeds=offtarget) for a in genome.arenas]
        return EngineResident(self, genome, counts, guide_len, want_pre)

    def finalize_gathered(self, all_hits):
        """Root, after a sharded scan with --score-finalize=host: the gathered f64 column is `pre`."""
        if self.finalize == "host":
            for h in all_hits:
                for strand in ("plus", "minus"):
                    h["score_" + strand] = host_sigmoid(h["score_" + strand])
        return all_hits

    def rescore(self, rows_u8, order):
        """Seam 2 on a few rows in one of the BLAS tail orders (rows.Dataset.rows)."""
        pre, score = self.engine.score_30mers(rows_u8, order)
        return host_sigmoid(pre) if self.finalize == "host" else score

    def close(self):
        self.engine.close()


class NodeBackend:
    """The same hit provider over SEVERAL MI355X in ONE process: the library's node handle (crp_node_*, node.Node).  The cut
    of the genome into contiguous equal shares, the uploads, the scans on every device, the opt-in off-target scan and
    annotation join and the gatherv to the first device all happen inside libcropsr_hip.so; this class only calls them.
    What scan() returns is what EngineBackend.scan() returns on one GPU, bit for bit."""

    def __init__(self, devices, finalize="gpu"):
        from .node import Node
        self.node = Node(devices)
        self.finalize = finalize
        self.last_annotate_s = None
        self.last_gather = None  # node.gather_stats() of the last scan (--bench-json)
        self._engine = None      # seam 2 on a few rows (rescore): a context of its own on the first device, opened when needed
        self._devices = list(devices)

    def scan(self, contig_strings, guide_len, offtarget=False, annotation=None):
        want_pre = self.finalize == "host"
        node = self.node
        node.load(contig_strings)
        node.scan_score_device(guide_len, want_pre=want_pre, want_seeds=offtarget)
        if offtarget:
            node.offtarget(guide_len)
        if annotation is not None:
            t0 = time.perf_counter()
            node.annotate(annotation)
            self.last_annotate_s = time.perf_counter() - t0
        # CROPSR_GATHER=host (as for the process-per-GPU mode): the consumer is this host's CSV writer, so nothing needs to
        # cross xGMI -- every device's rows come over its own PCIe link (CRP_NODE_HOST_GATHER); default: the gatherv to device 0
        import os
        to_host = os.environ.get("CROPSR_GATHER", "rccl") == "host"
        self.last_gather = node.gather(0, pre=want_pre, offtarget=offtarget, features=annotation is not None, to_host=to_host)
        hits = node.fetch(guide_len)
        out = []
        for k in range(len(contig_strings)):
            h = hits.contig(k)
            if want_pre:  # the f64 column that travelled is the pre-sigmoid sum: CROPSR.py:313 on this host's numpy
                h["score_plus"], h["score_minus"] = host_sigmoid(h["score_plus"]), host_sigmoid(h["score_minus"])
            out.append(h)
        return out

    def rescore(self, rows_u8, order):
        if self._engine is None:
            from .engine import Engine
            self._engine = Engine(self._devices[0])
        pre, score = self._engine.score_30mers(rows_u8, order)
        return host_sigmoid(pre) if self.finalize == "host" else score

    def close(self):
        if self._engine is not None:
            self._engine.close()
        self.node.close()


def host_sigmoid(pre):
    """`1/(1+np.exp(score))` of CROPSR.py:313 -- the reference's own expression, evaluated by the numpy
    of the host this runs on (so its last bit is this host's, like the reference's)."""
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(np.asarray(pre, dtype=np.float64)))


def _distributed():
    """The rendezvous.Group of a multi-process launch (python -m torch.distributed.run ... -m cropsr_amd
    or any launcher that exports RANK / WORLD_SIZE / LOCAL_RANK / MASTER_PORT), else None.  One process
    per GPU; no PyTorch: the control plane is rendezvous.py, the data plane RCCL inside the library."""
    global _ACTIVE_GROUP
    from . import rendezvous
    _ACTIVE_GROUP = rendezvous.Group.from_env()
    return _ACTIVE_GROUP


_ACTIVE_GROUP = None  # the group main() aborts when this rank fails outside an agreed error (Group.check)


NATIVE_GUIDE_LENGTHS = (1, 50)  # what the kernels' window logic and the native row formatter are built for
BATCH_ROWS = 4_000_000  # --each-contig-once: consecutive passes are formatted together until they hold this many rows (CROPSR_BATCH_ROWS)


def device_guide_length(l):
    """The guide length the engine scans with for the reference's `-l l` (any integer, CROPSR.py:38-40).  Inside
    0..50 it is l itself; outside, the nearest end of that range, whose kept hits are a SUPERSET of the reference's
    (the keep-filters of CROPSR.py:419 / :430 only get stricter as |l| grows) -- refilter_hits() then applies
    the literal filter.  No row is scored at those lengths (long_sequence has l + 10 characters, or is cut by the end
    of the string to more than 30 for l > 35): what remains of the reference's work there is the filter."""
    return min(max(int(l), 0), NATIVE_GUIDE_LENGTHS[1])


def refilter_hits(hits, n, l):
    """CROPSR.py:419 and :430, all four clauses each, on the hit tables of one contig string of n characters (match
    indices i of (?=.GG), j of (?=CC.)) -- for guide lengths the engine scanned with a clamped length
    (device_guide_length).  Every surviving row is unscored (-1), like the reference writes it."""
    keep = {}
    for strand in hitcols.STRANDS:
        p = np.asarray(hits["pos_" + strand]).astype(np.int64)
        a, b = (p - l, p) if strand == "plus" else (p + 3, p + 3 + l)  # pam_location (:418 / :429)
        keep[strand] = (a >= 5) & (a + 5 <= n + 10) & (b >= 5) & (b <= n + 10)
    out = hitcols.take(hits, keep["plus"], keep["minus"])
    for strand in hitcols.STRANDS:
        out["score_" + strand] = np.full(int(keep[strand].sum()), -1.0)
    return out


SPECIFICITY_MISMATCHES, SPECIFICITY_PAM = 3, "NRG"


def _device_list(args):
    return [d for d in str(getattr(args, "devices", None) or "").split(",") if d.strip()]


def specificity_request(args):
    """--specificity and its options, checked: None without it, else the arguments of search.specificity_columns
    (max_mm, candidate_pam, score).  Everything the command line alone can get wrong ends the run here, with a message,
    before any file is written or the GPU opened."""
    def refuse(msg):
        sys.exit("cropsr_amd: --specificity: " + msg)

    given = [o for o, k in (("--specificity-mismatches", "specificity_mismatches"), ("--specificity-pam", "specificity_pam"),
                            ("--specificity-weights", "specificity_weights"), ("--specificity-table", "specificity_table"))
             if getattr(args, k, None) is not None]
    if not getattr(args, "specificity", False):
        if given:
            sys.exit("cropsr_amd: %s belongs to --specificity" % given[0])
        return None
    from . import search
    M = getattr(args, "specificity_mismatches", None)
    M = SPECIFICITY_MISMATCHES if M is None else M
    pam = getattr(args, "specificity_pam", None) or SPECIFICITY_PAM
    wfile, tfile = getattr(args, "specificity_weights", None), getattr(args, "specificity_table", None)
    if wfile and tfile:
        refuse("--specificity-weights and --specificity-table are two forms of the hit score: give one of them")
    if not 0 <= M <= search.MAX_SELF_MM:
        refuse("--specificity-mismatches must be 0..%d, not %d" % (search.MAX_SELF_MM, M))
    l = args.l
    if l + search.SPECIFICITY_PAM_LEN > search.MAX_T:
        refuse("guide and PAM are compared as one pattern of at most %d letters: -l %d is more than %d" % (
            search.MAX_T, l, search.MAX_T - search.SPECIFICITY_PAM_LEN))
    if l < M + 1:
        refuse("-l %d is too short for %d mismatches (a guide of at least %d letters)" % (l, M, M + 1))
    if len(_device_list(args)) > 1:
        refuse("the self search runs on one GPU: --devices names %d" % len(_device_list(args)))
    if getattr(args, "gpus", 1) > 1:
        refuse("the self search runs on one GPU: drop --gpus %d" % args.gpus)
    score = "hsu2013"
    try:
        if wfile:
            with open(wfile, "rb") as f:
                score = search.parse_weights(f.read())
        elif tfile:
            with open(tfile, "rb") as f:
                score = search.parse_pair_table(f.read())
        elif l != len(search.HSU2013_W):
            refuse("the Hsu 2013 weights are defined for -l %d, not %d: give --specificity-weights or --specificity-table" % (
                len(search.HSU2013_W), l))
        search.check_specificity(l, M, pam, score)
    except (search.SearchInputError, OSError, UnicodeDecodeError) as e:
        refuse(str(e))
    return dict(max_mm=M, candidate_pam=pam.upper(), score=score)


def select_request(args, spec, world=1):
    """--select and its options, checked: None without it, else dict(params (select.Params), output, only).  Like
    specificity_request, everything the command line alone can get wrong ends the run here, before any side effect."""
    def refuse(msg):
        sys.exit("cropsr_amd: --select: " + msg)

    given = [o for o, k, unset in (("--select-output", "select_output", None), ("--select-min-score", "select_min_score", None),
                                   ("--select-max-perfect", "select_max_perfect", None),
                                   ("--select-min-specificity", "select_min_specificity", None), ("--select-cds", "select_cds", False),
                                   ("--select-only", "select_only", False), ("--select-min-spacing", "select_min_spacing", None),
                                   ("--select-gc-min", "select_gc_min", None),
                                   ("--select-gc-max", "select_gc_max", None), ("--select-max-run", "select_max_run", None),
                                   ("--select-max-t-run", "select_max_t_run", None), ("--select-max-stem", "select_max_stem", None),
                                   ("--repair-scores", "repair_scores", False), ("--repair-flank", "repair_flank", None),
                                   ("--select-min-oof", "select_min_oof", None), ("--select-min-mh", "select_min_mh", None),
                                   ("--coding", "coding", False), ("--select-coding-min", "select_coding_min", None),
                                   ("--select-coding-max", "select_coding_max", None), ("--select-transcripts", "select_transcripts", None),
                                   ("--base-edit", "base_edit", False), ("--base-edit-window", "base_edit_window", None),
                                   ("--select-stop", "select_stop", False), ("--select-stop-min", "select_stop_min", None),
                                   ("--select-stop-max", "select_stop_max", None), ("--select-max-edit-targets", "select_max_edit_targets", None),
                                   ("--base-editor", "base_editor", None), ("--splice-edit", "splice_edit", False),
                                   ("--select-splice", "select_splice", None), ("--select-splice-min", "select_splice_min", None),
                                   ("--select-splice-max", "select_splice_max", None), ("--families", "families", None),
                                   ("--family-cover-mismatches", "family_cover_mismatches", None),
                                   ("--select-min-members", "select_min_members", None),
                                   ("--select-max-perfect-outside", "select_max_perfect_outside", None),
                                   ("--select-min-specificity-outside", "select_min_specificity_outside", None),
                                   ("--family-sets", "family_sets", None), ("--family-sets-output", "family_sets_output", None))
             if getattr(args, k, unset) not in (unset, None)]
    KP = getattr(args, "select_pairs", None)
    pair_given = [o for o, k, unset in (("--pairs-min-distance", "pairs_min_distance", None), ("--pairs-max-distance", "pairs_max_distance", None),
                                        ("--pairs-frameshift", "pairs_frameshift", False), ("--pairs-orientation", "pairs_orientation", None),
                                        ("--pairs-output", "pairs_output", None), ("--pairs-distinct", "pairs_distinct", False))
                  if getattr(args, k, unset) not in (unset, None)]
    if KP is None and pair_given:
        sys.exit("cropsr_amd: --select: %s belongs to --select-pairs" % pair_given[0])
    K = getattr(args, "select", None)
    if K is None:
        if KP is not None:
            sys.exit("cropsr_amd: --select-pairs belongs to --select")
        if given:
            sys.exit("cropsr_amd: %s belongs to --select" % given[0])
        return None
    from . import select
    if not args.g:
        refuse("the genes come from the GFF: --select needs -g")
    if not 1 <= K <= select.MAX_K:
        refuse("K must be 1..%d, not %d" % (select.MAX_K, K))
    if args.l != select.GUIDE_LEN:
        refuse("guides are ranked by on_site_score, which exists for -l %d only, not -l %d" % (select.GUIDE_LEN, args.l))
    for opt, key in (("--select-max-perfect", "select_max_perfect"), ("--select-min-specificity", "select_min_specificity")):
        if getattr(args, key, None) is not None and spec is None:
            refuse("%s is a threshold on the columns of --specificity: give --specificity too" % opt)
    if len(_device_list(args)) > 1:
        refuse("the selection runs on one GPU: --devices names %d" % len(_device_list(args)))
    if getattr(args, "gpus", 1) > 1:
        refuse("the selection runs on one GPU: drop --gpus %d" % args.gpus)
    if world > 1:
        refuse("the selection runs on one GPU, and a launcher started %d ranks" % world)
    for opt, key in (("--select-gc-min", "select_gc_min"), ("--select-gc-max", "select_gc_max")):
        v = getattr(args, key, None)
        if v is not None and not 0 <= v <= 100:
            refuse("%s is a percentage, an integer 0..100, not %d" % (opt, v))
    for opt, key in (("--select-max-run", "select_max_run"), ("--select-max-t-run", "select_max_t_run"), ("--select-max-stem", "select_max_stem")):
        v = getattr(args, key, None)
        if v is not None and v < 0:
            refuse("%s is a number of letters, not %d" % (opt, v))
    from . import properties
    gc_min, gc_max = properties.gc_count_bounds(getattr(args, "select_gc_min", None), getattr(args, "select_gc_max", None), args.l)
    limits = dict(gc_min=gc_min if getattr(args, "select_gc_min", None) is not None else None,
                  gc_max=gc_max if getattr(args, "select_gc_max", None) is not None else None,
                  max_run=getattr(args, "select_max_run", None), max_t_run=getattr(args, "select_max_t_run", None),
                  max_stem=getattr(args, "select_max_stem", None))
    from . import repair
    with_scores = bool(getattr(args, "repair_scores", False))
    flank, min_oof, min_mh = (getattr(args, k, None) for k in ("repair_flank", "select_min_oof", "select_min_mh"))
    if flank is not None and not (with_scores or min_oof is not None or min_mh is not None):
        refuse("--repair-flank belongs to --repair-scores, --select-min-oof or --select-min-mh")

    def integer(text):
        t = str(text).strip()
        return int(t) if t.isascii() and t.isdigit() else None

    if flank is not None:
        if integer(flank) is None or not repair.FLANKS[0] <= integer(flank) <= repair.FLANKS[1]:
            refuse("--repair-flank is a number of letters %d..%d, not %s" % (repair.FLANKS + (flank,)))
        flank = integer(flank)
    if min_oof is not None:
        if integer(min_oof) is None or integer(min_oof) > 100:
            refuse("--select-min-oof is a percentage, an integer 0..100, not %s" % min_oof)
        min_oof = integer(min_oof)
    if min_mh is not None:
        try:
            min_mh = repair.parse_min_mh(min_mh)
        except ValueError as e:
            refuse("--select-min-mh: " + str(e))
    # the coding position: percentages, whole numbers 0..100, min <= max; the limits are relative to the gene, so not with pairs
    pct = {}
    for opt, key in (("--select-coding-min", "select_coding_min"), ("--select-coding-max", "select_coding_max"),
                     ("--select-transcripts", "select_transcripts")):
        v = getattr(args, key, None)
        if v is not None:
            if integer(v) is None or integer(v) > 100:
                refuse("%s is a percentage, an integer 0..100, not %s" % (opt, v))
            pct[key] = integer(v)
    if pct.get("select_coding_min", 0) > pct.get("select_coding_max", 100):
        refuse("--select-coding-min %d lies above --select-coding-max %d" % (pct.get("select_coding_min", 0), pct.get("select_coding_max", 100)))
    with_coding = bool(getattr(args, "coding", False)) or bool(pct)
    if with_coding and KP is not None:
        refuse("%s: the coding position is relative to the gene and the pairs' eligibility is per table row: not together with --select-pairs"
               % ([o for o, k in (("--select-coding-min", "select_coding_min"), ("--select-coding-max", "select_coding_max"),
                                  ("--select-transcripts", "select_transcripts")) if k in pct] + ["--coding"])[0])
    coding_args = {}
    if with_coding:  # (the keywords a select.Request only meets with the coding position)
        from . import coding
        coding_args = dict(coding=True, coding_limits=coding.Limits(pct.get("select_coding_min", 0), pct.get("select_coding_max", 100),
                                                                    pct.get("select_transcripts", 0)) if pct else None)
    # base editing: a window LO-HI, percentages, a count 0..20; the limits are relative to the gene and a kernel of their own, so
    # neither with pairs nor with the coding filters
    from . import baseedit
    window = None
    if getattr(args, "base_edit_window", None) is not None:
        try:
            window = baseedit.Window.parse(args.base_edit_window)
        except ValueError as e:
            refuse("--base-edit-window: " + str(e))
    stop = {}
    for opt, key, top, what in (("--select-stop-min", "select_stop_min", 100, "a percentage, an integer 0..100"),
                                ("--select-stop-max", "select_stop_max", 100, "a percentage, an integer 0..100"),
                                ("--select-max-edit-targets", "select_max_edit_targets", baseedit.GUIDE_LEN, "a number of letters 0..20")):
        v = getattr(args, key, None)
        if v is not None:
            if integer(v) is None or integer(v) > top:
                refuse("%s is %s, not %s" % (opt, what, v))
            stop[key] = (opt, integer(v))
    if "select_stop_min" in stop and "select_stop_max" in stop and stop["select_stop_min"][1] > stop["select_stop_max"][1]:
        refuse("--select-stop-min %d lies above --select-stop-max %d" % (stop["select_stop_min"][1], stop["select_stop_max"][1]))
    # splice-site editing: the editor's name, a kind, percentages; --select-max-edit-targets bounds both tests, and next to a
    # splice limit it no longer asks for the stop test by itself
    editor = None
    if getattr(args, "base_editor", None) is not None:
        try:
            editor = baseedit.Editor(args.base_editor)
        except ValueError:
            refuse("--base-editor is cbe or abe, not %s" % args.base_editor)
    splice = {}
    kind = getattr(args, "select_splice", None)
    if kind is not None and kind not in baseedit.KINDS:
        refuse("--select-splice is donor, acceptor or any, not %s" % kind)
    for opt, key in (("--select-splice-min", "select_splice_min"), ("--select-splice-max", "select_splice_max")):
        v = getattr(args, key, None)
        if v is not None:
            if integer(v) is None or integer(v) > 100:
                refuse("%s is a percentage, an integer 0..100, not %s" % (opt, v))
            splice[key] = (opt, integer(v))
    if "select_splice_min" in splice and "select_splice_max" in splice and splice["select_splice_min"][1] > splice["select_splice_max"][1]:
        refuse("--select-splice-min %d lies above --select-splice-max %d" % (splice["select_splice_min"][1], splice["select_splice_max"][1]))
    splice_limit = ([o for o, _ in splice.values()] + ["--select-splice"])[0] if splice or kind is not None else None
    max_targets = stop.get("select_max_edit_targets", (None, baseedit.GUIDE_LEN))[1]
    if splice_limit is not None and not getattr(args, "select_stop", False) and "select_stop_min" not in stop and "select_stop_max" not in stop:
        stop = {}
    stop_limit = ([o for o, _ in stop.values()] + ["--select-stop"])[0] if stop or getattr(args, "select_stop", False) else None
    if editor is not None and editor.name == "abe":
        if getattr(args, "base_edit", False) or stop_limit is not None:
            refuse("--base-editor abe and %s: an adenine editor writes no stop codon; its knock-out route is --select-splice"
                   % ("--base-edit" if getattr(args, "base_edit", False) else stop_limit))
    if splice_limit is not None:
        if pct:
            refuse("%s and %s: the splice-site filter and the coding-position filter are two kernels' predicates: one or the other"
                   % (splice_limit, [o for o, k in (("--select-coding-min", "select_coding_min"), ("--select-coding-max", "select_coding_max"),
                                                    ("--select-transcripts", "select_transcripts")) if k in pct][0]))
        if KP is not None:
            refuse("%s: the splice site is relative to the gene and the pairs' eligibility is per table row: not together with --select-pairs"
                   % splice_limit)
    if stop_limit is not None:
        if pct:
            refuse("%s and %s: the stop-codon filter and the coding-position filter are two kernels' predicates: one or the other"
                   % (stop_limit, [o for o, k in (("--select-coding-min", "select_coding_min"), ("--select-coding-max", "select_coding_max"),
                                                  ("--select-transcripts", "select_transcripts")) if k in pct][0]))
        if KP is not None:
            refuse("%s: the stop codon is relative to the gene and the pairs' eligibility is per table row: not together with --select-pairs"
                   % stop_limit)
    with_splice = bool(getattr(args, "splice_edit", False)) or editor is not None or splice_limit is not None
    abe = editor is not None and editor.name == "abe"
    with_edit = bool(getattr(args, "base_edit", False)) or (window is not None and not abe) or stop_limit is not None
    if with_edit:  # (the keywords a select.Request only meets with base editing)
        val = lambda key, default: stop[key][1] if key in stop else default
        coding_args = dict(coding_args, edit_window=window or baseedit.Window(),
                           edit_limits=baseedit.Limits(val("select_stop_min", 0), val("select_stop_max", 100),
                                                       val("select_max_edit_targets", baseedit.GUIDE_LEN)) if stop_limit is not None else None)
    if with_splice:
        sval = lambda key, default: splice[key][1] if key in splice else default
        coding_args = dict(coding_args, edit_window=window or baseedit.Window(), editor=editor or baseedit.Editor(), edit=with_edit,
                           splice_limits=baseedit.SpliceLimits(sval("select_splice_min", 0), sval("select_splice_max", 100), max_targets,
                                                               kind or "any") if splice_limit is not None else None)
    # gene families: the file is read and checked here; its limits are relative to the gene and a kernel of their own, so neither
    # with pairs nor with the coding, stop or splice filters
    family_opts = [(o, getattr(args, k, None)) for o, k in (("--family-cover-mismatches", "family_cover_mismatches"),
                                                           ("--select-min-members", "select_min_members"),
                                                           ("--select-max-perfect-outside", "select_max_perfect_outside"),
                                                           ("--select-min-specificity-outside", "select_min_specificity_outside"))]
    family_limit = [o for o, v in family_opts[1:] if v is not None]
    family_pairs = None
    sets = getattr(args, "family_sets", None)
    if sets is None and getattr(args, "family_sets_output", None) is not None:
        refuse("--family-sets-output belongs to --family-sets")
    if getattr(args, "families", None) is None:
        for o, v in family_opts + [("--family-sets", sets)]:
            if v is not None:
                refuse("%s belongs to --families" % o)
    else:
        if sets is not None:  # the family sets: the greedy step is a kernel of its own, beside the family selection's
            for other, name in ((pct, "the coding-position filter"), (stop_limit, "the stop-codon filter"), (splice_limit, "the splice-site filter")):
                if other:
                    refuse("--family-sets and %s are two kernels' predicates: one or the other" % name)
            if KP is not None:
                refuse("--family-sets: a family's guides are chosen one by one, not in pairs: not together with --select-pairs")
            if integer(sets) is None or not 1 <= integer(sets) <= select.MAX_FAMILY_SET_STEPS:
                refuse("--family-sets is a number of guides 1..%d, not %s" % (select.MAX_FAMILY_SET_STEPS, sets))
            coding_args = dict(coding_args, family_sets=integer(sets))
        from . import families
        if spec is None:
            refuse("--families tells the hits of --specificity inside a gene's family from those outside it: give --specificity too")
        for other, name in ((pct, "the coding-position filter"), (stop_limit, "the stop-codon filter"), (splice_limit, "the splice-site filter")):
            if family_limit and other:
                refuse("%s and %s are two kernels' predicates: one or the other" % (family_limit[0], name))
        if family_limit and KP is not None:
            refuse("%s: a family is relative to the gene and the pairs' eligibility is per table row: not together with --select-pairs"
                   % family_limit[0])
        cover, members, perfect, outside = (v for _, v in family_opts)
        if cover is not None and (integer(cover) is None or integer(cover) > spec["max_mm"]):
            refuse("--family-cover-mismatches is 0..%d (the mismatches of --specificity), not %s" % (spec["max_mm"], cover))
        if members is not None and str(members).strip().lower() != "all":
            if integer(members) is None or not 1 <= integer(members) <= families.MAX_MEMBERS:
                refuse("--select-min-members is 1..%d or all, not %s" % (families.MAX_MEMBERS, members))
            members = integer(members)
        if perfect is not None:
            if integer(perfect) is None:
                refuse("--select-max-perfect-outside is a count, not %s" % perfect)
            perfect = integer(perfect)
        if outside is not None:
            try:
                outside = float(outside)
                select.max_hit_sum_for(outside)
            except ValueError:
                refuse("--select-min-specificity-outside is a specificity 0..1, not %s" % outside)
        try:
            family_pairs = families.read_families(args.families)
        except families.FamilyInputError as e:
            refuse("--families: " + str(e))
        coding_args = dict(coding_args, family_cover_mm=integer(cover) if cover is not None else 0, min_members=members,
                           max_perfect_outside=perfect, min_specificity_outside=outside)
    # the minimum spacing: its rounds read one pass key per table row, so not with the filters that are relative to the gene
    spacing = getattr(args, "select_min_spacing", None)
    if spacing is not None:
        if not 1 <= spacing <= select.MAX_SPACING:
            refuse("--select-min-spacing is a number of letters 1..%d, not %d" % (select.MAX_SPACING, spacing))
        for other, name in (([o for o, k in (("--select-coding-min", "select_coding_min"), ("--select-coding-max", "select_coding_max"),
                                             ("--select-transcripts", "select_transcripts")) if k in pct], "the coding-position filter"),
                            ([stop_limit] if stop_limit is not None else [], "the stop-codon filter"),
                            ([splice_limit] if splice_limit is not None else [], "the splice-site filter"),
                            (family_limit, "the family filter")):
            if other:
                refuse("--select-min-spacing and %s: %s is relative to the gene and the spacing's eligibility is per table row: one or the other"
                       % (other[0], name))
        coding_args = dict(coding_args, min_spacing=spacing)
    # (a flank makes the scan fetch the column: only where the file prints it, or where the filters ask for another flank than the default)
    repair_args = dict(min_mh=min_mh, min_oof=min_oof,
                       repair_flank=(repair.DEFAULT_FLANK if flank is None else flank) if with_scores else flank)
    try:
        params = select.Params(K, getattr(args, "select_min_score", None) or 0.0, getattr(args, "select_max_perfect", None),
                               getattr(args, "select_min_specificity", None), bool(getattr(args, "select_cds", False)))
    except ValueError as e:
        refuse(str(e))
    pairs = None
    if KP is not None:
        dmin, dmax = getattr(args, "pairs_min_distance", None), getattr(args, "pairs_max_distance", None)
        try:
            pairs = select.PairParams(KP, 50 if dmin is None else dmin, 500 if dmax is None else dmax,
                                      bool(getattr(args, "pairs_frameshift", False)), getattr(args, "pairs_orientation", None) or "any",
                                      distinct=bool(getattr(args, "pairs_distinct", False)))
        except ValueError as e:
            refuse("--select-pairs: " + str(e))
    return dict(params=params, output=getattr(args, "select_output", None) or (args.o + ".selected.csv"),
                only=bool(getattr(args, "select_only", False)), limits=dict(limits, **repair_args, **coding_args), repair_scores=with_scores,
                coding=with_coding, base_edit=with_edit, splice_edit=with_splice, families=family_pairs, pairs=pairs, pairs_output=getattr(args, "pairs_output", None) or (args.o + ".pairs.csv"),
                family_sets=integer(sets) if sets is not None else None,
                family_sets_output=getattr(args, "family_sets_output", None) or (args.o + ".family_sets.csv"))


def variants_request(args, world=1):
    """--variants and its options, checked like the other opt-in steps, before any side effect: None without it, else
    dict(path, samples, pass_only, seed, limits -- the keywords of select.Request)."""
    def refuse(msg):
        sys.exit("cropsr_amd: --variants: " + msg)

    limit_opts = (("--select-max-variants", "select_max_variants", "max_variants"),
                  ("--select-max-guide-variants", "select_max_guide_variants", "max_guide_variants"),
                  ("--select-max-seed-variants", "select_max_seed_variants", "max_seed_variants"),
                  ("--select-max-pam-variants", "select_max_pam_variants", "max_pam_variants"))
    given = [o for o, k, unset in [(o, k, None) for o, k, _ in limit_opts] + [("--variants-samples", "variants_samples", None),
                                                                             ("--variants-pass-only", "variants_pass_only", False),
                                                                             ("--variant-seed", "variant_seed", None)]
             if getattr(args, k, unset) not in (unset, None)]
    path = getattr(args, "variants", None)
    if path is None:
        if given:
            sys.exit("cropsr_amd: %s belongs to --variants" % given[0])
        return None
    from . import variants

    def integer(text):
        t = str(text).strip()
        return int(t) if t.isascii() and t.isdigit() else None

    if not 1 <= args.l <= variants.MAX_GUIDE:
        refuse("a guide of 1..%d letters has windows, not -l %d" % (variants.MAX_GUIDE, args.l))
    seed = getattr(args, "variant_seed", None)
    if seed is not None:
        if integer(seed) is None or not 1 <= integer(seed) <= args.l:
            refuse("--variant-seed is a number of letters 1..%d (-l), not %s" % (args.l, seed))
        seed = integer(seed)
    limits = {}
    for opt, key, kw in limit_opts:
        v = getattr(args, key, None)
        if v is not None:
            if integer(v) is None or integer(v) > 0xFFFFFFFF:
                refuse("%s is a number of variants, not %s" % (opt, v))
            limits[kw] = integer(v)
    samples = getattr(args, "variants_samples", None)
    if samples is not None:
        samples = [t for t in str(samples).split(",")]
        if not all(samples):
            refuse("--variants-samples is a comma-separated list of sample names, not %r" % getattr(args, "variants_samples"))
    if len(_device_list(args)) > 1:
        refuse("the variant column is not gathered: one GPU, and --devices names %d" % len(_device_list(args)))
    if getattr(args, "gpus", 1) > 1:
        refuse("the variant column is not gathered: one GPU, drop --gpus %d" % args.gpus)
    if world > 1:
        refuse("the variant column is not gathered: one GPU, and a launcher started %d ranks" % world)
    if getattr(args, "select", None) is None:
        refuse("the counts are printed in the selection file and bound the selection: --variants belongs to --select")
    import os
    if not os.path.isfile(path):
        refuse("no such file: %s" % path)
    return dict(path=path, samples=samples, pass_only=bool(getattr(args, "variants_pass_only", False)), seed=seed, limits=limits)


def sites_request(args, world=1):
    """--sites, --enzymes, --select-no-site, --select-assay and --assay-flank, checked like the other opt-in steps, before any
    side effect: None without them, else dict(fields -- print the two fields --, limits -- the keywords of select.Request).  The
    enzyme file is read here."""
    opts = (("--sites", "sites", False), ("--enzymes", "enzymes", None), ("--select-no-site", "select_no_site", None),
            ("--select-assay", "select_assay", None), ("--assay-flank", "assay_flank", None))
    given = [o for o, k, unset in opts if getattr(args, k, unset) not in (unset, None)]
    if not given:
        return None

    def refuse(msg):
        sys.exit("cropsr_amd: %s: %s" % (given[0], msg))

    from . import sites
    if not 1 <= args.l <= sites.MAX_GUIDE:
        refuse("a guide of 1..%d letters has a window, not -l %d" % (sites.MAX_GUIDE, args.l))
    if getattr(args, "select", None) is None:
        refuse("the enzymes are printed in the selection file and bound the selection: %s belongs to --select" % given[0])
    if len(_device_list(args)) > 1:
        refuse("the site column is not gathered: one GPU, and --devices names %d" % len(_device_list(args)))
    if getattr(args, "gpus", 1) > 1:
        refuse("the site column is not gathered: one GPU, drop --gpus %d" % args.gpus)
    if world > 1:
        refuse("the site column is not gathered: one GPU, and a launcher started %d ranks" % world)
    path = getattr(args, "enzymes", None)
    if path is None:
        enzymes = sites.EnzymeSet()
    else:
        import os
        if not os.path.isfile(path):
            sys.exit("cropsr_amd: --enzymes: no such file: %s" % path)
        try:
            enzymes = sites.load(path)
        except (ValueError, OSError, UnicodeDecodeError) as e:
            sys.exit("cropsr_amd: --enzymes: %s: %s" % (path, e))
    masks = {}
    for opt, key, kw in (("--select-no-site", "select_no_site", "forbid_sites"), ("--select-assay", "select_assay", "need_assay")):
        text = getattr(args, key, None)
        if text is None:
            continue
        names = [t.strip() for t in str(text).split(",")]
        if not all(names) or (kw == "forbid_sites" and "any" in [n.lower() for n in names]) or \
                (kw == "need_assay" and "cloning" in [n.lower() for n in names]):
            sys.exit("cropsr_amd: %s: a comma-separated list of enzyme names%s, not %r" % (opt, " or `any`" if kw == "need_assay" else " or `cloning`", text))
        try:
            masks[kw] = enzymes.mask(names)
        except ValueError as e:
            sys.exit("cropsr_amd: %s: %s" % (opt, e))
    flank = getattr(args, "assay_flank", None)
    t = None if flank is None else str(flank).strip()
    if t is not None and not (t.isascii() and t.isdigit()):
        sys.exit("cropsr_amd: --assay-flank: a number of letters %d..%d, not %s" % (enzymes.m_max, sites.MAX_FLANK, flank))
    try:
        flank = enzymes.check_flank(None if t is None else int(t))
    except ValueError as e:
        sys.exit("cropsr_amd: --assay-flank: %s" % e)
    fields = bool(getattr(args, "sites", False))
    return dict(fields=fields, names=list(enzymes.names), limits=dict(enzymes=enzymes, assay_flank=flank, site_fields=fields, **masks))


def properties_request(args, world=1):
    """--properties, checked like the other opt-in steps, before any side effect: True with it, False without."""
    if not getattr(args, "properties", False):
        return False

    def refuse(msg):
        sys.exit("cropsr_amd: --properties: " + msg)

    from . import properties
    if not properties.GUIDE_LENGTHS[0] <= args.l <= properties.GUIDE_LENGTHS[1]:
        refuse("a guide of %d..%d letters has properties, not -l %d" % (properties.GUIDE_LENGTHS + (args.l,)))
    if len(_device_list(args)) > 1:
        refuse("the property column is not gathered: one GPU, and --devices names %d" % len(_device_list(args)))
    if getattr(args, "gpus", 1) > 1:
        refuse("the property column is not gathered: one GPU, drop --gpus %d" % args.gpus)
    if world > 1:
        refuse("the property column is not gathered: one GPU, and a launcher started %d ranks" % world)
    return True


def _table_fields(sel_rows, names, strings, all_hits, guide_len, annotation):
    """Per row of sel_rows (its contig, strand and index fields name a table row) the main table's own fields for that row as
    rows.ContigRows builds them, without crispr_id."""
    fields = [None] * sel_rows.size
    for c in np.unique(sel_rows["contig"]).tolist():
        mine = np.flatnonzero(sel_rows["contig"] == c)
        minus = sel_rows["strand"][mine] == b"-"
        mine = np.concatenate([mine[~minus], mine[minus]])  # ('+' rows first, as ContigRows holds a contig's rows)
        n_plus = int((~minus).sum())
        index = sel_rows["index"][mine]
        mini = hitcols.take(all_hits[c], index[:n_plus], index[n_plus:])
        feats = None
        if annotation is not None:
            feats = (annotation.strings, hitcols.both(mini, "feat"))
        block = rows.ContigRows(names[c], bytes(strings[c]).decode("latin-1"), mini, guide_len, features=feats)
        for k, at in enumerate(mine.tolist()):
            fields[at] = block.row(k, "")[1:]
    return fields


def write_selection(path, selection, names, strings, all_hits, guide_len, offtarget, spec_M, annotation, properties=False,
                    repair_scores=False, coding=False, base_edit=False, splice_edit=False, families=None, variants=False, sites=None):
    """The selection file: a header, then per chosen row gene, rank (1-based), passing and the main table's own fields
    for that row as rows.ContigRows builds them, without crispr_id (those ids are random per run).  Genes in GFF order;
    genes with nothing selected are left out.  Python's csv module in the main table's dialect: the file is small.
    repair_scores: two more fields at the end of every row, mh_score and oof_score (repair.fields) of selection.mh / .oof.
    coding: five more after those, cds_offset, cds_length, cds_percent, transcripts_cut and transcripts (coding.fields).
    base_edit: four more after those, edit_targets, stop_codons, stop_codon and stop_percent (baseedit.fields).
    splice_edit: four more after those, splice_targets, splice_sites, donor_percent and acceptor_percent (baseedit.splice_fields).
    families (families.FamilyTable): seven more after those, family, family_size, members_hit, members (the covered members'
    labels, ;-joined, GFF order), outside_mm0, outside_hit_sum and outside_specificity (FAMILY_HEADER).
    variants: four more after everything else, var_site, var_guide, var_seed and var_pam (variants.fields) of selection.variants.
    sites (the enzyme set's names): two more after the variant fields, guide_sites and assay_enzymes (sites.fields) of
    selection.guide_sites / .assay_enzymes."""
    import csv
    from . import sites as site
    from . import variants as var
    from . import baseedit
    from . import coding as cod
    from . import repair
    sel_rows = selection.rows
    fields = _table_fields(sel_rows, names, strings, all_hits, guide_len, annotation)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["gene", "rank", "passing"] + rows.HEADER[1:] + rows.extra_header(offtarget, spec_M, properties)
                   + (repair.HEADER if repair_scores else []) + (cod.HEADER if coding else [])
                   + (baseedit.HEADER if base_edit else []) + (baseedit.SPLICE_HEADER if splice_edit else [])
                   + (FAMILY_HEADER if families is not None else []) + (var.HEADER if variants else [])
                   + (site.HEADER if sites is not None else []))
        for at, (r, rest) in enumerate(zip(sel_rows, fields)):
            more = repair.fields(repair.pack(selection.mh[at], selection.oof[at])) if repair_scores else ()
            if coding:
                more = tuple(more) + cod.fields(selection.cds_offset[at], selection.cds_length[at], selection.transcripts_cut[at], selection.transcripts[at])
            if base_edit:
                more = tuple(more) + baseedit.fields(selection.edit_targets[at], selection.stop_codons[at], selection.stop_offset[at], selection.cds_length[at])
            if splice_edit:
                more = tuple(more) + baseedit.splice_fields(selection.splice_targets[at], selection.donors[at], selection.acceptors[at],
                                                            selection.donor_offset[at], selection.acceptor_offset[at], selection.cds_length[at])
            if families is not None:
                more = tuple(more) + family_fields(families, selection, at)
            if variants:
                more = tuple(more) + var.fields(selection.variants[at])
            if sites is not None:
                more = tuple(more) + site.fields(int(selection.guide_sites[at]) | int(selection.assay_enzymes[at]) << 32, sites)
            w.writerow((selection.labels[int(r["gene"])], int(r["rank"]), int(selection.n_pass[int(r["gene"])])) + tuple(rest) + tuple(more))


FAMILY_HEADER = ["family", "family_size", "members_hit", "members", "outside_mm0", "outside_hit_sum", "outside_specificity"]


def family_fields(table, selection, at):
    """The seven family fields of row `at` of a selection (FAMILY_HEADER): hit_sum and specificity as the main table's
    specificity columns print them; an unscored join has no sum and no specificity.  A selected row is always a joined one:
    with families the selection runs on the joined columns, whose predicate fails every unjoined row, so no sentinel count
    reaches this file."""
    from .search import specificity
    g = int(selection.rows["gene"][at])
    hs = int(selection.outside_hit_sum[at])
    scored = hs != 0xFFFFFFFFFFFFFFFF
    return (table.family_name(g), int(selection.family_size[at]), int(selection.members_hit[at]), ";".join(selection.members[at]),
            int(selection.outside_mm0[at]), "%.6f" % (hs / float(1 << 30)) if scored else "",
            "%.6f" % float(specificity(np.uint64(hs))) if scored else "")


FAMILY_SET_HEADER = ["family", "family_size", "step", "members_new", "members_covered", "complete", "new_members", "gene"]
FAMILY_SET_TAIL = ["outside_mm0", "outside_hit_sum", "outside_specificity"]


def write_family_sets(path, selection, table, names, strings, all_hits, guide_len, offtarget, spec_M, annotation, properties=False):
    """The family-sets file (--family-sets): one row per pick, families in table order and steps ascending; families without
    a pick are left out.  FAMILY_SET_HEADER -- new_members: the labels of the members the pick covers first, ;-joined, GFF
    order; complete: 1 on every row of a family whose set covers all its members --, then the main table's own fields for the
    row as write_selection builds them, then FAMILY_SET_TAIL: what the guide hits outside the family, for the gene it was
    picked for.  Returns (families, complete, incomplete, without a passing guide)."""
    import csv
    from .search import specificity
    picks = selection.family_sets
    fields = _table_fields(picks, names, strings, all_hits, guide_len, annotation)
    mm0, hit_sum = selection.family_sets_stats["outside_mm0"], selection.family_sets_stats["outside_hit_sum"]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(FAMILY_SET_HEADER + rows.HEADER[1:] + rows.extra_header(offtarget, spec_M, properties) + FAMILY_SET_TAIL)
        before = {}
        for at, (p, rest) in enumerate(zip(picks, fields)):
            fam = int(p["family"])
            covered = int(p["covered"])
            new = covered & ~before.get(fam, 0)
            before[fam] = covered
            members = table.members(fam).tolist()
            hs = int(hit_sum[at])
            scored = hs != 0xFFFFFFFFFFFFFFFF
            w.writerow((table.names[fam], int(table.size[fam]), int(p["step"]), int(p["gain"]), bin(covered).count("1"),
                        int(bool(selection.family_complete[fam])), ";".join(table.labels[m] for j, m in enumerate(members) if new >> j & 1),
                        selection.labels[int(p["gene"])]) + tuple(rest)
                       + (int(mm0[at]), "%.6f" % (hs / float(1 << 30)) if scored else "", "%.6f" % float(specificity(np.uint64(hs))) if scored else ""))
    n = len(table.names)
    picked = set(picks["family"].tolist())
    complete = int(np.count_nonzero(selection.family_complete))
    return n, complete, len(picked) - complete, n - len(picked)


PAIR_HEADER = ["gene", "rank", "qualifying_pairs", "deletion_length", "in_frame", "chromosome"]
PAIR_GUIDE_FIELDS = ["start_pos", "end_pos", "cutsite", "strand", "sequence", "on_site_score"]


def write_pairs(path, selection, names, strings, all_hits, guide_len, repair_scores=False):
    """The pairs file: a header, then per chosen pair gene, rank (1-based), qualifying_pairs (all of the gene's),
    deletion_length, in_frame (1 when the length is a multiple of 3), chromosome and, for the left guide a and the right
    guide b, start_pos, end_pos, cutsite, strand, sequence and on_site_score as rows.ContigRows builds those fields (so
    `cutsite` is the main table's column; deletion_length is measured between the cut BOUNDARIES, select.py).  Genes in GFF
    order; genes without a pair are left out.  Python's csv module in the selection file's dialect.  repair_scores: mh_score
    and oof_score (repair.fields) of a and of b at the end of every row."""
    import csv
    from . import repair
    pairs = selection.pairs
    guides, chrom = {"a": [None] * pairs.size, "b": [None] * pairs.size}, [None] * pairs.size
    for c in np.unique(pairs["contig"]).tolist():
        mine = np.flatnonzero(pairs["contig"] == c)
        # both guides of the contig's pairs as one block of rows, '+' rows first, as ContigRows holds a contig's rows
        side = np.concatenate([np.zeros(mine.size, np.int64), np.ones(mine.size, np.int64)])
        at = np.concatenate([mine, mine])
        minus = np.concatenate([pairs["strand_a"][mine], pairs["strand_b"][mine]]) == b"-"
        index = np.concatenate([pairs["index_a"][mine], pairs["index_b"][mine]])
        order = np.concatenate([np.flatnonzero(~minus), np.flatnonzero(minus)])
        n_plus = int((~minus).sum())
        mini = hitcols.take(all_hits[c], index[order][:n_plus], index[order][n_plus:])
        block = rows.ContigRows(names[c], bytes(strings[c]).decode("latin-1"), mini, guide_len)
        for k, j in enumerate(order.tolist()):
            r = block.row(k, "")
            guides["ab"[side[j]]][at[j]] = (r[5], r[6], r[7], r[8], r[2], r[9])
            chrom[at[j]] = r[4]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(PAIR_HEADER + [n + "_a" for n in PAIR_GUIDE_FIELDS] + [n + "_b" for n in PAIR_GUIDE_FIELDS]
                   + ([n + s for s in ("_a", "_b") for n in repair.HEADER] if repair_scores else []))
        for at, r in enumerate(pairs):
            D = int(r["deletion_length"])
            more = sum((repair.fields(v) for v in selection.pairs_repair[at]), ()) if repair_scores else ()
            w.writerow((selection.labels[int(r["gene"])], int(r["rank"]), int(selection.n_pairs[int(r["gene"])]), D, int(D % 3 == 0),
                        chrom[at]) + guides["a"][at] + guides["b"][at] + tuple(more))


class _Early:
    """fn() on a helper thread; get() joins and returns its result or raises what it raised."""

    def __init__(self, fn, start=True):
        """start=False: nothing runs ahead; get() calls fn itself (for work that is only worth starting when the
        cheap checks of the command line have passed)."""
        import threading
        self._out = []
        self._fn = fn
        self._thread = threading.Thread(target=self._run, args=(fn,), name="cropsr-early") if start else None
        if start:
            self._thread.start()

    def _run(self, fn):
        try:
            self._out.append((fn(), None))
        except BaseException as e:  # handed to the caller of get()
            self._out.append((None, e))

    def get(self):
        if self._thread is None:
            if not self._out:
                self._run(self._fn)
        else:
            self._thread.join()
        value, error = self._out[0]
        if error is not None:
            raise error
        return value


def run(args, backend=None, out=sys.stdout, group=None):
    """main() of the reference (CROPSR.py:333-486) with the hot path swapped out.

    `backend` provides scan(contig_strings, guide_len) -> [hits dict per contig]
    and rescore(rows_u8, order) -> scores; it defaults to the HIP engine.  The CPU
    test-suite injects the oracle here to pin this host logic against the golden
    CSVs without a GPU.  `group`: the rendezvous.Group of a multi-process run
    (default: from the launcher's environment).
    """
    import os
    begin = time.time()
    if not args.cas9:
        sys.exit("Please select at least one CRISPR system: Cas9")  # CROPSR.py:335-336
    offtarget = bool(getattr(args, "offtarget", False))
    l_dev = device_guide_length(args.l)
    if offtarget and not NATIVE_GUIDE_LENGTHS[0] <= args.l <= NATIVE_GUIDE_LENGTHS[1]:  # (before any side effect, on every rank)
        sys.exit("cropsr_amd: --offtarget needs a guide length between %d and %d (got %d)" % (NATIVE_GUIDE_LENGTHS + (args.l,)))
    spec = specificity_request(args)  # (before any side effect, on every rank)
    selecting = select_request(args, spec, 1 if group is None else group.world)
    with_properties = properties_request(args, 1 if group is None else group.world)
    varying = variants_request(args, 1 if group is None else group.world)
    siting = sites_request(args, 1 if group is None else group.world)
    finalize = getattr(args, "score_finalize", "gpu")
    stages = {}  # --bench-json
    variant_set = None
    if varying is not None:  # the VCF is read here, before any side effect: a malformed line or an unknown sample ends the run
        from . import variants
        t_vcf = time.perf_counter()
        try:
            variant_set = variants.VariantSet(varying["path"], samples=varying["samples"], pass_only=varying["pass_only"])
        except (ValueError, OSError, EOFError) as e:
            sys.exit("cropsr_amd: --variants: %s: %s" % (varying["path"], e))
        stages["variants"] = dict(parse_s=time.perf_counter() - t_vcf, **variant_set.stats)
    own_group = group is None
    if own_group:
        group = _distributed()
    max_piece = int(os.environ.get("CROPSR_DIST_MAX_PIECE", "0")) or None
    if getattr(args, "devices", None) and group is not None and group.world > 1:
        # an external launcher started several ranks AND the command line asks for one process over several devices: every
        # rank would open every listed GPU, and only rank 0 would have a use for them
        sys.exit("cropsr_amd: --devices (one process over several GPUs) cannot run under a launcher that started %d ranks "
                 "(one process per GPU): give one of them" % group.world)

    if spec is not None and group is not None and group.world > 1:
        sys.exit("cropsr_amd: --specificity: the self search runs on one GPU, and a launcher started %d ranks" % group.world)
    if selecting is not None and group is not None and group.world > 1:
        select_request(args, spec, group.world)
    if group is not None and group.world > 1:
        properties_request(args, group.world)
        variants_request(args, group.world)
        sites_request(args, group.world)
    one_gpu = spec is not None or selecting is not None or with_properties  # the opt-in steps that take the arena path on one device

    def make_backend():
        if getattr(args, "devices", None) and not (one_gpu and len(_device_list(args)) == 1):
            return NodeBackend([int(d) for d in str(args.devices).split(",")], finalize)
        device = getattr(args, "device", None)
        if one_gpu and getattr(args, "devices", None):  # (one device named the --devices way: the arena path on it)
            device = int(_device_list(args)[0])
        if device is None:
            device = group.local_rank if group is not None else 0
        b = EngineBackend(device, group, finalize)
        try:  # (a genome of a few slices at least: below that there is nothing to prepare, one small lane is made on the spot)
            big = isinstance(args.f, str) and os.path.getsize(args.f) >= (256 << 20)
        except OSError:
            big = False
        if big and not offtarget and not one_gpu and not getattr(args, "annotate", False):
            b.warm_up()
        return b

    # Opening the GPU (HIP start-up, code object, two pinned staging buffers: ~0.3 s) starts NOW on a helper thread and
    # is collected where the backend is first needed: it overlaps reading and parsing the FASTA.
    # (not for a FASTA that is not there: that run ends with the reference's own exception and needs no GPU)
    readable = isinstance(args.f, str) and os.path.isfile(args.f)
    early = _Early(make_backend, start=readable) if backend is None else None
    # --annotate: the GFF (+ annotation_info) is parsed natively (crp_annotation_build releases the GIL) beside the FASTA read
    annotating = bool(getattr(args, "annotate", False))
    def build_annotation():
        from . import annotate
        t0 = time.perf_counter()
        a = annotate.Annotation(args.g, args.p)
        stages["annotation_build_s"] = time.perf_counter() - t0  # (on its own thread, beside the FASTA read and the GPU start-up)
        return a

    early_annot = _Early(build_annotation, start=readable) if annotating or selecting is not None else None

    def annotation_request(data, table):
        """annotate.Request for the contig strings of `table` (every rank builds the same one)."""
        from . import annotate
        formatted = 2 * fasta.count_byte(data, b">") != fasta.count_byte(data, b"\n") + 1  # CROPSR.py:61: dec = 1
        # (the Annotation itself is collected from its helper thread when the join first needs it: after the scan)
        return annotate.Request(early_annot.get, [annotate.contig_name(k) for k, _ in table], 1 if formatted else 0)

    if group is not None and group.rank != 0:
        # Ranks other than 0 of a multi-GPU run: read the same FASTA, scan their share of the contigs,
        # hand the tables to rank 0 -- which alone prints, draws ids and writes files -- and leave.
        # Whatever fails here is reported to every rank (group.check inside sharded_scan).
        from . import parallel
        own_backend = backend is None
        err, strings, request = None, [], None
        try:
            data = fasta.read_text_bytes(args.f)
            table = fasta.table_from_bytes(data)
            strings = [v for _, v in table]
            if annotating:
                request = annotation_request(data, table)
            del data, table
            if own_backend:
                backend = early.get()
        except Exception as e:
            err = "%s: %s" % (type(e).__name__, e)
        try:
            group.check(err)
            if hasattr(backend, "connect"):
                backend.connect()
            parallel.sharded_scan(backend, strings, l_dev, group, max_piece=max_piece, offtarget=offtarget, annotation=request)
        finally:
            if own_backend and backend is not None:
                backend.close()
            if own_group:
                group.close()
        return
    verbose = args.verbose
    if verbose:
        print(BANNER + f"""
        You are currently utilizing the following settings:

        CROPSR version:                                 {__version__}
        Path to genome file in FASTA format:            {args.f}
        Path to output file:                            {args.o}
        Length of the gRNA sequence:                    {args.l}
        Length of flanking region for verification:     {args.L}
        Number of available CPUs:                       {cpu_count()}
        Path to annotation file in GFF format:          {args.g}
        Path to annotation_info file in TXT format:     {args.p}
        Designing for CRISPR system:
            Streptococcus pyogenes Cas9                 {args.cas9}
        """, file=out)

    timing = open("time.txt", "w")  # CROPSR.py:371 (CWD side effect, kept)
    # CROPSR.py:375 reads the GFF into a DataFrame it never uses (pandas: 0.2 s to import, ~1 s per 40 MB of GFF).  Its
    # observable behaviour -- two -v messages, the exceptions of a missing or malformed file -- is kept, at the place the
    # reference has it; the work itself starts NOW on a helper thread, beside the FASTA read and the scan
    import io as _io
    gff_messages = _io.StringIO()

    def reference_gff_import():
        t0 = time.perf_counter()
        try:
            return import_gff_file(args.g, verbose, gff_messages)
        finally:
            stages["reference_gff_import_s"] = time.perf_counter() - t0  # (thread time; what the run waits for: ..._wait_s)

    early_gff = _Early(reference_gff_import)

    # CROPSR.py:374, 54-74 -- read as text mode would (universal newlines), kept as bytes
    t_stage = time.perf_counter()
    data = fasta.read_text_bytes(args.f)
    if verbose:
        print(f"Genome file {args.f} successfully imported", file=out)
        if 2 * fasta.count_byte(data, b">") != fasta.count_byte(data, b"\n") + 1:
            print("formatting genome", file=out)
            print(f"Genome file {args.f} successfully formatted", file=out)
    table = fasta.table_from_bytes(data)  # == fasta.contig_table(text).items(), without printing the genome
    stages["read_fasta_s"] = time.perf_counter() - t_stage
    request, request_err = None, None
    if annotating or selecting is not None:  # (--select names its genes through the same request)
        try:
            request = annotation_request(data, table)
        except Exception as e:  # (single process: raised below, after the reference's own GFF import had its say)
            request_err = e
    del data
    if verbose:
        print("The genome was successfully converted to a dictionary", file=out)
    t_wait = time.perf_counter()
    try:
        early_gff.get()  # CROPSR.py:375 (raises like the reference if -g is missing or unreadable)
    finally:
        out.write(gff_messages.getvalue())
        stages["reference_gff_import_wait_s"] = time.perf_counter() - t_wait

    if verbose:
        # (the blank line in the middle carries the reference's 12 blanks of indentation)
        print("\n            Initiating PAM site detection.\n            \n"
              "            Please wait, this may take a while...\n            ", file=out)

    if getattr(args, "seed", None) is not None:
        np.random.seed(args.seed)

    if selecting is not None and selecting["families"] is not None:  # the family table: before the output file is touched
        from . import families
        if request_err is not None:
            raise request_err
        try:
            family_table = families.FamilyTable(selecting["families"], request.annotation.genes()[0])
        except families.FamilyInputError as e:
            sys.exit("cropsr_amd: --select: --families: " + str(e))
        if family_table.n_unknown:
            print("cropsr_amd: --families: %d names of %s are no gene of %s" % (family_table.n_unknown, args.families, args.g), file=sys.stderr)
        selecting["limits"]["families"] = family_table
    if varying is not None:
        from . import variants
        if request_err is not None:
            raise request_err
        unknown = [c for c in variant_set.chrom_index if c not in set(request.names)]
        if unknown:
            print("cropsr_amd: --variants: %d CHROMs of %s name no contig of %s" % (len(unknown), varying["path"], args.f), file=sys.stderr)
        selecting["limits"].update(variants=variants.Request(variant_set, request.names, request.dec), variant_seed=varying["seed"],
                                   **varying["limits"])
    if siting is not None:
        selecting["limits"].update(siting["limits"])
    select_only = selecting is not None and selecting["only"]
    if not select_only:
        rows.write_header(args.o, offtarget=offtarget, specificity=None if spec is None else spec["max_mm"],
                          properties=with_properties)  # CROPSR.py:402-405

    names = [k for k, _ in table]
    strings = [v for _, v in table]  # contig strings as bytes, one byte per character
    own_backend = backend is None
    t_stage = time.perf_counter()
    if group is None:
        if own_backend:
            backend = early.get()
        if request_err is not None:
            raise request_err
        extra = dict(offtarget=True) if offtarget else {}
        if request is not None and annotating:
            extra["annotation"] = request
        if spec is not None:
            extra["specificity"] = spec
        if selecting is not None:  # (the keyword a backend only meets when selecting)
            from . import select
            more = dict(pairs=selecting["pairs"]) if selecting["pairs"] is not None else {}  # (likewise: only with --select-pairs)
            extra["select"] = select.Request(selecting["params"], request, **selecting["limits"], **more)
        if with_properties:  # (likewise: only a scan that is asked for the columns meets the keyword)
            extra["properties"] = True
        from .search import SelfCapacityError
        try:
            all_hits = backend.scan(strings, l_dev, **extra)
        except SelfCapacityError as e:
            sys.exit("cropsr_amd: --specificity: the self search needs %d bytes of device memory for one arena of this genome: "
                     "more than it may take" % e.needed)
    else:  # contigs (cut where longer than a rank's share) over all GPUs, tables gathered here
        from . import parallel
        err = None
        try:
            if request_err is not None:
                raise request_err
            if own_backend:
                backend = early.get()
        except Exception as e:
            err = "%s: %s" % (type(e).__name__, e)
        group.check(err)
        if hasattr(backend, "connect"):
            backend.connect()
        all_hits = parallel.sharded_scan(backend, strings, l_dev, group, max_piece=max_piece, offtarget=offtarget, annotation=request)
        if hasattr(backend, "finalize_gathered"):
            all_hits = backend.finalize_gathered(all_hits)
    if l_dev != args.l:  # a length outside the engine's range: the literal keep-filter, on the host
        all_hits = [refilter_hits(h, len(s), args.l) for h, s in zip(all_hits, strings)]
    world = 1 if group is None else group.world
    if own_group and group is not None:
        # the exchange is over: the other ranks leave now (Group.close is a barrier) instead of waiting, watched by
        # each other's abort channels, for however long this rank formats and writes the CSV
        group.close()
        group = None
    stages["upload_scan_fetch_s"] = time.perf_counter() - t_stage
    if selecting is not None:
        t_select = time.perf_counter()
        selection = all_hits.selection
        write_selection(selecting["output"], selection, names, strings, all_hits, args.l, offtarget, None if spec is None else spec["max_mm"],
                        request.annotation if annotating else None, properties=with_properties, repair_scores=selecting["repair_scores"],
                        coding=selecting["coding"], base_edit=selecting["base_edit"], splice_edit=selecting["splice_edit"],
                        families=selecting["limits"].get("families"), variants=varying is not None,
                        sites=siting["names"] if siting is not None and siting["fields"] else None)
        stages["select"] = dict(selection.stats, write_s=time.perf_counter() - t_select, genes=len(selection.labels),
                                rows_selected=int(selection.rows.size), k=selecting["params"].k)
        if selecting["family_sets"] is not None:
            t_sets = time.perf_counter()
            counts = write_family_sets(selecting["family_sets_output"], selection, selecting["limits"]["families"], names, strings, all_hits,
                                       args.l, offtarget, None if spec is None else spec["max_mm"], request.annotation if annotating else None,
                                       properties=with_properties)
            print("cropsr_amd: --family-sets %d: %d families, %d complete, %d incomplete, %d without a passing guide"
                  % ((selecting["family_sets"],) + counts), file=sys.stderr)
            stages["family_sets"] = dict({k: v for k, v in selection.family_sets_stats.items() if not k.startswith("outside_")},
                                         write_s=time.perf_counter() - t_sets, picks=int(selection.family_sets.size))
        if selecting["pairs"] is not None:
            t_pairs = time.perf_counter()
            write_pairs(selecting["pairs_output"], selection, names, strings, all_hits, args.l, repair_scores=selecting["repair_scores"])
            stages["pairs"] = dict(selection.pairs_stats, write_s=time.perf_counter() - t_pairs, pairs_selected=int(selection.pairs.size),
                                   kp=selecting["pairs"].k)
            if selecting["pairs"].distinct:
                stages["pairs"]["distinct"] = True
    if not annotating:
        request = None  # (from here on the request means the `features` column)
    if request is not None:
        stages["annotation_join_s"] = getattr(backend, "last_annotate_s", None)  # part of upload_scan_fetch_s (this rank's share)
        stages["annotation_strings"] = len(request.annotation.strings)

    # (the native formatter's row buffers are sized for guide lengths 1..50; other lengths take the csv module)
    native = getattr(args, "csv_writer", "native") == "native" and NATIVE_GUIDE_LENGTHS[0] <= args.l <= NATIVE_GUIDE_LENGTHS[1]
    once = getattr(args, "each_contig_once", False)
    dataset = rows.NativeDataset() if native else rows.Dataset()  # Complete_dataset, CROPSR.py:407
    ids = None
    if native and not select_only:
        # every pass draws its ids from one RNG stream, in order; the pass sizes are known now,
        # so a worker draws pass k+1's ids while pass k is formatted and written
        per_contig = [int(h["pos_plus"].size + h["pos_minus"].size) for h in all_hits]
        sizes = per_contig if once else np.cumsum(per_contig).tolist()
        ids = rows.IdStream(sizes, reverse=True)
    t_stage = time.perf_counter()
    n_rows_written = 0
    # --each-contig-once with the native writer: a pass is one contig and independent of the others, so consecutive passes
    # go to the formatter TOGETHER until they make up four million rows (one call, one team of threads, blocks that span short
    # contigs: a scaffold of 3 500 rows on its own is formatted by a single thread, and a genome has hundreds of them);
    # the bytes are the passes' bytes one after the other, the per-pass lines of time.txt are written when their rows are
    import os
    batching = native and once and not getattr(args, "reference_sleep", False) and os.environ.get("CROPSR_BATCH_PASSES", "1") != "0"
    batch_limit = int(os.environ.get("CROPSR_BATCH_ROWS", BATCH_ROWS))
    batch, batch_rows = [], 0
    in_flight = []  # at most one: (thread, the passes it writes, [its exception]) -- a batch is formatted and written on a
                    # helper thread while this one builds the next batch's tables and collects its ids

    def finish_write(swallow=False):
        nonlocal n_rows_written
        while in_flight:
            th, passes, err = in_flight.pop()
            th.join()
            if err and not swallow:
                raise err[0]
            for ds, _ in passes:
                n_rows_written += len(ds)
                timing.write("Total runtime of the program is " + str(time.time() - begin))  # CROPSR.py:477, once per pass

    def flush_batch():
        nonlocal batch, batch_rows
        if not batch:
            return
        finish_write()  # (the file takes one writer at a time, in order)
        import threading
        passes, err = batch, []

        def work():
            try:
                rows.write_passes_native(args.o, passes, backend.rescore)
            except BaseException as e:
                err.append(e)

        th = threading.Thread(target=work, name="cropsr-csv")
        in_flight.append((th, passes, err))
        th.start()
        batch, batch_rows = [], 0

    try:
        for name, s, hits in zip(names, strings, all_hits):
            print("Searching on Chromosome: ", name[:25], file=out)  # CROPSR.py:410-411
            print("With start of sequence: ", bytes(s[:25]).decode("latin-1"), file=out)
            if select_only:  # the selection file is the output: no rows, no ids
                continue
            feats = None
            if request is not None:  # the device's label-set id per row ('+' rows, then '-' rows) + the string table
                feats = (request.annotation.strings, hitcols.both(hits, "feat"))
            block = (rows.ContigTable(name, s, hits, args.l, features=feats) if native
                     else rows.ContigRows(name, bytes(s).decode("latin-1"), hits, args.l, features=feats))
            if once:
                dataset = rows.NativeDataset() if native else rows.Dataset()  # opt-in fix of CROPSR.py:407
            dataset.append(block)
            if verbose:
                # CROPSR.py:436-439 counts regex matches BEFORE the keep-filter; the
                # engine reports kept hits, so re-count only for this message.
                import re
                n_sites = sum(1 for _ in re.finditer(rb"(?=.GG)", s)) + sum(1 for _ in re.finditer(rb"(?=CC.)", s))
                print(f"""
                {n_sites:n} Cas9 PAM sites were found on {name[1::]}
                """, file=out)
            if batching:
                batch.append((dataset, ids.next(len(dataset))))
                batch_rows += len(dataset)
                if batch_rows >= batch_limit:
                    flush_batch()
                continue
            if native:  # CROPSR.py:442-474
                rows.write_pass_native(args.o, dataset, backend.rescore, ids)
            else:
                rows.write_pass(args.o, dataset, backend.rescore)
            n_rows_written += len(dataset)
            end = time.time()
            timing.write("Total runtime of the program is " + str(end - begin))  # CROPSR.py:477
            if getattr(args, "reference_sleep", False):
                time.sleep(5)  # CROPSR.py:478
        flush_batch()
        finish_write()
    except BaseException:
        finish_write(swallow=True)  # (no writer thread outlives a failing run)
        raise
    stages["format_write_s"] = time.perf_counter() - t_stage
    timing.close()
    if ids is not None:
        ids.close()
    if getattr(backend, "last_stream", None):  # the pipelined scan's own account of the upload + scan + fetch stage
        stages["scan_stream"] = backend.last_stream
    if getattr(backend, "last_properties", None):  # --properties / the --select-* property filters: the kernel's time and rows
        stages["properties"] = backend.last_properties
    if getattr(backend, "last_repair", None):  # --repair-scores / --select-min-oof / --select-min-mh: the repair kernel's time and rows
        stages["repair"] = backend.last_repair
    if getattr(backend, "last_sites", None):  # --sites / --select-no-site / --select-assay: plane build, rank build and column kernel
        stages["sites"] = backend.last_sites
    if getattr(backend, "last_variants", None):  # --variants: the VCF's parse time and counts, the track's size, the kernel's time and rows
        stages["variants"] = dict(stages.get("variants", {}), **backend.last_variants)
    if getattr(backend, "last_specificity", None):  # --specificity: the handles' kernel times, the join's among them
        stages["specificity"] = backend.last_specificity
    if getattr(backend, "last_gather", None):  # one process over several devices (--devices): the node's gatherv, in numbers
        stages["node_gatherv"] = backend.last_gather
        stages["devices"] = list(backend.node.devices)
    if own_backend:
        backend.close()
    if verbose:
        print(f"The output file has been generated at {args.o}", file=out)
    if getattr(args, "bench_json", None):
        import json
        kept = int(sum(h["pos_plus"].size + h["pos_minus"].size for h in all_hits))
        stages.update(total_s=time.time() - begin, contigs=len(strings), characters=int(sum(len(v) for v in strings)),
                      kept_hits=kept, rows_written=int(n_rows_written), world=world,
                      gRNAs_per_s_end_to_end=kept / max(1e-9, time.time() - begin))
        with open(args.bench_json, "w") as f:
            json.dump(stages, f)
            f.write("\n")


def _leave(status):
    """The one way out of main() for a process that opened the GPU: if a communicator bootstrap never returned
    (Engine.comm_init), a helper thread still sits inside RCCL and the runtime's tear-down at a normal exit may wait for
    it -- flush and leave through os._exit, on the error paths too."""
    eng_mod = sys.modules.get(__package__ + ".engine")  # (only a run that opened the GPU has imported it)
    if eng_mod is not None:
        eng_mod.leave_if_comm_stuck(status)
    node_mod = sys.modules.get(__package__ + ".node")  # (--devices: ncclCommInitAll runs on a helper thread of the library)
    if node_mod is not None and node_mod.comm_stuck():
        import os
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(status)


def main(argv=None):
    import os
    args = build_parser().parse_args(argv)
    from . import launch
    if getattr(args, "devices", None) and getattr(args, "gpus", 1) > 1:
        sys.exit("cropsr_amd: --devices (one process over several GPUs) and --gpus N (one process per GPU) are two ways to the "
                 "same result: give one of them")
    select_request(args, specificity_request(args))  # (--gpus N: refused here, before any rank is started)
    properties_request(args)
    variants_request(args)
    sites_request(args)
    if launch.wanted(getattr(args, "gpus", 1)):
        # no launcher in the environment: this process (which never touches the GPU) starts the ranks as fresh
        # children of the same command line and leaves with their status (cropsr_amd/launch.py)
        if getattr(args, "device", None) is not None and os.environ.get("CROPSR_GATHER", "rccl") != "host":
            # every rank would open the same GPU, RCCL would refuse the duplicate device after a whole bootstrap round
            # and the run would crawl on over the host transport without a word
            sys.exit("cropsr_amd: --device names ONE GPU, but --gpus %d puts every rank on the GPU of its own rank; drop "
                     "--device (or, to rehearse several ranks on one GPU, set CROPSR_GATHER=host)" % args.gpus)
        sys.stdout.flush()
        sys.exit(launch.spawn_ranks([sys.executable, "-m", "cropsr_amd"] + list(sys.argv[1:] if argv is None else argv),
                                    args.gpus))
    status = 0
    try:
        run(args)
    except SystemExit as e:  # (sys.exit(message) inside run: the message goes to stderr, the status is 1)
        if isinstance(e.code, str):
            sys.stderr.write(e.code + "\n")
        status = e.code if isinstance(e.code, int) else (1 if e.code else 0)
    except Exception as e:
        import traceback
        from . import rendezvous
        status = 1
        if isinstance(e, rendezvous.RankError):  # agreed on by every rank: all leave the same way, together
            if _ACTIVE_GROUP is not None:
                _ACTIVE_GROUP.close()
            sys.stderr.write("cropsr_amd: " + str(e) + "\n")
        else:
            traceback.print_exc()
            if _ACTIVE_GROUP is not None and _ACTIVE_GROUP.world > 1:
                # this rank alone failed (a HIP or RCCL error in the middle of the exchange, ...): its peers may sit in
                # a collective that will never complete -- take the whole run down with the reason
                _ACTIVE_GROUP.abort("%s: %s" % (type(e).__name__, e))
    # every way out of a process that may have opened the GPU ends here
    _leave(status)
    sys.exit(status)


if __name__ == "__main__":
    main()
