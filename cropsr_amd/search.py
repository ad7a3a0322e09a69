"""Off-target search of given guides against the genome (not reference behaviour).

A Cas-OFFinder-style search: a PAM pattern and query guides in, every site of the genome within M mismatches of each
query out, on both strands.  The work runs in libcropsr_hip.so (crp_search_*, kernels in crp_search.hip) on the
arenas the genome already sits in; this module validates input, maps arena positions back to contigs and writes TSV.

    python -m cropsr_amd.search -f genome.fa --pattern NNNNNNNNNNNNNNNNNNNNNRG --pam-length 3 --guides guides.txt -m 4 \
        -o sites.tsv

Definition (what the tests check):
  genome   FASTA records, parsed plainly (read_fasta): name = header up to its first whitespace, sequence = the
           record's lines with all ASCII whitespace removed, positions 0-based in it
  base     acgtACGT, and U (read as A); anything else (N, IUPAC codes, u, punctuation) is not a base
  pattern  T (1..32) letters of ACGTRYSWKMBDHVN, 5' -> 3' on the target strand
  site     the window of T characters at forward start i of a contig (strand '+'), or its reverse complement
           (strand '-'); every pattern letter other than N needs a base of its set there (N: any character)
  query    T letters of ACGTN; mismatches = positions where the query has a base and the oriented site does not
           hold it (a non-base always mismatches); N positions are not compared
  result   the sites with <= M (0..8) mismatches, ordered by query, contig, position, strand ('+' first), and
           counts[q, k] = sites of query q with exactly k mismatches

Bulges (search_bulges, --dna-bulge / --rna-bulge; DESIGN.md section 15, Bulges).  They need the PAM's length P: the
guide region is the T - P positions outside the PAM (all N in the pattern), on its 5' side (...NGG) or 3' side (TTTV...).
  span     a query's first to last ACGT letter inside the guide region; a bulge lies strictly inside it, starting
           at query position s
  DNA d    (1 <= d <= D) the site is an oriented window of T + d characters that fits the pattern with d more N in
           its guide region; query position i pairs with window position i if i < s, else i + d, for
           span_first < s <= span_last; window positions s .. s + d - 1 stay unpaired
  RNA r    (1 <= r <= R) the window has T - r characters (r fewer N); query positions s .. s + r - 1 stay unpaired,
           span_first < s and s + r - 1 < span_last; i < s pairs with i, i >= s + r with i - r
  result   mismatches over the paired positions, by the rule above; one result per (query, kind, contig,
           position, strand), kinds none, DNA 1..D, RNA 1..R, with the fewest mismatches over s (<= M) and
           bulge_at = s - span_first for the smallest s that reaches them; ordered by query, kind, contig, position,
           strand.  No merging across kinds.  D, R in 0..2 and T + D <= 32; a span too short for a bulge (DNA: 2
           letters, RNA: r + 2) is refused
"""
import argparse
import ctypes
import sys

import numpy as np

from . import _native as nat

MAX_T = 32
MAX_MM = 8
IUPAC = "ACGTRYSWKMBDHVN"
SITE_DTYPE = np.dtype([("query", "<u4"), ("contig", "<u4"), ("position", "<i8"), ("strand", "S1"), ("mismatches", "u1")])
MAX_BULGE = 2
BULGE_SITE_DTYPE = np.dtype([("query", "<u4"), ("kind", "u1"), ("bulge_size", "u1"), ("bulge_at", "u1"), ("contig", "<u4"),
                             ("position", "<i8"), ("strand", "S1"), ("mismatches", "u1")])
_WS = b" \t\n\r\x0b\x0c"


class SearchInputError(ValueError):
    """A pattern, guide or mismatch bound outside the definition."""


class SiteCapacityError(RuntimeError):
    """More sites than site_cap: .counts are exact, .n_sites is what a repeat needs."""

    def __init__(self, counts, n_sites, site_cap):
        self.counts, self.n_sites = counts, n_sites
        super().__init__("%d sites exceed site_cap=%d" % (n_sites, site_cap))


def check_pattern(pattern):
    p = pattern.decode() if isinstance(pattern, bytes) else str(pattern)
    p = p.upper()
    if not 1 <= len(p) <= MAX_T:
        raise SearchInputError("pattern must have 1..%d letters, not %d" % (MAX_T, len(p)))
    bad = sorted(set(p) - set(IUPAC))
    if bad:
        raise SearchInputError("pattern %r: letters outside %s: %s" % (pattern, IUPAC, "".join(bad)))
    return p


def check_max_mm(max_mm):
    if not isinstance(max_mm, (int, np.integer)) or not 0 <= int(max_mm) <= MAX_MM:
        raise SearchInputError("mismatches must be an integer 0..%d, not %r" % (MAX_MM, max_mm))
    return int(max_mm)


def guide_run(pattern):
    """(start, length) of the pattern's N letters when they form one contiguous run, else None."""
    idx = [k for k, c in enumerate(pattern) if c == "N"]
    if not idx or idx[-1] - idx[0] + 1 != len(idx):
        return None
    return idx[0], len(idx)


def check_pam_len(pattern, pam_len):
    T = len(pattern)
    if not isinstance(pam_len, (int, np.integer)) or not 1 <= int(pam_len) < T:
        raise SearchInputError("PAM length must be 1..%d for a pattern of %d letters, not %r" % (T - 1, T, pam_len))
    return int(pam_len)


def check_query(pattern, query, pam_len=None):
    """A query of the pattern's length over ACGTN (upper-cased), or a shorter guide padded to one:

    pam_len None  the guide is exactly as long as the pattern's single contiguous run of N and fills it; the other
                  positions become N (21 letters for NNNNNNNNNNNNNNNNNNNNNGG, 23 for TTTVNNNNNNNNNNNNNNNNNNNNNNN)
    pam_len P     the PAM is the pattern's last P letters (or its first P, for a PAM on the 5' side such as Cas12a's),
                  every letter outside it is N, and a guide of at most T - P letters sits right next to it: a 20-nt
                  or a truncated 18-nt guide with ...NGG and P = 3, a 21-nt one with ...NNGRRT and P = 6

    The pattern alone cannot say which of its N letters belong to the PAM (NGG has one, NNGRRT two, TTTV none), so a
    guide of any other length is refused rather than placed by a guess."""
    q = query.decode() if isinstance(query, bytes) else str(query)
    q = q.upper()
    bad = sorted(set(q) - set("ACGTN"))
    if bad or not q:
        raise SearchInputError("guide %r: letters outside ACGTN: %s" % (query, "".join(bad)) if bad else "empty guide")
    T = len(pattern)
    if len(q) == T:
        return q
    if pam_len is None:
        run = guide_run(pattern)
        if run is not None and len(q) == run[1]:
            return "N" * run[0] + q + "N" * (T - run[0] - len(q))
        raise SearchInputError("guide %r has %d letters: the pattern has %d%s; a shorter guide needs the PAM's length "
                               "(--pam-length) or N at the PAM positions" % (
                                   query, len(q), T, "" if run is None else ", its N run %d" % run[1]))
    lo, hi, pam3 = guide_region(pattern, pam_len)
    if len(q) > hi - lo:
        raise SearchInputError("guide %r has %d letters: at most %d fit next to a PAM of %d in a pattern of %d" % (
            query, len(q), hi - lo, int(pam_len), T))
    at = hi - len(q) if pam3 else lo  # the guide ends where a 3' PAM begins, starts where a 5' PAM ends
    return "N" * at + q + "N" * (T - at - len(q))


def parse_guides(text, pattern, pam_len=None):
    """Guides file: one guide per non-empty line, `SEQUENCE [NAME]`; `#` starts a comment; the name defaults to the
    1-based line number; shorter guides are padded by check_query.  Returns (names, queries)."""
    if isinstance(text, bytes):
        text = text.decode()
    names, queries = [], []
    for k, line in enumerate(text.splitlines(), 1):
        fields = line.split("#", 1)[0].split()
        if not fields:
            continue
        queries.append(check_query(pattern, fields[0], pam_len))
        names.append(" ".join(fields[1:]) if len(fields) > 1 else str(k))
    if not queries:
        raise SearchInputError("no guides")
    return names, queries


def parse_fasta(data):
    """FASTA bytes -> (names, sequences as bytes): name = header up to its first whitespace, sequence = the record's
    lines with all ASCII whitespace removed."""
    names, seqs, cur = [], [], None
    for line in data.split(b"\n"):
        if line.startswith(b">"):
            if cur is not None:
                seqs.append(b"".join(cur).translate(None, _WS))
            head = line[1:].split()
            names.append(head[0].decode("utf-8", "replace") if head else "")
            cur = []
        elif cur is not None:
            cur.append(line)
        elif line.strip(_WS):
            raise SearchInputError("FASTA: sequence before the first '>' header")
    if cur is not None:
        seqs.append(b"".join(cur).translate(None, _WS))
    return names, seqs


def read_fasta(path):
    with open(path, "rb") as f:
        return parse_fasta(f.read())


class ArenaSearch:
    """One crp_search handle: the candidates of one arena for one pattern."""

    def __init__(self, arena, pattern, budget=None):
        self.pattern = check_pattern(pattern)
        self._arena = arena  # (the handle reads the arena's planes: keep it alive)
        h = ctypes.c_void_p()
        nat.check(nat.lib().crp_search_create(arena._h, self.pattern.encode(), len(self.pattern), ctypes.byref(h)),
                  "crp_search_create", arena._engine._ctx)
        self._h = h
        if budget is not None:
            nat.check(nat.lib().crp_search_set_budget(self._h, int(budget)), "crp_search_set_budget")

    def close(self):
        if self._h:
            nat.lib().crp_search_destroy(self._h)
            self._h = None

    __del__ = close

    def set_limits(self, batch_queries=0, first_site_slots=0):
        """crp_search_set_limits: queries per compare launch and first device site slots (0: the defaults)."""
        nat.check(nat.lib().crp_search_set_limits(self._h, int(batch_queries), int(first_site_slots)), "crp_search_set_limits")

    def candidates(self):
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        nat.check(nat.lib().crp_search_candidates(self._h, ctypes.byref(a), ctypes.byref(b)), "crp_search_candidates")
        return a.value, b.value

    def run(self, queries, max_mm, site_cap, kind=("-", 0), spans=None):
        """crp_search_run, or crp_search_run_bulge for a bulge kind (this handle's pattern: the kind's window pattern), as
        it is: (status, counts (Q, M + 1) uint32, n_sites).  queries: already checked strings; spans (bulge kinds): (Q, 2)
        query positions of each span's first and last letter."""
        bulge, size = kind
        Q = len(queries)
        blob = "".join(queries).encode()
        counts = np.zeros((Q, max_mm + 1), dtype=np.uint32)
        n = ctypes.c_uint64()
        tail = (int(max_mm), int(site_cap), counts.ctypes.data_as(nat.u32p), ctypes.byref(n))
        if size:
            sp = np.ascontiguousarray(spans, dtype=np.uint8).reshape(Q, 2)
            code = nat.SEARCH_BULGE_DNA if bulge == "DNA" else nat.SEARCH_BULGE_RNA
            st = nat.lib().crp_search_run_bulge(self._h, blob, Q, code, int(size), sp.ctypes.data_as(nat.u8p), *tail)
        else:
            st = nat.lib().crp_search_run(self._h, blob, Q, *tail)
        return st, counts, n.value

    def fetch(self, n, kind=("-", 0)):
        """(query u32, arena position u32, strand u8, mismatches u8) of the last run's n sites, and bulge_at u8 after a run
        of a bulge kind."""
        cols = [np.empty(n, np.uint32), np.empty(n, np.uint32)] + [np.empty(n, np.uint8) for _ in range(3 if kind[1] else 2)]
        ptrs = [c.ctypes.data_as(p) for c, p in zip(cols, (nat.u32p, nat.u32p, nat.u8p, nat.u8p, nat.u8p))]
        name = "crp_search_fetch_bulge" if kind[1] else "crp_search_fetch"
        nat.check(getattr(nat.lib(), name)(self._h, *ptrs, n), name)
        return tuple(cols)

    def stats(self):
        out = np.zeros(6, dtype=np.float64)
        nat.check(nat.lib().crp_search_stats(self._h, out.ctypes.data_as(nat.f64p), 6), "crp_search_stats")
        keys = ("extract_ms", "compare_ms", "extract_launches", "compare_launches", "chunks", "candidate_bytes")
        return dict(zip(keys, (float(v) for v in out)))


class SearchResult:
    def __init__(self, counts, sites, candidates):
        self.counts = counts          # (Q, M + 1) uint32
        self.sites = sites            # SITE_DTYPE, ordered by query, contig, position, strand
        self.candidates = candidates  # (n_plus, n_minus) over the whole genome


def search(genome, pattern, queries, max_mm, site_cap=None, budget=None, pam_len=None):
    """Every site of `genome` (engine.Genome) within max_mm mismatches of each query, over all its arenas.
    site_cap=None: as many sites as there are; else SiteCapacityError (with exact counts) beyond it.  budget: device
    bytes for one chunk of candidates (None: the library's default).  pam_len: how check_query pads shorter guides."""
    pattern = check_pattern(pattern)
    max_mm = check_max_mm(max_mm)
    queries = [check_query(pattern, q, pam_len) for q in queries]
    counts, sites, cands, n_total = _search_kinds(genome, pattern, None, queries, max_mm, [("-", 0)], None, site_cap, budget)
    if site_cap is not None and n_total > int(site_cap):
        raise SiteCapacityError(counts[:, 0], n_total, int(site_cap))
    return SearchResult(counts[:, 0], sites[list(SITE_DTYPE.names)].astype(SITE_DTYPE), cands[0])


def _search_kinds(genome, pattern, pam_len, queries, max_mm, kinds, spans, site_cap, budget):
    """Every kind of `kinds` over every arena of `genome`, on checked input: one library handle per kind and arena, on
    the kind's window pattern, and site_cap counts the sites of all kinds together.  Returns (counts (Q, kinds, M + 1)
    uint32, BULGE_SITE_DTYPE sites ordered by query, kind, contig, position, strand, per kind (n_plus, n_minus), the
    number of sites); the sites are only complete when that number is within site_cap."""
    counts = np.zeros((len(queries), len(kinds), max_mm + 1), dtype=np.uint64)
    parts, n_total, cands = [], 0, []
    for k, kind in enumerate(kinds):
        size = kind[1]
        kp = kind_pattern(pattern, pam_len, *kind) if size else pattern
        cand = [0, 0]
        for a, group in zip(genome.arenas, genome.groups):
            s = ArenaSearch(a, kp, budget)
            try:
                npl, nmi = s.candidates()
                cand[0] += npl
                cand[1] += nmi
                cap = (1 << 62) if site_cap is None else max(0, int(site_cap) - n_total)
                st, c, n = s.run(queries, max_mm, cap, kind, spans)
                if st not in (nat.CRP_OK, nat.CRP_ERR_CAPACITY):
                    nat.check(st, "crp_search_run_bulge" if size else "crp_search_run", a._engine._ctx)
                counts[:, k] += c
                n_total += n
                if st == nat.CRP_OK:  # (an arena after the cap was reached ran with cap 0: nothing to fetch)
                    qi, pos, strand, mm, *at = s.fetch(n, kind)
                    offs = np.asarray(a.offsets, dtype=np.int64)
                    j = np.searchsorted(offs, pos.astype(np.int64), "right") - 1
                    part = np.empty(n, BULGE_SITE_DTYPE)
                    part["query"] = qi
                    part["kind"] = k
                    part["bulge_size"] = size
                    part["bulge_at"] = at[0] if size else 0
                    part["contig"] = np.asarray(group, dtype=np.uint32)[j] if n else 0
                    part["position"] = pos.astype(np.int64) - offs[j]
                    part["strand"] = np.where(strand == 0, b"+", b"-")
                    part["mismatches"] = mm
                    parts.append(part)
            finally:
                s.close()
        cands.append(tuple(cand))
    sites = np.concatenate(parts) if parts else np.empty(0, BULGE_SITE_DTYPE)
    order = np.lexsort((sites["strand"] == b"-", sites["position"], sites["contig"], sites["kind"], sites["query"]))
    return counts.astype(np.uint32), sites[order], cands, n_total


# ---------------------------------------------------------------- bulges
def check_bulges(pattern, pam_len, dna_bulge, rna_bulge):
    """(D, R) of a bulge search: each 0..2, the PAM's length given when either is not 0, T + D <= 32."""
    for v, what in ((dna_bulge, "DNA"), (rna_bulge, "RNA")):
        if not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= MAX_BULGE:
            raise SearchInputError("%s bulge size must be an integer 0..%d, not %r" % (what, MAX_BULGE, v))
    D, R = int(dna_bulge), int(rna_bulge)
    if D or R:
        if pam_len is None:
            raise SearchInputError("a bulge search needs the PAM's length (--pam-length)")
        guide_region(pattern, pam_len)
    if len(pattern) + D > MAX_T:
        raise SearchInputError("a DNA bulge of %d needs windows of %d letters: at most %d" % (D, len(pattern) + D, MAX_T))
    return D, R


def guide_region(pattern, pam_len):
    """(lo, hi, pam_3prime): the pattern positions [lo, hi) outside the PAM, all N; which side the PAM is on."""
    T = len(pattern)
    P = check_pam_len(pattern, pam_len)
    if set(pattern[:T - P]) <= {"N"}:
        return 0, T - P, True
    if set(pattern[P:]) <= {"N"}:
        return P, T, False
    raise SearchInputError("pattern %s has letters other than N outside its first or last %d" % (pattern, P))


def bulge_kinds(D, R):
    """[(bulge, size)] in result order: ("-", 0), ("DNA", 1..D), ("RNA", 1..R)."""
    return [("-", 0)] + [("DNA", d) for d in range(1, D + 1)] + [("RNA", r) for r in range(1, R + 1)]


def kind_pattern(pattern, pam_len, bulge, size):
    """The window pattern of one kind: the guide region's N run longer by a DNA bulge, shorter by an RNA bulge."""
    lo, hi, pam3 = guide_region(pattern, pam_len)
    n = hi - lo + (size if bulge == "DNA" else -size if bulge == "RNA" else 0)
    return "N" * n + pattern[hi:] if pam3 else pattern[:lo] + "N" * n


def query_spans(pattern, pam_len, queries, D, R):
    """(Q, 2) uint8: each query's span (first, last ACGT position in the guide region); refuses a span too short."""
    lo, hi, _ = guide_region(pattern, pam_len)
    need = max(2 if D else 0, R + 2 if R else 0)
    out = np.zeros((len(queries), 2), dtype=np.uint8)
    for k, q in enumerate(queries):
        idx = [i for i in range(lo, hi) if q[i] in "ACGT"]
        if len(idx) == 0 or idx[-1] - idx[0] + 1 < need:
            raise SearchInputError("guide %r: its span of %d letters is too short for the bulge (at least %d)" % (
                q, idx[-1] - idx[0] + 1 if idx else 0, need))
        out[k] = idx[0], idx[-1]
    return out


class BulgeSearchResult:
    def __init__(self, counts, sites, kinds, spans, candidates):
        self.counts = counts          # (Q, kinds, M + 1) uint32
        self.sites = sites            # BULGE_SITE_DTYPE, ordered by query, kind, contig, position, strand
        self.kinds = kinds            # [(bulge, size)]: kind k of .counts and .sites
        self.spans = spans            # (Q, 2) uint8: each query's span (bulge_at counts from its first letter)
        self.candidates = candidates  # per kind: (n_plus, n_minus) over the whole genome


def search_bulges(genome, pattern, queries, max_mm, pam_len, dna_bulge, rna_bulge, site_cap=None, budget=None):
    """search() plus every site with a DNA bulge of 1..dna_bulge or an RNA bulge of 1..rna_bulge (see the module's
    docstring), over all arenas of `genome`: one library handle per kind and arena, on the kind's window pattern.
    The kind-none slice is what search() returns.  site_cap counts the sites of all kinds together."""
    pattern = check_pattern(pattern)
    max_mm = check_max_mm(max_mm)
    D, R = check_bulges(pattern, pam_len, dna_bulge, rna_bulge)
    queries = [check_query(pattern, q, pam_len) for q in queries]
    spans = query_spans(pattern, pam_len, queries, D, R) if D or R else np.zeros((len(queries), 2), np.uint8)
    kinds = bulge_kinds(D, R)
    counts, sites, cands, n_total = _search_kinds(genome, pattern, pam_len, queries, max_mm, kinds, spans, site_cap, budget)
    if site_cap is not None and n_total > int(site_cap):
        raise SiteCapacityError(counts, n_total, int(site_cap))
    return BulgeSearchResult(counts, sites, kinds, spans, cands)


# ---------------------------------------------------------------- TSV
_CODE = np.full(256, 4, dtype=np.uint8)  # 0..3 = A C G T, 4 = not a base
for _c, _v in zip(b"ACGTUacgt", (0, 1, 2, 3, 0, 0, 1, 2, 3)):
    _CODE[_c] = _v


def site_string(contig, position, strand, query):
    """The oriented window: bases upper case, mismatched positions lower case, non-base characters N (n where the
    query compares them)."""
    return bulge_alignment(contig, position, strand, query, "-", 0, 0)[0]


def format_sites(names, queries, contig_names, contigs, sites):
    return _format_site_rows(names, queries, contig_names, contigs, sites, None, None)


def bulge_alignment(contig, position, strand, query, bulge, size, s):
    """(site, query_aligned) of a site of one kind with its bulge at query position s: the oriented window with '-'
    at RNA-bulge positions (case as site_string: paired mismatches in lower case; unpaired DNA-bulge characters upper
    case), and the query with '-' at DNA-bulge positions."""
    T = len(query)
    W = T + size if bulge == "DNA" else T - size if bulge == "RNA" else T
    codes = _CODE[np.frombuffer(contig[position:position + W], dtype=np.uint8)]
    if strand in (b"-", "-"):
        codes = np.where(codes == 4, 4, 3 - codes)[::-1]
    win = ["ACGTN"[c] for c in codes]

    def paired(ch, q):
        return ch.lower() if q != "N" and ch != q else ch

    if bulge == "DNA":
        site = [ch if s <= p < s + size else paired(ch, query[p if p < s else p - size]) for p, ch in enumerate(win)]
        return "".join(site), query[:s] + "-" * size + query[s:]
    if bulge == "RNA":
        site = [paired(win[i], query[i]) for i in range(s)] + ["-"] * size + \
               [paired(win[i - size], query[i]) for i in range(s + size, T)]
        return "".join(site), query
    return "".join(paired(ch, query[p]) for p, ch in enumerate(win)), query


def format_bulge_sites(names, queries, contig_names, contigs, res):
    """The sites TSV of a bulge search (BulgeSearchResult): today's columns plus bulge (-, DNA, RNA), bulge_size,
    bulge_at, and the aligned site and query."""
    return _format_site_rows(names, queries, contig_names, contigs, res.sites, res.kinds, res.spans)


def _format_site_rows(names, queries, contig_names, contigs, sites, kinds, spans):
    """The sites TSV; with the kinds and spans of a bulge search, the bulge columns and the aligned query too."""
    head = ["name", "query", "contig", "position", "strand", "mismatches"]
    lines = ["\t".join(head + (["bulge", "bulge_size", "bulge_at", "site", "query_aligned"] if kinds else ["site"])) + "\n"]
    for r in sites:
        q, k, pos, strand = int(r["query"]), int(r["contig"]), int(r["position"]), r["strand"]
        row = [names[q], queries[q], contig_names[k], pos, strand.decode(), int(r["mismatches"])]
        if kinds:
            (bulge, size), at = kinds[int(r["kind"])], int(r["bulge_at"])
            site, qa = bulge_alignment(contigs[k], pos, strand, queries[q], bulge, size, int(spans[q, 0]) + at)
            row += [bulge, size, at, site, qa]
        else:
            row.append(site_string(contigs[k], pos, strand, queries[q]))
        lines.append("\t".join(map(str, row)) + "\n")
    return "".join(lines)


def format_bulge_counts(names, queries, kinds, counts):
    return _format_count_rows(names, queries, counts, kinds)


def format_counts(names, queries, counts):
    return _format_count_rows(names, queries, counts[:, None], None)


def _format_count_rows(names, queries, counts, kinds):
    """The counts TSV of counts (Q, kinds, M + 1): one line per query and kind; with the kinds of a bulge search, the
    bulge and bulge_size columns too."""
    head = ["name", "query"] + (["bulge", "bulge_size"] if kinds else []) + ["mm%d" % k for k in range(counts.shape[2])]
    lines = ["\t".join(head) + "\n"]
    for q in range(len(queries)):
        for k, kind in enumerate(kinds or [()]):
            lines.append("\t".join(map(str, [names[q], queries[q], *kind, *counts[q, k].tolist()])) + "\n")
    return "".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cropsr_amd.search",
                                 description="Every genome site within M mismatches of each given guide, on both strands "
                                             "(MI355X; DESIGN.md section 15).")
    ap.add_argument("-f", "--fasta", required=True, help="genome FASTA")
    ap.add_argument("--pattern", required=True, help="PAM pattern over ACGTRYSWKMBDHVN, e.g. NNNNNNNNNNNNNNNNNNNNNRG")
    ap.add_argument("--guides", required=True, help="one guide per line: SEQUENCE [NAME]; '#' starts a comment")
    ap.add_argument("--pam-length", type=int, default=None, metavar="P",
                    help="the PAM is the pattern's last (or, for a 5' PAM, first) P letters: guides shorter than the pattern "
                         "sit right next to it (3 for ...NGG, 6 for ...NNGRRT, 4 for TTTV...); without it a shorter guide "
                         "must be exactly as long as the pattern's N run")
    ap.add_argument("-m", "--mismatches", type=int, default=4, help="most mismatches reported (0..8, default 4)")
    ap.add_argument("-o", "--output", required=True, help="sites TSV")
    ap.add_argument("--dna-bulge", type=int, default=0, metavar="D",
                    help="also report sites with a DNA bulge (extra genomic bases) of 1..D (0..2, default 0); needs "
                         "--pam-length; adds the columns bulge, bulge_size, bulge_at, query_aligned")
    ap.add_argument("--rna-bulge", type=int, default=0, metavar="R",
                    help="also report sites with an RNA bulge (unpaired guide letters) of 1..R (0..2, default 0); needs "
                         "--pam-length")
    ap.add_argument("--counts", help="per-guide counts TSV (mm0..mmM; with bulges one line per guide and kind)")
    ap.add_argument("--device", type=int, default=0, help="HIP device")
    args = ap.parse_args(argv)
    try:
        pattern = check_pattern(args.pattern)
        max_mm = check_max_mm(args.mismatches)
        if args.pam_length is not None:
            check_pam_len(pattern, args.pam_length)
        D, R = check_bulges(pattern, args.pam_length, args.dna_bulge, args.rna_bulge)
        with open(args.guides, "rb") as f:
            names, queries = parse_guides(f.read(), pattern, args.pam_length)
        if D or R:
            query_spans(pattern, args.pam_length, queries, D, R)
        contig_names, contigs = read_fasta(args.fasta)
    except (SearchInputError, OSError, UnicodeDecodeError) as e:
        ap.error(str(e))
    from .engine import Engine
    with Engine(args.device) as eng:
        g = eng.genome(contigs)
        try:
            res = search_bulges(g, pattern, queries, max_mm, args.pam_length, D, R)
        finally:
            g.close()
    kinds = res.kinds if D or R else None  # (None: the plain TSV columns)
    with open(args.output, "w") as f:
        f.write(_format_site_rows(names, queries, contig_names, contigs, res.sites, kinds, res.spans))
    if args.counts:
        with open(args.counts, "w") as f:
            f.write(_format_count_rows(names, queries, res.counts, kinds))
    if D or R:
        print("%d guides, %d kinds, %d sites within %d mismatches" % (len(queries), len(res.kinds), res.sites.size, max_mm),
              file=sys.stderr)
    else:
        print("%d guides, %d + %d candidate sites, %d sites within %d mismatches" % (
            len(queries), res.candidates[0][0], res.candidates[0][1], res.sites.size, max_mm), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
