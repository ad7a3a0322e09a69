"""Off-target search of given guides against the genome (not reference behaviour).

A Cas-OFFinder-style search: a PAM pattern and query guides in, every site of the genome within M mismatches of each
query out, on both strands.  The work runs in libcropsr_hip.so (crp_search_*, kernels in crp_search.hip) on the
arenas the genome already sits in; this module validates input, maps arena positions back to contigs and writes TSV.

    python -m cropsr_amd.search -f genome.fa --pattern NNNNNNNNNNNNNNNNNNNNNRG --pam-length 3 --guides guides.txt -m 4 \
        -o sites.tsv
    python -m cropsr_amd.search -f genome.fa --pattern NNNNNNNNNNNNNNNNNNNNNGG --pam-length 3 --guides guides.txt -m 4 \
        --score hsu2013 --no-sites --counts ranking.tsv

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

Specificity score (score=, --score / --weights; DESIGN.md section 15, Specificity score).  It needs the PAM's length too.
  g        the guide region's positions numbered 0 .. G - 1 from the PAM-distal end (3' PAM: g = pattern position;
           5' PAM: g counts down from the pattern's last position), so g = G - 1 is next to the PAM on either side
  scheme   factor[g] in [0, 1] and shape[n][d], n = 0..8 mismatches, d = 0..31 = last - first mismatching g
  hit      for a site of kind none with n >= 1 mismatches at g1 < .. < gn: h = factor[g1] * .. * factor[gn] * shape[n][gn - g1]
           (float64, left to right), v = rint(h * 2^30) as an integer; n = 0 (the target or a perfect copy) adds nothing
  result   hit_sum[q] = the sum of v over the query's sites with 1..M mismatches (exact, summed on the device),
           specificity[q] = 1 / (1 + hit_sum[q] / 2^30).  A query with a base at a PAM position is refused

Pair table (score=PairTable(..), --score-table; DESIGN.md section 15, Pair tables): the CFD form of a hit's value, next
to the scheme above.  It needs the PAM's length P; G, g, hit_sum and specificity are as above, there is no shape term.
  pair     pair[g][a][b] in [0, 1]: a the query's letter at g, b the oriented site's letter, both over A, C, G, T in
           that order and both read 5' -> 3' on the target strand's sense (as the sites TSV prints them); the 12 entries
           with a != b matter, the diagonal is ignored
  pam      pam_offsets: k = 0..3 offsets inside the PAM, strictly ascending, 0 = the PAM's 5'-most letter, each on a
           pattern letter other than N (so the site holds a base there); pam: 4^k values in [0, 1] indexed by the site's
           letters at those offsets, first offset most significant, A, C, G, T = 0..3; with k = 0 the PAM factor is 1.0
  hit      for a site of kind none with n >= 1 mismatches at g1 < .. < gn: h = 1.0; h = h * pair[g][query letter][site
           letter] for g = g1 .. gn; h = h * pam[index of the site's PAM letters] (float64, one correctly rounded multiply
           per step); v = rint(h * 2^30) as an integer.  A non-base site character at a mismatching position: v = 0 (the
           site still counts).  n = 0 adds nothing; a query with a base at a PAM position is refused

    python -m cropsr_amd.search -f genome.fa --pattern NNNNNNNNNNNNNNNNNNNNNRG --pam-length 3 --guides guides.txt -m 4 \
        --score-table cfd.txt --no-sites --counts ranking.tsv

Self search (search_self, --self; DESIGN.md section 15, Self search): every guide site of the genome is a query.
  input    the (candidate) pattern, the PAM's length P (required), M in 0..4, optionally a guide pattern of the same
           length (default: the pattern) and a score.  The guide pattern has the same guide region (all N there) and at
           every PAM position a letter whose base set is contained in the pattern's (...NGG guides against ...NRG
           candidates); anything else is refused
  guide    a guide site is a site of the guide pattern, either strand, whose G guide-region characters are all bases;
           its query is those G letters (upper case, U as A) with N at the PAM positions
  result   per guide site s, ordered by contig, position, strand ('+' first): counts[s][k], k = 0..M = the candidate
           sites other than s itself (same contig, position and strand) with exactly k mismatches against s's query;
           hit_sum[s] = the sum of v over those with 1..M mismatches; specificity[s] = 1 / (1 + hit_sum[s] / 2^30).
           The site on the other strand of the same position, and perfect copies elsewhere, count like any site: row s
           is search(genome, pattern, [query of s], M, pam_len=P, score=.., sites=False) with 1 taken off counts[0]

    python -m cropsr_amd.search -f genome.fa --pattern NNNNNNNNNNNNNNNNNNNNNRG --guide-pattern NNNNNNNNNNNNNNNNNNNNNGG \
        --pam-length 3 --self -m 3 --score hsu2013 -o guides.tsv

CSV join (specificity_columns, ArenaSelfSearch.join_hits, crp_search_self_join_hits; `python -m cropsr_amd --specificity`;
DESIGN.md section 15, CSV join): the self search's rows handed to the hits of the guide table's scan, on the GPU.
  between  the last scan of an arena at guide length l (crp_scan_score: the kept .GG / CC. hits, positions = regex match
           indices shifted by the contig's arena offset) and a self-search handle of the same arena whose candidate pattern
           has T = l + 3 letters, P = 3 and its PAM on the 3' side: its guide region is the l letters the scan calls `sequence`
  '+' hit  match index i (guide s[i-l:i], PAM s[i:i+3]): its site is forward start i - l, strand '+'
  '-' hit  match index j (CC. at j, guide s[j+3:j+3+l]): its site is forward start j, strand '-'
  joined   if that site is a guide site of the handle, the hit gets that site's counts[0..M] and hit_sum
  unjoined every count is 0xFFFFFFFF and hit_sum 2^64 - 1: the site is only a candidate; a guide-region character is not
           a base; a '-' hit whose window the contig end cuts (the reference keeps those up to len + 10)
  where    positions are arena positions throughout; a hit and its site always lie in the same contig.  A handle without
           a score joins the counts only (hit_sum all-ones).  specificity comes from hit_sum on the host (specificity())
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
SCORE_SHIFT = 30   # a hit's value is rint(h * 2^SCORE_SHIFT)
SHAPE_N, SHAPE_D = MAX_MM + 1, 32
# Hsu et al. 2013 (Nat Biotechnol 31:827, "DNA targeting specificity of RNA-guided Cas9 nucleases"): the experimentally
# determined mismatch weights of the 20 guide positions, PAM-distal first, as the MIT / CRISPOR specificity score uses them
HSU2013_W = (0, 0, 0.014, 0, 0, 0.395, 0.317, 0, 0.389, 0.079, 0.445, 0.508, 0.613, 0.851, 0.732, 0.828, 0.615, 0.804, 0.685, 0.583)
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

    def set_scheme(self, scheme):
        """crp_search_set_scheme with a Scheme, crp_search_set_pair_scheme with a PairScheme, or None to clear either."""
        if scheme is None:
            st = nat.lib().crp_search_set_scheme(self._h, None, 0, 0, None)
        elif isinstance(scheme, PairScheme):
            pair, G, offs, k, pam = scheme.native_args()
            st = nat.lib().crp_search_set_pair_scheme(self._h, pair, G, nat.SEARCH_PAM_3PRIME if scheme.pam3 else nat.SEARCH_PAM_5PRIME,
                                                      offs, k, pam)
        else:
            f = np.ascontiguousarray(scheme.factor, dtype=np.float64)
            sh = np.ascontiguousarray(scheme.shape, dtype=np.float64).reshape(-1)
            st = nat.lib().crp_search_set_scheme(self._h, f.ctypes.data_as(nat.f64p), f.size,
                                                 nat.SEARCH_PAM_3PRIME if scheme.pam3 else nat.SEARCH_PAM_5PRIME,
                                                 sh.ctypes.data_as(nat.f64p))
        nat.check(st, "crp_search_set_pair_scheme" if isinstance(scheme, PairScheme) else "crp_search_set_scheme", self._arena._engine._ctx)

    def run_scored(self, queries, max_mm, site_cap):
        """crp_search_run_scored as it is: (status, counts (Q, M + 1) uint32, n_sites, hit_sum (Q,) uint64)."""
        Q = len(queries)
        counts = np.zeros((Q, max_mm + 1), dtype=np.uint32)
        hit_sum = np.zeros(Q, dtype=np.uint64)
        n = ctypes.c_uint64()
        st = nat.lib().crp_search_run_scored(self._h, "".join(queries).encode(), Q, int(max_mm), int(site_cap),
                                             counts.ctypes.data_as(nat.u32p), ctypes.byref(n), hit_sum.ctypes.data_as(nat.u64p))
        return st, counts, n.value, hit_sum

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
    def __init__(self, counts, sites, candidates, hit_sum=None):
        self.counts = counts          # (Q, M + 1) uint32
        self.sites = sites            # SITE_DTYPE, ordered by query, contig, position, strand
        self.candidates = candidates  # (n_plus, n_minus) over the whole genome
        self.hit_sum = hit_sum        # (Q,) uint64: the sum of the hits' values (None without score=)
        self.specificity = None if hit_sum is None else specificity(hit_sum)  # (Q,) float64


def search(genome, pattern, queries, max_mm, site_cap=None, budget=None, pam_len=None, score=None, sites=True):
    """Every site of `genome` (engine.Genome) within max_mm mismatches of each query, over all its arenas.
    site_cap=None: as many sites as there are; else SiteCapacityError (with exact counts) beyond it.  budget: device
    bytes for one chunk of candidates (None: the library's default).  pam_len: how check_query pads shorter guides.
    score: "hsu2013", G weights or a PairTable (see check_score; needs pam_len): the result's .hit_sum and .specificity, summed on
    the device.  sites=False: no site list is kept or fetched (.sites is empty, no SiteCapacityError): counts and sums
    only."""
    pattern = check_pattern(pattern)
    max_mm = check_max_mm(max_mm)
    queries = [check_query(pattern, q, pam_len) for q in queries]
    scheme = check_score(pattern, pam_len, score, queries)
    if not sites:
        site_cap = 0
    counts, rows, cands, n_total, hit_sum = _search_kinds(genome, pattern, None, queries, max_mm, [("-", 0)], None, site_cap, budget,
                                                           scheme)
    if sites and site_cap is not None and n_total > int(site_cap):
        raise SiteCapacityError(counts[:, 0], n_total, int(site_cap))
    return SearchResult(counts[:, 0], rows[list(SITE_DTYPE.names)].astype(SITE_DTYPE), cands[0], hit_sum)


def _search_kinds(genome, pattern, pam_len, queries, max_mm, kinds, spans, site_cap, budget, scheme=None):
    """Every kind of `kinds` over every arena of `genome`, on checked input: one library handle per kind and arena, on
    the kind's window pattern, and site_cap counts the sites of all kinds together.  With a scheme the kind-none runs
    are scored.  Returns (counts (Q, kinds, M + 1) uint32, BULGE_SITE_DTYPE sites ordered by query, kind, contig,
    position, strand, per kind (n_plus, n_minus), the number of sites, hit_sum (Q,) uint64 or None); the sites are only
    complete when that number is within site_cap."""
    counts = np.zeros((len(queries), len(kinds), max_mm + 1), dtype=np.uint64)
    hit_sum = None if scheme is None else np.zeros(len(queries), dtype=np.uint64)
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
                if scheme is not None and not size:
                    s.set_scheme(scheme)
                    st, c, n, hs = s.run_scored(queries, max_mm, cap)
                    hit_sum += hs  # (a handle's sum is below 2^62: the arenas are added here)
                else:
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
    return counts.astype(np.uint32), sites[order], cands, n_total, hit_sum


# ---------------------------------------------------------------- specificity score
class Scheme:
    """factor (G,) and shape (9, 32) float64 in [0, 1]; the guide region [lo, hi) of the pattern and the PAM's side."""

    def __init__(self, factor, shape, lo, hi, pam3):
        self.factor, self.shape, self.lo, self.hi, self.pam3 = factor, shape, lo, hi, pam3

    def g_positions(self):
        """(G,) the pattern position of g = 0 .. G - 1."""
        return np.arange(self.lo, self.hi) if self.pam3 else np.arange(self.hi - 1, self.lo - 1, -1)


class PairTable:
    """The score= argument of the pair-table form (see the module's docstring): pair (G, 4, 4), pam_offsets (k offsets
    inside the PAM) and pam (4^k values, or None with no offsets).  make_scheme checks it against a pattern."""

    def __init__(self, pair, pam_offsets=(), pam=None):
        self.pair, self.pam_offsets, self.pam = pair, pam_offsets, pam


class PairScheme:
    """A checked PairTable on a pattern: pair (G, 4, 4) float64 with 1.0 on the diagonal, pam_offsets, pam (4^k,), the
    PAM letters' pattern positions, the guide region [lo, hi) of the pattern and the PAM's side."""

    def __init__(self, pair, pam_offsets, pam, pam_positions, lo, hi, pam3):
        self.pair, self.pam_offsets, self.pam, self.pam_positions = pair, pam_offsets, pam, pam_positions
        self.lo, self.hi, self.pam3 = lo, hi, pam3

    g_positions = Scheme.g_positions

    def native_args(self):
        """(pair, G, pam_offsets, k, pam) as crp_search_set_pair_scheme takes them."""
        self._c = (np.ascontiguousarray(self.pair, dtype=np.float64).reshape(-1), np.array(self.pam_offsets, dtype=np.intc),
                   np.ascontiguousarray(self.pam, dtype=np.float64))  # (kept alive while the call runs)
        k = len(self.pam_offsets)
        return (self._c[0].ctypes.data_as(nat.f64p), self.pair.shape[0], self._c[1].ctypes.data_as(nat.i32p) if k else None, k,
                self._c[2].ctypes.data_as(nat.f64p) if k else None)


MAX_PAM_OFFSETS = 3


def _make_pair_scheme(pattern, pam_len, table):
    lo, hi, pam3 = guide_region(pattern, pam_len)
    G, P = hi - lo, int(pam_len)
    try:
        pair = np.array(table.pair, dtype=np.float64)
    except (TypeError, ValueError):
        raise SearchInputError("pair table: the pair values must be numbers, G x 4 x 4 of them") from None
    if pair.ndim != 3 or pair.shape[1:] != (4, 4):
        raise SearchInputError("pair table: the pair values must be G x 4 x 4, not %s" % (pair.shape,))
    if pair.shape[0] != G:
        raise SearchInputError("pair table for a guide region of %d positions: the pattern's has %d" % (pair.shape[0], G))
    pair = pair.copy()
    pair[:, np.arange(4), np.arange(4)] = 1.0  # (the diagonal is ignored)
    if not (np.isfinite(pair).all() and (pair >= 0).all() and (pair <= 1).all()):
        raise SearchInputError("pair table: every pair value (12 per position) must be present, finite and in [0, 1]")
    try:
        offs = tuple(table.pam_offsets)
    except TypeError:
        raise SearchInputError("pair table: pam_offsets must be a sequence of integers") from None
    if len(offs) > MAX_PAM_OFFSETS:
        raise SearchInputError("pair table: at most %d PAM offsets, not %d" % (MAX_PAM_OFFSETS, len(offs)))
    pam_at = hi if pam3 else 0
    for k, o in enumerate(offs):
        if not isinstance(o, (int, np.integer)) or not 0 <= int(o) < P:
            raise SearchInputError("pair table: PAM offset %r outside 0..%d" % (o, P - 1))
        if k and int(o) <= int(offs[k - 1]):
            raise SearchInputError("pair table: PAM offsets must be strictly ascending")
        if pattern[pam_at + int(o)] == "N":
            raise SearchInputError("pair table: PAM offset %d is on an N of pattern %s: a site may hold no base there" % (o, pattern))
    offs = tuple(int(o) for o in offs)
    if table.pam is None:
        if offs:
            raise SearchInputError("pair table: PAM offsets without PAM values")
        pam = np.ones(1, dtype=np.float64)
    else:
        try:
            pam = np.array(table.pam, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise SearchInputError("pair table: the PAM values must be numbers") from None
        if not offs or pam.size != 4 ** len(offs):
            raise SearchInputError("pair table: %d PAM values for %d offsets (4^k of them; none without offsets)" % (pam.size, len(offs)))
        if not (np.isfinite(pam).all() and (pam >= 0).all() and (pam <= 1).all()):
            raise SearchInputError("pair table: PAM values must be finite and in [0, 1]")
    return PairScheme(pair, offs, pam, tuple(pam_at + o for o in offs), lo, hi, pam3)


def hsu_shape(G):
    """shape[n][d] of the Hsu et al. 2013 score for a guide region of G: 1 for n = 0, 1 / n^2 for n = 1, and for n >= 2
    1 / (((G - 1 - d / (n - 1)) / (G - 1)) * 4 + 1) / n^2, d / (n - 1) being the mean distance between consecutive
    mismatches (0 where d < n - 1, which n mismatches cannot have, and where d > G - 1)."""
    shape = np.zeros((SHAPE_N, SHAPE_D), dtype=np.float64)
    shape[0, :] = 1.0
    shape[1, :] = 1.0
    for n in range(2, SHAPE_N):
        for d in range(n - 1, min(G, SHAPE_D)):
            shape[n, d] = 1.0 / (((float(G - 1) - d / float(n - 1)) / float(G - 1)) * 4.0 + 1.0) / float(n * n)
    return shape


def make_scheme(pattern, pam_len, score):
    """The Scheme of score = "hsu2013" (G = 20 only) or a sequence of G weights W in [0, 1], PAM-distal first
    (factor = 1 - W, the Hsu shape with 19 -> G - 1); the PairScheme of a PairTable."""
    if pam_len is None:
        raise SearchInputError("a specificity score needs the PAM's length (--pam-length)")
    if isinstance(score, PairTable):
        return _make_pair_scheme(pattern, pam_len, score)
    lo, hi, pam3 = guide_region(pattern, pam_len)
    G = hi - lo
    if isinstance(score, str):
        if score != "hsu2013":
            raise SearchInputError("unknown scoring scheme %r (hsu2013, or a list of weights)" % score)
        if G != len(HSU2013_W):
            raise SearchInputError("hsu2013 is defined for a guide region of %d positions, not %d" % (len(HSU2013_W), G))
        w = np.array(HSU2013_W, dtype=np.float64)
    else:
        try:
            w = np.array([float(v) for v in score], dtype=np.float64)
        except (TypeError, ValueError):
            raise SearchInputError("weights must be numbers: %r" % (score,)) from None
        if w.size != G:
            raise SearchInputError("%d weights for a guide region of %d positions" % (w.size, G))
        if not (np.isfinite(w).all() and (w >= 0).all() and (w <= 1).all()):
            raise SearchInputError("weights must be finite and in [0, 1]")
    return Scheme(1.0 - w, hsu_shape(G), lo, hi, pam3)


def check_score(pattern, pam_len, score, queries):
    """None without a score; else its Scheme, after refusing every query with a base at a PAM position (a mismatch
    there would have no g)."""
    if score is None:
        return None
    scheme = make_scheme(pattern, pam_len, score)
    for q in queries:
        if set(q[:scheme.lo] + q[scheme.hi:]) - {"N"}:
            raise SearchInputError("guide %r has a base at a PAM position: a scored search needs N there" % q)
    return scheme


def parse_weights(text):
    """A weights file: numbers separated by whitespace or commas, PAM-distal first; `#` starts a comment."""
    if isinstance(text, bytes):
        text = text.decode()
    fields = " ".join(line.split("#", 1)[0] for line in text.splitlines()).replace(",", " ").split()
    try:
        return [float(v) for v in fields]
    except ValueError as e:
        raise SearchInputError("weights file: %s" % e) from None


def parse_pair_table(text):
    """A pair-table file -> PairTable.  One statement per line, `#` starts a comment:

        pam-offsets 1 2        optional, once; absent = no PAM factor
        pam AG 0.25            one line per combination of letters at those offsets; unlisted combinations are 0
        pair 19 A C 0.5        g (0-based, PAM-distal first), query letter, site letter, value

    G is the largest g + 1; all 12 G pair values with different letters must be present (a line with equal letters is
    read and ignored, like the diagonal)."""
    if isinstance(text, bytes):
        text = text.decode()
    offs, pams, pairs = None, {}, {}
    for no, line in enumerate(text.splitlines(), 1):
        f = line.split("#", 1)[0].split()
        if not f:
            continue
        try:
            if f[0] == "pam-offsets" and offs is None:
                offs = tuple(int(v) for v in f[1:])
            elif f[0] == "pam" and len(f) == 3 and set(f[1].upper()) <= set("ACGT") and f[1].upper() not in pams:
                pams[f[1].upper()] = float(f[2])
            elif f[0] == "pair" and len(f) == 5 and f[2].upper() in "ACGT" and f[3].upper() in "ACGT" and len(f[2]) == len(f[3]) == 1:
                key = (int(f[1]), "ACGT".index(f[2].upper()), "ACGT".index(f[3].upper()))
                if key in pairs or not 0 <= key[0] < MAX_T:
                    raise ValueError("a repeated entry or g outside 0..%d" % (MAX_T - 1))
                pairs[key] = float(f[4])
            else:
                raise ValueError("not a pam-offsets, pam or pair statement (or a repeated one)")
        except ValueError as e:
            raise SearchInputError("pair table, line %d: %s" % (no, e)) from None
    if not pairs:
        raise SearchInputError("pair table: no pair entries")
    G = max(k[0] for k in pairs) + 1
    pair = np.full((G, 4, 4), np.nan)
    for (g, a, b), v in pairs.items():
        pair[g, a, b] = v
    missing = [(g, a, b) for g in range(G) for a in range(4) for b in range(4) if a != b and np.isnan(pair[g, a, b])]
    if missing:
        g, a, b = missing[0]
        raise SearchInputError("pair table: %d of the %d pair entries are missing or not numbers, the first: pair %d %s %s" % (
            len(missing), 12 * G, g, "ACGT"[a], "ACGT"[b]))
    if pams and not offs:
        raise SearchInputError("pair table: pam lines without pam-offsets")
    pam = None
    if offs:
        pam = np.zeros(4 ** len(offs) if len(offs) <= MAX_PAM_OFFSETS else 1)
        for letters, v in pams.items():
            if len(letters) != len(offs):
                raise SearchInputError("pair table: pam %s has %d letters for %d offsets" % (letters, len(letters), len(offs)))
            if pam.size > 1:
                pam[sum("ACGT".index(c) << (2 * (len(offs) - 1 - k)) for k, c in enumerate(letters))] = v
    return PairTable(pair, offs or (), pam)


def pair_values(qcodes, scodes, pam_index, scheme):
    """v under a PairScheme, uint64: the definition in numpy.  qcodes, scodes: (m, G) letters of the query and of the
    oriented site at g = 0 .. G - 1 as codes 0..3 = A, C, G, T; 4 = N in the query (not compared), a non-base in the
    site.  pam_index: (m,) the index of each site's PAM letters into scheme.pam (0 without offsets).  The product runs
    over g ascending, one float64 multiply per step, then the PAM value, like the device's."""
    q = np.asarray(qcodes, dtype=np.int64).reshape(-1, scheme.pair.shape[0])
    s = np.asarray(scodes, dtype=np.int64).reshape(q.shape)
    h = np.ones(q.shape[0], dtype=np.float64)
    n = np.zeros(q.shape[0], dtype=np.int64)
    dead = np.zeros(q.shape[0], dtype=bool)
    for g in range(q.shape[1]):
        mis = (q[:, g] != 4) & (s[:, g] != q[:, g])
        h = np.where(mis, h * scheme.pair[g][np.minimum(q[:, g], 3), np.minimum(s[:, g], 3)], h)
        dead |= mis & (s[:, g] == 4)
        n += mis
    h = h * scheme.pam[np.asarray(pam_index, dtype=np.int64).reshape(-1)]
    v = np.rint(h * float(1 << SCORE_SHIFT)).astype(np.uint64)
    return np.where((n > 0) & ~dead, v, np.uint64(0))


def site_codes(sites, queries, contigs, scheme):
    """(qcodes (m, G), scodes (m, G), pam_index (m,)) of kind-none sites, from the sites' letters: what pair_values takes."""
    gpos = scheme.g_positions()
    T = len(queries[0]) if queries else 0
    qall = [np.array([_QCODE[ord(ch)] for ch in q], dtype=np.uint8) for q in queries]
    qc = np.zeros((len(sites), gpos.size), dtype=np.uint8)
    sc = np.zeros((len(sites), gpos.size), dtype=np.uint8)
    at = np.zeros(len(sites), dtype=np.int64)
    for k, r in enumerate(sites):
        pos, contig = int(r["position"]), contigs[int(r["contig"])]
        codes = _CODE[np.frombuffer(bytes(contig[pos:pos + T]), dtype=np.uint8)]
        if r["strand"] in (b"-", "-"):
            codes = np.where(codes == 4, 4, 3 - codes)[::-1]
        qc[k], sc[k] = qall[int(r["query"])][gpos], codes[gpos]
        for p in scheme.pam_positions:
            if codes[p] == 4:
                raise ValueError("a site without a base at PAM position %d" % p)
            at[k] = at[k] << 2 | int(codes[p])
    return qc, sc, at


def specificity(hit_sum):
    """1 / (1 + hit_sum / 2^30), float64."""
    return 1.0 / (1.0 + np.asarray(hit_sum, dtype=np.uint64).astype(np.float64) / float(1 << SCORE_SHIFT))


def mask_values(masks, scheme):
    """v of mismatch masks (bit g = a mismatch at guide-region position g), uint64: the definition in numpy.  The
    product runs over g ascending, one float64 multiply per step, like the device's."""
    masks = np.asarray(masks, dtype=np.uint64)
    G = scheme.factor.size
    h = np.ones(masks.shape, dtype=np.float64)
    n = np.zeros(masks.shape, dtype=np.int64)
    first = np.full(masks.shape, -1, dtype=np.int64)
    last = np.zeros(masks.shape, dtype=np.int64)
    for g in range(G):
        bit = ((masks >> np.uint64(g)) & np.uint64(1)).astype(bool)
        h = np.where(bit, h * scheme.factor[g], h)
        n += bit
        first = np.where(bit & (first < 0), g, first)
        last = np.where(bit, g, last)
    if (masks >> np.uint64(G)).any() or (n > MAX_MM).any():
        raise ValueError("a mask outside the guide region or with more than %d mismatches" % MAX_MM)
    d = np.where(n > 0, last - first, 0)
    h = h * scheme.shape[n, d]
    v = np.rint(h * float(1 << SCORE_SHIFT)).astype(np.uint64)
    return np.where(n > 0, v, np.uint64(0))


def site_masks(sites, queries, contigs, scheme):
    """Per site its mismatch mask over g, from the site's letters (kind-none sites: SITE_DTYPE, or BULGE_SITE_DTYPE
    rows of kind 0)."""
    gpos = scheme.g_positions()
    T = len(queries[0]) if queries else 0
    qcodes = [np.array([_QCODE[ord(ch)] for ch in q], dtype=np.uint8) for q in queries]
    w = np.uint64(1) << np.arange(gpos.size, dtype=np.uint64)
    out = np.zeros(len(sites), dtype=np.uint64)
    for k, r in enumerate(sites):
        pos, contig = int(r["position"]), contigs[int(r["contig"])]
        codes = _CODE[np.frombuffer(bytes(contig[pos:pos + T]), dtype=np.uint8)]
        if r["strand"] in (b"-", "-"):
            codes = np.where(codes == 4, 4, 3 - codes)[::-1]
        qc = qcodes[int(r["query"])]
        mism = (qc != 4) & (codes != qc)
        out[k] = (mism[gpos].astype(np.uint64) * w).sum(dtype=np.uint64)
    return out


def hit_values(sites, queries, contigs, scheme):
    """v of every fetched site (uint64), from the site's letters by the same integer definition as the device's sums:
    the sum of a query's values is its hit_sum.  Sites of kind none only: a bulge kind's site (BULGE_SITE_DTYPE with
    kind != 0) and a site without mismatches have the value 0."""
    sites = np.asarray(sites)
    v = np.zeros(sites.size, dtype=np.uint64)
    plain = np.ones(sites.size, dtype=bool) if "kind" not in (sites.dtype.names or ()) else sites["kind"] == 0
    idx = np.nonzero(plain)[0]
    if idx.size and isinstance(scheme, PairScheme):
        v[idx] = pair_values(*site_codes(sites[idx], queries, contigs, scheme), scheme)
    elif idx.size:
        v[idx] = mask_values(site_masks(sites[idx], queries, contigs, scheme), scheme)
    return v


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
    def __init__(self, counts, sites, kinds, spans, candidates, hit_sum=None):
        self.hit_sum = hit_sum        # (Q,) uint64 over the sites of kind none (None without score=)
        self.specificity = None if hit_sum is None else specificity(hit_sum)
        self.counts = counts          # (Q, kinds, M + 1) uint32
        self.sites = sites            # BULGE_SITE_DTYPE, ordered by query, kind, contig, position, strand
        self.kinds = kinds            # [(bulge, size)]: kind k of .counts and .sites
        self.spans = spans            # (Q, 2) uint8: each query's span (bulge_at counts from its first letter)
        self.candidates = candidates  # per kind: (n_plus, n_minus) over the whole genome


def search_bulges(genome, pattern, queries, max_mm, pam_len, dna_bulge, rna_bulge, site_cap=None, budget=None, score=None, sites=True):
    """search() plus every site with a DNA bulge of 1..dna_bulge or an RNA bulge of 1..rna_bulge (see the module's
    docstring), over all arenas of `genome`: one library handle per kind and arena, on the kind's window pattern.
    The kind-none slice is what search() returns.  site_cap counts the sites of all kinds together.  score, sites: as
    in search(); .hit_sum and .specificity cover the sites of kind none only (a bulge site has no score)."""
    pattern = check_pattern(pattern)
    max_mm = check_max_mm(max_mm)
    D, R = check_bulges(pattern, pam_len, dna_bulge, rna_bulge)
    queries = [check_query(pattern, q, pam_len) for q in queries]
    spans = query_spans(pattern, pam_len, queries, D, R) if D or R else np.zeros((len(queries), 2), np.uint8)
    kinds = bulge_kinds(D, R)
    scheme = check_score(pattern, pam_len, score, queries)
    if not sites:
        site_cap = 0
    counts, rows, cands, n_total, hit_sum = _search_kinds(genome, pattern, pam_len, queries, max_mm, kinds, spans, site_cap, budget, scheme)
    if sites and site_cap is not None and n_total > int(site_cap):
        raise SiteCapacityError(counts, n_total, int(site_cap))
    return BulgeSearchResult(counts, rows, kinds, spans, cands, hit_sum)


# ---------------------------------------------------------------- self search
MAX_SELF_MM = 4
SELF_SITE_DTYPE = np.dtype([("contig", "<u4"), ("position", "<i8"), ("strand", "S1")])
_IUPAC_SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
               "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}


class SelfCapacityError(RuntimeError):
    """The self search of an arena needs more device memory than the budget: .needed bytes."""

    def __init__(self, needed, budget):
        self.needed, self.budget = int(needed), budget
        super().__init__("the self search needs %d bytes of device memory for one arena: more than the budget%s" % (
            needed, "" if budget is None else " of %d" % budget))


def check_self(pattern, max_mm, pam_len, guide_pattern=None, score=None):
    """The checked input of a self search: (pattern, guide pattern, M, P, Scheme or None).  Refuses a missing PAM
    length, M outside 0..4, a guide pattern that is not the pattern narrowed at PAM positions, and score input that
    check_score refuses."""
    pattern = check_pattern(pattern)
    if pam_len is None:
        raise SearchInputError("the self search needs the PAM's length (--pam-length)")
    lo, hi, _ = guide_region(pattern, pam_len)
    if not isinstance(max_mm, (int, np.integer)) or not 0 <= int(max_mm) <= MAX_SELF_MM:
        raise SearchInputError("mismatches of a self search must be an integer 0..%d, not %r" % (MAX_SELF_MM, max_mm))
    if hi - lo < int(max_mm) + 1:
        raise SearchInputError("a guide region of %d positions is too short for %d mismatches" % (hi - lo, max_mm))
    gp = pattern if guide_pattern is None else check_pattern(guide_pattern)
    if len(gp) != len(pattern):
        raise SearchInputError("guide pattern %s has %d letters, the pattern %d" % (gp, len(gp), len(pattern)))
    if set(gp[lo:hi]) != {"N"}:
        raise SearchInputError("guide pattern %s has letters other than N in the guide region" % gp)
    for p, (g, c) in enumerate(zip(gp, pattern)):
        if not set(_IUPAC_SETS[g]) <= set(_IUPAC_SETS[c]):
            raise SearchInputError("guide pattern %s: %s at position %d accepts bases that %s of the pattern does not" % (gp, g, p, c))
    scheme = check_score(pattern, pam_len, score, [])
    return pattern, gp, int(max_mm), int(pam_len), scheme


class ArenaSelfSearch:
    """One crp_search_self handle: the candidates, guide flags and result rows of one arena."""

    def __init__(self, arena, pattern, guide_pattern, pam_len, max_mm, budget=None):
        self._arena = arena
        self.max_mm = int(max_mm)
        h, need = ctypes.c_void_p(), ctypes.c_uint64()
        st = nat.lib().crp_search_self_create(arena._h, pattern.encode(), guide_pattern.encode(), len(pattern), int(pam_len), self.max_mm,
                                              0 if budget is None else max(1, int(budget)), ctypes.byref(need), ctypes.byref(h))
        self._h = None
        if st == nat.CRP_ERR_CAPACITY:
            raise SelfCapacityError(need.value, budget)
        nat.check(st, "crp_search_self_create", arena._engine._ctx)
        self._h = h
        self.needed = need.value

    def close(self):
        if self._h:
            nat.lib().crp_search_self_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, st, what):
        nat.check(st, what, self._arena._engine._ctx)

    def set_limits(self, pairs_per_launch=0):
        self._check(nat.lib().crp_search_self_set_limits(self._h, int(pairs_per_launch)), "crp_search_self_set_limits")

    def set_scheme(self, scheme):
        if isinstance(scheme, PairScheme):
            pair, G, offs, k, pam = scheme.native_args()
            self._check(nat.lib().crp_search_self_set_pair_scheme(self._h, pair, G, offs, k, pam), "crp_search_self_set_pair_scheme")
            return
        f = np.ascontiguousarray(scheme.factor, dtype=np.float64)
        sh = np.ascontiguousarray(scheme.shape, dtype=np.float64).reshape(-1)
        self._check(nat.lib().crp_search_self_set_scheme(self._h, f.ctypes.data_as(nat.f64p), f.size, sh.ctypes.data_as(nat.f64p)),
                    "crp_search_self_set_scheme")

    def sizes(self):
        a, b, g = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(nat.lib().crp_search_self_sizes(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(g)), "crp_search_self_sizes")
        return a.value, b.value, g.value

    def order(self, segment):
        self._check(nat.lib().crp_search_self_order(self._h, int(segment)), "crp_search_self_order")

    def compare(self, other):
        self._check(nat.lib().crp_search_self_compare(self._h, other._h), "crp_search_self_compare")

    def fetch(self, scored):
        """(arena position u32, strand u8, hi u32, lo u32, counts (n, M + 1) u32, hit_sum u64 or None) of the guide sites."""
        n = self.sizes()[2]
        pos, strand = np.empty(n, np.uint32), np.empty(n, np.uint8)
        hi, lo = np.empty(n, np.uint32), np.empty(n, np.uint32)
        counts = np.empty((n, self.max_mm + 1), np.uint32)
        hs = np.empty(n, np.uint64) if scored else None
        self._check(nat.lib().crp_search_self_fetch(self._h, pos.ctypes.data_as(nat.u32p), strand.ctypes.data_as(nat.u8p),
                                                    hi.ctypes.data_as(nat.u32p), lo.ctypes.data_as(nat.u32p), counts.ctypes.data_as(nat.u32p),
                                                    hs.ctypes.data_as(nat.u64p) if scored else None, n), "crp_search_self_fetch")
        return pos, strand, hi, lo, counts, hs

    def stats(self):
        out = np.zeros(9, dtype=np.float64)
        self._check(nat.lib().crp_search_self_stats(self._h, out.ctypes.data_as(nat.f64p), 9), "crp_search_self_stats")
        keys = ("extract_ms", "order_ms", "compare_ms", "compare_launches", "longest_launch_ms", "pairs", "device_bytes", "order_launches",
                "join_ms")
        return dict(zip(keys, (float(v) for v in out)))

    def set_model(self, model, guide_letters):
        """crp_search_self_set_model: an ontarget.Model for this handle's pattern (guide_letters: its G)."""
        gc = model.gc_table(guide_letters)
        single, pair = np.ascontiguousarray(model.single, np.float64), np.ascontiguousarray(model.pair, np.float64)
        self._check(nat.lib().crp_search_self_set_model(self._h, model.window, model.left, model.intercept, single.ctypes.data_as(nat.f64p),
                                                        pair.ctypes.data_as(nat.f64p) if pair.size else None,
                                                        gc.ctypes.data_as(nat.f64p) if gc is not None else None,
                                                        0 if gc is None else gc.size), "crp_search_self_set_model")

    def run_model(self):
        self._check(nat.lib().crp_search_self_run_model(self._h), "crp_search_self_run_model")

    def fetch_model(self):
        """(n,) float64: the on-target sum of every guide site in fetch()'s order, NaN where a site has none."""
        out = np.empty(self.sizes()[2], np.float64)
        self._check(nat.lib().crp_search_self_fetch_model(self._h, out.ctypes.data_as(nat.f64p), out.size), "crp_search_self_fetch_model")
        return out

    def model_stats(self):
        out = np.zeros(2, dtype=np.float64)
        self._check(nat.lib().crp_search_self_model_stats(self._h, out.ctypes.data_as(nat.f64p), 2), "crp_search_self_model_stats")
        return dict(model_ms=float(out[0]), model_rows=float(out[1]))

    def join_hits(self, guide_len, fetch=True):
        """crp_search_self_join_hits: this handle's rows handed to the hits of its arena's last scan at guide_len (the
        module's docstring, CSV join).  Returns (counts_plus (n_plus, M + 1) uint32, sum_plus (n_plus,) uint64, counts_minus,
        sum_minus) in hit-table order; fetch=False leaves the columns in HBM (join_device) and returns None."""
        L = nat.lib()
        if not fetch:
            self._check(L.crp_search_self_join_hits(self._h, int(guide_len), None, None, None, None), "crp_search_self_join_hits")
            return None
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        nat.check(L.crp_hits_counts(self._arena._h, ctypes.byref(a), ctypes.byref(b)), "crp_hits_counts")
        cols = []
        for n in (a.value, b.value):
            cols += [np.empty((n, self.max_mm + 1), np.uint32), np.empty(n, np.uint64)]
        self._check(L.crp_search_self_join_hits(self._h, int(guide_len), cols[0].ctypes.data_as(nat.u32p), cols[1].ctypes.data_as(nat.u64p),
                                                cols[2].ctypes.data_as(nat.u32p), cols[3].ctypes.data_as(nat.u64p)),
                    "crp_search_self_join_hits")
        return tuple(cols)

    def join_device(self):
        """Device addresses (counts_plus, sum_plus, counts_minus, sum_minus) of the last join_hits."""
        p = [ctypes.c_void_p() for _ in range(4)]
        self._check(nat.lib().crp_search_self_join_device(self._h, *[ctypes.byref(x) for x in p]), "crp_search_self_join_device")
        return tuple(x.value for x in p)

    # ---- gene families (families.py has the definition)
    def set_families(self, rows, cover_mm=0):
        """crp_search_self_set_families: rows is a families.ArenaRows of this handle's arena (None takes families off)."""
        L = nat.lib()
        if rows is None:
            self._check(L.crp_search_self_set_families(self._h, None, None, None, None, 0, 0), "crp_search_self_set_families")
            return
        cols = [np.ascontiguousarray(c, dtype=np.uint32) if len(rows) else np.zeros(1, np.uint32)  # (an arena without family genes)
                for c in (rows.lo, rows.hi, rows.family, rows.member)]
        self._check(L.crp_search_self_set_families(self._h, *[c.ctypes.data_as(nat.u32p) for c in cols], len(rows), int(cover_mm)),
                    "crp_search_self_set_families")

    def family_set_limits(self, pairs_per_launch=0, slice_min=0):
        self._check(nat.lib().crp_search_self_family_set_limits(self._h, int(pairs_per_launch), int(slice_min)),
                    "crp_search_self_family_set_limits")

    def family_assign(self):
        self._check(nat.lib().crp_search_self_family_assign(self._h), "crp_search_self_family_assign")

    def family_compare(self, other):
        self._check(nat.lib().crp_search_self_family_compare(self._h, other._h), "crp_search_self_family_compare")

    def family_fetch(self, scored=True):
        """(owner row u32, family u32, fam_counts (n, M + 1) u32, fam_sum u64 or None, fam_cover u64) of the guide sites, in
        fetch()'s order; 0xFFFFFFFF is no owner / no family."""
        n = self.sizes()[2]
        owner, fam = np.empty(n, np.uint32), np.empty(n, np.uint32)
        counts = np.empty((n, self.max_mm + 1), np.uint32)
        fs = np.empty(n, np.uint64) if scored else None
        cover = np.empty(n, np.uint64)
        self._check(nat.lib().crp_search_self_family_fetch(self._h, owner.ctypes.data_as(nat.u32p), fam.ctypes.data_as(nat.u32p),
                                                           counts.ctypes.data_as(nat.u32p), fs.ctypes.data_as(nat.u64p) if scored else None,
                                                           cover.ctypes.data_as(nat.u64p), n), "crp_search_self_family_fetch")
        return owner, fam, counts, fs, cover

    def family_join_hits(self, guide_len):
        """crp_search_self_family_join_hits: (counts, sum, cover, family) of the '+' table, then of the '-' table."""
        L = nat.lib()
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        nat.check(L.crp_hits_counts(self._arena._h, ctypes.byref(a), ctypes.byref(b)), "crp_hits_counts")
        cols, args = [], []
        for n in (a.value, b.value):
            part = [np.empty((n, self.max_mm + 1), np.uint32), np.empty(n, np.uint64), np.empty(n, np.uint64), np.empty(n, np.uint32)]
            cols += part
            args += [c.ctypes.data_as(t) for c, t in zip(part, (nat.u32p, nat.u64p, nat.u64p, nat.u32p))]
        self._check(L.crp_search_self_family_join_hits(self._h, int(guide_len), *args), "crp_search_self_family_join_hits")
        return tuple(cols)

    def family_stats(self):
        out = np.zeros(6, dtype=np.float64)
        self._check(nat.lib().crp_search_self_family_stats(self._h, out.ctypes.data_as(nat.f64p), 6), "crp_search_self_family_stats")
        keys = ("assign_ms", "family_compare_ms", "family_pairs", "family_compare_launches", "family_bytes", "family_join_ms")
        return dict(zip(keys, (float(v) for v in out)))


class SelfSearchResult:
    site_family = site_gene = fam_counts = fam_sum = fam_cover = None  # with families=: per guide site (families.py)
    selection = None  # with select=: the select_self.Selection
    n_guides = None   # the guide sites of the genome (len(sites), also where sites=False left them on the device)
    on_target_sum = on_target = None  # with on_target=: per guide site, the model's sum (NaN: none) and its value under the link

    def __init__(self, sites, guides, counts, hit_sum, candidates, pairs, stats=None):
        self.sites = sites            # SELF_SITE_DTYPE, ordered by contig, position, strand
        self.guides = guides          # (n,) S<G>: each guide site's G guide-region letters
        self.counts = counts          # (n, M + 1) uint32
        self.hit_sum = hit_sum        # (n,) uint64 (None without score=)
        self.specificity = None if hit_sum is None else specificity(hit_sum)
        self.candidates = candidates  # (n_plus, n_minus) over the whole genome
        self.pairs = pairs            # (compared, brute force = guide sites x candidates)
        self.stats = stats or {}      # the handles' times and launch counts, summed over the arenas


def _guide_letters(hi, lo, lo_pos, G):
    """(n,) S<G> from the windows' code bits over pattern positions lo_pos .. lo_pos + G - 1 (A=00 T=01 C=10 G=11)."""
    out = np.empty((hi.size, G), dtype=np.uint8)
    table = np.frombuffer(b"ATCG", dtype=np.uint8)
    for k in range(G):  # (a column at a time: a real genome has 10^8 rows)
        code = (((hi >> np.uint32(lo_pos + k)) & np.uint32(1)) << np.uint32(1) | ((lo >> np.uint32(lo_pos + k)) & np.uint32(1))).astype(np.uint8)
        out[:, k] = table[code]
    return out.view("S%d" % G).reshape(-1)


def _self_handles(genome, pattern, gp, pam_len, max_mm, scheme, budget, pairs_per_launch, handles):
    """One handle per arena of `genome`, appended to `handles` as they are made (the caller closes them)."""
    for a in genome.arenas:
        h = ArenaSelfSearch(a, pattern, gp, pam_len, max_mm, budget)
        handles.append(h)
        if scheme is not None:
            h.set_scheme(scheme)
        if pairs_per_launch:
            h.set_limits(pairs_per_launch)


def _self_compare_all(handles, max_mm):
    """The whole search over the handles of a genome: segment by segment, every handle's ordering, then the guide sites of
    each arena against the buckets of every arena."""
    for j in range(max_mm + 1):
        for h in handles:
            h.order(j)
        for hq in handles:
            for hc in handles:
                hq.compare(hc)


def _family_compare_all(handles, rows, cover_mm=0, limits=None):
    """The family rows over the handles of a genome (families.py): rows[a] is arena a's families.ArenaRows.  Owners first,
    on every handle; then the guide sites of each arena against the family members of every arena (homeologs sit on
    different chromosomes).  limits: (pairs per launch, smallest slice), lowered by tests."""
    if len(rows) != len(handles):
        raise SearchInputError("%d family layouts for %d arenas" % (len(rows), len(handles)))
    for h, r in zip(handles, rows):
        h.set_families(r, cover_mm)
        if limits:
            h.family_set_limits(*limits)
        h.family_assign()
    for hq in handles:
        for hc in handles:
            hq.family_compare(hc)


def check_family_geometry(pattern, pam_len):
    """The owner of a site is defined by the selection's cut-site rule: a PAM of 3 letters on the 3' side."""
    lo, _, _ = guide_region(pattern, pam_len)
    if int(pam_len) != SPECIFICITY_PAM_LEN or lo != 0:
        raise SearchInputError("gene families need a pattern with a PAM of %d letters on the 3' side" % SPECIFICITY_PAM_LEN)


def search_self(genome, pattern, max_mm, pam_len, guide_pattern=None, score=None, budget=None, pairs_per_launch=None, families=None,
                family_cover_mm=0, family_limits=None, select=None, sites=True, on_target=None):
    """The self search over all arenas of `genome` (engine.Genome): see the module's docstring.  budget: device bytes
    one arena's handle may take (None: the library's default); SelfCapacityError (.needed) beyond it.
    pairs_per_launch: lowers the pairs one compare launch covers (results do not depend on it).
    families: one families.ArenaRows per arena; the result then carries site_family, site_gene (the owner's gene index),
    fam_counts, fam_sum (None without score=) and fam_cover per guide site (families.py has the definition), with
    family_cover_mm as the cover limit C.
    select: a select_self.Request; the K most specific guide sites of every gene of its annotation are then chosen on the
    GPU between the compares and the closing of the handles (select_self.py has the definition), and the result carries
    them as .selection (select_self.Selection).  sites=False (with select=, without families=): the per-site rows are not
    copied to the host -- the result's sites, guides, counts and hit_sum are empty and only .selection, .candidates, .n_guides
    and .pairs are filled.
    on_target: an ontarget.Model of the pattern's geometry; its sum is then evaluated on the GPU for every guide site of every
    arena (ontarget.py has the definition) and the result carries on_target_sum (float64, NaN where a site has none) and
    on_target (the value under the model's link) in the result's site order; a selection may rank and bound by it
    (select_self.Params: rank, min_on_target)."""
    pattern, gp, max_mm, pam_len, scheme = check_self(pattern, max_mm, pam_len, guide_pattern, score)
    lo, hi, pam3 = guide_region(pattern, pam_len)
    if on_target is not None:
        try:
            on_target.check_geometry(len(pattern), pam_len, pam3)
        except ValueError as e:
            raise SearchInputError(str(e))
    if select is not None:
        try:
            select.params.bind_model(on_target)
        except ValueError as e:
            raise SearchInputError(str(e))
    if not sites and (select is None or families is not None):
        raise SearchInputError("sites=False keeps only the selection: it needs select= and goes without families=")
    if select is not None:
        if select.params.needs_score and scheme is None:
            raise SearchInputError("a specificity threshold needs a scored search (score=)")
        try:
            select.params.resolve(len(pattern), pam_len, pam3)
        except ValueError as e:
            raise SearchInputError(str(e))
    if families is not None:
        check_family_geometry(pattern, pam_len)
        if not isinstance(family_cover_mm, (int, np.integer)) or not 0 <= int(family_cover_mm) <= max_mm:
            raise SearchInputError("the family cover limit must be an integer 0..%d (the search's mismatches), not %r" % (max_mm, family_cover_mm))
    handles = []
    try:
        _self_handles(genome, pattern, gp, pam_len, max_mm, scheme, budget, pairs_per_launch, handles)
        _self_compare_all(handles, max_mm)
        if on_target is not None:
            for h in handles:
                h.set_model(on_target, hi - lo)
                h.run_model()
        fam_parts = []
        if families is not None:
            _family_compare_all(handles, families, int(family_cover_mm), family_limits)
            for h, r in zip(handles, families):
                owner, fam, fc, fs, cover = h.family_fetch(scheme is not None)
                gene = np.full(owner.size, 0xFFFFFFFF, np.uint32)
                has = owner != np.uint32(0xFFFFFFFF)
                gene[has] = np.asarray(r.gene, np.uint32)[owner[has]]
                fam_parts.append((fam, gene, fc, fs, cover))
        selection = None
        if select is not None:
            from . import select_self
            flags = select.annotation.annotation.cds_flags() if select.params.require_cds else None
            sel_parts, sel_stats = [], {}
            for k, (h, a, group) in enumerate(zip(handles, genome.arenas, genome.groups)):
                gene, got, st = select_self.select_arena(genome, k, select, h, flags)
                sel_parts.append(dict(got, offsets=a.offsets, lengths=a.lengths, group=group, gene=gene))
                for key, v in st.items():
                    sel_stats[key] = sel_stats.get(key, 0.0) + v
            selection = select_self.assemble(select.annotation.annotation.genes()[0], select.params.k, len(pattern),
                                             select.params.cut_offset, lo, hi - lo, scheme is not None, sel_parts,
                                             rank=select.params.rank, link=None if on_target is None else on_target.link)
            selection.stats = sel_stats
        parts, guides, counts, sums, model_sums = [], [], [], [], []
        cand, n_guides, stats = [0, 0], 0, {}
        for h, a, group in zip(handles, genome.arenas, genome.groups):
            npl, nmi, ng = h.sizes()
            cand[0] += npl
            cand[1] += nmi
            n_guides += ng
            for key, v in h.stats().items():
                stats[key] = max(stats.get(key, 0.0), v) if key == "longest_launch_ms" else stats.get(key, 0.0) + v
            if on_target is not None:
                for key, v in h.model_stats().items():
                    stats[key] = stats.get(key, 0.0) + v
            if not sites:
                continue
            if on_target is not None:
                model_sums.append(h.fetch_model())
            pos, strand, fh, fl, c, hs = h.fetch(scheme is not None)
            offs = np.asarray(a.offsets, dtype=np.int64)
            k = np.searchsorted(offs, pos.astype(np.int64), "right") - 1
            part = np.empty(ng, SELF_SITE_DTYPE)
            part["contig"] = np.asarray(group, dtype=np.uint32)[k] if ng else 0
            part["position"] = pos.astype(np.int64) - offs[k]
            part["strand"] = np.where(strand == 0, b"+", b"-")
            parts.append(part)
            guides.append(_guide_letters(fh, fl, lo, hi - lo))
            counts.append(c)
            if hs is not None:
                sums.append(hs)
            if families is not None:
                for key, v in h.family_stats().items():
                    stats[key] = stats.get(key, 0.0) + v
    finally:
        for h in handles:
            h.close()
    if not parts:  # (sites=False, or a genome without arenas)
        parts, guides = [np.empty(0, SELF_SITE_DTYPE)], [np.empty(0, "S%d" % (hi - lo))]
        counts, sums = [np.empty((0, max_mm + 1), np.uint32)], [np.empty(0, np.uint64)]
    sites = np.concatenate(parts)
    order = np.lexsort((sites["strand"] == b"-", sites["position"], sites["contig"]))
    res = SelfSearchResult(sites[order], np.concatenate(guides)[order], np.concatenate(counts)[order],
                           np.concatenate(sums)[order] if scheme is not None else None, tuple(cand),
                           (int(stats.get("pairs", 0)), n_guides * (cand[0] + cand[1])), stats)
    res.selection, res.n_guides = selection, n_guides
    if on_target is not None:
        from . import ontarget
        res.on_target_sum = np.concatenate(model_sums)[order] if model_sums else np.empty(0, np.float64)
        res.on_target = ontarget.value(res.on_target_sum, on_target.link)
    if families is not None:
        res.site_family, res.site_gene, res.fam_counts, res.fam_cover = (np.concatenate([p[k] for p in fam_parts])[order] for k in (0, 1, 2, 4))
        res.fam_sum = np.concatenate([p[3] for p in fam_parts])[order] if scheme is not None else None
    return res


SPECIFICITY_PAM_LEN = 3  # the scan's PAM: .GG / CC.


def check_specificity(guide_len, max_mm=3, candidate_pam="NRG", score="hsu2013"):
    """The checked input of the CSV join for a scan at guide_len: (candidate pattern, guide pattern, M, Scheme or None).
    The guide pattern is N * l + NGG, the candidate pattern N * l + candidate_pam (3 letters that accept what NGG accepts);
    refuses l + 3 > 32, l < M + 1, M outside 0..4, hsu2013 with l != 20 and whatever else check_self refuses."""
    if not isinstance(guide_len, (int, np.integer)) or int(guide_len) < 1:
        raise SearchInputError("the specificity join needs a guide length of at least 1, not %r" % (guide_len,))
    l = int(guide_len)
    if l + SPECIFICITY_PAM_LEN > MAX_T:
        raise SearchInputError("the specificity join compares guide and PAM as one pattern of at most %d letters: guide length %d is "
                               "more than %d" % (MAX_T, l, MAX_T - SPECIFICITY_PAM_LEN))
    pam = candidate_pam.decode() if isinstance(candidate_pam, bytes) else str(candidate_pam)
    if len(pam) != SPECIFICITY_PAM_LEN:
        raise SearchInputError("the candidate PAM must have %d letters, not %r" % (SPECIFICITY_PAM_LEN, candidate_pam))
    pattern, gp, M, _, scheme = check_self("N" * l + pam, max_mm, SPECIFICITY_PAM_LEN, "N" * l + "NGG", score)
    return pattern, gp, M, scheme


def specificity_columns(genome, guide_len, max_mm=3, candidate_pam="NRG", score="hsu2013", budget=None, after_join=None, families=None,
                        family_cover_mm=0, family_limits=None):
    """The genome-wide specificity of every hit of a scanned `genome` (engine.Genome whose arenas hold the tables of a scan
    at guide_len): the self search of N * l + NGG guides among N * l + candidate_pam candidates over all arenas, then each
    arena's tables joined against its own handle on the GPU (the module's docstring, CSV join).  Returns one dict per
    contig, in contig order: self_counts_plus / self_counts_minus (n, M + 1) uint32 and self_sum_plus / self_sum_minus (n,)
    uint64, rows as Hits.contig(k) has them.  score=None: counts only (the sums are all-ones).  The dicts' list carries
    .stats, the handles' times summed over the arenas (join_ms among them).  after_join(arena index, handle, (counts_plus,
    sum_plus, counts_minus, sum_minus)) is called for every arena while its joined columns are still in HBM on the handle
    (the guide selection reads them there: they die when the handles close).
    families: one families.ArenaRows per arena (families.py has the definition); the family rows are computed after the
    self search and joined like the plain rows: the dicts also carry fam_counts_plus / _minus (n, M + 1) uint32, fam_sum_plus
    / _minus, fam_cover_plus / _minus (n,) uint64 and site_family_plus / _minus (n,) uint32 (0xFFFFFFFF: none), and after_join
    gets them as a fifth argument, (counts, sum, cover, family) of '+' and then of '-'.  An unscored handle's fam_sum is 0."""
    pattern, gp, M, scheme = check_specificity(guide_len, max_mm, candidate_pam, score)
    if families is not None and (not isinstance(family_cover_mm, (int, np.integer)) or not 0 <= int(family_cover_mm) <= M):
        raise SearchInputError("the family cover limit must be an integer 0..%d (the join's mismatches), not %r" % (M, family_cover_mm))
    out = [None] * genome.n_contigs
    handles, stats = [], {}
    try:
        _self_handles(genome, pattern, gp, SPECIFICITY_PAM_LEN, M, scheme, budget, None, handles)
        _self_compare_all(handles, M)
        if families is not None:
            _family_compare_all(handles, families, int(family_cover_mm), family_limits)
        for index, (h, a, group) in enumerate(zip(handles, genome.arenas, genome.groups)):
            cp, sp, cm, sm = h.join_hits(guide_len)
            fam = h.family_join_hits(guide_len) if families is not None else None
            if after_join is not None:
                if fam is None:
                    after_join(index, h, (cp, sp, cm, sm))
                else:
                    after_join(index, h, (cp, sp, cm, sm), fam)
            pos_plus, pos_minus = np.empty(len(sp), np.uint32), np.empty(len(sm), np.uint32)
            nat.check(nat.lib().crp_fetch_hits(a._h, pos_plus.ctypes.data_as(nat.u32p), None, None, pos_minus.ctypes.data_as(nat.u32p), None,
                                               None), "crp_fetch_hits", a._engine._ctx)
            ends = (np.asarray(a.offsets) + np.asarray(a.lengths)).astype(np.uint32)
            starts = np.asarray(a.offsets).astype(np.uint32)
            for j, k in enumerate(group):  # (the tables ascend in arena position: a contig's rows are one slice)
                p0, p1 = np.searchsorted(pos_plus, [starts[j], ends[j]], "left")
                m0, m1 = np.searchsorted(pos_minus, [starts[j], ends[j]], "left")
                out[k] = dict(self_counts_plus=cp[p0:p1], self_sum_plus=sp[p0:p1], self_counts_minus=cm[m0:m1], self_sum_minus=sm[m0:m1])
                if fam is not None:
                    for name, plus, minus in zip(("fam_counts", "fam_sum", "fam_cover", "site_family"), fam[:4], fam[4:]):
                        out[k][name + "_plus"], out[k][name + "_minus"] = plus[p0:p1], minus[m0:m1]
            for key, v in h.stats().items():
                stats[key] = max(stats.get(key, 0.0), v) if key == "longest_launch_ms" else stats.get(key, 0.0) + v
            if families is not None:
                for key, v in h.family_stats().items():
                    stats[key] = stats.get(key, 0.0) + v
    finally:
        for h in handles:
            h.close()
    out = _Columns(out)
    out.stats = stats
    return out


class _Columns(list):
    """specificity_columns' result: the per-contig dicts, with .stats."""


def format_self(contig_names, res, block=1 << 16):
    """The TSV of a self search, as an iterator of text blocks: contig, position, strand, guide, n0 .. nM and, when
    scored, hit_sum (as a sum of hit scores, hit_sum / 2^30) and specificity.  The columns are formatted with numpy, a
    block of rows at a time.  With an on-target model every row ends with on_target: repr of the value, empty for a site
    without a sum."""
    M1 = res.counts.shape[1]
    head = ["contig", "position", "strand", "guide"] + ["n%d" % k for k in range(M1)]
    model = getattr(res, "on_target", None) is not None
    yield "\t".join(head + ([] if res.hit_sum is None else ["hit_sum", "specificity"]) + (["on_target"] if model else [])) + "\n"
    names = np.array(list(contig_names) or [""], dtype=object)
    for i0 in range(0, len(res.sites), block):
        s = res.sites[i0:i0 + block]
        cols = [names[s["contig"]].astype(str), s["position"].astype(str), s["strand"].astype(str), res.guides[i0:i0 + block].astype(str)]
        cols += [res.counts[i0:i0 + block, k].astype(str) for k in range(M1)]
        if res.hit_sum is not None:
            hs = res.hit_sum[i0:i0 + block].astype(np.float64) / float(1 << SCORE_SHIFT)
            cols += [np.char.mod("%.6f", hs), np.char.mod("%.6f", res.specificity[i0:i0 + block])]
        if model:
            cols.append(np.array(["" if v != v else repr(v) for v in res.on_target[i0:i0 + block].tolist()], dtype=str))
        line = cols[0]
        for c in cols[1:]:
            line = np.char.add(np.char.add(line, "\t"), c)
        yield "\n".join(line.tolist()) + "\n"


# ---------------------------------------------------------------- TSV
_CODE = np.full(256, 4, dtype=np.uint8)  # 0..3 = A C G T, 4 = not a base
for _c, _v in zip(b"ACGTUacgt", (0, 1, 2, 3, 0, 0, 1, 2, 3)):
    _CODE[_c] = _v
_QCODE = np.full(256, 4, dtype=np.uint8)  # a query's letters: N (not compared) = 4
for _c, _v in zip(b"ACGT", (0, 1, 2, 3)):
    _QCODE[_c] = _v


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


def format_scored_sites(names, queries, contig_names, contigs, res, scheme):
    """The sites TSV of a scored search (SearchResult or BulgeSearchResult): the unscored columns plus hit_score."""
    kinds, spans = getattr(res, "kinds", None), getattr(res, "spans", None)
    if kinds is not None and len(kinds) == 1:
        kinds = None
    return _format_site_rows(names, queries, contig_names, contigs, res.sites, kinds, spans,
                             hit_values(res.sites, queries, contigs, scheme))


def format_scored_counts(names, queries, res):
    """The counts TSV of a scored search: the unscored columns plus hit_sum and specificity."""
    kinds = getattr(res, "kinds", None)
    if kinds is None or len(kinds) == 1:
        return _format_count_rows(names, queries, res.counts.reshape(len(queries), 1, -1), None, res.hit_sum)
    return _format_count_rows(names, queries, res.counts, kinds, res.hit_sum)


def _format_site_rows(names, queries, contig_names, contigs, sites, kinds, spans, values=None):
    """The sites TSV; with the kinds and spans of a bulge search, the bulge columns and the aligned query too; with the
    sites' hit values, a last column hit_score = v / 2^30 (empty for a bulge kind's site and for a site without
    mismatches: neither is summed)."""
    head = ["name", "query", "contig", "position", "strand", "mismatches"]
    head += ["bulge", "bulge_size", "bulge_at", "site", "query_aligned"] if kinds else ["site"]
    lines = ["\t".join(head + ([] if values is None else ["hit_score"])) + "\n"]
    for i, r in enumerate(sites):
        q, k, pos, strand = int(r["query"]), int(r["contig"]), int(r["position"]), r["strand"]
        row = [names[q], queries[q], contig_names[k], pos, strand.decode(), int(r["mismatches"])]
        if kinds:
            (bulge, size), at = kinds[int(r["kind"])], int(r["bulge_at"])
            site, qa = bulge_alignment(contigs[k], pos, strand, queries[q], bulge, size, int(spans[q, 0]) + at)
            row += [bulge, size, at, site, qa]
        else:
            row.append(site_string(contigs[k], pos, strand, queries[q]))
        if values is not None:
            scored = int(r["mismatches"]) > 0 and not (kinds and kinds[int(r["kind"])][1])
            row.append("%.6f" % (int(values[i]) / float(1 << SCORE_SHIFT)) if scored else "")
        lines.append("\t".join(map(str, row)) + "\n")
    return "".join(lines)


def format_bulge_counts(names, queries, kinds, counts):
    return _format_count_rows(names, queries, counts, kinds)


def format_counts(names, queries, counts):
    return _format_count_rows(names, queries, counts[:, None], None)


def _format_count_rows(names, queries, counts, kinds, hit_sum=None):
    """The counts TSV of counts (Q, kinds, M + 1): one line per query and kind; with the kinds of a bulge search, the
    bulge and bulge_size columns too; with hit_sum, the columns hit_sum (as a sum of hit scores, hit_sum / 2^30) and
    specificity, filled on the kind-none line only."""
    head = ["name", "query"] + (["bulge", "bulge_size"] if kinds else []) + ["mm%d" % k for k in range(counts.shape[2])]
    lines = ["\t".join(head + ([] if hit_sum is None else ["hit_sum", "specificity"])) + "\n"]
    spec = None if hit_sum is None else specificity(hit_sum)
    for q in range(len(queries)):
        for k, kind in enumerate(kinds or [()]):
            row = [names[q], queries[q], *kind, *counts[q, k].tolist()]
            if hit_sum is not None:
                row += ["%.6f" % (int(hit_sum[q]) / float(1 << SCORE_SHIFT)), "%.6f" % spec[q]] if k == 0 else ["", ""]
            lines.append("\t".join(map(str, row)) + "\n")
    return "".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cropsr_amd.search",
                                 description="Every genome site within M mismatches of each given guide, on both strands "
                                             "(MI355X; DESIGN.md section 15).")
    ap.add_argument("-f", "--fasta", required=True, help="genome FASTA")
    ap.add_argument("--pattern", required=True, help="PAM pattern over ACGTRYSWKMBDHVN, e.g. NNNNNNNNNNNNNNNNNNNNNRG")
    ap.add_argument("--guides", help="one guide per line: SEQUENCE [NAME]; '#' starts a comment (required without --self)")
    ap.add_argument("--self", dest="self_search", action="store_true",
                    help="the self search: every guide site of the genome is a query; -o gets one line per guide site (contig, "
                         "position, strand, guide, n0..nM and, when scored, hit_sum and specificity); needs --pam-length, -m 0..4; "
                         "not with --guides, --dna-bulge, --rna-bulge, --no-sites or --counts")
    ap.add_argument("--guide-pattern", help="with --self: the pattern of the guide sites (default: --pattern), e.g. ...NGG guides "
                                            "against ...NRG candidates")
    ap.add_argument("--pam-length", type=int, default=None, metavar="P",
                    help="the PAM is the pattern's last (or, for a 5' PAM, first) P letters: guides shorter than the pattern "
                         "sit right next to it (3 for ...NGG, 6 for ...NNGRRT, 4 for TTTV...); without it a shorter guide "
                         "must be exactly as long as the pattern's N run")
    ap.add_argument("-m", "--mismatches", type=int, default=4, help="most mismatches reported (0..8, default 4)")
    ap.add_argument("-o", "--output", help="sites TSV (required without --no-sites)")
    ap.add_argument("--dna-bulge", type=int, default=0, metavar="D",
                    help="also report sites with a DNA bulge (extra genomic bases) of 1..D (0..2, default 0); needs "
                         "--pam-length; adds the columns bulge, bulge_size, bulge_at, query_aligned")
    ap.add_argument("--rna-bulge", type=int, default=0, metavar="R",
                    help="also report sites with an RNA bulge (unpaired guide letters) of 1..R (0..2, default 0); needs "
                         "--pam-length")
    ap.add_argument("--counts", help="per-guide counts TSV (mm0..mmM; with bulges one line per guide and kind)")
    sc = ap.add_mutually_exclusive_group()
    sc.add_argument("--score", choices=["hsu2013"],
                    help="per-guide specificity 1 / (1 + sum of hit scores), summed on the GPU over the sites with 1..M mismatches "
                         "(hsu2013: the MIT score's weights, 20-nt guide regions); needs --pam-length; adds the column hit_score "
                         "to the sites TSV, hit_sum and specificity to --counts")
    sc.add_argument("--weights", metavar="FILE",
                    help="the same with the weights of FILE in place of hsu2013's: one number in [0, 1] per guide-region "
                         "position, PAM-distal first")
    sc.add_argument("--score-table", metavar="FILE",
                    help="the same with a hit score of the CFD form: the pair table of FILE (pair values per position, query "
                         "letter and site letter; values per PAM letters; see parse_pair_table, tools/cfd_to_table.py)")
    ap.add_argument("--no-sites", action="store_true", help="keep and write no site list: only --counts (with the scores, if asked for)")
    ap.add_argument("--device", type=int, default=0, help="HIP device")
    sg = ap.add_argument_group("guide selection for any nuclease (with --self; DESIGN.md section 28)")
    sg.add_argument("-g", "--gff", metavar="FILE", help="with --select: the GFF3 whose `gene` rows are selected for")
    sg.add_argument("--select", type=int, default=None, metavar="K",
                    help="with --self and -g: also choose, on the GPU, the K (1..64) most specific guide sites of every gene -- "
                         "ranked by hit_sum when scored, by the mismatch counts otherwise -- and write them to --select-output")
    sg.add_argument("--select-output", metavar="FILE", help="the selection TSV (default: the -o name + .selected.tsv)")
    sg.add_argument("--cut-offset", type=int, default=None, metavar="C",
                    help="with --select: the cut lies before pattern position C (1..T-1) of the oriented site; default G-3 with "
                         "the PAM on the 3' side, P+min(18, G-1) with the PAM on the 5' side")
    sg.add_argument("--select-max-perfect", type=int, default=None, metavar="N", help="with --select: only sites with at most N other perfect copies (n0)")
    sg.add_argument("--select-min-specificity", type=float, default=None, metavar="S",
                    help="with --select: only sites of specificity at least S (needs --score, --weights or --score-table)")
    sg.add_argument("--select-cds", action="store_true", help="with --select: only sites whose cut letter lies in a CDS of the GFF")
    sg.add_argument("--select-gc-min", type=int, default=None, metavar="PCT",
                    help="with --select: only guides with at least PCT %% GC (an integer 0..100; as a count: ceil(PCT * G / 100))")
    sg.add_argument("--select-gc-max", type=int, default=None, metavar="PCT",
                    help="with --select: only guides with at most PCT %% GC (an integer 0..100; as a count: floor(PCT * G / 100))")
    sg.add_argument("--select-max-t-run", type=int, default=None, metavar="N", help="with --select: only guides whose longest run of T is at most N")
    sg.add_argument("--select-only", action="store_true", help="with --select: write only the selection, no sites TSV (-o is then not required)")
    og = ap.add_argument_group("on-target model for any nuclease (with --self; DESIGN.md section 30)")
    og.add_argument("--on-target", metavar="FILE|rs1",
                    help="with --self: evaluate, on the GPU, the position-specific linear model of FILE (window, left, link, intercept, "
                         "single, pair, gc statements; cropsr_amd/ontarget.py) for every guide site, or the built-in rs1 (the scan's own "
                         "model, N20 NGG only); both TSVs then end every row with on_target")
    og.add_argument("--select-rank", choices=["specificity", "on-target"], default=None,
                    help="with --select: the order inside a gene (default specificity; on-target needs --on-target: larger model sum first)")
    og.add_argument("--select-min-on-target", type=float, default=None, metavar="X",
                    help="with --select and --on-target: only sites whose on_target is at least X (in (0, 1) under a logistic link)")
    args = ap.parse_args(argv)
    if args.on_target is not None and not args.self_search:
        ap.error("--on-target belongs to --self")
    if args.select is None:
        for opt, given in _select_options(args):
            if given:
                ap.error("%s belongs to --select" % opt)
    elif not args.self_search:
        ap.error("--select belongs to --self (the scan's selection is python -m cropsr_amd --select)")
    if args.self_search:
        return _main_self(ap, args)
    if not args.guides:
        ap.error("the following arguments are required: --guides (or --self)")
    if args.guide_pattern:
        ap.error("--guide-pattern belongs to --self")
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
        score = args.score
        if args.weights:
            with open(args.weights, "rb") as f:
                score = parse_weights(f.read())
        if args.score_table:
            with open(args.score_table, "rb") as f:
                score = parse_pair_table(f.read())
        scheme = check_score(pattern, args.pam_length, score, queries)
        if args.no_sites and (args.output or not args.counts):
            raise SearchInputError("--no-sites writes only --counts: give --counts and no -o")
        if not args.no_sites and not args.output:
            raise SearchInputError("-o/--output is required (or --no-sites with --counts)")
        contig_names, contigs = read_fasta(args.fasta)
    except (SearchInputError, OSError, UnicodeDecodeError) as e:
        ap.error(str(e))
    from .engine import Engine
    with Engine(args.device) as eng:
        g = eng.genome(contigs)
        try:
            res = search_bulges(g, pattern, queries, max_mm, args.pam_length, D, R, score=score, sites=not args.no_sites)
        finally:
            g.close()
    kinds = res.kinds if D or R else None  # (None: the plain TSV columns)
    if not args.no_sites:
        values = None if scheme is None else hit_values(res.sites, queries, contigs, scheme)
        with open(args.output, "w") as f:
            f.write(_format_site_rows(names, queries, contig_names, contigs, res.sites, kinds, res.spans, values))
    if args.counts:
        with open(args.counts, "w") as f:
            f.write(_format_count_rows(names, queries, res.counts, kinds, res.hit_sum))
    if D or R:
        print("%d guides, %d kinds, %d sites within %d mismatches" % (len(queries), len(res.kinds), int(res.counts.sum()), max_mm),
              file=sys.stderr)
    else:
        print("%d guides, %d + %d candidate sites, %d sites within %d mismatches" % (
            len(queries), res.candidates[0][0], res.candidates[0][1], int(res.counts.sum()), max_mm), file=sys.stderr)
    return 0


def _select_options(args):
    """[(option, whether it was given)] of the options that belong to --select."""
    return [("-g/--gff", args.gff is not None), ("--select-output", args.select_output is not None), ("--cut-offset", args.cut_offset is not None),
            ("--select-max-perfect", args.select_max_perfect is not None), ("--select-min-specificity", args.select_min_specificity is not None),
            ("--select-cds", args.select_cds), ("--select-gc-min", args.select_gc_min is not None),
            ("--select-gc-max", args.select_gc_max is not None), ("--select-max-t-run", args.select_max_t_run is not None),
            ("--select-only", args.select_only), ("--select-rank", args.select_rank is not None),
            ("--select-min-on-target", args.select_min_on_target is not None)]


def _self_select_params(args, pattern, pam_len, scored, model=None):
    """The select_self.Params of --select and its options, checked against the pattern and the --on-target model;
    SearchInputError otherwise."""
    from . import select_self
    if not args.gff:
        raise SearchInputError("--select needs -g/--gff: the genes to select for")
    if model is None:
        if args.select_rank == "on-target":
            raise SearchInputError("--select-rank on-target needs --on-target: the model to rank by")
        if args.select_min_on_target is not None:
            raise SearchInputError("--select-min-on-target needs --on-target: the model to bound")
    if not 1 <= args.select <= select_self.MAX_K:
        raise SearchInputError("--select K must be 1..%d, not %d" % (select_self.MAX_K, args.select))
    if args.select_min_specificity is not None and not scored:
        raise SearchInputError("--select-min-specificity needs a scored search (--score, --weights or --score-table)")
    lo, hi, pam3 = guide_region(pattern, pam_len)
    for name, v in (("--select-gc-min", args.select_gc_min), ("--select-gc-max", args.select_gc_max)):
        if v is not None and not 0 <= v <= 100:
            raise SearchInputError("%s is a percentage 0..100, not %d" % (name, v))
    for name, v in (("--select-max-perfect", args.select_max_perfect), ("--select-max-t-run", args.select_max_t_run)):
        if v is not None and v < 0:
            raise SearchInputError("%s is a count, not %d" % (name, v))
    gc_min, gc_max = select_self.gc_bounds(args.select_gc_min, args.select_gc_max, hi - lo)
    try:
        params = select_self.Params(args.select, args.cut_offset, args.select_max_perfect, args.select_min_specificity, args.select_cds,
                                    gc_min, gc_max, args.select_max_t_run, rank=args.select_rank or "specificity",
                                    min_on_target=args.select_min_on_target)
        return params.bind_model(model).resolve(len(pattern), pam_len, pam3)
    except ValueError as e:
        raise SearchInputError("--select: %s" % e)


def _main_self(ap, args):
    """--self: checks, then search_self and the TSV."""
    try:
        for opt, given in (("--guides", args.guides), ("--dna-bulge", args.dna_bulge), ("--rna-bulge", args.rna_bulge),
                           ("--no-sites", args.no_sites), ("--counts", args.counts)):
            if given:
                raise SearchInputError("--self does not go with %s" % opt)
        if not args.output and not (args.select is not None and args.select_only and args.select_output):
            raise SearchInputError("--self needs -o/--output" + (" (or --select-only with --select-output)" if args.select is not None else ""))
        score = args.score
        if args.weights:
            with open(args.weights, "rb") as f:
                score = parse_weights(f.read())
        if args.score_table:
            with open(args.score_table, "rb") as f:
                score = parse_pair_table(f.read())
        pattern, gp, max_mm, pam_len, scheme = check_self(args.pattern, args.mismatches, args.pam_length, args.guide_pattern, score)
        model = None
        if args.on_target is not None:
            from . import ontarget
            lo, hi, pam3 = guide_region(pattern, pam_len)
            try:
                model = ontarget.load(args.on_target, hi - lo)
                model.check_geometry(len(pattern), pam_len, pam3)
            except ValueError as e:
                raise SearchInputError("--on-target %s: %s" % (args.on_target, e))
        params = None if args.select is None else _self_select_params(args, pattern, pam_len, scheme is not None, model)
        if params is not None:
            with open(args.gff, "rb"):  # (unreadable: refused here, before the GPU is opened)
                pass
        contig_names, contigs = read_fasta(args.fasta)
    except (SearchInputError, OSError, UnicodeDecodeError) as e:
        ap.error(str(e))
    from .engine import Engine
    request = annotation = None
    if params is not None:
        from . import annotate, select_self
        annotation = annotate.Annotation(args.gff)
        request = select_self.Request(params, annotate.Request(annotation, contig_names, 0))
    try:
        with Engine(args.device) as eng:
            g = eng.genome(contigs)
            try:
                res = search_self(g, pattern, max_mm, pam_len, guide_pattern=gp, score=score, select=request,
                                  sites=not (params is not None and args.select_only), on_target=model)
            finally:
                g.close()
    finally:
        if annotation is not None:
            annotation.close()
    if not (params is not None and args.select_only):
        with open(args.output, "w") as f:
            for text in format_self(contig_names, res):
                f.write(text)
    print("%d guide sites, %d + %d candidate sites, %d of %d pairs compared" % (
        res.n_guides, res.candidates[0], res.candidates[1], res.pairs[0], res.pairs[1]), file=sys.stderr)
    if params is not None:
        from . import select_self
        sel = res.selection
        with open(args.select_output or args.output + ".selected.tsv", "w") as f:
            f.write(select_self.format_selection(contig_names, sel))
        print("%d genes, %d guide sites inside them, %d passing, %d selected" % (
            len(sel.labels), int(sel.n_in.sum()), int(sel.n_pass.sum()), len(sel.rows)), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
