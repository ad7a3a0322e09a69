"""--variants: how many variants of a cultivar lie under every guide's target site.

Not in the reference, opt-in.  The guides are scanned from a reference assembly; the plant that is transformed is almost never
that accession, and a SNP in the PAM-proximal seed or a lost GG means the guide does not cut.  A VCF of the cultivar against the
assembly gives, per kept hit, four counts that the selection can bound (select.Request(max_variants=...)).

Definition (include/cropsr_hip.h states the same; tests/variant_reference.py restates it twice).

  variant    for every VCF record and each kept ALT allele: strip the common prefix of REF and ALT (letters compared without
  intervals  case), then the common suffix of what is left -> REF', ALT' and p, the 1-based coordinate of the first letter after
             the stripped prefix.  The allele is the closed interval [s, e] of contig coordinates, s = p, e = p + len(REF') - 1.
             A pure insertion (REF' empty) is [p, p - 1]: an empty interval at the junction between p - 1 and p.  An allele with
             REF' and ALT' both empty is dropped.  Always e >= s - 1.
  arena      the mapping is the annotation track's: entries (FASTA name, first, length, offset) of the arena's texts and dec.  A
  layout     coordinate c of a contig whose FASTA name equals CHROM exactly has string index c + dec - 1; inside a text it has
             arena position index - first + offset.  An interval is clipped to the text: s' = max(s, first), e' = min(e, first
             + length - 1), kept when e' >= s' - 1.  Equal (s', e') pairs of one arena count once: a multi-allelic SNP is one
             variant.  The track is two uint32 arrays of one length, each sorted ascending ON ITS OWN: starts holds every s',
             ends1 every e' + 1; all values are below 2^31.
  windows    of a hit after a scan at guide length l = 1..50 with seed length S, 1 <= S <= l (default min(12, l)): closed ranges
             of arena positions in the forward text, pos being the match index i ('+' row, .GG at i) or j ('-' row, CC. at j)

                             '+' row             '-' row
               site          [i - l, i + 2]      [j, j + 2 + l]          guide + PAM
               guide         [i - l, i - 1]      [j + 3, j + 2 + l]
               seed          [i - S, i - 1]      [j + 3, j + 2 + S]      the PAM-proximal S letters
               pam           [i + 1, i + 2]      [j, j + 1]              the two fixed letters

  touch      a variant [s, e] touches a window [a, b] when s <= b and e >= a.  An insertion touches it exactly when both
             letters around its junction lie inside: one between guide and PAM counts for `site` only.
  count      #(starts <= b) - #(ends1 <= a), exact because e >= s - 1.  Every row has a value -- unscored rows and '-' rows
             whose window runs past the contig's end too: the void between texts carries no variant.  A substitution at the
             PAM's N counts in `site` only.
  packing    one uint32 per row: site | guide << 8 | seed << 16 | pam << 24, each SATURATING at 255.

The VCF reader is native (csrc/crp_variants.cpp): text VCF, `#` lines skipped except #CHROM (the sample names), tab-separated
columns, POS a plain digit string >= 1, REF / ALT letters of ACGTNacgtn; an ALT of `.`, `*`, a symbolic <...> or a breakend is
skipped and counted; a malformed line is a ValueError naming the line.  pass_only: FILTER must be PASS or `.`.  samples: ALT
allele k is kept only when the GT of at least one named sample holds k.  Allele-frequency filters and symbolic structural
variants (END=) are out of scope.
"""
import ctypes
import gzip

import numpy as np

from . import _native as nat

HEADER = ["var_site", "var_guide", "var_seed", "var_pam"]
MAX_GUIDE = 50
DEFAULT_SEED = 12
SATURATED = 255
STATS = ("lines", "records", "filtered", "alleles", "skipped_alt", "not_carried", "same_as_ref", "chroms")
CHUNK = 4 << 20


def default_seed(guide_len):
    return min(DEFAULT_SEED, int(guide_len))


def check_seed(seed, guide_len):
    """The seed length S for a scan at guide_len (None: the default), or ValueError."""
    l = int(guide_len)
    if not 1 <= l <= MAX_GUIDE:
        raise ValueError("variant counts exist for guide lengths 1..%d, not %d" % (MAX_GUIDE, l))
    s = default_seed(l) if seed is None else int(seed)
    if not 1 <= s <= l:
        raise ValueError("the seed is 1..%d letters of the guide, not %r" % (l, seed))
    return s


def pack(site, guide, seed, pam):
    """The packed column of four count arrays (each saturates at 255)."""
    c = [np.minimum(np.asarray(v).astype(np.int64), SATURATED).astype(np.uint32) for v in (site, guide, seed, pam)]
    return c[0] | c[1] << np.uint32(8) | c[2] << np.uint32(16) | c[3] << np.uint32(24)


def unpack(col):
    """(site, guide, seed, pam) uint32 arrays of a packed column."""
    c = np.asarray(col, dtype=np.uint32)
    return tuple((c >> np.uint32(sh)) & np.uint32(255) for sh in (0, 8, 16, 24))


def fields(value):
    """The four CSV fields of one packed value."""
    v = int(value)
    return v & 255, v >> 8 & 255, v >> 16 & 255, v >> 24 & 255


class Limits:
    """The bounds a selection puts on the variant counts: site <= max_site, guide <= max_guide, seed <= max_seed, pam <=
    max_pam (None: no bound; the counts saturate at 255, so a bound of 255 or more holds for every row)."""

    def __init__(self, max_site=None, max_guide=None, max_seed=None, max_pam=None):
        vals = []
        for name, v in (("max_site", max_site), ("max_guide", max_guide), ("max_seed", max_seed), ("max_pam", max_pam)):
            n = SATURATED if v is None else int(v)
            if not 0 <= n <= 0xFFFFFFFF:
                raise ValueError("%s is a number of variants, not %r" % (name, v))
            vals.append(n)
        self.max_site, self.max_guide, self.max_seed, self.max_pam = vals

    def astuple(self):
        return (self.max_site, self.max_guide, self.max_seed, self.max_pam)

    def passes(self, col):
        """Boolean array: which rows of a packed column pass."""
        site, guide, seed, pam = unpack(col)
        return (site <= self.max_site) & (guide <= self.max_guide) & (seed <= self.max_seed) & (pam <= self.max_pam)


class VariantSet:
    """The parsed VCF (native handle): per CHROM the intervals of its kept alleles.  path may end in .gz; source: the bytes
    themselves, or an iterable of byte chunks, instead of a file."""

    def __init__(self, path=None, samples=None, pass_only=False, source=None):
        L = nat.lib()
        self._h = None
        names = [s if isinstance(s, bytes) else str(s).encode() for s in (samples or [])]
        arr = (ctypes.c_char_p * max(1, len(names)))(*names)
        h = ctypes.c_void_p()
        nat.check(L.crp_variants_create(arr if names else None, len(names), int(bool(pass_only)), ctypes.byref(h)), "crp_variants_create")
        self._h = h
        self.samples, self.pass_only = [n.decode() for n in names], bool(pass_only)
        for chunk in self._chunks(path, source):
            if chunk:
                buf = np.frombuffer(chunk, dtype=np.uint8)
                self._check(L.crp_variants_add_bytes(self._h, buf.ctypes.data_as(nat.u8p), buf.size), "crp_variants_add_bytes")
        self._check(L.crp_variants_finish(self._h), "crp_variants_finish")
        out = np.zeros(len(STATS), dtype=np.uint64)
        nat.check(L.crp_variants_stats(self._h, out.ctypes.data_as(nat.u64p), out.size), "crp_variants_stats")
        self.stats = {k: int(v) for k, v in zip(STATS, out)}
        self.chrom_index = {}
        for k in range(self.stats["chroms"]):
            name, n = ctypes.c_void_p(), ctypes.c_uint64()
            nat.check(L.crp_variants_chrom(self._h, k, ctypes.byref(name), ctypes.byref(n)), "crp_variants_chrom")
            self.chrom_index[ctypes.string_at(name.value, n.value).decode("utf-8", "replace") if n.value else ""] = k

    @staticmethod
    def _chunks(path, source):
        if source is not None:
            if isinstance(source, (bytes, bytearray, memoryview)):
                yield bytes(source)
            else:
                yield from source
            return
        opener = gzip.open if str(path).endswith(".gz") else open
        with opener(path, "rb") as f:
            while True:
                chunk = f.read(CHUNK)
                if not chunk:
                    return
                yield chunk

    def _check(self, status, what):
        if status != nat.CRP_OK:
            text = nat.lib().crp_variants_error(self._h).decode("utf-8", "replace")
            if text:
                raise ValueError("VCF " + text)
            nat.check(status, what)

    def track(self, entries, dec):
        """(starts uint32, ends1 uint32) for Arena.variant_set_track: entries = [(FASTA name, index of the text's first
        character inside its contig string, length of the text, arena offset)] in arena order."""
        e = np.empty((len(entries), 4), dtype=np.uint64)
        none = np.uint64(0xFFFFFFFFFFFFFFFF)
        for r, (name, lo, length, off) in enumerate(entries):
            k = self.chrom_index.get(name)
            e[r] = (none if k is None else k, lo, length, off)
        n = ctypes.c_uint64()
        L = nat.lib()
        st = L.crp_variants_track(self._h, e.ctypes.data_as(nat.u64p), e.shape[0], int(dec), None, None, 0, ctypes.byref(n))
        if st not in (nat.CRP_OK, nat.CRP_ERR_CAPACITY):
            nat.check(st, "crp_variants_track")
        starts, ends1 = np.empty(n.value, dtype=np.uint32), np.empty(n.value, dtype=np.uint32)
        nat.check(L.crp_variants_track(self._h, e.ctypes.data_as(nat.u64p), e.shape[0], int(dec), starts.ctypes.data_as(nat.u32p),
                                       ends1.ctypes.data_as(nat.u32p), n.value, ctypes.byref(n)), "crp_variants_track")
        return starts, ends1

    def close(self):
        if self._h:
            nat.lib().crp_variants_destroy(self._h)
            self._h = None

    def __del__(self):
        try:  # (at interpreter exit the module globals may already be gone)
            self.close()
        except Exception:
            pass


class Request:
    """What a backend needs to count variants under the texts it scans: the VariantSet, the FASTA name of the contig every
    text comes from, where the text starts inside that contig's string, `dec` -- the annotate.Request's piece layout -- and
    the seed length (None: min(12, guide length))."""

    def __init__(self, variants, names, dec, starts=None, seed=None):
        self.variants, self.names, self.dec = variants, list(names), int(dec)
        self.starts = [0] * len(self.names) if starts is None else [int(s) for s in starts]
        self.seed = seed

    def track(self, layout):
        """layout: [(text index, arena offset, length)] of ONE arena in arena order -> (starts, ends1)."""
        return self.variants.track([(self.names[t], self.starts[t], ln, off) for t, off, ln in layout], self.dec)
