// crp_splice.h -- the splice-site test of the guide selection (cropsr_amd/baseedit.py states the
// definition): from the arena's bit-planes, a gene row's step function (crp_coding.h has its form) and a row of the hit
// tables to the number of targets a cytosine or an adenine base editor has in the window, the number of canonical donor
// and acceptor sites of the gene's primary transcript P the edit destroys, and the coding letters 5' of the first intron
// of each kind; and on to pass / fail against the splice limits.  One statement, compiled for the host and the device:
// the selection kernel and the evaluation kernel (crp_select_splice.hip) and a CPU driver (tests/native/splice_driver.cpp)
// call these very functions.  No HIP header is needed on the host.
//
// Everything is a bit mask over crp_edit.h's SPAN: the window's letters plus two on either side, bit b = position x0 + b.
// That is enough: the edited letter is a window letter, its site partner is at most one letter away, and the coding letter
// on the far side of the boundary at most one more.  An intron of P is a place where the step function's grow bit goes off
// with cum_P < L_P and comes on again with cum_P > 0; a site is two non-coding letters next to such a boundary.  The
// letters are looked at first: most rows hold no target next to the right partner letter and read no step.
#pragma once
#include <stdint.h>

#include "crp_edit.h"

namespace crp {

constexpr uint32_t SPLICE_NO_SITE = 0xFFFFFFFFu;  // donor_off / acceptor_off of a row whose edit destroys no such site
constexpr uint32_t SPLICE_CBE = 0u, SPLICE_ABE = 1u;          // the editor: C -> T (G -> A on a '-' row), A -> G (T -> C)
constexpr uint32_t SPLICE_DONOR = 1u, SPLICE_ACCEPTOR = 2u;   // bits of SpliceLimits::kinds

struct SpliceLimits {
    uint32_t min_pct, max_pct, max_targets;  // percentages 0..100, min_pct <= max_pct
    uint32_t kinds;                          // SPLICE_DONOR, SPLICE_ACCEPTOR or both
};

struct SpliceOutcome {
    uint32_t targets;       // 0 .. 20: the window's letters the editor converts; depends on no gene
    uint32_t donors;        // evaluated donor sites with a converted letter
    uint32_t acceptors;     // evaluated acceptor sites with a converted letter
    uint32_t donor_off;     // P's coding letters 5' of the intron of the destroyed donor nearest the gene's 5' end, or SPLICE_NO_SITE
    uint32_t acceptor_off;  // the same of the acceptors
};

// What the editor does to P's splice sites at the row with match index `pos` on the '+' (minus_row false) or '-' table, for
// a gene row with n steps at at / word / cum (n may be 0), P's length L and info word `info`.  The steps obey
// crp_select_set_coding's checks and the layout's invariant cum_P <= L_P.
CRP_CODING_FN SpliceOutcome splice_outcome(const EditPlanes &pl, const uint32_t *at, const uint32_t *word, const uint32_t *cum, uint32_t n, uint32_t L,
                                           uint32_t info, uint32_t pos, bool minus_row, const EditWindow &win, uint32_t editor)
{
    const uint32_t wn = win.hi - win.lo + 1u, ns = wn + 4u;  // the span: ns <= 24 letters
    const long long x0 = minus_row ? (long long)pos + 21 - (long long)win.hi : (long long)pos - 23 + (long long)win.lo;
    const uint32_t AC = edit_span(pl.ac, pl.n_words, x0, ns);
    const uint32_t H = edit_span(pl.hi, pl.n_words, x0, ns) & AC, Lo = edit_span(pl.lo, pl.n_words, x0, ns) & AC;
    // the planes' codes: A 00, T 01, C 10, G 11
    const uint32_t A = AC & ~H & ~Lo, T = ~H & Lo, C = H & ~Lo, G = H & Lo;
    const uint32_t W = ((1u << wn) - 1u) << 2;
    const uint32_t tg = W & (editor == SPLICE_ABE ? (minus_row ? T : A) : (minus_row ? G : C));
    SpliceOutcome out = {(uint32_t)__builtin_popcount(tg), 0u, 0u, SPLICE_NO_SITE, SPLICE_NO_SITE};
    const long long end = x0 + (long long)ns;
    if (!(info & CODING_MODEL_BIT) || !n || end <= 0) return out;
    const bool minus_gene = (info & CODING_MINUS_BIT) != 0;
    // what the letters alone make a destroyed site of, by the site's lower letter: the site that begins an intron in ascending
    // positions is forward GT ('+' gene: the donor) or CT ('-' gene: the acceptor), the one that ends it AG or AC
    const uint32_t hit = tg | tg >> 1;
    uint32_t s_site = (minus_gene ? C : G) & T >> 1 & hit;
    uint32_t e_site = A & (minus_gene ? C : G) >> 1 & hit;
    if (!(s_site | e_site)) return out;
    const uint32_t c0 = x0 > 0 ? (uint32_t)x0 : 0u, c1 = (uint32_t)end;
    // the first step that begins after c0: the one before it holds at c0
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (at[mid] <= c0) a = mid + 1;
        else b = mid;
    }
    uint32_t k = a ? a - 1u : 0u;
    // cum_P(c0): before at[0] nothing holds, so nothing is counted between c0 and at[0]
    const uint32_t cum0 = a ? cum[k] + ((word[k] & CODING_GROW_BIT) ? c0 - at[k] : 0u) : cum[0];
    uint32_t grow = 0;  // P's coding letters of the span
    for (; k < n; ++k) {
        const uint32_t from = at[k];
        if (from >= c1) break;
        if (!(word[k] & CODING_GROW_BIT)) continue;
        const uint32_t s = from > c0 ? from : c0;
        uint32_t e = c1;
        if (k + 1 < n && at[k + 1] < c1) e = at[k + 1];
        if (e <= s) continue;
        const uint32_t rb = (uint32_t)((long long)s - x0), re = (uint32_t)((long long)e - x0);  // 0 <= rb < re <= 24
        grow |= ((1u << re) - 1u) & ~((1u << rb) - 1u);
    }
    if (!grow) return out;
    // by the site's lower letter b: an intron start at boundary b (letter b - 1 coding, b and b + 1 not), an intron end at
    // boundary b + 2 (b and b + 1 not coding, b + 2 coding).  A destroyed site has b >= 1 and b + 2 < ns: nothing outside the
    // span is asked for.
    uint32_t starts = grow << 1 & ~grow & ~(grow >> 1), ends = ~grow & ~(grow >> 1) & grow >> 2;
    // the interior: cum_P < L_P where an intron starts, so not behind P's last coding letter -- cum_P is L_P only above the
    // span's highest coding letter, and only if the span's coding letters bring cum0 up to L_P; cum_P > 0 where one ends, so
    // not before P's first -- cum_P is 0 only at the span's lowest coding letter, and only if cum0 is 0
    const uint32_t top = 31u - (uint32_t)__builtin_clz(grow), low = (uint32_t)__builtin_ctz(grow);
    if (cum0 + (uint32_t)__builtin_popcount(grow) >= L) starts &= (2u << top) - 1u;
    if (!cum0) ends &= ~(1u << low >> 2);
    s_site &= starts;
    e_site &= ends;
    if (!(s_site | e_site)) return out;
    const uint32_t n_s = (uint32_t)__builtin_popcount(s_site), n_e = (uint32_t)__builtin_popcount(e_site);
    uint32_t off_s = SPLICE_NO_SITE, off_e = SPLICE_NO_SITE;
    // cum_P at the intron's boundary: the coding letters below the site.  Nearest the 5' end is the lowest position on a
    // '+' gene and the highest on a '-' gene, where the letters 5' of the intron are the L_P - cum_P above it
    if (s_site) {
        const uint32_t bit = minus_gene ? 31u - (uint32_t)__builtin_clz(s_site) : (uint32_t)__builtin_ctz(s_site);
        const uint32_t before = cum0 + (uint32_t)__builtin_popcount(grow & ((1u << bit) - 1u));
        off_s = minus_gene ? L - before : before;
    }
    if (e_site) {
        const uint32_t bit = minus_gene ? 31u - (uint32_t)__builtin_clz(e_site) : (uint32_t)__builtin_ctz(e_site);
        const uint32_t before = cum0 + (uint32_t)__builtin_popcount(grow & ((1u << bit) - 1u));
        off_e = minus_gene ? L - before : before;
    }
    out.donors = minus_gene ? n_e : n_s;
    out.acceptors = minus_gene ? n_s : n_e;
    out.donor_off = minus_gene ? off_e : off_s;
    out.acceptor_off = minus_gene ? off_s : off_e;
    return out;
}

// The limits of the definition, in integers with 64-bit products: for some allowed kind the edit destroys a site of it
// and min_pct L <= 100 off <= max_pct L; and targets <= max_targets.
CRP_CODING_FN bool splice_pass(const SpliceOutcome &o, uint32_t L, const SpliceLimits &lim)
{
    if (o.targets > lim.max_targets) return false;
    const uint64_t lo = (uint64_t)lim.min_pct * L, hi = (uint64_t)lim.max_pct * L;
    const uint64_t d100 = 100ull * o.donor_off, a100 = 100ull * o.acceptor_off;
    const bool donor = (lim.kinds & SPLICE_DONOR) && o.donor_off != SPLICE_NO_SITE && lo <= d100 && d100 <= hi;
    const bool acceptor = (lim.kinds & SPLICE_ACCEPTOR) && o.acceptor_off != SPLICE_NO_SITE && lo <= a100 && a100 <= hi;
    return donor || acceptor;
}

}  // namespace crp
