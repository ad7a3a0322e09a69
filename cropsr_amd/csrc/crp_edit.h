// crp_edit.h -- the base-editing test of the guide selection (cropsr_amd/baseedit.py states the
// definition): from the arena's bit-planes, a gene row's step function (crp_coding.h has its form) and a row of the hit
// tables to the number of cytosine-editor targets in the window, the number of codons of the gene's primary transcript the
// edit turns into a stop, and the coding offset of the first of them; and on to pass / fail against the edit limits.  One
// statement, compiled for the host and the device: the selection kernel and the evaluation kernel (crp_select_edit.hip)
// and a CPU driver (tests/native/edit_driver.cpp) call these very functions.  No HIP header is needed on the host.
//
// Everything is a bit mask over the SPAN: the window's letters plus two on either side, at most 24 arena positions, bit b
// = position x0 + b.  Per plane that is at most two words, joined by a funnel shift; the step function gives a mask of P's
// coding letters (grow) and a mask of the letters whose coding index is the first of a codon in the span's reading
// direction; the four (gene strand, row strand) cases are a handful of shifted ANDs each.  No recursion, no arrays.
#pragma once
#include <stdint.h>

#include "crp_coding.h"

namespace crp {

constexpr uint32_t EDIT_NO_STOP = 0xFFFFFFFFu;  // stop_off of a row whose edit writes no stop codon
constexpr uint32_t EDIT_GUIDE_LEN = 20;

struct EditWindow {
    uint32_t lo, hi;  // protospacer positions counted from the PAM-distal end, 1 <= lo <= hi <= 20
};

struct EditLimits {
    uint32_t min_pct, max_pct, max_targets;  // percentages 0..100, min_pct <= max_pct
};

struct EditPlanes {
    const uint64_t *hi, *lo, *ac;
    uint64_t n_words;  // a word at or beyond this index is never read: its positions are non-bases
};

struct EditOutcome {
    uint32_t targets;   // 0 .. 20: the window's letters the editor converts; depends on no gene
    uint32_t stops;     // evaluated codons that are no stop and become one
    uint32_t stop_off;  // 3 q of the one with the smallest q, EDIT_NO_STOP if there is none
};

// bits [start, start + n) of a plane as the low n bits (n <= 32); positions below 0 and words at or beyond n_words read
// as zero and are not touched
CRP_CODING_FN uint32_t edit_span(const uint64_t *plane, uint64_t n_words, long long start, uint32_t n)
{
    const long long w = start >= 0 ? start >> 6 : -((-start + 63) >> 6);  // (floor: -1 for a start in -64 .. -1)
    const uint32_t sh = (uint32_t)(start - w * 64);
    const uint64_t x0 = w >= 0 && (uint64_t)w < n_words ? plane[w] : 0ull;
    uint64_t v = x0 >> sh;
    if (sh + n > 64u) {  // (sh >= 33 here: the shift below is 1 .. 31, and the word after a word inside may lie outside)
        const uint64_t x1 = w + 1 >= 0 && (uint64_t)(w + 1) < n_words ? plane[w + 1] : 0ull;
        v |= x1 << (64u - sh);
    }
    return (uint32_t)v & (uint32_t)((1ull << n) - 1ull);
}

// What the editor does at the row with match index `pos` on the '+' (minus_row false) or '-' table, for a gene row with n
// steps at at / word / cum (n may be 0), P's length L and info word `info`.  The steps obey crp_select_set_coding's checks
// and the layout's invariant cum_P <= L_P.
CRP_CODING_FN EditOutcome edit_outcome(const EditPlanes &pl, const uint32_t *at, const uint32_t *word, const uint32_t *cum, uint32_t n, uint32_t L,
                                       uint32_t info, uint32_t pos, bool minus_row, const EditWindow &win)
{
    const uint32_t wn = win.hi - win.lo + 1u, ns = wn + 4u;  // the span: ns <= 24 letters
    // window letter p is x = i - 21 + p on a '+' row and x = j + 23 - p on a '-' row; the span begins two letters before
    const long long x0 = minus_row ? (long long)pos + 21 - (long long)win.hi : (long long)pos - 23 + (long long)win.lo;
    const uint32_t AC = edit_span(pl.ac, pl.n_words, x0, ns);
    const uint32_t H = edit_span(pl.hi, pl.n_words, x0, ns) & AC, Lo = edit_span(pl.lo, pl.n_words, x0, ns) & AC;
    // the planes' codes: A 00, T 01, C 10, G 11
    const uint32_t A = AC & ~H & ~Lo, T = ~H & Lo, C = H & ~Lo, G = H & Lo;
    const uint32_t W = ((1u << wn) - 1u) << 2;
    EditOutcome out = {(uint32_t)__builtin_popcount(W & (minus_row ? G : C)), 0u, EDIT_NO_STOP};
    const long long end = x0 + (long long)ns;
    if (!(info & CODING_MODEL_BIT) || !n || end <= 0) return out;
    const bool minus_gene = (info & CODING_MINUS_BIT) != 0;
    // what the letters alone make a stop of, by the codon's lowest letter: most rows have none and read no step
    uint32_t st;
    if (!minus_gene && !minus_row)  // C -> T in the gene's orientation: CAA, CAG, CGA with the C in the window
        st = C & W & ((A >> 1 & (A | G) >> 2) | (G >> 1 & A >> 2));
    else if (!minus_gene)           // G -> A: TGG with its second or third letter in the window
        st = T & G >> 1 & G >> 2 & (W >> 1 | W >> 2);
    else if (!minus_row)            // forward C -> T, the gene reads G -> A: TGG is CCA forward, third letter first
        st = C & C >> 1 & A >> 2 & (W | W >> 1);
    else                            // forward G -> A, the gene reads C -> T: CAA / CAG / CGA are TTG / CTG / TCG forward
        st = (G & W) >> 2 & ((T >> 1 & (T | C)) | (C >> 1 & T));
    if (!st) return out;
    // a codon begins (in ascending positions) at the letter whose cum_P is 0 mod 3 on a '+' gene; on a '-' gene its
    // ascending-first letter is the codon's third: index L - 1 - cum_P = 2 mod 3, cum_P = L mod 3
    const uint32_t want = minus_gene ? L % 3u : 0u;
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
    uint32_t grow = 0, first = 0;  // P's coding letters of the span; those that begin a codon in ascending positions
    for (; k < n; ++k) {
        const uint32_t from = at[k];
        if (from >= c1) break;
        if (!(word[k] & CODING_GROW_BIT)) continue;
        const uint32_t s = from > c0 ? from : c0;
        uint32_t e = c1;
        if (k + 1 < n && at[k + 1] < c1) e = at[k + 1];
        if (e <= s) continue;
        const uint32_t rb = (uint32_t)((long long)s - x0), re = (uint32_t)((long long)e - x0);  // 0 <= rb < re <= 24
        const uint32_t run = ((1u << re) - 1u) & ~((1u << rb) - 1u);
        const uint32_t d = (want + 3u - (cum[k] + (s - from)) % 3u) % 3u;  // the run's first letter with cum_P = want mod 3
        grow |= run;
        first |= (0x49249249u << (rb + d)) & run;
    }
    const uint32_t whole = first & grow & grow >> 1 & grow >> 2;  // evaluated codons, by their lowest letter (st asks for three bases)
    st &= whole;
    if (!st) return out;
    out.stops = (uint32_t)__builtin_popcount(st);
    if (!minus_gene) {  // the smallest q is the lowest position; 3 q = cum_P of its first letter
        const uint32_t bit = (uint32_t)__builtin_ctz(st);
        out.stop_off = cum0 + (uint32_t)__builtin_popcount(grow & ((1u << bit) - 1u));
    } else {            // the smallest q is the highest position x; 3 q = L - 1 - cum_P(x + 2)
        const uint32_t bit = 31u - (uint32_t)__builtin_clz(st);
        out.stop_off = L - 3u - (cum0 + (uint32_t)__builtin_popcount(grow & ((1u << bit) - 1u)));
    }
    return out;
}

// The limits of the definition, in integers with 64-bit products: the edit writes a stop, min_pct L <= 100 stop_off <=
// max_pct L, and targets <= max_targets.
CRP_CODING_FN bool edit_pass(const EditOutcome &o, uint32_t L, const EditLimits &lim)
{
    if (o.stop_off == EDIT_NO_STOP || o.targets > lim.max_targets) return false;
    const uint64_t off100 = 100ull * o.stop_off;
    return (uint64_t)lim.min_pct * L <= off100 && off100 <= (uint64_t)lim.max_pct * L;
}

}  // namespace crp
