// crp_search.h -- launch interface of crp_search.hip (the off-target search of given guides),
// shared with its host side crp_search.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crp_kernels.h"

struct crp_ctx;

namespace crp {

constexpr int SEARCH_WORDS = BLOCK;  // arena words per workgroup of the two extraction kernels (one word per thread)
constexpr int SEARCH_CPL = 8;        // candidates per lane of the compare kernel
constexpr int SEARCH_MAX_T = 32;
constexpr int SEARCH_MAX_MM = 8;

// The pattern as the extraction kernels read it: a 4-bit base set (bit = code, A=0 T=1 C=2 G=3; 15 = N, no base test)
// per FORWARD window offset o, 16 sets per word.  plus: what the '+' site needs at offset o; minus: what the forward
// character at offset o must be for the '-' site (the pattern letter at T - 1 - o, complemented).
struct SearchSets {
    uint64_t plus[2], minus[2];
    int T;
};

// Candidate sites, SoA: the oriented window as three 32-bit fields (bit p = pattern position p) and where it is.
struct SearchCands {
    uint32_t *hi, *lo, *nb;  // base codes (high bit, low bit) and "not a base"
    uint32_t *pos;           // forward start in the arena | strand << 31 ('-' = 1)
};

// A scoring scheme on the device (Specificity score) and where a scored run sums.  tab holds
// SEARCH_SCORE_WALK factors in the order the kernel walks a mismatch mask (bit b of the mask, or of the bit-reversed mask
// when rev: ascending g either way), then shape[n][d] for n = 0 .. SEARCH_MAX_MM mismatches over a spread of d positions.
constexpr int SEARCH_SCORE_WALK = 32;
constexpr int SEARCH_SCORE_SPREAD = 32;
constexpr int SEARCH_SCORE_TAB = SEARCH_SCORE_WALK + (SEARCH_MAX_MM + 1) * SEARCH_SCORE_SPREAD;
constexpr int SEARCH_SCORE_SHIFT = 30;  // a hit's value is rint(h * 2^30)
struct SearchScore {
    const double *tab;            // SEARCH_SCORE_TAB doubles, each in [0, 1]
    int rev;                      // walk the bit-reversed mask (g descends with the pattern position: PAM on the 5' side)
    unsigned long long *hit_sum;  // per query: the sum of its hits' values
};

// A pair table on the device (Pair tables): a hit's value depends on which query letter faces which
// site letter at every mismatching position, and on the site's PAM letters.  tab holds SEARCH_PAIR_WALK x 16 pair values
// in walk order (bit b of the mask, or of the bit-reversed mask when rev: ascending g either way), each block indexed
// by query code << 2 | site code in the planes' coding (A=00 T=01 C=10 G=11), then SEARCH_PAIR_PAM PAM values indexed by
// the site's codes at the n_pam pattern positions of pam_pos (8 bits each, first position in the low byte and most
// significant in the index; entry 0 is 1.0 when n_pam is 0).
constexpr int SEARCH_PAIR_WALK = 32;
constexpr int SEARCH_PAIR_MAX_PAM = 3;
constexpr int SEARCH_PAIR_PAM = 64;
constexpr int SEARCH_PAIR_TAB = SEARCH_PAIR_WALK * 16 + SEARCH_PAIR_PAM;
struct SearchPair {
    const double *tab;            // SEARCH_PAIR_TAB doubles, each in [0, 1]
    int rev;                      // walk the bit-reversed mask (PAM on the 5' side)
    int n_pam;                    // 0 .. SEARCH_PAIR_MAX_PAM
    uint32_t pam_pos;             // pattern positions of the PAM letters that index the PAM values
    unsigned long long *hit_sum;  // per query: the sum of its hits' values
};

// (x ^ q) | y in one v_bitop3_b32 (truth table over x, q, y = 0xF0, 0xCC, 0xAA): the compiler leaves it as xor + or3
__device__ __forceinline__ uint32_t xor_or(uint32_t x, uint32_t q, uint32_t y) { return __builtin_amdgcn_bitop3_b32(x, q, y, 0xBE); }

// The value of one hit under the scheme (Specificity score): the factors of the mask's bits, walked
// in ascending g, times shape[n][d], as round-to-nearest-even of h * 2^30.  Every step is one correctly rounded f64
// multiply (__dmul_rn: nothing to fuse or reorder), so the host's numpy statement gives the same integer.  A handle
// whose g runs against the bit order (PAM on the 5' side) walks the reversed mask; its walk table is laid out for that.
__device__ __forceinline__ uint32_t hit_value(uint32_t mask, int n, const SearchScore &sc)
{
    uint32_t m = sc.rev ? __builtin_bitreverse32(mask) : mask;
    const int d = 31 - __builtin_clz(mask) - __builtin_ctz(mask);  // last - first mismatching position (mask != 0)
    double hv = 1.0;
    while (m) {
        hv = __dmul_rn(hv, sc.tab[__builtin_ctz(m)]);
        m &= m - 1;
    }
    hv = __dmul_rn(hv, sc.tab[SEARCH_SCORE_WALK + n * SEARCH_SCORE_SPREAD + d]);
    return (uint32_t)__builtin_rint(__dmul_rn(hv, (double)(1u << SEARCH_SCORE_SHIFT)));  // factors and shape are in [0, 1]: <= 2^30
}

// The 2-bit code of a window's letter at pattern position p.
__device__ __forceinline__ uint32_t search_code_at(uint32_t h, uint32_t l, uint32_t p) { return ((h >> p) & 1u) << 1 | ((l >> p) & 1u); }

// The pair factors of a mismatch mask (not 0), walked in ascending g, one correctly rounded f64 multiply per step
// (__dmul_rn: nothing to fuse or reorder), from the window's and the query's code bits behind every set bit.
__device__ __forceinline__ double search_pair_walk(uint32_t mask, uint32_t h, uint32_t l, uint32_t qh, uint32_t ql, const SearchPair &sp)
{
    uint32_t m = sp.rev ? __builtin_bitreverse32(mask) : mask;
    const uint32_t flip = sp.rev ? 31u : 0u;  // bit b of the reversed mask is pattern position 31 - b
    double hv = 1.0;
    while (m) {
        const uint32_t b = (uint32_t)__builtin_ctz(m), p = b ^ flip;
        hv = __dmul_rn(hv, sp.tab[b * 16u + (search_code_at(qh, ql, p) << 2 | search_code_at(h, l, p))]);
        m &= m - 1;
    }
    return hv;
}

// The window's PAM value: h, l must hold the PAM positions (the extraction's fields, not an ordering's masked ones).
__device__ __forceinline__ double search_pair_pam(uint32_t h, uint32_t l, const SearchPair &sp)
{
    uint32_t at = 0;
    for (int k = 0; k < sp.n_pam; ++k) at = at << 2 | search_code_at(h, l, (sp.pam_pos >> (8 * k)) & 255u);
    return sp.tab[SEARCH_PAIR_WALK * 16 + at];
}

// v = rint(walk * pam * 2^30); every value is in [0, 1], so v <= 2^30.
__device__ __forceinline__ uint32_t search_pair_value(double walk, double pam)
{
    return (uint32_t)__builtin_rint(__dmul_rn(__dmul_rn(walk, pam), (double)(1u << SEARCH_SCORE_SHIFT)));
}

// Host side of a scheme (crp_search.cpp), shared by the two handles.  factor[n_factor] and shape[] (CRP_SEARCH_SHAPE_DOUBLES
// values) become tab[SEARCH_SCORE_TAB] as SearchScore wants it.  The walk table: with the PAM on the 3' side the guide
// region is positions 0 .. G - 1 and g is the position, so the mask is walked as it is.  On the 5' side the region is
// positions T - G .. T - 1 and g = T - 1 - position; the kernel walks the bit-reversed mask, where position p is bit
// 31 - p, so g = b - (32 - T) ascends with the bit again.  False when shape is missing, n_factor is outside 1 .. T or a
// value is outside [0, 1] or not finite.
bool search_scheme_layout(int T, const double *factor, int n_factor, bool pam3, const double *shape, double *tab);

// Host side of a pair table, likewise.  pair[n_factor][4][4] (query letter, site letter
// over A, C, G, T; the diagonal is ignored) and pam[4^n_pam_offsets] (the site's letters at those offsets inside the PAM,
// first offset most significant) become tab[SEARCH_PAIR_TAB] and *pam_pos as SearchPair wants them.  False when the
// input is outside the definition: a value outside [0, 1] or not finite, a guide region of n_factor positions on that
// side that is not all N, more than SEARCH_PAIR_MAX_PAM offsets, an offset outside the PAM, not strictly ascending, or on
// a pattern letter N.
bool search_pair_layout(const SearchSets &sets, const double *pair, int n_factor, bool pam3, const int *pam_offsets, int n_pam_offsets,
                        const double *pam, double *tab, uint32_t *pam_pos);

// What a handle knows about how its hits are valued: a scheme or a pair table on the device (one at a time: setting one
// clears the other), the side the walk starts from and the positions that have a factor.  Both handles embed one.  The
// setters return CRP_* codes (CRP_ERR_INVALID for an input the layout functions reject); the callers check what is
// theirs alone (which n_factor and which side the handle allows) before.
struct SearchValueState {
    double *d_scheme = nullptr, *d_pair = nullptr;  // SEARCH_SCORE_TAB / SEARCH_PAIR_TAB doubles, allocated on first use
    bool have_scheme = false, have_pair = false;
    int rev = 0;          // PAM on the 5' side
    uint32_t region = 0;  // the pattern positions that have a factor
    int n_pam = 0;
    uint32_t pam_pos = 0;

    bool any() const { return have_scheme || have_pair; }
    void clear() { have_scheme = have_pair = false; }
    int set_scheme(crp_ctx *ctx, int T, const double *factor, int n_factor, bool pam3, const double *shape);
    int set_pair(crp_ctx *ctx, const SearchSets &sets, const double *pair, int n_factor, bool pam3, const int *pam_offsets, int n_pam_offsets,
                 const double *pam);
    void free();
    SearchScore score(unsigned long long *hit_sum) const { return SearchScore{d_scheme, rev, hit_sum}; }
    SearchPair pair(unsigned long long *hit_sum) const { return SearchPair{d_pair, rev, n_pam, pam_pos, hit_sum}; }
};

// Per workgroup of SEARCH_WORDS words: {'+' candidates, '-' candidates}.
hipError_t launch_search_count(hipStream_t s, const Planes &pl, uint64_t used_words, const SearchSets &sets, uint2 *block_cnt);
// Writes the candidates of workgroups [block_first, block_first + n_blocks): those of workgroup b start at block_off[b]
// (relative to the chunk), in word order, each word's '+' starts ascending before its '-' starts.
hipError_t launch_search_emit(hipStream_t s, const Planes &pl, uint64_t used_words, const SearchSets &sets, uint32_t block_first,
                              uint32_t n_blocks, const uint32_t *block_off, SearchCands out);
// Compares candidates [0, n) with queries [q0, q0 + nq) of `queries` ({hi, lo, compare mask, 0} per query): every pair
// within max_mm adds one to counts[q * (max_mm + 1) + mm] and appends {q << 4 | mm, pos} to sites (slots >= site_cap are
// counted in *site_ctr, not written).
hipError_t launch_search_compare(hipStream_t s, const SearchCands &c, uint32_t n, const uint4 *queries, uint32_t q0, uint32_t nq,
                                 int max_mm, uint32_t *counts, uint2 *sites, uint64_t site_cap, unsigned long long *site_ctr);
// launch_search_compare plus the score: every pair with 1 .. max_mm mismatches also adds its value to score.hit_sum[q].
// No query may have a base at a position without a factor (outside the guide region).
hipError_t launch_search_score_compare(hipStream_t s, const SearchCands &c, uint32_t n, const uint4 *queries, uint32_t q0, uint32_t nq,
                                       int max_mm, uint32_t *counts, uint2 *sites, uint64_t site_cap, unsigned long long *site_ctr,
                                       const SearchScore &score);
// launch_search_score_compare under a pair table: every pair with 1 .. max_mm mismatches adds its value to
// pair.hit_sum[q] (0 when a mismatching position of the site holds a non-base).
hipError_t launch_search_pair_compare(hipStream_t s, const SearchCands &c, uint32_t n, const uint4 *queries, uint32_t q0, uint32_t nq,
                                      int max_mm, uint32_t *counts, uint2 *sites, uint64_t site_cap, unsigned long long *site_ctr,
                                      const SearchPair &pair);
// The same for the windows of one bulge kind (Bulges): candidates of T + dna or T - rna characters
// (one of dna, rna is 0, the other 1 or 2), queries of T letters as {hi, lo, compare mask, s_min | s_max << 8} (the
// placements s of the bulge's first query position).  Every pair whose fewest mismatches over s is within max_mm adds
// one to counts[q * (max_mm + 1) + mm] and appends {q << 9 | s << 4 | mm, pos}, s the smallest placement with mm
// (q < 2^23).
hipError_t launch_search_bulge_compare(hipStream_t s, const SearchCands &c, uint32_t n, const uint4 *queries, uint32_t q0, uint32_t nq,
                                       int max_mm, int dna, int rna, uint32_t *counts, uint2 *sites, uint64_t site_cap,
                                       unsigned long long *site_ctr);

}  // namespace crp
