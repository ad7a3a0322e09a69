// crp_search_self.h -- launch interface of crp_search_self.hip (the self search: every guide site of the genome against
// every candidate site, DESIGN section 15, Self search), shared with its host side crp_search_self.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crp_search.h"

struct crp_arena;
struct crp_search_self;

namespace crp {

constexpr int SELF_MAX_MM = 4;         // M + 1 segments of at least 4 letters in a guide region of 20
constexpr int SELF_MAX_SEG_LETTERS = 8;  // 4^8 buckets x {guide site, other candidate} = 2^17 keys of the counting sort
constexpr int SELF_TILE = BLOCK;       // guide sites per workgroup of the compare kernel: one per lane
constexpr int SELF_UNROLL = 8;         // candidates per trip of the no-hit loop (one scalar load of 8 words per field)
constexpr int SELF_PAD = SELF_UNROLL;  // words behind an ordering that the last trip of a slice may read
constexpr uint32_t SELF_NO_KEY = 0xFFFFFFFFu;  // a candidate with a non-base in the segment: in no bucket

// What a guide site needs beyond being a candidate: at PAM position pos[k] a base of the 4-bit set set[k] (bit = code,
// A=0 T=1 C=2 G=3), and no non-base anywhere in the guide region.
struct SelfGuideRule {
    uint32_t region;   // the guide region's pattern positions
    int n;             // PAM positions where the guide pattern is narrower than the candidate pattern
    uint8_t pos[SEARCH_MAX_T], set[SEARCH_MAX_T];
};

// One ordering of a handle's candidates: by the 2-bit codes of one segment, a bucket's guide sites before its other
// candidates.  The fields are masked to the guide region; idx is the candidate's index in extraction order (its row).
struct SelfOrder {
    const uint32_t *hi, *lo, *nb, *idx;
};

// The compare of one segment: its own mask is not needed (a bucket's members agree there), the masks of the segments
// before it decide whether a pair was already counted.
struct SelfCompare {
    uint32_t before[SELF_MAX_MM];  // masks of segments 0 .. n_before - 1
    int n_before;
    int max_mm;
    int skip_same;  // queries and candidates are one ordering: entry i against entry i is a site against itself
};

// flag[i] = 1 when candidate i is a guide site; adds their number to *n_guides.
hipError_t launch_self_flag(hipStream_t s, const SearchCands &c, uint32_t n, const SelfGuideRule &rule, uint8_t *flag,
                            unsigned long long *n_guides);
// key[i] = (segment code << 1 | not a guide site), or SELF_NO_KEY; hist[key] counts them.  The segment is `len`
// letters from bit `shift`.
hipError_t launch_self_key(hipStream_t s, const SearchCands &c, uint32_t n, const uint8_t *flag, int shift, int len, uint32_t *key,
                           uint32_t *hist);
// Writes every keyed candidate to the next free slot of its key (cursor[key], set to each key's first slot before).
hipError_t launch_self_scatter(hipStream_t s, const SearchCands &c, uint32_t n, const uint32_t *key, uint32_t region, uint32_t *cursor,
                               uint32_t *hi, uint32_t *lo, uint32_t *nb, uint32_t *idx);
// One workgroup per item {first query, queries (<= SELF_TILE), first candidate, candidates}: every pair within
// max_mm mismatches that no earlier segment has counted adds one to counts[row * (max_mm + 1) + mm] and, with a
// score table, its value to hit_sum[row], row = q.idx of the query.
hipError_t launch_self_compare(hipStream_t s, const SelfOrder &q, const SelfOrder &c, const uint4 *items, uint32_t n_items,
                               const SelfCompare &cmp, uint32_t *counts, const SearchScore *score);
// launch_self_compare under a pair table: c_fields are the unmasked fields, in extraction order, of the handle whose
// ordering c is (c.idx indexes them): the candidates' PAM letters are read there.  Values add to pair.hit_sum[row].
hipError_t launch_self_pair_compare(hipStream_t s, const SelfOrder &q, const SelfOrder &c, const SearchCands &c_fields, const uint4 *items,
                                    uint32_t n_items, const SelfCompare &cmp, uint32_t *counts, const SearchPair &pair);
// The CSV join: hit k of a strand's scan table (hit_pos ascending arena match indices; strand 0 '+', 1 '-'; the scan's
// guide length) gets the row of its site -- forward start hit_pos - guide_len for '+', hit_pos for '-' -- when that is a
// guide site among the n_cand candidates c (extraction order): out_counts[k * (max_mm + 1) ..] and out_sum[k]; all-ones
// otherwise, and an all-ones out_sum with hit_sum == nullptr (an unscored handle).
hipError_t launch_self_join(hipStream_t s, const uint32_t *hit_pos, uint32_t n_hits, int strand, int guide_len, const SearchCands &c, uint32_t n_cand,
                            const uint8_t *flag, const uint32_t *counts, const unsigned long long *hit_sum, int max_mm, uint32_t *out_counts,
                            unsigned long long *out_sum);

// The joined columns of a handle's last crp_search_self_join_hits, for the kernels that read them where they lie
// (crp_select.cpp); false without a join.
struct SelfJoined {
    const uint32_t *counts[2];            // stride per row
    const unsigned long long *sum[2];
    uint64_t rows[2];                     // the tables' rows when they were joined
    int stride;                           // max_mm + 1
    const struct ::crp_arena *arena;
};
bool self_joined(const struct ::crp_search_self *s, SelfJoined *out);

}  // namespace crp
