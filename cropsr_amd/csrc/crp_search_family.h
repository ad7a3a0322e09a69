// crp_search_family.h -- launch interface of crp_search_family.hip (gene families on a self-search handle: which
// family gene a candidate site cuts in, and every guide site's row restricted to the candidates of its own family;
// DESIGN section 23), shared with its host side in crp_search_self.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crp_search_self.h"

namespace crp {

constexpr uint32_t FAMILY_NONE = 0xFFFFFFFFu;    // no owner, no family
constexpr uint32_t FAMILY_GUIDE = 0x80000000u;   // a candidate's tag: owner row (31 bits, all-ones = none) | guide site << 31
constexpr uint32_t FAMILY_NO_ROW = 0x7FFFFFFFu;
constexpr int FAMILY_MAX_MEMBERS = 64;           // the cover set is one 64-bit word per site

// One family gene of the handle's arena: its clipped range of arena positions (closed), its family and its bit in the
// family's cover word.  The rows are in GFF order, so the smallest row index is the first owner.
struct FamilyRow {
    uint32_t lo, hi, family, member;
};

// The candidates of a handle as the family kernels read them: the extraction's fields (not masked) and the tag.
struct FamilyCands {
    const uint32_t *hi, *lo, *nb, *tag;
};

struct FamilyCompare {
    uint32_t region;  // the guide region's pattern positions
    int max_mm;
    int cover_mm;     // a guide site within this many mismatches covers its owner
    int same;         // queries and candidates are one handle: index i against index i is a site against itself
};

// run[r] = {first, end}: the candidates (extraction order) whose 64-position word can hold a site that cuts in row r's
// range.  T is the pattern's length (PAM of 3 on the 3' side: a '+' site at start p cuts at p + T - 6, a '-' site at j).
hipError_t launch_family_bounds(hipStream_t s, const FamilyRow *rows, uint32_t n_rows, const uint32_t *cand_pos, uint32_t n_cand, int T,
                                uint2 *run);
// owner[c] = min(owner[c], r) for every candidate c of run[r] that cuts inside row r's range (owner starts all-ones).
hipError_t launch_family_assign(hipStream_t s, const FamilyRow *rows, uint32_t n_rows, const uint2 *run, const uint32_t *cand_pos, int T,
                                uint32_t *owner);
// Turns owner[c] into the tag, writes family[c] (FAMILY_NONE without an owner) and starts cover[c]: the owner's own
// bit for a guide site with an owner, 0 otherwise.
hipError_t launch_family_finish(hipStream_t s, const FamilyRow *rows, const uint8_t *flag, uint32_t n_cand, uint32_t *owner_tag,
                                uint32_t *family, unsigned long long *cover);
// One workgroup per item, two uint4 each: {first query, queries (<= SELF_TILE), first candidate, candidates} and
// {owner row a of the queries, owner row b of the candidates, b's member bit, 0}.  Every query that is a guide site
// owned by a, against every candidate owned by b: counts[q * (max_mm + 1) + mm] += 1, sum[q] += the pair's value
// (score: a scheme, pair: a pair table, both null: counts only), cover[q] |= 1 << member when a candidate that is a
// guide site lies within cover_mm.
hipError_t launch_family_compare(hipStream_t s, const FamilyCands &q, const FamilyCands &c, const uint4 *items, uint32_t n_items,
                                 const FamilyCompare &cmp, uint32_t *counts, unsigned long long *sum, unsigned long long *cover,
                                 const SearchScore *score, const SearchPair *pair);
// The family columns of the CSV join: hit k of a strand's table gets its site's row as launch_self_join finds it
// (a guide site among the candidates), FAMILY_NONE as family without one or when the site has no family; the unjoined
// get all-ones counts and sum like the self join's columns, cover 0.
hipError_t launch_family_join(hipStream_t s, const uint32_t *hit_pos, uint32_t n_hits, int strand, int guide_len, const uint32_t *cand_pos,
                              uint32_t n_cand, const uint32_t *tag, const uint32_t *family, const uint32_t *counts,
                              const unsigned long long *sum, const unsigned long long *cover, int max_mm, uint32_t *out_counts,
                              unsigned long long *out_sum, unsigned long long *out_cover, uint32_t *out_family);


// The joined family columns of a handle's last crp_search_self_family_join_hits, for the selection kernels that read
// them where they lie (crp_select.cpp); false without such a join.
struct SelfFamilyJoined {
    const uint32_t *counts[2];  // max_mm + 1 per row, like SelfJoined's
    const unsigned long long *sum[2], *cover[2];
    const uint32_t *family[2];
    uint64_t rows[2];           // the tables' rows when they were joined
};
bool self_family_joined(const struct ::crp_search_self *s, SelfFamilyJoined *out);

}  // namespace crp
