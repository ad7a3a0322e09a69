// crp_select_family.h -- launch interface of crp_select_family.hip (the guide selection with
// family limits, and the family values of given (gene, row) pairs), shared with crp_select.cpp.
#pragma once
#include "crp_select.h"

namespace crp {

constexpr uint32_t SELECT_ALL_MEMBERS = 0xFFFFFFFFu;  // min_members: the size of the gene's family

// The joined plain and family columns of both strands' tables (crp_search_self_join_hits and
// crp_search_self_family_join_hits of one handle: `stride` counts per row in both) and, per gene of the selection
// handle, its family id (0xFFFFFFFF: none) and the size of that family (1 for none).
struct SelectFamily {
    const uint32_t *counts[2];
    const unsigned long long *sum[2];
    const uint32_t *fam_counts[2];
    const unsigned long long *fam_sum[2], *fam_cover[2];
    const uint32_t *site_family[2];
    uint32_t stride;
    const uint32_t *gene_family, *gene_size;
};

struct FamilyLimits {
    unsigned long long max_hit_sum_outside;
    uint32_t max_mm0_outside;
    uint32_t min_members;  // SELECT_ALL_MEMBERS: every member of the gene's family
};

// What a row is worth to gene g's family: the row's site belongs to g's family -> what lies outside
// it and the members covered; else the plain columns and one member.
struct FamilyValues {
    unsigned long long outside_sum;
    unsigned long long cover;  // the row's cover word where its family is the gene's, else 0
    uint32_t outside_mm0, members_hit;
};

__device__ __forceinline__ FamilyValues family_values(const SelectFamily &f, int s, uint32_t row, uint32_t gene_family)
{
    FamilyValues v;
    v.outside_mm0 = f.counts[s][(uint64_t)row * f.stride];
    v.outside_sum = f.sum[s][row];
    v.members_hit = 1u;
    v.cover = 0ull;
    // (An unjoined row has no family and would get the join's all-ones sentinels here.  The selection never sees one: it
    // runs with the joined columns, so the predicate before this has already failed it, and only selected rows are evaluated.)
    if (gene_family != SELECT_NONE && f.site_family[s][row] == gene_family) {
        v.outside_mm0 -= f.fam_counts[s][(uint64_t)row * f.stride];
        v.outside_sum -= f.fam_sum[s][row];
        v.cover = f.fam_cover[s][row];  // (never 0: the site's own member is in it)
        v.members_hit = (uint32_t)__popcll(v.cover);
    }
    return v;
}

// select_items_kernel's work and results (crp_select.h), with the family limits as the predicate's last terms
hipError_t launch_select_items_family(hipStream_t s, const SelectTable &plus, const SelectTable &minus, const SelectPredicate &pred,
                                      const SelectFamily &fam, const FamilyLimits &lim, const SelectItem *items, uint32_t n_items,
                                      const SelectPartials &part, const SelectResult &res);
// The family values of packed_row[q] (row | strand << 31; rows inside the tables) for gene gene_row[q] (inside the
// handle's genes): the host has checked both
hipError_t launch_family_eval(hipStream_t s, const SelectFamily &fam, const uint32_t *gene_row, const uint32_t *packed_row, uint32_t n,
                              uint32_t *outside_mm0, unsigned long long *outside_sum, uint32_t *members_hit, uint32_t *family_size,
                              unsigned long long *cover);

}  // namespace crp
