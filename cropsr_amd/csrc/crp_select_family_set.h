// crp_select_family_set.h -- launch interface of crp_select_family_set.hip (one greedy step of the
// family sets -- per family the candidate that covers most members not yet covered), shared with crp_select.cpp.
#pragma once
#include "crp_select_family.h"

namespace crp {

// A proposal: the best candidate of one work item (step kernel) or of one family in this arena (pick kernel).  gain 0: none.
// key = the score's bits, cover = the candidate's cover word c, tie = cut << 1 | strand, row = table row | strand << 31,
// gene = the layout row the candidate was found for.  The layout of crp_family_step_best (include/cropsr_hip.h).
struct FamilyProposal {
    unsigned long long key, cover;
    uint32_t gain, tie, row, gene;
};

// The order of the greedy step inside one arena: more new members, then the higher score, then the smaller cut site and
// strand, then the smaller layout row.  (tie, gene) names a candidate of an arena, so the order is total.
__host__ __device__ __forceinline__ bool set_better(uint32_t ga, unsigned long long ka, uint32_t ta, uint32_t ra, uint32_t gb,
                                                    unsigned long long kb, uint32_t tb, uint32_t rb)
{
    if (ga != gb) return ga > gb;
    if (ka != kb) return ka > kb;
    if (ta != tb) return ta < tb;
    return ra < rb;
}

// One wave per item (SelectItem::slot is not read): prop[item] = the item's best candidate against covered[family of the
// item's gene].  Every item's gene has a family below the length of `covered`, its rows lie inside the tables and its gene
// inside gene_member: the host has checked all three.
hipError_t launch_family_set_step(hipStream_t s, const SelectTable &plus, const SelectTable &minus, const SelectPredicate &pred,
                                  const SelectFamily &fam, const FamilyLimits &lim, const uint32_t *gene_member,
                                  const unsigned long long *covered, const SelectItem *items, uint32_t n_items, FamilyProposal *prop);
// One wave per family: best[f] = the best of prop[slots[i]], start[f] <= i < start[f + 1] (gain 0 without one).
hipError_t launch_family_set_pick(hipStream_t s, const FamilyProposal *prop, const uint32_t *start, const uint32_t *slots,
                                  uint32_t n_families, FamilyProposal *best);

}  // namespace crp
