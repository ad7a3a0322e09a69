// crp_select_spaced.h -- launch interface of crp_select_spaced.hip (spaced selection: K guides per gene whose cut sites
// lie at least D apart), shared with its host side crp_select.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crp_select.h"

namespace crp {

// An item's best candidate of one round (key = the score's bits, 0: none; tie = cut site << 1 | strand; row = row |
// strand << 31).  Of a cut gene after a pick: the pick itself, which the next round's candidates must come after.
struct SpacedProposal {
    unsigned long long key;
    uint32_t tie, row;
};

// What the rounds of the cut genes carry from launch to launch, per gene of the handle: cuts[g * k + u] the cut site of
// pick u, last[g] the latest pick, and per slot the proposals and (round 0) the passing rows; picked[m] = 1 where cut
// gene m took a row this round.
struct SpacedRounds {
    uint32_t *cuts;
    SpacedProposal *last;
    SpacedProposal *prop;
    uint32_t *slot_pass;
    uint32_t *picked;
};

struct SpacedResult {
    uint32_t *n_pass, *n_spaced, *sel;
};

// Whole-gene items (slot == SELECT_NONE) run every round themselves and write the gene's result; `round` is not read
// for them.  A piece of a cut gene runs round `round` alone and writes its proposal.
hipError_t launch_spaced_items(hipStream_t s, const uint32_t *pos_plus, const uint32_t *pos_minus, const unsigned long long *key_plus,
                               const unsigned long long *key_minus, int k, uint32_t min_distance, uint32_t round, const SelectItem *items,
                               uint32_t n_items, const SpacedRounds &rounds, const SpacedResult &res);
// One wave per cut gene: the best of its items' proposals becomes pick `round`.  first_gene: the index of genes[0] among
// the cut genes (picked is indexed by it).
hipError_t launch_spaced_pick(hipStream_t s, const SelectMerge *genes, uint32_t n_genes, uint32_t first_gene, int k, uint32_t round,
                              const SpacedRounds &rounds, const SpacedResult &res);

}  // namespace crp
