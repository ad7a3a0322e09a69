// crp_select_pairs_distinct.h -- launch interface of crp_select_pairs_distinct.hip (distinct pair selection: KP pairs per
// gene that share no guide), shared with its host side crp_select.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crp_select.h"

namespace crp {

// A piece's best candidate of one round, in the pairs' order: kmin / kmax (the smaller and the larger score's bits),
// tie = c_a << 32 | c_b, a / b (row | strand << 31; a SELECT_NONE: no candidate).
struct PairProposal {
    unsigned long long kmin, kmax, tie;
    uint32_t a, b;
};

// What the rounds of the cut genes carry from launch to launch, beside the taken rows -- those are the gene's 2 k packed
// rows in PairDistinctResult::pairs, which the pick kernel appends to: per slot the proposals and (round 0) the passing
// a-rows and the qualifying pairs; picked[m] = 1 where cut gene m took a pair this round.
struct PairDistinctRounds {
    PairProposal *prop;
    uint32_t *slot_pass;
    unsigned long long *slot_pairs;
    uint32_t *picked;
};

struct PairDistinctResult {
    uint32_t *n_pass;             // per gene
    unsigned long long *n_pairs;  // per gene
    uint32_t *n_distinct;         // per gene: the pairs taken
    uint32_t *pairs;              // per gene k * 2: a then b, in pick order
};

// Whole-gene items (slot == SELECT_NONE) run every round themselves and write the gene's result; `round` is not read
// for them.  A piece of a cut gene runs round `round` alone and writes its proposal.  evals[item]: partner rows the item
// streamed, summed over its rounds.
hipError_t launch_pair_distinct_items(hipStream_t s, const uint32_t *pos_plus, const uint32_t *pos_minus, const unsigned long long *key_plus,
                                      const unsigned long long *key_minus, const PairParams &pp, uint32_t round, const PairItem *items,
                                      uint32_t n_items, unsigned long long *evals, const PairDistinctRounds &rounds,
                                      const PairDistinctResult &res);
// One wave per cut gene: the best of its items' proposals becomes pick `round`.  first_gene: the index of genes[0] among
// the cut genes (picked is indexed by it).
hipError_t launch_pair_distinct_pick(hipStream_t s, const SelectMerge *genes, uint32_t n_genes, uint32_t first_gene, int k, uint32_t round,
                                     const PairDistinctRounds &rounds, const PairDistinctResult &res);

}  // namespace crp
